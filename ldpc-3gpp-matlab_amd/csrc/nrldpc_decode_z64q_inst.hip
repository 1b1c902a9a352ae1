// nrldpc_decode_z64q_inst.hip -- one (BG, Z) instantiation of the compile-time-Z decoder whose split form searches the two
// smallest magnitudes over pairs of edges (nrldpc_decode_z64_pair.h).  build.py compiles the pairs of Z64_PAIR from this file
// and every other pair from nrldpc_decode_z64_inst.hip, with the same -D flags and the same object names:
//     hipcc -c -DNRLDPC_Z64_BG=1 -DNRLDPC_Z64_Z=384 nrldpc_decode_z64q_inst.hip -o z64_1_384.o
// Order matters: the partial specialisations of GroupZ64 in the pair header must be seen after the primary template and before
// the launcher, which is the first non-template use -- everything in between is a template that the launcher instantiates.
#ifndef NRLDPC_Z64_BG
#define NRLDPC_Z64_BG 1
#endif
#ifndef NRLDPC_Z64_Z
#define NRLDPC_Z64_Z 384
#endif
#include "nrldpc_decode_z64.h"
#include "nrldpc_decode_z64_pair.h"
#include "nrldpc_decode_z64_inst.hip"

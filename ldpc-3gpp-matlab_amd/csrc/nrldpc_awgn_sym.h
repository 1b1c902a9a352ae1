// nrldpc_awgn_sym.h -- the per-symbol device code of the stand-alone AWGN stage, one copy for the kernel of one configuration
// (nrldpc_awgn.hip) and for the mixed-batch kernel (nrldpc_mix_modem.hip).  The text stood in nrldpc_awgn.hip.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// Include it AFTER the unit's `#pragma clang fp contract(off)`: both units compile this code without floating-point contraction
// (why: nrldpc_awgn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_noise.h"

namespace nrldpc {

// (re, im) + the noise of one symbol.  sigma = sqrt(N0 / 2) per rail is formed here from the f32 N0, for the scalar and for the array
// alike: the two give the same bits.  N0 == 0 gives sigma == 0 and noise +-0: the symbol comes back as the number it was.
__device__ __forceinline__ void add_noise(uint32_t w1, uint32_t w2, float n0, float& re, float& im) {
    float rad, cs, sn;
    box_muller(w1, w2, sqrtf(0.5f * n0), rad, cs, sn);
    const float ni = rad * cs, nq = rad * sn;
    re += ni;
    im += nq;
}

} // namespace nrldpc

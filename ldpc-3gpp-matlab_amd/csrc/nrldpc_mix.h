// nrldpc_mix.h -- mixed transport-block batches: the packed layout, the device-side tables and the workgroup mapping of
// nrldpc_mix_rate_recover_dev / nrldpc_mix_crc_check_dev and their HARQ forms nrldpc_mix_rate_recover_harq_dev /
// nrldpc_mix_crc_check_harq_dev (nrldpc_mix.hip; semantics: include/nrldpc.h, DESIGN.md sections 4.15 and 4.16).
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// The first part -- layout arithmetic, table records, the workgroup -> (configuration, code block, tile) mapping -- is plain C++
// that a host compiler reads too: tests/mix_host/mix_map_check.cpp walks both grids of a mix on the CPU (address and undefined-
// behaviour sanitizers on) and checks that every index the kernels form stays inside its segment.  An out-of-range index in a
// table-driven kernel is a fault.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NRLDPC_MIX_HD __host__ __device__ __forceinline__
#else
#define NRLDPC_MIX_HD inline
#endif

namespace nrldpc {

constexpr int MIX_ALIGN = 16;                    // every segment of every packed array starts at a multiple of 16 ELEMENTS
constexpr int MIX_RM_SWEEPS = 2;                 // sweeps of 256 consecutive positions per wave (= RRX_SWEEPS, nrldpc_ratematch_ex.hip)
constexpr int MIX_RM_TILE = 64 * 4 * MIX_RM_SWEEPS; // positions per wave
constexpr int MIX_RM_WG = 4 * MIX_RM_TILE;       // positions per workgroup of four waves

NRLDPC_MIX_HD int64_t mix_round_up(int64_t x) { return (x + (MIX_ALIGN - 1)) / MIX_ALIGN * MIX_ALIGN; }

// the seven packed arrays, in the order of nrldpc_mix_offsets (include/nrldpc.h)
enum { MIX_G = 0, MIX_HARQ, MIX_CW, MIX_C_HAT, MIX_CB, MIX_B_HAT, MIX_TB, MIX_FIELDS };

// elements configuration i takes in each array: exactly the arrays of the single-configuration calls
NRLDPC_MIX_HD void mix_sizes(int64_t n_tb, int64_t C, int64_t G, int64_t N_cb, int64_t N_cw, int64_t K, int64_t B, int64_t (&s)[MIX_FIELDS]) {
    s[MIX_G] = n_tb * G;
    s[MIX_HARQ] = n_tb * C * N_cb;
    s[MIX_CW] = n_tb * C * N_cw;
    s[MIX_C_HAT] = n_tb * C * K;
    s[MIX_CB] = n_tb * C;
    s[MIX_B_HAT] = n_tb * B;
    s[MIX_TB] = n_tb;
}

// One configuration of the rate-recovery launch.  `form` is what the single-configuration launch rule picks for it:
//   0 general (some E_r exceeds the buffer's non-filler positions: the repetition walk), 1 the plain gather;
//   echo != 0: with a soft buffer the single call runs its input-driven form, which leaves a buffer position that receives nothing
//   as it is (the gathers store buffer + 0 back: the same number, but -0 becomes +0) -- the mix kernel does the same.
struct MixRmRec {
    int64_t g_off, harq_off, cw_off; // element offsets of the segment in g_tilde, the soft buffer, the codeword LLRs
    int32_t n_tb, C, G, Z, K, Kp, N, N_cb, k0, Qm;
    int32_t form, echo;
    int32_t e_base;                  // E_r[r] = e_tab[e_base + r], offset of block r inside a g_tilde row = off_tab[e_base + r]
    int32_t wg_per_cb;               // workgroups per code block = ceil((2Z + N) / MIX_RM_WG)
};

struct MixRmWork {
    int32_t cfg;   // configuration
    int32_t blk;   // tb * C + r inside the configuration
    int32_t tile0; // first position of wave 0's tile inside the code block's decoder input
};

// prefix[0 .. n]: prefix[i] = work items (workgroups / transport blocks) of the configurations before i.  The configuration
// of item x is the LAST i with prefix[i] <= x: empty configurations share their prefix with the next one and are skipped.
// Requires 0 <= x < prefix[n].
NRLDPC_MIX_HD int32_t mix_find(const int32_t* prefix, int32_t n, int32_t x) {
    int32_t lo = 0, hi = n; // invariant: prefix[lo] <= x < prefix[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// workgroup wg of the rate-recovery grid -> its configuration, code block and first position
NRLDPC_MIX_HD MixRmWork mix_rm_work(const int32_t* prefix, const MixRmRec* recs, int32_t n, int32_t wg) {
    MixRmWork w;
    w.cfg = mix_find(prefix, n, wg);
    const int32_t local = wg - prefix[w.cfg];
    const int32_t per = recs[w.cfg].wg_per_cb;
    w.blk = local / per;
    w.tile0 = (local - w.blk * per) * MIX_RM_WG;
    return w;
}

NRLDPC_MIX_HD int32_t mix_rm_wg_per_cb(int32_t ncwz) { return (ncwz + MIX_RM_WG - 1) / MIX_RM_WG; }

// ---- the flag arrays of the HARQ forms (tests/mix_host/mix_harq_check.cpp walks these on the CPU too) ----------------------------------
// d_new: one byte per transport block in the packed `tb` layout; d_cbgti: one byte per code block in the packed `cb` layout.
// tb_off / cb_off: where the configuration's segment starts in that layout (nrldpc_mix_offsets::tb / ::cb).
NRLDPC_MIX_HD int64_t mix_new_index(int64_t tb_off, int32_t tb) { return tb_off + tb; }
NRLDPC_MIX_HD int64_t mix_cbgti_index(int64_t cb_off, int32_t C, int32_t tb, int32_t r) { return cb_off + (int64_t)tb * C + r; }
// the d_new element of a rate-recovery workgroup (a workgroup is one code block of ONE transport block: the flag is workgroup-uniform);
// tb_offs[i] = nrldpc_mix_offsets::tb of configuration i
NRLDPC_MIX_HD int64_t mix_rm_new_index(const int64_t* tb_offs, const MixRmRec* recs, const MixRmWork& w) {
    return mix_new_index(tb_offs[w.cfg], w.blk / recs[w.cfg].C);
}

} // namespace nrldpc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "nrldpc_kernels.h" // CrcPlan

namespace nrldpc {

// One configuration of the CRC launch.  A workgroup is one transport block; tb_prefix gives its configuration.
struct MixCrcRec {
    int64_t c_hat_off, b_hat_off, cb_off, tb_off;
    int32_t C, K, Kp, Lcb, A, B;
    int32_t pad_[2];
    CrcPlan cb, tb;
};

struct MixRmLaunch {
    const MixRmRec* recs;     // device, [n]
    const int32_t* prefix;    // device, [n + 1] workgroups
    const int32_t* e_tab;     // device: E_r of every configuration
    const int32_t* off_tab;   // device: offsets of the code blocks inside a g_tilde row
    int32_t n, n_wg;
    const void* g;
    void* harq;
    void* out;
    int32_t in_f16, harq_f16, out_f16;
};
hipError_t launch_mix_rate_recover(const MixRmLaunch& a, hipStream_t stream);

// The HARQ form: the same launch block plus the per-transport-block "starts a new HARQ process" flags.  A structure of its own, so
// that the argument block -- and with it the code -- of the plain kernels stays what it was.
struct MixRmHarqLaunch {
    MixRmLaunch b;            // b.harq is never null here
    const int64_t* tb_offs;   // device, [n]: nrldpc_mix_offsets::tb of every configuration
    const uint8_t* is_new;    // device, packed tb layout; never null (no flags: the plain kernel is launched)
};
hipError_t launch_mix_rate_recover_harq(const MixRmHarqLaunch& a, hipStream_t stream);

struct MixCrcLaunch {
    const MixCrcRec* recs;    // device, [n]
    const int32_t* prefix;    // device, [n + 1] transport blocks
    int32_t n, n_tb_total;
    int32_t waves;            // waves per workgroup: min(4, largest C of the plan)
    int32_t k_max, c_max;     // largest K and C of the plan: the LDS a workgroup needs
    const uint8_t* c_hat;
    uint8_t* b_hat;
    int32_t* ok;
    int32_t* cb_pass;         // nullable
};
hipError_t launch_mix_crc_check(const MixCrcLaunch& a, hipStream_t stream);

// The HARQ form (the state machine of nrldpc_crc_check_kernel per transport block): b.cb_pass is in/out and never null
struct MixCrcHarqLaunch {
    MixCrcLaunch b;
    const uint8_t* cbgti;     // device, packed cb layout; null = every flag 1
    const uint8_t* is_new;    // device, packed tb layout; null = no transport block starts a new HARQ process
};
hipError_t launch_mix_crc_check_harq(const MixCrcHarqLaunch& a, hipStream_t stream);

} // namespace nrldpc
#endif

// nrldpc_ratematch_ex.h -- launch arguments of nrldpc_rate_recover_ex_dev (nrldpc_ratematch_ex.hip): rate recovery with the
// element types of the demodulator LLRs, of the HARQ soft buffer and of the codeword LLRs chosen per call.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrldpc {

constexpr int RMX_MAX_C = 160; // = NRLDPC_MAX_C (nrldpc_kernels.h)

struct RmExArgs {
    const void* g;    // [n_tb][G] demodulator LLRs, f32 or f16 (in_f16)
    void* harq;       // [n_tb][C][N_cb] soft buffer, f32 or f16 (harq_f16), accumulated in place; null when I_HARQ == 0
    void* out;        // [n_tb*C][2Z+N] f32 or f16 (out_f16)
    int32_t in_f16, harq_f16, out_f16;
    int32_t n_tb, C, G, Z, K, Kp, N, N_cb, k0, Qm;
    int32_t E[RMX_MAX_C];   // E_r
    int32_t off[RMX_MAX_C]; // offset of code block r inside g_tilde
};
hipError_t launch_rate_recover_ex(const RmExArgs& a, hipStream_t stream);

} // namespace nrldpc

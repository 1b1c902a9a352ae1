// nrldpc_channel_sym.h -- the per-symbol device code of the fused channel kernel, one copy for the kernel of one configuration
// (nrldpc_channel.hip) and for the mixed-batch kernel (nrldpc_mix_chan.hip).  The text stood in nrldpc_channel.hip.  Both units
// compile it with floating-point contraction allowed (neither sets a pragma): which multiply-adds become one instruction is the
// compiler's choice per kernel it is inlined into (DESIGN.md section 4.20 says what the two kernels ended on).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_kernels.h" // ChanArgs
#include "nrldpc_modem.h"
#include "nrldpc_noise.h"

namespace nrldpc {

// LLRs of one symbol from its bits and the two uniform words of its noise sample
template <int QM> __device__ __forceinline__ void symbol_llr(const ChanArgs& a, const uint8_t* g, uint32_t w1, uint32_t w2, float* o) {
    // Box-Muller on the hardware's transcendentals (nrldpc_noise.h).  The kernel issues VALU instructions, not bytes (438 per thread
    // before, most of them there and in Philox): it is bound by that, not by HBM.  Results move by ~1e-6 relative; the test's tolerance
    // on an LLR is 5e-4 (tests/test_chain_gpu.py).
    float rad, cs, sn;
    box_muller(w1, w2, a.sigma, rad, cs, sn); // sigma = sqrt(N0/2) per rail
    const float ni = rad * cs, nq = rad * sn;
    if constexpr (QM == 1) { // comm.PSKModulator order 2, phase offset pi/4 (NRModulator.m:73): LLR = 4 Re(rx e^{-j pi/4}) / N0
        const float tx = (g[0] & 1u) ? -1.0f : 1.0f;
        const float y = tx + (ni + nq) * 0.70710678118654752f; // noise projected onto the signalling axis
        o[0] = 4.0f * y * a.inv_n0;
    } else {
        constexpr int NB = QM / 2;
        uint32_t wi = 0, wq = 0;
#pragma unroll
        for (int k = 0; k < NB; ++k) { wi = (wi << 1) | (g[2 * k] & 1u); wq = (wq << 1) | (g[2 * k + 1] & 1u); }
        const float yi = pam_level<NB>(wi) * a.inv_norm + ni, yq = pam_level<NB>(wq) * a.inv_norm + nq;
        float li[NB], lq[NB];
        rail_llr<NB>(yi, a.inv_n0, a.inv_norm, li);
        rail_llr<NB>(yq, a.inv_n0, a.inv_norm, lq);
#pragma unroll
        for (int k = 0; k < NB; ++k) { o[2 * k] = li[k]; o[2 * k + 1] = lq[k]; }
    }
}

} // namespace nrldpc

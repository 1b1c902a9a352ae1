// nrldpc_modem_sym.h -- the per-symbol device code of the stand-alone symbol mapper and soft demapper, one copy for the kernels of one
// configuration (nrldpc_modem.hip) and for the mixed-batch kernels (nrldpc_mix_modem.hip): symbols per thread, the map of one symbol,
// the max-log rail, the Q_m values of one symbol by decision method, the clamped f16 conversion.  The text stood in nrldpc_modem.hip.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// Include it AFTER the unit's `#pragma clang fp contract(off)`: both units compile this code without floating-point contraction
// (why: nrldpc_modem.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "nrldpc.h"
#include "nrldpc_modem.h"

namespace nrldpc {

template <int QM> struct SymbolsPerThread { static constexpr int value = QM == 1 ? 4 : 2; };

// ---- mapper ----------------------------------------------------------------------------------------------------------------------
template <int QM> __device__ __forceinline__ void map_symbol(const uint8_t* g, float inv_norm, float& re, float& im) {
    if constexpr (QM == 1) { // comm.PSKModulator order 2, phase offset pi/4 (NRModulator.m:73)
        re = im = (g[0] & 1u) ? -0.70710678118654752f : 0.70710678118654752f;
    } else {
        constexpr int NB = QM / 2;
        uint32_t wi = 0, wq = 0;
#pragma unroll
        for (int k = 0; k < NB; ++k) { wi = (wi << 1) | (g[2 * k] & 1u); wq = (wq << 1) | (g[2 * k + 1] & 1u); }
        re = pam_level<NB>(wi) * inv_norm;
        im = pam_level<NB>(wq) * inv_norm;
    }
}

// ---- demapper --------------------------------------------------------------------------------------------------------------------
// max-log rail: d[k] = min over the levels with bit k = 1 of (y - level)^2  -  min over those with bit k = 0; LLR_k = d[k] / N0 and
// the hard bit is d[k] < 0 (nearest level; a tie gives 0).  d[k] is never -0 for a finite y, so the sign bit of the LLR is the hard bit.
template <int NB> __device__ __forceinline__ void rail_maxlog(float y, float inv_norm, float (&d)[NB]) {
    if constexpr (NB == 1) { // one level per bit value: ((y+p)^2 - (y-p)^2) = 4 p y, the exact LLR's numerator
        d[0] = 4.0f * inv_norm * y + 0.0f;
        return;
    }
    float mn[NB][2];
#pragma unroll
    for (int k = 0; k < NB; ++k) mn[k][0] = mn[k][1] = 3.0e38f;
#pragma unroll
    for (uint32_t c = 0; c < (1u << NB); ++c) {
        const float e = y - pam_level<NB>(c) * inv_norm, e2 = e * e;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int bit = (c >> (NB - 1 - k)) & 1u;
            mn[k][bit] = fminf(mn[k][bit], e2);
        }
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) d[k] = mn[k][1] - mn[k][0];
}

// Q_m values of one symbol: LLRs (METHOD 0 exact, 1 max-log) or, for METHOD 2, the max-log numerators whose sign is the hard bit
template <int QM, int METHOD> __device__ __forceinline__ void demap_symbol(float re, float im, float inv_n0, float inv_norm, float* o) {
    if constexpr (QM == 1) { // the signalling axis is e^{j pi/4}: LLR = 4 Re(rx e^{-j pi/4}) / N0
        const float y = (re + im) * 0.70710678118654752f;
        if constexpr (METHOD == NRLDPC_DEMOD_LLR) o[0] = 4.0f * y * inv_n0;
        else if constexpr (METHOD == NRLDPC_DEMOD_APPROX_LLR) o[0] = (4.0f * y + 0.0f) * inv_n0;
        else o[0] = 4.0f * y + 0.0f;
    } else {
        constexpr int NB = QM / 2;
        float li[NB], lq[NB];
        if constexpr (METHOD == NRLDPC_DEMOD_LLR) {
            rail_llr<NB>(re, inv_n0, inv_norm, li);
            rail_llr<NB>(im, inv_n0, inv_norm, lq);
        } else {
            rail_maxlog<NB>(re, inv_norm, li);
            rail_maxlog<NB>(im, inv_norm, lq);
            if constexpr (METHOD == NRLDPC_DEMOD_APPROX_LLR) {
#pragma unroll
                for (int k = 0; k < NB; ++k) { li[k] *= inv_n0; lq[k] *= inv_n0; }
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) { o[2 * k] = li[k]; o[2 * k + 1] = lq[k]; }
    }
}

// f16 with the clamp: a strong symbol must not become +inf, which the decoder reads as a filler bit (nrldpc.h, LLR conventions)
__device__ __forceinline__ uint32_t f16_bits(float x) {
    return __half_as_ushort(__float2half_rn(fminf(fmaxf(x, -65504.0f), 65504.0f)));
}

} // namespace nrldpc

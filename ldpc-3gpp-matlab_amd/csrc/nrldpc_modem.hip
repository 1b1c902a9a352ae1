// nrldpc_modem.hip -- the stand-alone symbol mapper and soft demapper: NRModulator.m:73-81 and NRDemodulator.m:76-96 as kernels of
// their own, for a caller whose channel is not the library's (a capture, an equaliser's output with per-symbol noise variance, a
// fading model).  The Monte-Carlo loop keeps the fused kernel (nrldpc_channel.hip), where the symbols never exist in memory; the
// rail arithmetic of the two is the same code (nrldpc_modem.h).
//
// Elementwise and stateless: a thread owns S consecutive symbols -- 2, or 4 for BPSK -- so that everything it reads and writes
// (S*Q_m bit bytes, S (re, im) pairs, S*Q_m LLRs or hard-bit bytes) is a whole number of dwords; both rails of a symbol stay in
// registers; no LDS, no atomics.  Wide accesses are made through pointers that only promise dword alignment (what a float array
// gives; global_load/store_dwordx2/x4 need no more on gfx950), so float arrays have one path for every legal address.  Byte and
// half arrays (bits in, hard bits or f16 LLRs out) take the dword path when their base is dword-aligned -- one test per launch,
// the per-thread stride is a multiple of 4 bytes -- and element accesses otherwise; the last thread of an n_sym that is no
// multiple of S takes guarded element accesses.  One thread per S symbols at every size a link produces (a one-shot grid: a
// persistent 2048-workgroup copy measured an eighth slower than a one-shot one at the stage sizes,
// profiles/r06_hbm_copy_at_stage_sizes.txt); the grid-stride loop only serves counts beyond 2^20 workgroups.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

// No floating-point contraction in this unit (the shared rail arithmetic included): which multiply-add pairs the compiler fuses
// differs between the S symbols of a thread, and a symbol's LLR must not depend on which of a thread's slots it falls into -- a
// call over a buffer has to equal calls over its parts bit for bit.  Every operation left is a single IEEE operation or one
// deterministic hardware instruction (v_exp_f32, v_log_f32) on the symbol's own values.
#pragma clang fp contract(off)

#include "nrldpc.h"
#include "nrldpc_modem.h"
#include "nrldpc_modem_sym.h"

namespace nrldpc {

// load_words<N> / store_words<N>, the wide accesses at a dword-aligned address: nrldpc_modem.h (shared with nrldpc_awgn.hip)

constexpr int MODEM_BLOCK = 256, MODEM_MAX_GRID = 1 << 20;
// SymbolsPerThread, map_symbol, rail_maxlog, demap_symbol, f16_bits, the per-symbol code: nrldpc_modem_sym.h (shared with nrldpc_mix_modem.hip)

// ---- mapper ----------------------------------------------------------------------------------------------------------------------
template <int QM> __global__ __launch_bounds__(MODEM_BLOCK) void nrldpc_modulate_kernel(const ModArgs a, const int g_words) {
    constexpr int S = SymbolsPerThread<QM>::value, NBYTE = S * QM;
    const int64_t nthr = (a.n_sym + S - 1) / S;
    for (int64_t t = (int64_t)blockIdx.x * MODEM_BLOCK + threadIdx.x; t < nthr; t += (int64_t)gridDim.x * MODEM_BLOCK) {
        const int64_t s0 = t * S;
        const int nv = (int)(a.n_sym - s0 < S ? a.n_sym - s0 : S); // symbols of this thread that exist
        const uint8_t* g = a.g + s0 * QM;
        float* dst = a.tx + 2 * s0;
        uint8_t bits[NBYTE];
        if (nv == S && g_words) {
            uint32_t w[NBYTE / 4];
            load_words(g, w);
#pragma unroll
            for (int k = 0; k < NBYTE; ++k) bits[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        } else {
#pragma unroll
            for (int k = 0; k < NBYTE; ++k) bits[k] = k < nv * QM ? g[k] : (uint8_t)0;
        }
        float o[2 * S];
#pragma unroll
        for (int s = 0; s < S; ++s) map_symbol<QM>(bits + s * QM, a.inv_norm, o[2 * s], o[2 * s + 1]);
        if (nv == S) {
            uint32_t w[2 * S];
#pragma unroll
            for (int k = 0; k < 2 * S; ++k) w[k] = __float_as_uint(o[k]);
            store_words(dst, w);
        } else {
#pragma unroll
            for (int k = 0; k < 2 * S; ++k)
                if (k < 2 * nv) dst[k] = o[k];
        }
    }
}

// ---- demapper --------------------------------------------------------------------------------------------------------------------
// OUT: 0 f32 LLRs, 1 f16 LLRs, 2 hard-bit bytes (METHOD 2 only)
template <int QM, int METHOD, int OUT> __global__ __launch_bounds__(MODEM_BLOCK) void nrldpc_demodulate_kernel(const DemodArgs a, const int out_words) {
    constexpr int S = SymbolsPerThread<QM>::value, NV = S * QM;
    const int64_t nthr = (a.n_sym + S - 1) / S;
    for (int64_t t = (int64_t)blockIdx.x * MODEM_BLOCK + threadIdx.x; t < nthr; t += (int64_t)gridDim.x * MODEM_BLOCK) {
        const int64_t s0 = t * S;
        const int nv = (int)(a.n_sym - s0 < S ? a.n_sym - s0 : S);
        const bool full = nv == S;
        const float* src = a.rx + 2 * s0;
        float y[2 * S], n0[S];
        if (full) {
            uint32_t w[2 * S];
            load_words(src, w);
#pragma unroll
            for (int k = 0; k < 2 * S; ++k) y[k] = __uint_as_float(w[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 2 * S; ++k) y[k] = k < 2 * nv ? src[k] : 0.0f;
        }
#pragma unroll
        for (int s = 0; s < S; ++s) n0[s] = a.variance;
        if (METHOD != NRLDPC_DEMOD_HARD && a.var) { // (the hard decision does not depend on the variance)
            if (full) {
                uint32_t w[S];
                load_words(a.var + s0, w);
#pragma unroll
                for (int s = 0; s < S; ++s) n0[s] = __uint_as_float(w[s]);
            } else {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (s < nv) n0[s] = a.var[s0 + s];
            }
        }
        float o[NV];
#pragma unroll
        for (int s = 0; s < S; ++s) // 1 / N0 here for the scalar and for the array alike: the two give the same bits
            demap_symbol<QM, METHOD>(y[2 * s], y[2 * s + 1], 1.0f / n0[s], a.inv_norm, o + s * QM);
        if constexpr (OUT == 0) {
            float* dst = static_cast<float*>(a.out) + s0 * QM;
            if (full) {
                uint32_t w[NV];
#pragma unroll
                for (int k = 0; k < NV; ++k) w[k] = __float_as_uint(o[k]);
                store_words(dst, w);
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (k < nv * QM) dst[k] = o[k];
            }
        } else if constexpr (OUT == 1) {
            uint16_t* dst = static_cast<uint16_t*>(a.out) + s0 * QM;
            if (full && out_words) {
                uint32_t w[NV / 2];
#pragma unroll
                for (int k = 0; k < NV / 2; ++k) w[k] = f16_bits(o[2 * k]) | (f16_bits(o[2 * k + 1]) << 16);
                store_words(dst, w);
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (k < nv * QM) dst[k] = (uint16_t)f16_bits(o[k]);
            }
        } else {
            uint8_t* dst = static_cast<uint8_t*>(a.out) + s0 * QM;
            if (full && out_words) {
                uint32_t w[NV / 4];
#pragma unroll
                for (int k = 0; k < NV / 4; ++k)
                    w[k] = (o[4 * k] < 0.0f ? 1u : 0u) | (o[4 * k + 1] < 0.0f ? 0x100u : 0u) | (o[4 * k + 2] < 0.0f ? 0x10000u : 0u) |
                           (o[4 * k + 3] < 0.0f ? 0x1000000u : 0u);
                store_words(dst, w);
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k)
                    if (k < nv * QM) dst[k] = o[k] < 0.0f ? (uint8_t)1 : (uint8_t)0;
            }
        }
    }
}

static dim3 modem_grid(int64_t n_sym, int S) {
    const int64_t blocks = ((n_sym + S - 1) / S + MODEM_BLOCK - 1) / MODEM_BLOCK;
    return dim3((unsigned)(blocks < MODEM_MAX_GRID ? blocks : MODEM_MAX_GRID));
}
static int dword_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

hipError_t launch_modulate(const ModArgs& a, hipStream_t stream) {
    const dim3 block(MODEM_BLOCK);
    const int gw = dword_aligned(a.g);
    switch (a.Qm) {
#define NRLDPC_MOD_CASE(QM) \
    case QM: hipLaunchKernelGGL(nrldpc_modulate_kernel<QM>, modem_grid(a.n_sym, SymbolsPerThread<QM>::value), block, 0, stream, a, gw); break;
        NRLDPC_MOD_CASE(1) NRLDPC_MOD_CASE(2) NRLDPC_MOD_CASE(4) NRLDPC_MOD_CASE(6) NRLDPC_MOD_CASE(8)
#undef NRLDPC_MOD_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int QM> static hipError_t launch_demodulate_qm(const DemodArgs& a, hipStream_t stream) {
    const dim3 grid = modem_grid(a.n_sym, SymbolsPerThread<QM>::value), block(MODEM_BLOCK);
    const int ow = dword_aligned(a.out);
    if (a.method == NRLDPC_DEMOD_HARD) {
        hipLaunchKernelGGL((nrldpc_demodulate_kernel<QM, NRLDPC_DEMOD_HARD, 2>), grid, block, 0, stream, a, ow);
    } else if (a.method == NRLDPC_DEMOD_LLR) {
        if (a.out_dtype == NRLDPC_LLR_F16) hipLaunchKernelGGL((nrldpc_demodulate_kernel<QM, NRLDPC_DEMOD_LLR, 1>), grid, block, 0, stream, a, ow);
        else hipLaunchKernelGGL((nrldpc_demodulate_kernel<QM, NRLDPC_DEMOD_LLR, 0>), grid, block, 0, stream, a, ow);
    } else if (a.method == NRLDPC_DEMOD_APPROX_LLR) {
        if (a.out_dtype == NRLDPC_LLR_F16) hipLaunchKernelGGL((nrldpc_demodulate_kernel<QM, NRLDPC_DEMOD_APPROX_LLR, 1>), grid, block, 0, stream, a, ow);
        else hipLaunchKernelGGL((nrldpc_demodulate_kernel<QM, NRLDPC_DEMOD_APPROX_LLR, 0>), grid, block, 0, stream, a, ow);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_demodulate(const DemodArgs& a, hipStream_t stream) {
    switch (a.Qm) {
        case 1: return launch_demodulate_qm<1>(a, stream);
        case 2: return launch_demodulate_qm<2>(a, stream);
        case 4: return launch_demodulate_qm<4>(a, stream);
        case 6: return launch_demodulate_qm<6>(a, stream);
        case 8: return launch_demodulate_qm<8>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

} // namespace nrldpc

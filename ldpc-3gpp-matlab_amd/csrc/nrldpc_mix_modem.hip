// nrldpc_mix_modem.hip -- the symbol mapper, the stand-alone AWGN stage and the soft demapper for a MIX of transport-block
// configurations in one launch each: nrldpc_mix_chan_modulate_dev, nrldpc_mix_chan_awgn_dev, nrldpc_mix_chan_demodulate_dev
// (semantics: include/nrldpc.h).  The fused form of the three has a unit of its own (nrldpc_mix_chan.hip),
// because it is compiled with floating-point contraction allowed and these are not.
//
// Table driven, like the other mixed stages: the per-configuration records (offsets, symbol count, Q_m, 1/norm) and one prefix table
// per grid live in device memory, uploaded once by nrldpc_mix_chan_create and never written again; a workgroup finds its
// configuration by a binary search of the prefix table (nrldpc_mix.h: mix_find), so everything that selects a code path --
// configuration, Q_m -- is workgroup-uniform.  The operating points are read from the caller's device array of records.
//
// The bodies are those of nrldpc_modulate_kernel / nrldpc_demodulate_kernel (nrldpc_modem.hip) and nrldpc_awgn_kernel
// (nrldpc_awgn.hip) for one thread: the same symbols per thread, the same full / ragged split, the same wide accesses through
// pointers that promise dword alignment only, the same per-launch alignment test for byte and half arrays (a segment starts at a
// multiple of 16 elements, so its alignment class is its base pointer's), and the per-symbol arithmetic is the one shared copy
// (nrldpc_modem_sym.h, nrldpc_awgn_sym.h).  With contraction off every operation is a single IEEE operation or one deterministic
// hardware instruction, so each segment holds bit for bit what the single call leaves.  One writer per element, no LDS, no atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

// No floating-point contraction in this unit (the shared per-symbol code included): nrldpc_modem.hip and nrldpc_awgn.hip say why.
#pragma clang fp contract(off)

#include "nrldpc.h"
#include "nrldpc_modem.h"
#include "nrldpc_noise.h"
#include "nrldpc_modem_sym.h"
#include "nrldpc_awgn_sym.h"
#include "nrldpc_mix_chan.h"

namespace nrldpc {

static_assert(sizeof(MixChanRec) == 32, "records are laid out as an array with int64 members");
static_assert(mix_chan_spt(1) == SymbolsPerThread<1>::value && mix_chan_spt(2) == SymbolsPerThread<2>::value &&
              mix_chan_spt(4) == SymbolsPerThread<4>::value && mix_chan_spt(6) == SymbolsPerThread<6>::value &&
              mix_chan_spt(8) == SymbolsPerThread<8>::value, "the plan sizes the grid by the kernels' symbols per thread");

// ---- mapper ----------------------------------------------------------------------------------------------------------------------
template <int QM> __device__ __forceinline__ void mix_chan_modulate_thread(const MixChanModLaunch& a, const MixChanRec& c, int64_t t, int g_words) {
    constexpr int S = SymbolsPerThread<QM>::value, NBYTE = S * QM;
    const MixChanModemThread th = mix_chan_modem_thread(c.n_sym, S, t);
    const int nv = th.nv; // symbols of this thread that exist
    if (nv == 0) return;
    const uint8_t* g = a.g + mix_chan_g_index(c, th.s0);
    float* dst = a.tx + 2 * mix_chan_sym_index(c, th.s0);
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
    for (int s = 0; s < S; ++s) map_symbol<QM>(bits + s * QM, c.inv_norm, o[2 * s], o[2 * s + 1]);
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

// Q_m is workgroup-uniform: one switch to the QM-templated body.  nrldpc_mix_chan_create admits no other Q_m than these five.
__global__ __launch_bounds__(MIX_CHAN_BLOCK) void nrldpc_mix_chan_modulate_kernel(const MixChanModLaunch a, const int g_words) {
    const MixChanWork w = mix_chan_work(a.t.prefix, a.t.n, (int)blockIdx.x, (int)threadIdx.x);
    const MixChanRec c = a.t.recs[w.cfg]; // (a copy: the record is read once, before the switch)
    switch (c.Qm) {
        case 1: mix_chan_modulate_thread<1>(a, c, w.t, g_words); break;
        case 2: mix_chan_modulate_thread<2>(a, c, w.t, g_words); break;
        case 4: mix_chan_modulate_thread<4>(a, c, w.t, g_words); break;
        case 6: mix_chan_modulate_thread<6>(a, c, w.t, g_words); break;
        case 8: mix_chan_modulate_thread<8>(a, c, w.t, g_words); break;
        default: break;
    }
}

// ---- stand-alone noise -----------------------------------------------------------------------------------------------------------
template <bool VAR> __global__ __launch_bounds__(MIX_CHAN_BLOCK) void nrldpc_mix_chan_awgn_kernel(const MixChanAwgnLaunch a) {
    const MixChanWork wk = mix_chan_work(a.t.prefix, a.t.n, (int)blockIdx.x, (int)threadIdx.x);
    const MixChanRec c = a.t.recs[wk.cfg]; // (copies: each record is read once)
    const nrldpc_mix_chan_point pt = a.pt[wk.cfg];
    const uint64_t seed = pt.seed;
    const MixChanPairThread th = mix_chan_pair_thread(c.n_sym, pt.first_symbol, wk.t);
    const bool v0 = th.v0, v1 = th.v1;
    if (!v0 && !v1) return;
    float variance = 0.0f; // (not read when the array is given)
    if constexpr (!VAR) variance = pt.variance;
    uint32_t r[4];
    philox4x32_10((uint32_t)th.c, (uint32_t)(th.c >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    if (v0 && v1) {
        const int64_t s0 = mix_chan_sym_index(c, th.s0);
        uint32_t w[4];
        load_words(a.tx + 2 * s0, w);
        float n0[2] = {variance, variance};
        if constexpr (VAR) {
            uint32_t v[2];
            load_words(a.var + s0, v);
            n0[0] = __uint_as_float(v[0]); n0[1] = __uint_as_float(v[1]);
        }
        float y[4] = {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3])};
        add_noise(r[0], r[1], n0[0], y[0], y[1]);
        add_noise(r[2], r[3], n0[1], y[2], y[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = __float_as_uint(y[k]);
        store_words(a.rx + 2 * s0, w);
    } else { // one symbol: the odd one of the pair at the front (v1 alone), the even one at the back (v0 alone)
        const int64_t s = mix_chan_sym_index(c, v0 ? th.s0 : th.s0 + 1);
        uint32_t w[2];
        load_words(a.tx + 2 * s, w);
        float n0 = variance;
        if constexpr (VAR) n0 = a.var[s];
        float y[2] = {__uint_as_float(w[0]), __uint_as_float(w[1])};
        add_noise(v0 ? r[0] : r[2], v0 ? r[1] : r[3], n0, y[0], y[1]);
        w[0] = __float_as_uint(y[0]); w[1] = __float_as_uint(y[1]);
        store_words(a.rx + 2 * s, w);
    }
}

// ---- demapper --------------------------------------------------------------------------------------------------------------------
// OUT: 0 f32 LLRs, 1 f16 LLRs, 2 hard-bit bytes (METHOD 2 only)
template <int QM, int METHOD, int OUT>
__device__ __forceinline__ void mix_chan_demodulate_thread(const MixChanDemodLaunch& a, const MixChanRec& c, float variance, int64_t t, int out_words) {
    constexpr int S = SymbolsPerThread<QM>::value, NV = S * QM;
    const MixChanModemThread th = mix_chan_modem_thread(c.n_sym, S, t);
    const int nv = th.nv;
    if (nv == 0) return;
    const bool full = nv == S;
    const int64_t s0 = mix_chan_sym_index(c, th.s0); // in the symbol and variance arrays
    const int64_t e0 = mix_chan_g_index(c, th.s0);   // in the output array
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
    for (int s = 0; s < S; ++s) n0[s] = variance;
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
        demap_symbol<QM, METHOD>(y[2 * s], y[2 * s + 1], 1.0f / n0[s], c.inv_norm, o + s * QM);
    if constexpr (OUT == 0) {
        float* dst = static_cast<float*>(a.out) + e0;
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
        uint16_t* dst = static_cast<uint16_t*>(a.out) + e0;
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
        uint8_t* dst = static_cast<uint8_t*>(a.out) + e0;
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

template <int METHOD, int OUT> __global__ __launch_bounds__(MIX_CHAN_BLOCK) void nrldpc_mix_chan_demodulate_kernel(const MixChanDemodLaunch a, const int out_words) {
    const MixChanWork w = mix_chan_work(a.t.prefix, a.t.n, (int)blockIdx.x, (int)threadIdx.x);
    const MixChanRec c = a.t.recs[w.cfg]; // (a copy: the record is read once, before the switch)
    // the single call's scalar: the record's variance, 1 when the array replaces it; the operating points are not read for the hard
    // decision or with the array
    float variance = 1.0f;
    if (METHOD != NRLDPC_DEMOD_HARD && !a.var) variance = a.pt[w.cfg].variance;
    switch (c.Qm) {
        case 1: mix_chan_demodulate_thread<1, METHOD, OUT>(a, c, variance, w.t, out_words); break;
        case 2: mix_chan_demodulate_thread<2, METHOD, OUT>(a, c, variance, w.t, out_words); break;
        case 4: mix_chan_demodulate_thread<4, METHOD, OUT>(a, c, variance, w.t, out_words); break;
        case 6: mix_chan_demodulate_thread<6, METHOD, OUT>(a, c, variance, w.t, out_words); break;
        case 8: mix_chan_demodulate_thread<8, METHOD, OUT>(a, c, variance, w.t, out_words); break;
        default: break;
    }
}

static int mix_chan_dword_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

hipError_t launch_mix_chan_modulate(const MixChanModLaunch& a, hipStream_t stream) {
    if (a.t.n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_chan_modulate_kernel, dim3(a.t.n_wg), dim3(MIX_CHAN_BLOCK), 0, stream, a, mix_chan_dword_aligned(a.g));
    return hipGetLastError();
}

hipError_t launch_mix_chan_awgn(const MixChanAwgnLaunch& a, hipStream_t stream) {
    if (a.t.n_wg <= 0) return hipSuccess;
    const dim3 grid(a.t.n_wg), block(MIX_CHAN_BLOCK);
    if (a.var) hipLaunchKernelGGL(nrldpc_mix_chan_awgn_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(nrldpc_mix_chan_awgn_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mix_chan_demodulate(const MixChanDemodLaunch& a, hipStream_t stream) {
    if (a.t.n_wg <= 0) return hipSuccess;
    const dim3 grid(a.t.n_wg), block(MIX_CHAN_BLOCK);
    const int ow = mix_chan_dword_aligned(a.out);
    if (a.method == NRLDPC_DEMOD_HARD) {
        hipLaunchKernelGGL((nrldpc_mix_chan_demodulate_kernel<NRLDPC_DEMOD_HARD, 2>), grid, block, 0, stream, a, ow);
    } else if (a.method == NRLDPC_DEMOD_LLR) {
        if (a.out_dtype == NRLDPC_LLR_F16) hipLaunchKernelGGL((nrldpc_mix_chan_demodulate_kernel<NRLDPC_DEMOD_LLR, 1>), grid, block, 0, stream, a, ow);
        else hipLaunchKernelGGL((nrldpc_mix_chan_demodulate_kernel<NRLDPC_DEMOD_LLR, 0>), grid, block, 0, stream, a, ow);
    } else if (a.method == NRLDPC_DEMOD_APPROX_LLR) {
        if (a.out_dtype == NRLDPC_LLR_F16) hipLaunchKernelGGL((nrldpc_mix_chan_demodulate_kernel<NRLDPC_DEMOD_APPROX_LLR, 1>), grid, block, 0, stream, a, ow);
        else hipLaunchKernelGGL((nrldpc_mix_chan_demodulate_kernel<NRLDPC_DEMOD_APPROX_LLR, 0>), grid, block, 0, stream, a, ow);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace nrldpc

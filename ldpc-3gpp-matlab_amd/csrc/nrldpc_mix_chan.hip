// nrldpc_mix_chan.hip -- the fused channel leg (modulation + AWGN + exact LLRs) for a MIX of transport-block configurations in one
// launch: nrldpc_mix_chan_awgn_llr_dev (semantics: include/nrldpc.h).  The symbols never exist in memory,
// as in nrldpc_channel.hip.
//
// Table driven, like the other mixed stages: the per-configuration records (offsets, symbol count, Q_m, 1/norm) and a prefix table over
// the workgroups live in device memory, uploaded once by nrldpc_mix_chan_create and never written again; a workgroup finds its
// configuration by a binary search of the prefix table (nrldpc_mix.h: mix_find), so everything that selects a code path is
// workgroup-uniform.  The operating point (sigma, 1/N0, seed, first_symbol) is read from the caller's device array of records.
//
// The body is nrldpc_awgn_llr_kernel's (nrldpc_channel.hip): a thread owns the aligned pair (2c, 2c+1) of the configuration's GLOBAL
// symbol count, one Philox block feeds both, the per-symbol arithmetic is the shared symbol_llr (nrldpc_channel_sym.h), the QPSK
// dword load and 16-byte store are taken under the same address tests.  The plan sizes a configuration for n_sym / 2 + 1 pairs, which
// serves either parity of first_symbol; a thread without a symbol in range leaves.
//
// No `#pragma clang fp contract(off)` here, as nrldpc_channel.hip has none: the single kernel is compiled with contraction allowed,
// and this one equals it bit for bit only if the compiler fuses the same multiply-adds in symbol_llr here
// (profiles/r10_mix_chan_isa.txt compares the two; tests/test_mix_chan_gpu.py holds them to equality on the device).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_channel_sym.h"
#include "nrldpc_mix_chan.h"

namespace nrldpc {

static_assert(sizeof(MixChanRec) == 32, "records are laid out as an array with int64 members");

template <int QM>
__device__ __forceinline__ void mix_chan_awgn_llr_thread(const MixChanLlrLaunch& l, const MixChanRec& c, const ChanArgs& a, int64_t t) {
    const MixChanPairThread th = mix_chan_pair_thread(c.n_sym, a.first_symbol, t);
    const bool v0 = th.v0, v1 = th.v1;
    if (!v0 && !v1) return;
    const int64_t s0 = th.s0;
    uint32_t r[4];
    philox4x32_10((uint32_t)th.c, (uint32_t)(th.c >> 32), 0u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
    float o[2 * QM];
    uint8_t bits[2 * QM];
    const uint8_t* g = l.g + mix_chan_g_index(c, s0);
    float* dst = l.llr + mix_chan_g_index(c, s0);
    const bool both = v0 && v1;
    if (QM == 2 && both && (reinterpret_cast<uintptr_t>(g) & 3) == 0) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(g);
#pragma unroll
        for (int k = 0; k < 4; ++k) bits[k < 2 * QM ? k : 0] = (uint8_t)(w >> (8 * k));
    } else {
#pragma unroll
        for (int k = 0; k < 2 * QM; ++k) bits[k] = ((k < QM ? v0 : v1) ? g[k] : (uint8_t)0);
    }
    symbol_llr<QM>(a, bits, r[0], r[1], o);
    symbol_llr<QM>(a, bits + QM, r[2], r[3], o + QM);
    if (QM == 2 && both && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[QM < 2 ? 0 : 2], o[QM < 2 ? 0 : 3]);
    } else {
#pragma unroll
        for (int k = 0; k < QM; ++k) {
            if (v0) dst[k] = o[k];
            if (v1) dst[QM + k] = o[QM + k];
        }
    }
}

// Q_m is workgroup-uniform: one switch to the QM-templated body.  nrldpc_mix_chan_create admits no other Q_m than these five.
__global__ __launch_bounds__(MIX_CHAN_BLOCK) void nrldpc_mix_chan_awgn_llr_kernel(const MixChanLlrLaunch l) {
    const MixChanWork w = mix_chan_work(l.t.prefix, l.t.n, (int)blockIdx.x, (int)threadIdx.x);
    const MixChanRec c = l.t.recs[w.cfg]; // (copies: each record is read once, before the switch)
    const nrldpc_mix_chan_point p = l.pt[w.cfg];
    ChanArgs a; // what the single kernel gets as its argument block (g, llr and n_sym are taken from the record)
    a.g = nullptr; a.llr = nullptr; a.n_sym = c.n_sym;
    a.seed = p.seed; a.first_symbol = p.first_symbol; a.Qm = c.Qm;
    a.sigma = p.sigma; a.inv_n0 = p.inv_n0; a.inv_norm = c.inv_norm;
    switch (c.Qm) {
        case 1: mix_chan_awgn_llr_thread<1>(l, c, a, w.t); break;
        case 2: mix_chan_awgn_llr_thread<2>(l, c, a, w.t); break;
        case 4: mix_chan_awgn_llr_thread<4>(l, c, a, w.t); break;
        case 6: mix_chan_awgn_llr_thread<6>(l, c, a, w.t); break;
        case 8: mix_chan_awgn_llr_thread<8>(l, c, a, w.t); break;
        default: break;
    }
}

hipError_t launch_mix_chan_awgn_llr(const MixChanLlrLaunch& a, hipStream_t stream) {
    if (a.t.n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_chan_awgn_llr_kernel, dim3(a.t.n_wg), dim3(MIX_CHAN_BLOCK), 0, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

// nrldpc_channel.hip -- modulation + AWGN + exact-LLR demodulation fused into one kernel.
//
// Replaces, in the Monte-Carlo loop of plot_BLER_vs_SNR.m:130-132,
//     tx = step(hMod, g);  rx = step(hChan, tx);  g_tilde = step(hDemod, rx);
// i.e. NRModulator.m:73-81 (TS 38.211 Gray maps through the reference's custom symbol tables, unit average power),
// comm.AWGNChannel at Es/N0 (plot_BLER_vs_SNR.m:50,105) and NRDemodulator.m:76-84 ('Log-likelihood ratio' = exact
// LLRs with Variance = N0 = 10^(-EsN0/10), :106).  The symbols never exist in memory: a thread owns one symbol, reads its
// Q_m bits (1 byte each, the boundary format of the rate-matching stage), draws its noise from a counter-based
// generator (Philox-4x32-10, counter = global symbol index, key = seed: reproducible for any launch geometry, and
// restated in numpy by the test oracle), and writes Q_m LLRs (f32, positive = bit 0).  HBM-bound: 1 byte in,
// 4 bytes out per bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_kernels.h"
#include "nrldpc_modem.h"
#include "nrldpc_noise.h"
#include "nrldpc_channel_sym.h"
#include "nrldpc_payload_bits.h"

namespace nrldpc {

// philox4x32_10 / box_muller, the noise draw: nrldpc_noise.h (shared with the stand-alone AWGN stage, nrldpc_awgn.hip)
// pam_level<NB> / rail_llr<NB>, the rail arithmetic: nrldpc_modem.h (shared with the stand-alone demapper)

// symbol_llr<QM>, the LLRs of one symbol from its bits and its noise words: nrldpc_channel_sym.h (shared with nrldpc_mix_chan.hip)

// A thread owns the pair of symbols (2c, 2c+1) of the global symbol count: one Philox call -- counter c, four words -- feeds
// both (words 0,1 the even symbol, words 2,3 the odd one); a generator call per symbol threw half of its output away and was
// what the kernel spent most of its instructions on.  Pairs are aligned to the global count, so the noise of a symbol does not
// depend on how the symbols are split over launches.
template <int QM> __global__ __launch_bounds__(256) void nrldpc_awgn_llr_kernel(const ChanArgs a) {
    const uint64_t c = (a.first_symbol >> 1) + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; // pair index = Philox counter
    const int64_t s0 = (int64_t)(2 * c - a.first_symbol);                                        // local index of the even symbol
    if (s0 >= a.n_sym) return;
    uint32_t r[4];
    philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
    const bool v0 = s0 >= 0, v1 = s0 + 1 < a.n_sym;
    float o[2 * QM];
    uint8_t bits[2 * QM];
    const uint8_t* g = a.g + s0 * QM;
    float* dst = a.llr + s0 * QM;
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

// ---- payload bits of the Monte-Carlo loop (plot_BLER_vs_SNR.m:118: a = round(rand(A,1)) per block) ---------------------------------
// Bit i of transport block b = bit (i mod 64) of splitmix64(seed + (b*W + i div 64 + 1) * golden), W = ceil(A/64): a function of the
// GLOBAL block index alone (harness.payload_bits_np is the definition), so any split of a batch over devices draws the same payloads.
// One kernel instead of the fifteen small tensor operations the harness made of it (round 6: a fifth of a demo-sized step).
// A thread writes four consecutive bits of a block as four bytes: splitmix64, payload_nibble and payload_store_chunk of
// nrldpc_payload_bits.h (shared with the mixed-batch draw, nrldpc_mix_mc.hip).
__global__ __launch_bounds__(256) void nrldpc_payload_bits_kernel(uint64_t seed, uint64_t first_block, int32_t n_tb, int32_t A, uint8_t* out) {
    const int q4 = payload_chunks(A);
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_tb * q4) return;
    const int b = (int)(t / q4), c = (int)(t - (int64_t)b * q4);
    const int i0 = 4 * c, W = payload_words(A);
    const uint32_t nib = payload_nibble(seed, first_block + (uint64_t)b, W, i0);
    payload_store_chunk(out + (size_t)b * A + i0, nib, i0, A);
}
hipError_t launch_payload_bits(uint64_t seed, uint64_t first_block, int32_t n_tb, int32_t A, uint8_t* out, hipStream_t stream) {
    const int64_t n = (int64_t)n_tb * ((A + 3) >> 2);
    hipLaunchKernelGGL(nrldpc_payload_bits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, seed, first_block, n_tb, A, out);
    return hipGetLastError();
}

hipError_t launch_awgn_llr(const ChanArgs& a, hipStream_t stream) {
    // pairs of the global symbol count that the launch touches
    const uint64_t npairs = ((a.first_symbol + (uint64_t)a.n_sym - 1) >> 1) - (a.first_symbol >> 1) + 1;
    const dim3 grid((unsigned)((npairs + 255) / 256)), block(256);
    switch (a.Qm) {
        case 1: hipLaunchKernelGGL(nrldpc_awgn_llr_kernel<1>, grid, block, 0, stream, a); break;
        case 2: hipLaunchKernelGGL(nrldpc_awgn_llr_kernel<2>, grid, block, 0, stream, a); break;
        case 4: hipLaunchKernelGGL(nrldpc_awgn_llr_kernel<4>, grid, block, 0, stream, a); break;
        case 6: hipLaunchKernelGGL(nrldpc_awgn_llr_kernel<6>, grid, block, 0, stream, a); break;
        case 8: hipLaunchKernelGGL(nrldpc_awgn_llr_kernel<8>, grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace nrldpc

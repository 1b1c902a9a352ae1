// nrldpc_awgn.hip -- the stand-alone AWGN stage: comm.AWGNChannel of plot_BLER_vs_SNR.m:50,105,131 as a kernel of its own,
// rx[s] = tx[s] + w[s], between the stand-alone mapper and demapper (nrldpc_modem.hip) or after a caller's own channel stages (a
// fading gain, interference, then thermal noise with a per-symbol variance).  w is the fused kernel's noise (nrldpc_channel.hip) for
// the same (seed, first_symbol), drawn by the same code (nrldpc_noise.h): the Monte-Carlo loop keeps the fused kernel, where the
// noisy symbols never exist in memory, and this stage gives the same draw to whoever needs them.
//
// A thread owns the aligned pair (2c, 2c+1) of the GLOBAL symbol count -- one Philox block, as in the fused kernel -- so a symbol's
// noise does not depend on how the symbols are split over launches.  A thread with both symbols in range makes one 16-byte load and one
// 16-byte store through pointers that only promise dword alignment (what a float array gives; global_load/store_dwordx4 need no more
// on gfx950: nrldpc_modem.hip); the first thread of an odd first_symbol and the last one of a count that ends on an even symbol hold
// one symbol and take 8-byte accesses.  A thread reads its symbols before it writes them and no other thread touches them, so
// rx == tx (in place) is served.  No LDS, no atomics, no scratch; one thread per pair at every size a link produces, the grid-stride
// loop only serves counts beyond 2^20 workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

// No floating-point contraction in this unit (the shared noise draw included): each noise component is rounded to f32 and then added
// to the symbol with one f32 add.  A contracted rad * cos + tx would make the sum depend on what the compiler fuses, and the stage's
// identities -- awgn(tx) == tx + awgn(0), a call over a buffer == calls over its parts -- hold bit for bit only without it.
#pragma clang fp contract(off)

#include "nrldpc_modem.h"
#include "nrldpc_noise.h"
#include "nrldpc_awgn_sym.h"

namespace nrldpc {

constexpr int AWGN_BLOCK = 256, AWGN_MAX_GRID = 1 << 20;

// add_noise, (re, im) + the noise of one symbol: nrldpc_awgn_sym.h (shared with nrldpc_mix_modem.hip)

template <bool VAR> __global__ __launch_bounds__(AWGN_BLOCK) void nrldpc_awgn_kernel(const AwgnArgs a, const uint64_t npairs) {
    for (uint64_t p = (uint64_t)blockIdx.x * AWGN_BLOCK + threadIdx.x; p < npairs; p += (uint64_t)gridDim.x * AWGN_BLOCK) {
        const uint64_t c = (a.first_symbol >> 1) + p;          // pair index = Philox counter
        const int64_t s0 = (int64_t)(2 * c - a.first_symbol); // local index of the even symbol: -1 for the first pair of an odd first_symbol
        const bool v0 = s0 >= 0, v1 = s0 + 1 < a.n_sym;       // (s0 < n_sym by the choice of npairs: at least one of the two holds)
        uint32_t r[4];
        philox4x32_10((uint32_t)c, (uint32_t)(c >> 32), 0u, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
        if (v0 && v1) {
            uint32_t w[4];
            load_words(a.tx + 2 * s0, w);
            float n0[2] = {a.variance, a.variance};
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
            const int64_t s = v0 ? s0 : s0 + 1;
            uint32_t w[2];
            load_words(a.tx + 2 * s, w);
            float n0 = a.variance;
            if constexpr (VAR) n0 = a.var[s];
            float y[2] = {__uint_as_float(w[0]), __uint_as_float(w[1])};
            add_noise(v0 ? r[0] : r[2], v0 ? r[1] : r[3], n0, y[0], y[1]);
            w[0] = __float_as_uint(y[0]); w[1] = __float_as_uint(y[1]);
            store_words(a.rx + 2 * s, w);
        }
    }
}

hipError_t launch_awgn(const AwgnArgs& a, hipStream_t stream) {
    // pairs of the global symbol count that the launch touches (n_sym >= 1, first_symbol + n_sym does not wrap: the caller's checks)
    const uint64_t npairs = ((a.first_symbol + (uint64_t)a.n_sym - 1) >> 1) - (a.first_symbol >> 1) + 1;
    const uint64_t blocks = (npairs + AWGN_BLOCK - 1) / AWGN_BLOCK;
    const dim3 grid((unsigned)(blocks < (uint64_t)AWGN_MAX_GRID ? blocks : (uint64_t)AWGN_MAX_GRID)), block(AWGN_BLOCK);
    if (a.var) hipLaunchKernelGGL(nrldpc_awgn_kernel<true>, grid, block, 0, stream, a, npairs);
    else hipLaunchKernelGGL(nrldpc_awgn_kernel<false>, grid, block, 0, stream, a, npairs);
    return hipGetLastError();
}

} // namespace nrldpc

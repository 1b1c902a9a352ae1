// nrldpc_ratematch_ex.hip -- rate recovery with f32 or f16 demodulator LLRs, an f32 or f16 HARQ soft buffer and f32 or f16
// codeword LLRs (nrldpc_rate_recover_ex_dev; semantics: include/nrldpc.h).
//
// The three forms of nrldpc_ratematch.hip -- the general gather with the repetition walk, the branch-free gather per Q_m, the
// input-driven scatter -- from the one copy of the geometry, the gather bodies, the element rules and the launch rule in
// nrldpc_rm_core.h: the same f32 sums in the same order.  What differs is the mapping.  There a lane
// owns a pair of neighbouring positions, 8 bytes of f32 but 4 of f16; here it owns FOUR (gathers, fill waves) or four interleaver
// columns (scatter), so that a lane's access to an f16 buffer, f16 output or f16 input run is 8 bytes and to an f32 one 16.  An
// f16 array may start at any even address (rows of g_tilde when G is odd, rows of the buffer when N_cb is odd, sub-ranges of
// larger allocations): every wide access is taken by a test on the address it would use -- a multi-dword global access needs
// dword alignment -- and is element by element otherwise, as it is at run boundaries (end of the buffer, filler gap, last columns).
// Every buffer position is read and written by exactly one thread.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

#include "nrldpc_ratematch_ex.h"
#include "nrldpc_rm_core.h"

namespace nrldpc {
using namespace rm_dev;

constexpr int RRX_SWEEPS = 2;                  // sweeps of 256 consecutive positions per wave
constexpr int RRX_TILE = 64 * 4 * RRX_SWEEPS;  // positions per wave

// ---- the general gather: repetitions summed in ascending k (NRLDPCDecoder.m:229-231), then the buffer --------------------------------
template <typename InT, typename HbT, typename OutT>
__global__ __launch_bounds__(256) void nrldpc_rate_recover_ex_kernel(const RmExArgs a) {
    const int blk = blockIdx.y; // tb * C + r
    const int tb = blk / a.C, r = blk - tb * a.C;
    const int ncwz = 2 * a.Z + a.N;
    const int lane = threadIdx.x & 63;
    const int tile0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RRX_TILE;
    if (tile0 >= ncwz) return;
    const RmGeom geo(a.Z, a.K, a.Kp, a.N_cb, a.k0);
    const int E = a.E[r];
    const int rows = E > 0 ? E / a.Qm : 1;
    const int Pq = geo.P / rows, Pr = geo.P - Pq * rows;
    const InT* f = static_cast<const InT*>(a.g) + (size_t)tb * a.G + a.off[r];
    HbT* hb = a.harq ? static_cast<HbT*>(a.harq) + (size_t)blk * a.N_cb : nullptr;
    OutT* out = static_cast<OutT*>(a.out) + (size_t)blk * ncwz;
#pragma unroll
    for (int s = 0; s < RRX_SWEEPS; ++s) {
        const int pos0 = tile0 + s * 256 + 4 * lane;
        if (pos0 >= ncwz) break;
        float val[4];
        bool fill[4], inb[4];
        gather_general(geo, f, pos0 - 2 * a.Z, a.N_cb, E, rows, a.Qm, Pq, Pr, val, fill, inb);
        finish4<false>(hb, out, pos0, pos0 - 2 * a.Z, ncwz, val, fill, inb, {false, false, false, false}, false);
    }
}

// ---- the branch-free gather for the usual case, no repetition: a position takes exactly one e(k) or none -------------------------
// Its own copy of the geometry and of the gather body (as in nrldpc_mix.hip): through RmGeom and a shared body these kernels measured
// 0.15-0.25 % slower at 64QAM with a buffer, outside the parent's own spread (profiles/r08_stage_refactor_isa.txt).
template <typename InT, typename HbT, typename OutT, int QM>
__global__ __launch_bounds__(256) void nrldpc_rate_recover_ex_fast_kernel(const RmExArgs a) {
    const int blk = blockIdx.y;
    const int tb = blk / a.C, r = blk - tb * a.C;
    const int ncwz = 2 * a.Z + a.N;
    const int lane = threadIdx.x & 63;
    const int tile0 = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RRX_TILE;
    if (tile0 >= ncwz) return;
    const int lo_f = a.Kp - 2 * a.Z > 0 ? a.Kp - 2 * a.Z : 0, hi_f = a.K - 2 * a.Z;
    const int f_hi = hi_f < a.N_cb ? hi_f : a.N_cb;
    const int F = f_hi > lo_f ? f_hi - lo_f : 0;
    const int P = a.N_cb - F;
    int nfk0 = a.k0 - lo_f;
    nfk0 = a.k0 - (nfk0 < 0 ? 0 : (nfk0 > F ? F : nfk0));
    const int E = a.E[r];
    const int rows = E > 0 ? E / QM : 1;
    const InT* f = static_cast<const InT*>(a.g) + (size_t)tb * a.G + a.off[r];
    HbT* hb = a.harq ? static_cast<HbT*>(a.harq) + (size_t)blk * a.N_cb : nullptr;
    OutT* out = static_cast<OutT*>(a.out) + (size_t)blk * ncwz;
#pragma unroll
    for (int s = 0; s < RRX_SWEEPS; ++s) {
        const int pos0 = tile0 + s * 256 + 4 * lane;
        if (pos0 >= ncwz) break;
        float val[4];
        bool fill[4], inb[4], live[4];
        int idx[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = pos0 + t - 2 * a.Z;
            fill[t] = p >= lo_f && p < hi_f;
            inb[t] = p >= 0 && p < a.N_cb && !fill[t];
            int c = p - lo_f;
            c = c < 0 ? 0 : (c > F ? F : c);
            int q = p - c - nfk0;
            q += q < 0 ? P : 0;
            int i = 0;
#pragma unroll
            for (int m = 1; m < QM; ++m) i += (q >= m * rows);
            const int j = q - i * rows;
            live[t] = inb[t] && q < E;
            idx[t] = live[t] ? j * QM + i : 0;
        }
        // predicated: a position that receives nothing must not touch g_tilde at all -- for a trailing code block with
        // E_r == 0 (not retransmitted under CBGTI) f already points one past the transport block's LLRs
#pragma unroll
        for (int t = 0; t < 4; ++t) val[t] = live[t] ? (float)f[idx[t]] : 0.0f;
        finish4<false>(hb, out, pos0, pos0 - 2 * a.Z, ncwz, val, fill, inb, {false, false, false, false}, false);
    }
}

// ---- the input-driven form (no repetition): a lane owns four interleaver columns j of all Qm rows = 4*Qm consecutive elements of
// g_tilde, read as 16-byte words (f32) / 8- or 16-byte words (f16), and scatters them: row i's four values are four neighbouring
// positions of the circular buffer unless the run crosses its end or the filler gap.  Positions no e(k) lands on are written by a
// second set of waves of the same launch that only store (with the buffer: echo it), four neighbouring positions per lane.
constexpr int RRX_J = 4;
constexpr int RRX_FILL_TILE = 512; // positions per wave of the fill part

template <typename T, int N> struct Word { typedef T __attribute__((ext_vector_type(N), aligned(4))) type; };

template <typename InT, typename HbT, typename OutT, int QM>
__global__ __launch_bounds__(256) void nrldpc_rate_recover_ex_scatter_kernel(const RmExArgs a, const int in_blocks) {
    constexpr int J = RRX_J, NV = J * QM; // elements per lane
    const int blk = blockIdx.y;
    const int tb = blk / a.C, r = blk - tb * a.C;
    const int ncwz = 2 * a.Z + a.N;
    const RmGeom geo(a.Z, a.K, a.Kp, a.N_cb, a.k0);
    const int E = a.E[r];
    const int rows = E / QM;
    HbT* hb = a.harq ? static_cast<HbT*>(a.harq) + (size_t)blk * a.N_cb : nullptr;
    OutT* out = static_cast<OutT*>(a.out) + (size_t)blk * ncwz;
    if ((int)blockIdx.x < in_blocks) {
        // ---- input part: lane -> columns j0 .. j0+3
        const int j0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * J;
        if (j0 >= rows) return;
        const InT* f = static_cast<const InT*>(a.g) + (size_t)tb * a.G + a.off[r] + (size_t)j0 * QM;
        const int nj = rows - j0 < J ? rows - j0 : J;
        float v[NV];
        if (nj == J && quad_ok(f)) {
            constexpr int W = 16 / (int)sizeof(InT) <= NV ? 16 / (int)sizeof(InT) : NV; // elements per word: 16 bytes, or the 8 of Q_m = 1 in f16
            typedef typename Word<InT, W>::type word_t;
#pragma unroll
            for (int k = 0; k < NV / W; ++k) {
                const word_t w = reinterpret_cast<const word_t*>(f)[k];
#pragma unroll
                for (int e = 0; e < W; ++e) v[W * k + e] = (float)w[e];
            }
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = k < nj * QM ? (float)f[k] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < QM; ++i) {
            // non-filler index of e(i*rows + j0) counted from 0, then its position in d (fillers skipped), then in the core's input
            const int n = geo.n_of(i * rows + j0);
            const int p = geo.pos_at(n);
            if (nj == J && geo.whole_run(n, J)) {
                float val[4];
                const bool no[4] = {false, false, false, false}, yes[4] = {true, true, true, true};
#pragma unroll
                for (int t = 0; t < J; ++t) val[t] = v[t * QM + i];
                finish4<false>(hb, out, 2 * a.Z + p, p, ncwz, val, no, yes, no, false);
            } else {
                for (int t = 0; t < nj; ++t) {
                    int nn = n + t;
                    nn -= nn >= geo.P ? geo.P : 0;
                    const int pp = geo.pos_at(nn);
                    float val = v[t * QM + i];
                    if (hb) {
                        HbT h = hb[pp];
                        val = combine(val, h);
                        hb[pp] = h;
                    }
                    out[2 * a.Z + pp] = narrow<OutT>(val);
                }
            }
        }
        return;
    }
    // ---- fill part: positions no e(k) lands on; whole tiles of covered positions skipped by a wave-uniform test
    const int wave = ((int)blockIdx.x - in_blocks) * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tile0 = wave * RRX_FILL_TILE;
    if (tile0 >= ncwz) return;
    if (fill_tile_covered(geo, tile0, RRX_FILL_TILE, ncwz, a.Z, a.N_cb, E)) return;
#pragma unroll
    for (int s = 0; s < RRX_FILL_TILE / 256; ++s) {
        const int pos0 = tile0 + s * 256 + 4 * lane;
        if (pos0 >= ncwz) break;
        bool skip[4], echo[4];
        OutT o[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = pos0 + t - 2 * a.Z;
            const bool filler = geo.filler(p);
            const bool inbuf = p >= 0 && p < a.N_cb && !filler;
            skip[t] = (inbuf && geo.covered(p, E)) || pos0 + t >= ncwz;
            echo[t] = hb && inbuf && !skip[t];
            o[t] = filler ? filler_mark<OutT>() : narrow<OutT>(0.0f);
        }
        // :236-239 with nothing received: the buffer as it is
        if (echo[0] && echo[1] && echo[2] && echo[3]) {
            HbT h[4];
            load4(hb + (pos0 - 2 * a.Z), h);
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = narrow<OutT>((float)h[t]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (echo[t]) o[t] = narrow<OutT>((float)hb[pos0 + t - 2 * a.Z]);
        }
        if (!skip[0] && !skip[1] && !skip[2] && !skip[3]) {
            store4(out + pos0, o);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (!skip[t]) out[pos0 + t] = o[t];
        }
    }
}

template <typename InT, typename HbT, typename OutT> static void launch_typed(const RmExArgs& a, const RmRule& rule, hipStream_t stream) {
    const int ncwz = 2 * a.Z + a.N;
    const dim3 grid((ncwz + 4 * RRX_TILE - 1) / (4 * RRX_TILE), a.n_tb * a.C);
    if (rule.form == RM_GENERAL) {
        hipLaunchKernelGGL((nrldpc_rate_recover_ex_kernel<InT, HbT, OutT>), grid, dim3(256), 0, stream, a);
    } else if (rule.form == RM_SCATTER) {
        const int fill_blocks = (ncwz + 4 * RRX_FILL_TILE - 1) / (4 * RRX_FILL_TILE);
        rm_per_qm(a.Qm, [&](auto qc) {
            constexpr int QM = decltype(qc)::value;
            const int rows = rule.emax / QM;
            const int in_blocks = (rows + 256 * RRX_J - 1) / (256 * RRX_J);
            hipLaunchKernelGGL((nrldpc_rate_recover_ex_scatter_kernel<InT, HbT, OutT, QM>), dim3(in_blocks + fill_blocks, a.n_tb * a.C), dim3(256), 0, stream, a, in_blocks);
        });
    } else {
        rm_per_qm(a.Qm, [&](auto qc) {
            constexpr int QM = decltype(qc)::value;
            hipLaunchKernelGGL((nrldpc_rate_recover_ex_fast_kernel<InT, HbT, OutT, QM>), grid, dim3(256), 0, stream, a);
        });
    }
}

hipError_t launch_rate_recover_ex(const RmExArgs& a, hipStream_t stream) {
    const RmRule rule = rm_launch_rule(RmGeom(a.Z, a.K, a.Kp, a.N_cb, a.k0), a.E, a.C, a.Qm, a.N, a.harq != nullptr, rm_env_switches());
    rm_with_types(a.in_f16, a.harq && a.harq_f16, a.out_f16, [&](auto in, auto hb, auto out) {
        launch_typed<decltype(in), decltype(hb), decltype(out)>(a, rule, stream);
    });
    return hipGetLastError();
}

} // namespace nrldpc

// nrldpc_ratematch_ex.hip -- rate recovery with f32 or f16 demodulator LLRs, an f32 or f16 HARQ soft buffer and f32 or f16
// codeword LLRs (nrldpc_rate_recover_ex_dev; semantics: include/nrldpc.h).
//
// The three forms of nrldpc_ratematch.hip -- the general gather with the repetition walk, the branch-free gather per Q_m, the
// input-driven scatter -- with the same index arithmetic, the same f32 sums in the same order and the same launch rule, as a unit
// of its own: the f32-only kernels of nrldpc_rate_recover_dev stay the code they are.  What differs is the mapping.  There a lane
// owns a pair of neighbouring positions, 8 bytes of f32 but 4 of f16; here it owns FOUR (gathers, fill waves) or four interleaver
// columns (scatter), so that a lane's access to an f16 buffer, f16 output or f16 input run is 8 bytes and to an f32 one 16.  An
// f16 array may start at any even address (rows of g_tilde when G is odd, rows of the buffer when N_cb is odd, sub-ranges of
// larger allocations): every wide access is taken by a test on the address it would use -- a multi-dword global access needs
// dword alignment -- and is element by element otherwise, as it is at run boundaries (end of the buffer, filler gap, last columns).
// Every buffer position is read and written by exactly one thread.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
#include <utility>

#include "nrldpc_ratematch_ex.h"

namespace nrldpc {
namespace {

typedef _Float16 half_t;

// value -> element: f32 as it is; f16 clamped to the largest finite half first, then round to nearest even -- +inf is the decoder's
// "filler bit, known 0" and must never come out of a sum (the demapper's rule, nrldpc_modem.hip)
template <typename T> __device__ __forceinline__ T narrow(float v) {
    if constexpr (std::is_same<T, float>::value) return v;
    else return (half_t)fminf(fmaxf(v, -65504.0f), 65504.0f);
}
template <typename T> __device__ __forceinline__ T filler_mark() { return (T)__builtin_inff(); }

template <typename T> struct Quad;
template <> struct Quad<float> { typedef float __attribute__((ext_vector_type(4), aligned(4))) type; };
template <> struct Quad<half_t> { typedef half_t __attribute__((ext_vector_type(4), aligned(4))) type; };
template <typename T> __device__ __forceinline__ bool quad_ok(const T* p) { return sizeof(T) == 4 || (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// four neighbouring elements: one 8- / 16-byte access when the address is dword aligned, four element accesses otherwise
template <typename T> __device__ __forceinline__ void load4(const T* p, T (&v)[4]) {
    if (quad_ok(p)) {
        const typename Quad<T>::type w = *reinterpret_cast<const typename Quad<T>::type*>(p);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = p[t];
    }
}
template <typename T> __device__ __forceinline__ void store4(T* p, const T (&v)[4]) {
    if (quad_ok(p)) {
        typename Quad<T>::type w;
        w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
        *reinterpret_cast<typename Quad<T>::type*>(p) = w;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) p[t] = v[t];
    }
}

// NRLDPCDecoder.m:236-239 for one position: the buffer takes sum + buffer (one f32 add) in its own element type and the decoder's
// LLR is what the buffer now holds
template <typename HbT> __device__ __forceinline__ float combine(float sum, HbT& h) {
    h = narrow<HbT>(sum + (float)h);
    return (float)h;
}

// The tail every form shares, for the four positions pos0 .. pos0+3 of a code block's decoder input (p0 = pos0 - 2Z in d):
// sum[t] = what this transmission delivers, fill[t] = filler (+inf), inb[t] = a non-filler position of the circular buffer.
template <typename HbT, typename OutT>
__device__ __forceinline__ void finish4(HbT* hb, OutT* out, int pos0, int p0, int ncwz, float (&val)[4], const bool (&fill)[4], const bool (&inb)[4]) {
    if (hb) {
        if (inb[0] && inb[1] && inb[2] && inb[3]) {
            HbT h[4];
            load4(hb + p0, h);
#pragma unroll
            for (int t = 0; t < 4; ++t) val[t] = combine(val[t], h[t]);
            store4(hb + p0, h);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (inb[t]) {
                    HbT h = hb[p0 + t];
                    val[t] = combine(val[t], h);
                    hb[p0 + t] = h;
                }
        }
    }
    OutT o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = fill[t] ? filler_mark<OutT>() : narrow<OutT>(val[t]);
    if (pos0 + 3 < ncwz) {
        store4(out + pos0, o);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (pos0 + t < ncwz) out[pos0 + t] = o[t];
    }
}

} // namespace

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
    const int lo_f = a.Kp - 2 * a.Z > 0 ? a.Kp - 2 * a.Z : 0, hi_f = a.K - 2 * a.Z; // fillers (:224)
    const int f_hi = hi_f < a.N_cb ? hi_f : a.N_cb;
    const int F = f_hi > lo_f ? f_hi - lo_f : 0;
    const int P = a.N_cb - F;
    auto nf = [&](int x) { int c = x - lo_f; c = c < 0 ? 0 : (c > F ? F : c); return x - c; };
    const int nfk0 = nf(a.k0);
    const int E = a.E[r];
    const int rows = E > 0 ? E / a.Qm : 1;
    const int Pq = P / rows, Pr = P - Pq * rows; // a repetition is P positions of e further on
    const InT* f = static_cast<const InT*>(a.g) + (size_t)tb * a.G + a.off[r];
    HbT* hb = a.harq ? static_cast<HbT*>(a.harq) + (size_t)blk * a.N_cb : nullptr;
    OutT* out = static_cast<OutT*>(a.out) + (size_t)blk * ncwz;
#pragma unroll
    for (int s = 0; s < RRX_SWEEPS; ++s) {
        const int pos0 = tile0 + s * 256 + 4 * lane;
        if (pos0 >= ncwz) break;
        float val[4];
        bool fill[4], inb[4];
        // q: index among the buffer's non-filler positions counted from k_0; e index q = i*rows + j
        int q = -1, j = 0, i = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = pos0 + t - 2 * a.Z;
            val[t] = 0.0f;
            fill[t] = p >= lo_f && p < hi_f;
            inb[t] = p >= 0 && !fill[t] && p < a.N_cb;
            if (inb[t]) {
                if (q < 0) {
                    q = nf(p) - nfk0;
                    if (q < 0) q += P;
                    for (int m = 1; m < a.Qm; ++m) i += (q >= m * rows); // q / rows when q < E = Qm * rows
                    j = q - i * rows;
                }
                if (q < E) { // (a position that receives nothing does not touch g_tilde)
                    float v = (float)f[j * a.Qm + i];
                    int jj = j, ii = i;
                    for (int k = q + P; k < E; k += P) {
                        jj += Pr; ii += Pq;
                        if (jj >= rows) { jj -= rows; ++ii; }
                        v += (float)f[jj * a.Qm + ii];
                    }
                    val[t] = v;
                }
                ++q; ++j;
                if (j == rows) { j = 0; ++i; }
                if (q == P) { q = 0; j = 0; i = 0; }
            }
        }
        finish4(hb, out, pos0, pos0 - 2 * a.Z, ncwz, val, fill, inb);
    }
}

// ---- the branch-free gather for the usual case, no repetition: a position takes exactly one e(k) or none -------------------------
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
        finish4(hb, out, pos0, pos0 - 2 * a.Z, ncwz, val, fill, inb);
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
    const int lo_f = a.Kp - 2 * a.Z > 0 ? a.Kp - 2 * a.Z : 0, hi_f = a.K - 2 * a.Z;
    const int f_hi = hi_f < a.N_cb ? hi_f : a.N_cb;
    const int F = f_hi > lo_f ? f_hi - lo_f : 0;
    const int P = a.N_cb - F;
    int nfk0 = a.k0 - lo_f;
    nfk0 = a.k0 - (nfk0 < 0 ? 0 : (nfk0 > F ? F : nfk0));
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
            int n = i * rows + j0 + nfk0;
            n -= n >= P ? P : 0;
            const int p = n < lo_f ? n : n + F;
            // the four values are neighbours in d unless the run crosses the end of the buffer or the filler gap
            const bool run = nj == J && n + J <= P && (n >= lo_f || n + J <= lo_f);
            if (run) {
                float val[4];
                const bool no[4] = {false, false, false, false}, yes[4] = {true, true, true, true};
#pragma unroll
                for (int t = 0; t < J; ++t) val[t] = v[t * QM + i];
                finish4(hb, out, 2 * a.Z + p, p, ncwz, val, no, yes);
            } else {
                for (int t = 0; t < nj; ++t) {
                    int nn = n + t;
                    nn -= nn >= P ? P : 0;
                    const int pp = nn < lo_f ? nn : nn + F;
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
    auto covered = [&](int p) -> bool { // p: position in d, 0 <= p < N_cb, not a filler
        int c = p - lo_f;
        c = c < 0 ? 0 : (c > F ? F : c);
        int q = p - c - nfk0;
        q += q < 0 ? P : 0;
        return q < E;
    };
    {
        // wave-uniform skip: the tile lies inside one stretch of d between two boundaries and that stretch is covered
        const int x0 = tile0, x1 = (tile0 + RRX_FILL_TILE < ncwz ? tile0 + RRX_FILL_TILE : ncwz) - 1; // inclusive
        const int p0 = x0 - 2 * a.Z, p1 = x1 - 2 * a.Z;
        const bool plain = p0 >= 0 && p1 < a.N_cb && !(p1 >= lo_f && p0 < hi_f); // no punctured column, nothing beyond the buffer, no filler
        if (plain) {
            // covered positions form a cyclic interval of non-filler indices: both ends covered and the same distance apart in q as in p
            int c0 = p0 - lo_f; c0 = c0 < 0 ? 0 : (c0 > F ? F : c0);
            int c1 = p1 - lo_f; c1 = c1 < 0 ? 0 : (c1 > F ? F : c1);
            int q0 = p0 - c0 - nfk0; q0 += q0 < 0 ? P : 0;
            int q1 = p1 - c1 - nfk0; q1 += q1 < 0 ? P : 0;
            if (q0 < E && q1 < E && q1 - q0 == p1 - p0) return;
        }
    }
#pragma unroll
    for (int s = 0; s < RRX_FILL_TILE / 256; ++s) {
        const int pos0 = tile0 + s * 256 + 4 * lane;
        if (pos0 >= ncwz) break;
        bool skip[4], echo[4];
        OutT o[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = pos0 + t - 2 * a.Z;
            const bool filler = p >= lo_f && p < hi_f;
            const bool inbuf = p >= 0 && p < a.N_cb && !filler;
            skip[t] = (inbuf && covered(p)) || pos0 + t >= ncwz;
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

template <typename InT, typename HbT, typename OutT> static void launch_typed(const RmExArgs& a, bool repeats, bool scatter, int emax, hipStream_t stream) {
    const int ncwz = 2 * a.Z + a.N;
    auto per_qm = [&](auto go) {
        switch (a.Qm) {
            case 1: go(std::integral_constant<int, 1>{}); break;
            case 2: go(std::integral_constant<int, 2>{}); break;
            case 4: go(std::integral_constant<int, 4>{}); break;
            case 6: go(std::integral_constant<int, 6>{}); break;
            default: go(std::integral_constant<int, 8>{}); break;
        }
    };
    const dim3 grid((ncwz + 4 * RRX_TILE - 1) / (4 * RRX_TILE), a.n_tb * a.C);
    if (repeats) {
        hipLaunchKernelGGL((nrldpc_rate_recover_ex_kernel<InT, HbT, OutT>), grid, dim3(256), 0, stream, a);
    } else if (scatter) {
        const int fill_blocks = (ncwz + 4 * RRX_FILL_TILE - 1) / (4 * RRX_FILL_TILE);
        per_qm([&](auto qc) {
            constexpr int QM = decltype(qc)::value;
            const int rows = emax / QM;
            const int in_blocks = (rows + 256 * RRX_J - 1) / (256 * RRX_J);
            hipLaunchKernelGGL((nrldpc_rate_recover_ex_scatter_kernel<InT, HbT, OutT, QM>), dim3(in_blocks + fill_blocks, a.n_tb * a.C), dim3(256), 0, stream, a, in_blocks);
        });
    } else {
        per_qm([&](auto qc) {
            constexpr int QM = decltype(qc)::value;
            hipLaunchKernelGGL((nrldpc_rate_recover_ex_fast_kernel<InT, HbT, OutT, QM>), grid, dim3(256), 0, stream, a);
        });
    }
}

hipError_t launch_rate_recover_ex(const RmExArgs& a, hipStream_t stream) {
    // the launch rule of launch_rate_recover (nrldpc_ratematch.hip), knobs included: measured there with f32 only
    const int lo_f = a.Kp - 2 * a.Z > 0 ? a.Kp - 2 * a.Z : 0, hi_f = a.K - 2 * a.Z;
    const int f_hi = hi_f < a.N_cb ? hi_f : a.N_cb;
    const int P = a.N_cb - (f_hi > lo_f ? f_hi - lo_f : 0);
    static const bool force_general = getenv("NRLDPC_RR_GENERAL") != nullptr;
    static const int env_scatter = getenv("NRLDPC_RR_SCATTER") ? atoi(getenv("NRLDPC_RR_SCATTER")) : -1;
    bool repeats = force_general;
    int emax = 0;
    for (int r = 0; r < a.C; ++r) { repeats = repeats || a.E[r] > P; emax = a.E[r] > emax ? a.E[r] : emax; }
    const bool qm_ok = a.Qm == 1 || a.Qm == 2 || a.Qm == 4 || a.Qm == 6 || a.Qm == 8;
    repeats = repeats || !qm_ok;
    const bool scatter = env_scatter >= 0 ? env_scatter != 0 : (a.harq != nullptr && a.Qm <= 2 && a.N >= 4096);
    auto with_out = [&](auto in, auto hb) {
        typedef decltype(in) InT;
        typedef decltype(hb) HbT;
        if (a.out_f16) launch_typed<InT, HbT, half_t>(a, repeats, scatter, emax, stream);
        else launch_typed<InT, HbT, float>(a, repeats, scatter, emax, stream);
    };
    auto with_hb = [&](auto in) {
        if (a.harq && a.harq_f16) with_out(in, half_t{});
        else with_out(in, float{}); // (without a buffer its type is never used)
    };
    if (a.in_f16) with_hb(half_t{});
    else with_hb(float{});
    return hipGetLastError();
}

} // namespace nrldpc

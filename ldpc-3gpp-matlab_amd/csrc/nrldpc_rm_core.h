// nrldpc_rm_core.h -- what the three rate-recovery units share: nrldpc_ratematch.hip ("f32": a lane owns a PAIR of positions),
// nrldpc_ratematch_ex.hip ("ex": a QUAD, typed input / buffer / output) and nrldpc_mix.hip ("mix": quads driven from a table, with
// the HARQ form).  The one copy of the circular-buffer geometry, of the launch rule, of the element rules, of the tail finish4, of
// the general gather of ex and mix and of the fill part's tile skip.  What the units keep for themselves, and why, is said where it
// stands: the branch-free gathers and the f32 unit's walk and tail.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// The first part -- geometry and launch rule -- is plain C++ that a host compiler reads too: tests/rm_host/rm_rule_check.cpp
// prints both for the parameter sets of the tests and the suite compares them with its own restatement, without a GPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define NRLDPC_RM_HD __host__ __device__ __forceinline__
#else
#define NRLDPC_RM_HD inline
#endif

namespace nrldpc {

// ---- the circular buffer of one code block ----------------------------------------------------------------------------------------
// Positions p count in d (the codeword without its 2Z punctured columns): [lo_f, hi_f) are the filler bits (NRLDPCDecoder.m:224),
// F of them lie inside the circular buffer [0, N_cb), P = N_cb - F positions of it carry a bit.  Bit selection walks those P
// positions cyclically from k_0: the q-th one receives e[q], e[q + P], e[q + 2P], ...
struct RmGeom {
    int lo_f, hi_f, F, P, nfk0;
    NRLDPC_RM_HD RmGeom(int Z, int K, int Kp, int N_cb, int k0) {
        lo_f = Kp - 2 * Z > 0 ? Kp - 2 * Z : 0;
        hi_f = K - 2 * Z;
        const int f_hi = hi_f < N_cb ? hi_f : N_cb;
        F = f_hi > lo_f ? f_hi - lo_f : 0;
        P = N_cb - F;
        const int c = k0 - lo_f;
        nfk0 = k0 - (c < 0 ? 0 : (c > F ? F : c));
    }
    // non-filler positions of the buffer before position x
    NRLDPC_RM_HD int nf(int x) const { int c = x - lo_f; c = c < 0 ? 0 : (c > F ? F : c); return x - c; }
    NRLDPC_RM_HD bool filler(int p) const { return p >= lo_f && p < hi_f; }
    // position (inside the buffer, not a filler) -> its index q among the non-filler positions counted from k_0
    NRLDPC_RM_HD int q_of(int p) const { int q = nf(p) - nfk0; q += q < 0 ? P : 0; return q; }
    // and back: q (< P) -> the non-filler index n counted from 0 -> the position (fillers skipped)
    NRLDPC_RM_HD int n_of(int q) const { int n = q + nfk0; n -= n >= P ? P : 0; return n; }
    NRLDPC_RM_HD int pos_at(int n) const { return n < lo_f ? n : n + F; }
    // J values from non-filler index n on are neighbours in d: the run crosses neither the end of the buffer nor the filler gap
    NRLDPC_RM_HD bool whole_run(int n, int J) const { return n + J <= P && (n >= lo_f || n + J <= lo_f); }
    // does a transmission of E bits deliver anything to position p?
    NRLDPC_RM_HD bool covered(int p, int E) const { return q_of(p) < E; }
};

// ---- the launch rule ----------------------------------------------------------------------------------------------------------------
enum { RM_GENERAL = 0, RM_FAST = 1, RM_SCATTER = 2 }; // (MixRmRec::form holds the first two)

struct RmSwitches {
    bool general; // NRLDPC_RR_GENERAL set: force the general kernel (A/B)
    int scatter;  // NRLDPC_RR_SCATTER=0 / 1: force the gather / the scatter wherever it applies (A/B); -1: not set
};
// the environment, read once per process
inline const RmSwitches& rm_env_switches() {
    static const RmSwitches s = {getenv("NRLDPC_RR_GENERAL") != nullptr, getenv("NRLDPC_RR_SCATTER") ? atoi(getenv("NRLDPC_RR_SCATTER")) : -1};
    return s;
}

struct RmRule {
    int form; // RM_GENERAL: the repetition walk; RM_SCATTER: the input-driven form (units f32 and ex); RM_FAST: the plain gather
    int emax; // largest E_r
    int echo; // MixRmRec::echo: with a soft buffer the single call would run its input-driven form
};

// A code block with more bits than the buffer has non-filler positions repeats: the general kernel (also for a Q_m the other
// forms are not instantiated for).  Else the input-driven form where it measured faster than the gather -- with the HARQ buffer
// and Q_m <= 2: -25 % on the headline code; it loses 6-17 % without the buffer, 21 % at 64QAM with it, and 2.4 x on kilobyte-sized
// blocks (profiles/r06_rate_recover_scatter_ab.txt; measured with f32 only).  Else the plain gather.
inline RmRule rm_launch_rule(const RmGeom& g, const int32_t* E, int C, int Qm, int N, bool buffer, const RmSwitches& sw = RmSwitches{false, -1}) {
    bool repeats = sw.general || !(Qm == 1 || Qm == 2 || Qm == 4 || Qm == 6 || Qm == 8);
    int emax = 0;
    for (int r = 0; r < C; ++r) { repeats = repeats || E[r] > g.P; emax = E[r] > emax ? E[r] : emax; }
    auto scatter = [&](bool harq) { return sw.scatter >= 0 ? sw.scatter != 0 : (harq && Qm <= 2 && N >= 4096); };
    return RmRule{repeats ? RM_GENERAL : scatter(buffer) ? RM_SCATTER : RM_FAST, emax, !repeats && scatter(true) ? 1 : 0};
}

} // namespace nrldpc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>

namespace nrldpc {

typedef _Float16 half_t;

// ---- launch helpers (host side; here because they name half_t) -------------------------------------------------------------------------
// (in_f16, harq_f16, out_f16) -> fn(InT{}, HbT{}, OutT{}); without a buffer pass harq_f16 = false: its type is never used
template <typename Fn> void rm_with_types(bool in_f16, bool harq_f16, bool out_f16, Fn&& fn) {
    auto with_out = [&](auto in, auto hb) {
        if (out_f16) fn(in, hb, half_t{});
        else fn(in, hb, float{});
    };
    auto with_hb = [&](auto in) {
        if (harq_f16) with_out(in, half_t{});
        else with_out(in, float{});
    };
    if (in_f16) with_hb(half_t{});
    else with_hb(float{});
}

// Q_m -> go(std::integral_constant<int, Q_m>{}) for the Q_m the per-Q_m kernels are instantiated for (the launch rule sends
// every other one to the general kernel)
template <typename Fn> void rm_per_qm(int Qm, Fn&& go) {
    switch (Qm) {
        case 1: go(std::integral_constant<int, 1>{}); break;
        case 2: go(std::integral_constant<int, 2>{}); break;
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 6: go(std::integral_constant<int, 6>{}); break;
        default: go(std::integral_constant<int, 8>{}); break;
    }
}

// ---- device code; in a name space of its own (short names: narrow, combine, Quad), which the three units open ----------------------------
namespace rm_dev {

// ---- element rules (units ex and mix)
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
// a multi-dword global access needs dword alignment: f32 always has it, f16 by the address
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

// The tail every form of ex and mix shares, for the four positions pos0 .. pos0+3 of a code block's decoder input (p0 = pos0 - 2Z
// in d): val[t] = what this transmission delivers, fill[t] = filler (+inf), inb[t] = a non-filler position of the circular buffer,
// keep[t] = the position receives nothing and the configuration leaves such buffer entries as they are (MixRmRec::echo): read, not
// written.  HARQ && fresh (workgroup-uniform): the transport block starts a new HARQ process -- the buffer counts as +0.0 and is NOT
// read; every non-filler position inside the circular buffer takes narrow(sum + 0), the kept ones included (they would echo the +0).
// The single-configuration unit calls it with HARQ = false and nothing kept.
template <bool HARQ, typename HbT, typename OutT>
__device__ __forceinline__ void finish4(HbT* hb, OutT* out, int pos0, int p0, int ncwz, float (&val)[4], const bool (&fill)[4], const bool (&inb)[4],
                                        const bool (&keep)[4], bool fresh) {
    bool done = false;
    if constexpr (HARQ) {
        if (fresh) {
            float zero = 0.0f;
            asm volatile("" : "+v"(zero)); // opaque to the optimiser: sum + 0 stays an add whatever the flags, and -0 becomes +0
            HbT h[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                h[t] = narrow<HbT>(val[t] + zero);
                if (inb[t]) val[t] = (float)h[t];
            }
            if (inb[0] && inb[1] && inb[2] && inb[3]) {
                store4(hb + p0, h);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (inb[t]) hb[p0 + t] = h[t];
            }
            done = true;
        }
    }
    if (hb && !done) {
        if (inb[0] && inb[1] && inb[2] && inb[3] && !(keep[0] || keep[1] || keep[2] || keep[3])) {
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
                    if (keep[t]) {
                        val[t] = (float)h;
                    } else {
                        val[t] = combine(val[t], h);
                        hb[p0 + t] = h;
                    }
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

// ---- the general gather of ex and mix, for the four neighbouring positions p0 .. p0+3 of d ------------------------------------------------
// f: the code block's bits of g_tilde, e[k] = f[(k mod rows)*Qm + k div rows] with rows = E/Qm (1 when E == 0).
// Out: val[t] = what this transmission delivers (0 when nothing), fill[t] = filler, inb[t] = a non-filler position of the buffer.
// The walk: repetitions summed in ascending k, the reference's accumulation order (NRLDPCDecoder.m:229-231).
// Pq = P / rows, Pr = P - Pq * rows: a repetition is P positions of e further on.
// (The f32 unit's general kernel keeps a copy at width 2 with the buffer inside the walk: through this body it took 2 more VGPRs.  The
// branch-free gather for the no-repetition case stays in the three units: shared, it measured slower, see nrldpc_ratematch_ex.hip.)
template <typename InT>
__device__ __forceinline__ void gather_general(const RmGeom& g, const InT* f, int p0, int N_cb, int E, int rows, int Qm, int Pq, int Pr,
                                               float (&val)[4], bool (&fill)[4], bool (&inb)[4]) {
    // q: index among the buffer's non-filler positions counted from k_0; e index q = i*rows + j
    int q = -1, j = 0, i = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = p0 + t;
        val[t] = 0.0f;
        fill[t] = g.filler(p);
        inb[t] = p >= 0 && !fill[t] && p < N_cb;
        if (inb[t]) {
            if (q < 0) {
                q = g.nf(p) - g.nfk0;
                if (q < 0) q += g.P;
                for (int m = 1; m < Qm; ++m) i += (q >= m * rows); // q / rows when q < E = Qm * rows
                j = q - i * rows;
            }
            if (q < E) { // (a position that receives nothing does not touch g_tilde)
                float v = (float)f[j * Qm + i];
                int jj = j, ii = i;
                for (int k = q + g.P; k < E; k += g.P) {
                    jj += Pr; ii += Pq;
                    if (jj >= rows) { jj -= rows; ++ii; }
                    v += (float)f[jj * Qm + ii];
                }
                val[t] = v;
            }
            ++q; ++j;
            if (j == rows) { j = 0; ++i; }
            if (q == g.P) { q = 0; j = 0; i = 0; }
        }
    }
}

// ---- the fill part of the input-driven form --------------------------------------------------------------------------------------------
// Wave-uniform: the positions [tile0, tile0 + tile) of the decoder input (cut at ncwz) lie inside one stretch of d between two
// boundaries -- no punctured column, nothing beyond the buffer, no filler -- and that stretch is covered: nothing to fill.
__device__ __forceinline__ bool fill_tile_covered(const RmGeom& g, int tile0, int tile, int ncwz, int Z, int N_cb, int E) {
    const int x0 = tile0, x1 = (tile0 + tile < ncwz ? tile0 + tile : ncwz) - 1; // inclusive
    const int p0 = x0 - 2 * Z, p1 = x1 - 2 * Z;
    const bool plain = p0 >= 0 && p1 < N_cb && !(p1 >= g.lo_f && p0 < g.hi_f);
    if (!plain) return false;
    // covered positions form a cyclic interval of non-filler indices: both ends covered and the same distance apart in q as in p
    const int q0 = g.q_of(p0), q1 = g.q_of(p1);
    return q0 < E && q1 < E && q1 - q0 == p1 - p0;
}

} // namespace rm_dev
} // namespace nrldpc
#endif

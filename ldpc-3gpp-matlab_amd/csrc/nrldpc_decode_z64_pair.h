// nrldpc_decode_z64_pair.h -- the split decoder's pass 1 with the two-smallest search over PAIRS of edges.
//
// LayerZ64::track3 (nrldpc_decode_z64.h) folds one edge at a time into the running sorted pair pm1 <= pm2:
//     pm2 = med3(|t|, pm1, pm2);  pm1 = min(pm1, |t|);                       2 ops per edge, both at the 4-cycle rate
// Two edges a, b fold in three ops (v_med3_f32, v_min3_f32, v_min_f32: the same rate, |x| as a source modifier):
//     s2  = med3(pm1, |a|, |b|);      the second smallest of {pm1, a, b}
//     pm1 = min3(pm1, |a|, |b|);
//     pm2 = min(s2, pm2);             pm2 >= old pm1 >= new pm1, so the sorted union of {pm1, a, b} and {pm2} starts pm1', min(s2, pm2)
// The two smallest values of a multiset do not depend on how they are found: ties, and the non-integer cap the search starts
// from, come out exactly as in the one-at-a-time search, so m1, m2 and the parity word -- and with them every message byte,
// a-posteriori word and hard bit -- are bit-identical (tests/test_pair_search_cpu.py, tests/test_pair_search_gpu.py).
//
// The sign parity already folds edges in pairs (pend holds the first edge's bits until the second arrives); the magnitude
// search reads |pend| for a, so the pairing costs no register.  Pairs form inside a part (LayerZ64::part_of: what is tracked
// before the barrier, what after); a part with an odd edge count ends with the single-edge step, except that the
// thread-private extension edge, which follows part 0, is the partner of that part's leftover where there is one.  Nothing is
// carried across the barrier (work deferred past the barrier costs more than it saves).
//
// How it is switched in.  nrldpc_decode_z64.h and nrldpc_decode_z64s.h are not edited: this header partially specialises
// GroupZ64 for the two halves of the split form (H = 0, 1) so that s_crit / s_early / s_dense and the split kernel pick up
// LayerZ64Pair through the group type they already name.  It must therefore be included after nrldpc_decode_z64.h and before
// the first non-template use of the split kernel (the launcher in nrldpc_decode_z64_inst.hip): nrldpc_decode_z64q_inst.hip
// does that.  The row form (H = -1) and LayerZ64::update are untouched.
#ifndef NRLDPC_DECODE_Z64_PAIR_H
#define NRLDPC_DECODE_Z64_PAIR_H
#include "nrldpc_decode_z64.h"

namespace nrldpc {
inline namespace NRLDPC_UNIT { // one name space per translation unit: see NRLDPC_UNIT in nrldpc_decode_z64.h

template <int BG, int ZC, int L, bool FULL, int NL, int H> struct LayerZ64Pair : LayerZ64<BG, ZC, L, FULL, NL, H> {
    using Base = LayerZ64<BG, ZC, L, FULL, NL, H>;
    using Base::HAS_EXT;
    using Base::XI;
    using Base::ncore;
    using Base::lam;
    using Base::pm1;
    using Base::pm2;
    using Base::pS;
    using Base::t;

    // one edge into the sorted pair (the leftover of an odd part)
    __device__ __forceinline__ void fold1(float x) {
        const float ax = fabsf(x);
        pm2 = __builtin_amdgcn_fmed3f(ax, pm1, pm2);
        pm1 = fminf(pm1, ax);
    }
    // two edges into the sorted pair
    __device__ __forceinline__ void fold2(float x, float y) {
        const float ax = fabsf(x), ay = fabsf(y);
        const float s2 = __builtin_amdgcn_fmed3f(pm1, ax, ay);
        pm1 = fminf(fminf(pm1, ax), ay);
        pm2 = fminf(s2, pm2);
    }

    template <int PART, bool XF = false, class St> __device__ __forceinline__ void track3(const St& st, float cap) {
        // cap = (127.49 + beta)/alpha: see LayerZ64::track3
        if constexpr (PART == 0) { pm1 = cap; pm2 = cap; pS = 0; }
        constexpr int npart = Base::template pcount_before<PART>(ncore);
        constexpr bool EXT_HERE = PART == (NRLDPC_Z64_DEFER_EXT ? 1 : 0) && HAS_EXT; // the extension bit is thread-private: never "late"
        float pend = 0.0f; // the first edge of a pair, for the sign parity and the magnitude search alike
        static_for<ncore>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if constexpr (Base::part_of(j) == PART) {
                constexpr int ce = Base::cidx(j);
                constexpr int k = Base::template pcount_before<PART>(j);
                const float tj = t[j] - byte_to_f32<ce & 3>(st.rm[ce >> 2]);
                t[j] = tj;
                if constexpr (k % 2 == 0) {
                    pend = tj;
                    if constexpr (k + 1 == npart && !EXT_HERE) fold1(tj); // the part's leftover, no extension edge to pair it with
                } else {
                    fold2(pend, tj);
                    pS = __builtin_amdgcn_bitop3_b32(pS, fbits(pend), fbits(tj), 0x96); // three-input xor
                }
            }
        });
        if constexpr (EXT_HERE) {
            lam = st.template ext<XI, XF>();
            if constexpr (npart % 2 == 1) {
                fold2(pend, lam);
                pS = __builtin_amdgcn_bitop3_b32(pS, fbits(pend), fbits(lam), 0x96);
            } else {
                fold1(lam);
                pS ^= fbits(lam);
            }
        } else {
            if constexpr (npart % 2 == 1) pS ^= fbits(pend);
        }
    }
    template <bool LATE, bool XF = false, class St> __device__ __forceinline__ void track_part(const St& st, float cap) {
        if constexpr (LATE) {
            if constexpr (NRLDPC_Z64_DEFER > 0 || NRLDPC_Z64_DEFER_EXT) track3<1, XF>(st, cap);
            track3<2, XF>(st, cap);
        } else {
            track3<0, XF>(st, cap);
        }
    }
};

// GroupZ64 (nrldpc_decode_z64.h) with LayerZ64Pair members
template <int BG, int ZC, int GI, int NL, int H> struct GroupZ64Pair {
    using LG = LGof<BG, ZC, NL, H>;
    static constexpr int GS = LG::group_first(GI);
    static constexpr int N = LG::group_last(GS) - GS + 1;
    static_assert(N >= 1 && N <= 3, "group size");
    struct NoLayer {}; // absent second / third layer: no storage, so copying a group copies only live state
    LayerZ64Pair<BG, ZC, GS, true, NL, H> l0;
    std::conditional_t<(N > 1), LayerZ64Pair<BG, ZC, (N > 1 ? GS + 1 : GS), true, NL, H>, NoLayer> l1;
    std::conditional_t<(N > 2), LayerZ64Pair<BG, ZC, (N > 2 ? GS + 2 : GS), true, NL, H>, NoLayer> l2;

    template <bool LATE> __device__ __forceinline__ void loads(const char* lds, const uint32_t (&R)[Z64<BG, ZC>::NBASE]) {
        l0.template load_part<LATE>(lds, R);
        if constexpr (N > 1) l1.template load_part<LATE>(lds, R);
        if constexpr (N > 2) l2.template load_part<LATE>(lds, R);
    }
    template <bool LATE, bool XF = false, class St> __device__ __forceinline__ void track(const St& st, float cap) {
        l0.template track_part<LATE, XF>(st, cap);
        if constexpr (N > 1) l1.template track_part<LATE, XF>(st, cap);
        if constexpr (N > 2) l2.template track_part<LATE, XF>(st, cap);
    }
    template <class St> __device__ __forceinline__ void finish(St& st, char* lds, const uint32_t (&R)[Z64<BG, ZC>::NBASE], const DecArgs& a) {
        l0.finish(st, lds, R, a);
        if constexpr (N > 1) l1.finish(st, lds, R, a);
        if constexpr (N > 2) l2.finish(st, lds, R, a);
    }
    __device__ __forceinline__ void ext(const DecArgs& a, uint32_t& esign_lo, uint32_t& esign_hi) const {
        l0.ext(a, esign_lo, esign_hi, nullptr);
        if constexpr (N > 1) l1.ext(a, esign_lo, esign_hi, nullptr);
        if constexpr (N > 2) l2.ext(a, esign_lo, esign_hi, nullptr);
    }
    // w: the wave's index within its codeword (block geometry) / its row-wave index (packed geometry)
    __device__ __forceinline__ void twins(char* lds, const uint32_t (&R)[Z64<BG, ZC>::NBASE], uint32_t RA, uint32_t RB, int w, int nl) const {
        dispatch_w<0, (z64_packed(ZC) ? z64p_rw(BG, ZC) : z64_nwv(ZC))>(w, [&](auto wc) {
            constexpr int WV = decltype(wc)::value;
            l0.template twins<WV>(lds, R, RA, RB, nl);
            if constexpr (N > 1) l1.template twins<WV>(lds, R, RA, RB, nl);
            if constexpr (N > 2) l2.template twins<WV>(lds, R, RA, RB, nl);
        });
    }
};

// the two halves of the split form (nrldpc_decode_z64s.h) take the paired search; H = -1, the row form, keeps the primary template
template <int BG, int ZC, int GI, int NL> struct GroupZ64<BG, ZC, GI, NL, 0> : GroupZ64Pair<BG, ZC, GI, NL, 0> {};
template <int BG, int ZC, int GI, int NL> struct GroupZ64<BG, ZC, GI, NL, 1> : GroupZ64Pair<BG, ZC, GI, NL, 1> {};

} // inline namespace NRLDPC_UNIT
} // namespace nrldpc
#endif

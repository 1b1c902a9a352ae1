// nrldpc_mix_skip.h -- mixed HARQ steps that decode only the code blocks still pending: the rule, the thread partition and scan of the
// compaction, and the workgroup mapping, chunk arithmetic and row copy of the gather / scatter (nrldpc_mix_pending_dev,
// nrldpc_mix_gather_cw_dev, nrldpc_mix_scatter_hard_dev; kernels: nrldpc_mix_skip.hip; semantics: include/nrldpc.h, DESIGN.md
// section 4.19).
// (Not in nrldpc_kernels.h and including nothing of the decoder: that header is part of the decoder kernels' identity.)
//
// Everything here is plain C++ that a host compiler reads too: tests/mix_host/mix_skip_check.cpp runs the rule, the compaction and the
// row copies on the CPU, thread by thread as the kernels do, under the address and undefined-behaviour sanitizers -- on arrays of
// exactly the packed sizes, so an index or a vector access the kernels would get wrong is an error there before it is a fault here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NRLDPC_SKIP_HD __host__ __device__ __forceinline__
#else
#define NRLDPC_SKIP_HD inline
#endif

namespace nrldpc {

enum { MIX_SKIP_UNSCHEDULED = 1, MIX_SKIP_SETTLED = 2 }; // = NRLDPC_MIX_SKIP_* (include/nrldpc.h)

constexpr int MIX_SKIP_THREADS = 1024;  // the pending kernel: one workgroup per configuration
constexpr int MIX_SKIP_SCAN_STEPS = 10; // 2^10 = MIX_SKIP_THREADS
constexpr int MIX_SKIP_COPY_THREADS = 256;
constexpr int MIX_SKIP_CHUNK = 8192;    // bytes of a row per gather / scatter workgroup: two 16-byte accesses per thread

// ---- the rule ----------------------------------------------------------------------------------------------------------------------
// f: the block is scheduled (CBGTI flag), w: its transport block starts a new HARQ process, p: the block's sticky CRC flag, o: the
// transport block's ok of the PREVIOUS step, single: C == 1 (no code-block CRC: p says nothing), allp: every block of the transport
// block has p (and o is still 0: the transport-block CRC fails, the whole block is decoded again).
NRLDPC_SKIP_HD bool mix_skip_pending(int32_t rule, bool f, bool w, bool p, bool o, bool single, bool allp) {
    if (rule == MIX_SKIP_UNSCHEDULED) return f;
    return f && (w || (!o && (single || !p || allp)));
}

// The state arrays of a call, as handed to the C ABI (packed tb / cb layouts; cbgti and is_new may be null).
struct MixSkipState {
    const int32_t* cb_pass;
    const int32_t* ok;
    const uint8_t* cbgti;
    const uint8_t* is_new;
};

// One configuration of the three launches.
struct MixSkipRec {
    int64_t cw_off, c_hat_off, cb_off, tb_off; // element offsets of the segment (nrldpc_mix_offsets)
    int32_t n_cb, C, N_cw, K;                  // code blocks (n_tb * C), blocks per transport block, LLRs and hard bits per row
};

// The rule for code block blk = tb * C + r of a configuration, reading only what decides it (UNSCHEDULED reads neither cb_pass nor ok;
// the C flags of allp are read only when everything else leaves the block to them).
NRLDPC_SKIP_HD bool mix_skip_block_pending(int32_t rule, const MixSkipState& s, const MixSkipRec& c, int32_t blk) {
    const int32_t tb = blk / c.C;
    const int64_t cb = c.cb_off + blk, t = c.tb_off + tb;
    if (s.cbgti && s.cbgti[cb] == 0) return false;
    if (rule == MIX_SKIP_UNSCHEDULED) return true;
    if (s.is_new && s.is_new[t] != 0) return true;
    if (s.ok[t] != 0) return false;
    if (c.C == 1 || s.cb_pass[cb] == 0) return true;
    const int32_t* row = s.cb_pass + c.cb_off + (int64_t)tb * c.C;
    for (int32_t r = 0; r < c.C; ++r)
        if (row[r] == 0) return false;
    return true;
}

// ---- the compaction: thread t of MIX_SKIP_THREADS owns the contiguous run [lo, hi) of the configuration's n_cb code blocks ----------
NRLDPC_SKIP_HD void mix_skip_run(int32_t n_cb, int32_t threads, int32_t t, int32_t& lo, int32_t& hi) {
    const int64_t per = ((int64_t)n_cb + threads - 1) / threads;
    const int64_t a = per * t, b = a + per;
    lo = (int32_t)(a < n_cb ? a : n_cb);
    hi = (int32_t)(b < n_cb ? b : n_cb);
}

template <typename Pend> NRLDPC_SKIP_HD int32_t mix_skip_count_run(int32_t lo, int32_t hi, const Pend& pend) {
    int32_t k = 0;
    for (int32_t b = lo; b < hi; ++b) k += pend(b) ? 1 : 0;
    return k;
}

// one step of the inclusive scan over the thread counts (distance d = 1, 2, 4, ...; `in` and the array the result goes to differ)
NRLDPC_SKIP_HD int32_t mix_skip_scan_step(const int32_t* in, int32_t t, int32_t d) { return in[t] + (t >= d ? in[t - d] : 0); }

// the thread's pending blocks, ascending, from its base (= the pending blocks of the threads before it)
template <typename Pend> NRLDPC_SKIP_HD void mix_skip_write_run(int32_t lo, int32_t hi, int32_t base, const Pend& pend, int32_t* index) {
    for (int32_t b = lo; b < hi; ++b)
        if (pend(b)) index[base++] = b;
}

// ---- gather / scatter: workgroup -> (configuration, dense slot, chunk of the row) ------------------------------------------------------
NRLDPC_SKIP_HD int32_t mix_skip_chunks(int64_t row_bytes) { return (int32_t)((row_bytes + MIX_SKIP_CHUNK - 1) / MIX_SKIP_CHUNK); }

// the rows a grid copies, named by the bytes per element: hard bits (K per row), f16 or f32 LLRs (N_cw per row)
enum { MIX_SKIP_ROW_HARD = 1, MIX_SKIP_ROW_F16 = 2, MIX_SKIP_ROW_F32 = 4 };
NRLDPC_SKIP_HD int64_t mix_skip_row_bytes(const MixSkipRec& c, int32_t esize) { return esize == MIX_SKIP_ROW_HARD ? (int64_t)c.K : (int64_t)c.N_cw * esize; }

struct MixSkipWork {
    int32_t cfg, slot, chunk;
};

// prefix[0 .. n] counts workgroups: prefix[i + 1] - prefix[i] = n_cb * chunks of configuration i (sized for EVERY row: how many are
// pending is known on the device only).  The search is mix_find's (nrldpc_mix.h), restated so that this header stands alone: the
// configuration of workgroup x is the LAST i with prefix[i] <= x.  Requires 0 <= x < prefix[n].
NRLDPC_SKIP_HD int32_t mix_skip_find(const int32_t* prefix, int32_t n, int32_t x) {
    int32_t lo = 0, hi = n; // invariant: prefix[lo] <= x < prefix[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

NRLDPC_SKIP_HD MixSkipWork mix_skip_work(const int32_t* prefix, const MixSkipRec* recs, int32_t n, int32_t esize, int32_t wg) {
    MixSkipWork w;
    w.cfg = mix_skip_find(prefix, n, wg);
    const int32_t local = wg - prefix[w.cfg];
    const int32_t chunks = mix_skip_chunks(mix_skip_row_bytes(recs[w.cfg], esize));
    w.slot = local / chunks;
    w.chunk = local - w.slot * chunks;
    return w;
}

// the bytes [lo, lo + len) of a row that chunk `chunk` covers
NRLDPC_SKIP_HD void mix_skip_span(int64_t row_bytes, int32_t chunk, int64_t& lo, int32_t& len) {
    lo = (int64_t)chunk * MIX_SKIP_CHUNK;
    const int64_t rest = row_bytes - lo;
    len = (int32_t)(rest < MIX_SKIP_CHUNK ? (rest > 0 ? rest : 0) : MIX_SKIP_CHUNK);
}

// ---- the row copy --------------------------------------------------------------------------------------------------------------------
// The widest access both addresses allow: LLR rows start 16-byte (f32) or 8-byte (f16, 16 for an even Z) aligned and are whole vectors
// long; a c_hat row (K = 22 Z or 10 Z bytes) is 2-byte aligned for an odd Z, and its last vector may be partial: the byte tail.
struct alignas(16) MixSkipV16 { uint32_t x, y, z, w; };
struct alignas(8) MixSkipV8 { uint32_t x, y; };

NRLDPC_SKIP_HD int32_t mix_skip_width(uintptr_t src, uintptr_t dst) {
    const uintptr_t a = src | dst | 16;
    return (int32_t)(a & (~a + 1)); // lowest set bit: 1, 2, 4, 8 or 16
}

// thread t of `threads`: vectors t, t + threads, ... of the span, then bytes of the tail (fewer than sizeof(V))
template <typename V> NRLDPC_SKIP_HD void mix_skip_copy_as(const uint8_t* src, uint8_t* dst, int32_t len, int32_t t, int32_t threads) {
    const int32_t nv = len / (int32_t)sizeof(V);
    const V* s = reinterpret_cast<const V*>(src);
    V* d = reinterpret_cast<V*>(dst);
    for (int32_t i = t; i < nv; i += threads) d[i] = s[i];
    for (int32_t i = nv * (int32_t)sizeof(V) + t; i < len; i += threads) dst[i] = src[i];
}

NRLDPC_SKIP_HD void mix_skip_copy(const uint8_t* src, uint8_t* dst, int32_t len, int32_t t, int32_t threads) {
    switch (mix_skip_width(reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst))) { // workgroup-uniform
    case 16: mix_skip_copy_as<MixSkipV16>(src, dst, len, t, threads); break;
    case 8: mix_skip_copy_as<MixSkipV8>(src, dst, len, t, threads); break;
    case 4: mix_skip_copy_as<uint32_t>(src, dst, len, t, threads); break;
    case 2: mix_skip_copy_as<uint16_t>(src, dst, len, t, threads); break;
    default: mix_skip_copy_as<uint8_t>(src, dst, len, t, threads); break;
    }
}

// ---- the iteration counts of the scatter ---------------------------------------------------------------------------------------------
// Slot j of a configuration with `count` pending blocks also zeroes the counts of the blocks that are NOT pending between its own
// block and the previous slot's: [index[j - 1] + 1, index[j]), from 0 for j = 0, and the last slot the blocks behind its own too.
// With count == 0 slot 0 zeroes all n_cb.  Every element has one writer.
NRLDPC_SKIP_HD void mix_skip_zero_range(const int32_t* index /* the configuration's */, int32_t count, int32_t n_cb, int32_t slot, int32_t& lo, int32_t& hi,
                                        int32_t& lo2, int32_t& hi2) {
    lo2 = hi2 = 0;
    if (count == 0) { lo = 0; hi = slot == 0 ? n_cb : 0; return; }
    lo = slot == 0 ? 0 : index[slot - 1] + 1;
    hi = index[slot];
    if (slot == count - 1) { lo2 = index[slot] + 1; hi2 = n_cb; }
}

} // namespace nrldpc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace nrldpc {

struct MixSkipLaunch {
    const MixSkipRec* recs;  // device, [n]
    const int32_t* prefix;   // device, [n + 1] workgroups of the gather / scatter grid in use (f32 rows, f16 rows or hard-bit rows)
    int32_t n, n_wg;
    int32_t esize;           // bytes per element of a row: 4 / 2 (gather), 1 (scatter)
};

hipError_t launch_mix_skip_pending(const MixSkipLaunch& a, int32_t rule, const MixSkipState& s, int32_t* index, int32_t* count, hipStream_t stream);
hipError_t launch_mix_skip_gather(const MixSkipLaunch& a, const void* cw, const int32_t* index, const int32_t* count, void* dense, hipStream_t stream);
hipError_t launch_mix_skip_scatter(const MixSkipLaunch& a, const uint8_t* dense, const int32_t* iters_dense, const int32_t* index, const int32_t* count,
                                   uint8_t* c_hat, int32_t* iters, hipStream_t stream);

} // namespace nrldpc
#endif

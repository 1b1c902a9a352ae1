// mix_skip_check.cpp -- stand-alone host check of the stages that let a mixed HARQ step decode only its pending code blocks
// (ldpc-3gpp-matlab_amd/csrc/nrldpc_mix_skip.h: the rule, the thread partition and scan of the compaction, the workgroup mapping, chunk
// arithmetic and row copy of the gather / scatter), meant to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_mix_skip_api.py does that).  The kernels of nrldpc_mix_skip.hip are these functions on a grid; the loops below walk the
// grids thread by thread as the kernels do, on arrays of exactly the packed sizes.
//
// Input (a text file, argv[1]): n, then per configuration
//     n_tb C Z N_cw K   and the offsets cw, c_hat, cb, tb nrldpc_mix_layout gave for it,
// then the four totals.  The LAST configuration must be the one with a 2-byte aligned hard-bit row: Z == 9, K == 90.
//
// Checked:
//  1. the rule, both forms, over every combination of (f, w, p, o, C == 1) and allp against literal if-chains, and the lazy reader
//     mix_skip_block_pending against the rule on arrays that hold those values (flag arrays null and non-null);
//  2. the compaction for n_cb in {0, 1, 63, 64, 65, 1023, 1024, 1025, 65537} under the patterns none / all / alternating / one at the
//     end / three random seeds: indices ascending and equal to the literal loop's, the count exact, nothing written from count on;
//  3. the row copy: for every access width and a set of lengths, every byte of a span has exactly one writing thread;
//  4. gather and scatter on the input mix for f32, f16 and hard-bit rows under several pending patterns: every byte of every pending
//     row is covered by exactly one workgroup span, dense rows below the count equal the indexed rows, everything else -- rows from the
//     count on, rows that are not pending, gaps -- keeps its sentinel, and every iteration count has exactly one writer.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <vector>

#include "nrldpc_mix_skip.h"

using namespace nrldpc;

static int fail(const char* what, long a = 0, long b = 0, long c = 0) {
    std::fprintf(stderr, "mix_skip_check: %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

// ---- 1. the rule ----------------------------------------------------------------------------------------------------------------------
static bool literal_rule(int rule, bool f, bool w, bool p, bool o, bool single, bool allp) {
    if (rule == 1) return f;
    if (!f) return false;     // not scheduled: never decoded
    if (w) return true;       // a new HARQ process: everything scheduled
    if (o) return false;      // acknowledged
    if (single) return true;  // no code-block CRC: cb_pass says nothing
    if (!p) return true;      // has not passed
    return allp;              // passed: again only when all passed and the transport-block CRC still fails
}

static int check_rule() {
    long cases = 0;
    for (int rule = 1; rule <= 2; ++rule)
        for (int bits = 0; bits < 32; ++bits)
            for (int others = 0; others < 2; ++others) {
                const bool f = bits & 1, w = bits & 2, p = bits & 4, o = bits & 8, single = bits & 16;
                const bool allp = single ? p : (p && others);
                const bool want = literal_rule(rule, f, w, p, o, single, allp);
                if (mix_skip_pending(rule, f, w, p, o, single, allp) != want) return fail("the rule", rule, bits, others);
                // the lazy reader: transport block 1 of 3 of a configuration, block r = 1 of C = 3 (or the only one); cb_pass holds
                // values other than 0 / 1
                MixSkipRec c{};
                c.C = single ? 1 : 3; c.n_cb = 3 * c.C; c.cb_off = 16; c.tb_off = 32;
                const int r = single ? 0 : 1, blk = 1 * c.C + r;
                std::vector<int32_t> cb_pass(16 + c.n_cb, 0), ok(32 + 3, 0);
                std::vector<uint8_t> cbgti(16 + c.n_cb, 1), is_new(32 + 3, 0);
                for (int q = 0; q < c.C; ++q) cb_pass[16 + c.C + q] = others ? 7 : 0;
                cb_pass[16 + blk] = p ? -3 : 0;
                ok[32 + 1] = o ? 1 : 0; is_new[32 + 1] = w ? 5 : 0; cbgti[16 + blk] = f ? 1 : 0;
                for (int nulls = 0; nulls < 4; ++nulls) {
                    if (((nulls & 1) && !f) || ((nulls & 2) && w)) continue; // a null array means f = 1 / w = 0
                    MixSkipState s{cb_pass.data(), ok.data(), (nulls & 1) ? nullptr : cbgti.data(), (nulls & 2) ? nullptr : is_new.data()};
                    if (rule == 1) s.cb_pass = s.ok = nullptr; // UNSCHEDULED reads neither
                    if (mix_skip_block_pending(rule, s, c, blk) != want) return fail("the lazy reader", rule, bits, others * 4 + nulls);
                    ++cases;
                }
            }
    std::printf("rule ok: %ld cases\n", cases);
    return 0;
}

// ---- 2. the compaction, thread by thread as nrldpc_mix_pending_kernel does it -----------------------------------------------------------
// index: the configuration's entries (exactly n_cb of them); returns the count thread 0 writes
template <typename Pend> static int32_t emulate_pending(int32_t n_cb, const Pend& pend, int32_t* index) {
    const int T = MIX_SKIP_THREADS;
    std::vector<int32_t> scan[2] = {std::vector<int32_t>(T), std::vector<int32_t>(T)}, own(T);
    for (int t = 0; t < T; ++t) {
        int32_t lo, hi;
        mix_skip_run(n_cb, T, t, lo, hi);
        own[t] = scan[0][t] = mix_skip_count_run(lo, hi, pend);
    }
    int from = 0;
    for (int k = 0; k < MIX_SKIP_SCAN_STEPS; ++k) {
        for (int t = 0; t < T; ++t) scan[from ^ 1][t] = mix_skip_scan_step(scan[from].data(), t, 1 << k);
        from ^= 1;
    }
    for (int t = 0; t < T; ++t) {
        int32_t lo, hi;
        mix_skip_run(n_cb, T, t, lo, hi);
        mix_skip_write_run(lo, hi, scan[from][t] - own[t], pend, index);
    }
    return scan[from][T - 1];
}

static std::vector<uint8_t> pattern(int32_t n_cb, int kind) {
    std::vector<uint8_t> v(n_cb, 0);
    std::mt19937 rng(1000 + kind);
    for (int32_t b = 0; b < n_cb; ++b)
        v[b] = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? (b & 1) : kind == 3 ? (b == n_cb - 1) : (rng() % (kind == 4 ? 2 : kind == 5 ? 10 : 50) == 0);
    return v;
}

static int check_compaction() {
    if ((1 << MIX_SKIP_SCAN_STEPS) != MIX_SKIP_THREADS) return fail("scan steps");
    const int32_t sizes[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 65537};
    for (int32_t n_cb : sizes) {
        // the partition: contiguous runs in thread order that cover [0, n_cb) exactly
        int32_t next = 0;
        for (int t = 0; t < MIX_SKIP_THREADS; ++t) {
            int32_t lo, hi;
            mix_skip_run(n_cb, MIX_SKIP_THREADS, t, lo, hi);
            if (lo != next || hi < lo || hi > n_cb) return fail("the partition", n_cb, t, lo);
            next = hi;
        }
        if (next != n_cb) return fail("the partition does not reach the end", n_cb, next);
        for (int kind = 0; kind < 7; ++kind) {
            const std::vector<uint8_t> pat = pattern(n_cb, kind);
            std::vector<int32_t> want;
            for (int32_t b = 0; b < n_cb; ++b)
                if (pat[b]) want.push_back(b);
            std::vector<int32_t> index(n_cb, -7);
            const int32_t count = emulate_pending(n_cb, [&](int32_t b) { return pat.at(b) != 0; }, index.data());
            if (count != (int32_t)want.size()) return fail("count", n_cb, kind, count);
            for (int32_t j = 0; j < n_cb; ++j)
                if (index[j] != (j < count ? want[j] : -7)) return fail("index", n_cb, kind, j);
        }
    }
    std::printf("compaction ok\n");
    return 0;
}

// ---- 3. the row copy: one writing thread per byte ----------------------------------------------------------------------------------------
static int check_copy() {
    const int32_t lens[] = {0, 1, 2, 15, 16, 17, 90, 198, 200, 255, 256, 4096 + 6, MIX_SKIP_CHUNK - 2, MIX_SKIP_CHUNK};
    const int T = MIX_SKIP_COPY_THREADS;
    for (int32_t len : lens)
        for (int shift : {0, 8, 4, 2, 1, 3}) {
            if (len + shift > MIX_SKIP_CHUNK + 16) continue;
            // 16-byte aligned stores with the span at `shift`; source values are never the sentinel 0
            alignas(16) static uint8_t src[MIX_SKIP_CHUNK + 32], dst[MIX_SKIP_CHUNK + 32];
            for (size_t i = 0; i < sizeof src; ++i) src[i] = (uint8_t)(1 + i % 255);
            const int32_t width = mix_skip_width(reinterpret_cast<uintptr_t>(src + shift), reinterpret_cast<uintptr_t>(dst + shift));
            const int32_t want_width = shift == 0 ? 16 : shift == 8 ? 8 : shift == 4 ? 4 : shift == 2 ? 2 : 1;
            if (width != want_width) return fail("access width", shift, width);
            std::vector<int32_t> writers(len, 0);
            for (int t = 0; t < T; ++t) {
                std::memset(dst, 0, sizeof dst);
                mix_skip_copy(src + shift, dst + shift, len, t, T);
                for (size_t i = 0; i < sizeof dst; ++i) {
                    if (!dst[i]) continue;
                    if ((int32_t)i < shift || (int32_t)i >= shift + len) return fail("a write outside the span", len, shift, (long)i);
                    if (dst[i] != src[i]) return fail("a wrong byte", len, shift, (long)i);
                    ++writers[i - shift];
                }
            }
            for (int32_t i = 0; i < len; ++i)
                if (writers[i] != 1) return fail("writers of a byte", len, shift, i);
        }
    std::printf("copy ok\n");
    return 0;
}

// ---- 4. gather and scatter on the mix ----------------------------------------------------------------------------------------------------
struct Mix {
    int32_t n = 0;
    std::vector<MixSkipRec> recs;
    std::vector<int32_t> Z;
    int64_t tot_cw = 0, tot_c_hat = 0, tot_cb = 0, tot_tb = 0;
};

// nrldpc_mix_skip_copy_kernel<SCATTER>, workgroup by workgroup.  cover: one counter per byte of the written array.
static int emulate_copy(const Mix& m, bool scatter, int32_t esize, const std::vector<int32_t>& prefix, const uint8_t* from, uint8_t* to, const int32_t* index,
                        const int32_t* count, const int32_t* iters_dense, int32_t* iters, std::vector<uint8_t>& cover, std::vector<int32_t>& iters_writers) {
    const int T = MIX_SKIP_COPY_THREADS;
    for (int32_t wg = 0; wg < prefix[m.n]; ++wg) {
        const MixSkipWork w = mix_skip_work(prefix.data(), m.recs.data(), m.n, esize, wg);
        if (w.cfg < 0 || w.cfg >= m.n) return fail("configuration out of range", wg, w.cfg);
        const MixSkipRec& c = m.recs[w.cfg];
        const int64_t row_bytes = mix_skip_row_bytes(c, esize);
        if (w.slot < 0 || w.slot >= c.n_cb || w.chunk < 0 || w.chunk >= mix_skip_chunks(row_bytes)) return fail("work item out of range", wg, w.slot, w.chunk);
        const int32_t cnt = count[w.cfg];
        const int32_t* idx = index + c.cb_off;
        const int32_t row = w.slot < cnt ? idx[w.slot] : -1;
        const bool valid = row >= 0 && row < c.n_cb;
        if (w.slot < cnt && !valid) return fail("an index outside its configuration", wg, row);
        if (scatter && iters && w.chunk == 0 && (valid || (w.slot == 0 && cnt == 0))) {
            int32_t lo, hi, lo2, hi2;
            mix_skip_zero_range(idx, cnt, c.n_cb, w.slot, lo, hi, lo2, hi2);
            if (lo < 0 || hi > c.n_cb || lo2 < 0 || hi2 > c.n_cb) return fail("a zero range leaves the configuration", wg, lo, hi);
            for (int t = 0; t < T; ++t) {
                for (int32_t b = lo + t; b < hi; b += T) { iters[c.cb_off + b] = 0; ++iters_writers[c.cb_off + b]; }
                for (int32_t b = lo2 + t; b < hi2; b += T) { iters[c.cb_off + b] = 0; ++iters_writers[c.cb_off + b]; }
            }
            if (valid && iters_dense) { iters[c.cb_off + row] = iters_dense[c.cb_off + w.slot]; ++iters_writers[c.cb_off + row]; }
        }
        if (!valid) continue;
        const int64_t seg = (scatter ? c.c_hat_off : c.cw_off) * esize;
        int64_t lo;
        int32_t len;
        mix_skip_span(row_bytes, w.chunk, lo, len);
        if (len <= 0 || lo + len > row_bytes) return fail("a span leaves its row", wg, (long)lo, len);
        const int64_t full = seg + (int64_t)row * row_bytes + lo, dense = seg + (int64_t)w.slot * row_bytes + lo;
        for (int t = 0; t < T; ++t) mix_skip_copy(from + (scatter ? dense : full), to + (scatter ? full : dense), len, t, T);
        for (int32_t i = 0; i < len; ++i) ++cover[(scatter ? full : dense) + i];
    }
    return 0;
}

static int check_mix(const Mix& m) {
    const int32_t esizes[3] = {MIX_SKIP_ROW_F32, MIX_SKIP_ROW_F16, MIX_SKIP_ROW_HARD};
    long rows = 0;
    for (int kind = 0; kind < 7; ++kind) {
        // the pending pattern, and index / count as the pending kernel leaves them (sentinel-filled: gaps and tails)
        std::vector<int32_t> index(m.tot_cb, -7), count(m.n, -7);
        std::vector<std::vector<uint8_t>> pats;
        for (int i = 0; i < m.n; ++i) {
            const MixSkipRec& c = m.recs[i];
            std::vector<uint8_t> pat = pattern(c.n_cb, kind);
            if (kind == 3 && i != m.n - 1) std::fill(pat.begin(), pat.end(), 0); // only the last row of the last configuration
            count[i] = emulate_pending(c.n_cb, [&](int32_t b) { return pat.at(b) != 0; }, index.data() + c.cb_off);
            pats.push_back(pat);
        }
        for (int e = 0; e < 3; ++e) {
            const int32_t esize = esizes[e];
            const bool scatter = esize == MIX_SKIP_ROW_HARD;
            std::vector<int32_t> prefix(m.n + 1, 0);
            for (int i = 0; i < m.n; ++i) prefix[i + 1] = prefix[i] + m.recs[i].n_cb * mix_skip_chunks(mix_skip_row_bytes(m.recs[i], esize));
            const int64_t total = (scatter ? m.tot_c_hat : m.tot_cw) * esize;
            // exactly the packed size.  `from` holds a value per byte that is never the sentinel 0xEE
            std::vector<uint8_t> from(total), to(total, 0xEE), cover(total, 0);
            for (int64_t k = 0; k < total; ++k) from[k] = (uint8_t)((k * 7 + k / 251) % 0xEE);
            std::vector<int32_t> iters_dense(m.tot_cb, -5), iters(m.tot_cb, -9), iters_writers(m.tot_cb, 0);
            for (int i = 0; i < m.n; ++i)
                for (int32_t j = 0; j < count[i]; ++j) iters_dense[m.recs[i].cb_off + j] = 100 + j;
            if (emulate_copy(m, scatter, esize, prefix, from.data(), to.data(), index.data(), count.data(), iters_dense.data(), scatter ? iters.data() : nullptr,
                             cover, iters_writers))
                return 1;
            std::vector<uint8_t> want(total, 0xEE), want_cover(total, 0);
            std::vector<int32_t> want_iters(m.tot_cb, -9), want_writers(m.tot_cb, 0);
            for (int i = 0; i < m.n; ++i) {
                const MixSkipRec& c = m.recs[i];
                const int64_t rb = mix_skip_row_bytes(c, esize), seg = (scatter ? c.c_hat_off : c.cw_off) * esize;
                int32_t j = 0;
                for (int32_t b = 0; b < c.n_cb; ++b) {
                    if (scatter) { want_iters[c.cb_off + b] = pats[i][b] ? 100 + j : 0; want_writers[c.cb_off + b] = 1; }
                    if (!pats[i][b]) continue;
                    const int64_t src = seg + (scatter ? j : b) * rb, dst = seg + (scatter ? b : j) * rb;
                    std::memcpy(want.data() + dst, from.data() + src, rb);
                    std::memset(want_cover.data() + dst, 1, rb);
                    ++j; ++rows;
                }
            }
            if (to != want) return fail("the written array", kind, esize);
            if (cover != want_cover) return fail("bytes covered other than exactly once", kind, esize);
            if (scatter && (iters != want_iters || iters_writers != want_writers)) return fail("iteration counts", kind, esize);
        }
    }
    std::printf("mix ok: %d configurations, %ld row copies\n", m.n, rows);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: mix_skip_check FILE");
    std::ifstream in(argv[1]);
    Mix m;
    in >> m.n;
    if (!in || m.n < 1) return fail("bad n");
    m.recs.resize(m.n);
    m.Z.resize(m.n);
    for (int i = 0; i < m.n; ++i) {
        MixSkipRec& c = m.recs[i];
        int32_t n_tb;
        c = MixSkipRec{};
        in >> n_tb >> c.C >> m.Z[i] >> c.N_cw >> c.K >> c.cw_off >> c.c_hat_off >> c.cb_off >> c.tb_off;
        if (!in || c.C < 1 || n_tb < 0) return fail("short file", i);
        c.n_cb = n_tb * c.C;
        if (c.N_cw % 4) return fail("N_cw is not a multiple of 4 elements", i, c.N_cw);
    }
    in >> m.tot_cw >> m.tot_c_hat >> m.tot_cb >> m.tot_tb;
    if (!in) return fail("short file (totals)");
    if (m.Z[m.n - 1] != 9 || m.recs[m.n - 1].K != 90 || m.recs[m.n - 1].n_cb < 2) return fail("the last configuration must have Z == 9, K == 90", m.Z[m.n - 1], m.recs[m.n - 1].K);
    if (check_rule() || check_compaction() || check_copy() || check_mix(m)) return 1;
    std::printf("mix_skip_check ok\n");
    return 0;
}

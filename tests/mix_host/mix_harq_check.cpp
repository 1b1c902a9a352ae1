// mix_harq_check.cpp -- stand-alone host check of the flag addressing of the mixed-batch HARQ stages
// (ldpc-3gpp-matlab_amd/csrc/nrldpc_mix.h: mix_new_index, mix_cbgti_index, mix_rm_new_index), meant to be compiled with
// -fsanitize=address,undefined and run on the CPU (tests/test_mix_harq_api.py does that).
//
// Input (a text file, argv[1]): the format of mix_map_check.cpp -- n, then per configuration
//     n_tb C G Z K Kp N N_cb B   E_r[0..C)   and the seven offsets nrldpc_mix_layout gave for it,
// then the seven totals.  The program rebuilds the tables with the header's functions, walks EVERY workgroup of the rate-recovery grid
// and of the CRC grid as the HARQ kernels map them, and reads flag arrays of exactly the packed sizes (d_new: totals.tb bytes, d_cbgti:
// totals.cb bytes) at the indices the kernels form.  Checked: every index lies inside its configuration's segment and names the
// workgroup's own transport block / code block; in the CRC grid every d_new element has exactly one reader (its transport block's
// workgroup) and every d_cbgti element exactly one (its code block's wave); in the rate-recovery grid a transport block's flag is read
// by exactly the C * wg_per_cb workgroups of its code blocks; no gap element is read at all.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "nrldpc_mix.h"

using namespace nrldpc;

struct Cfg {
    int32_t n_tb, C, G, Z, K, Kp, N, N_cb, B;
    int64_t lib_off[MIX_FIELDS];
};

static int fail(const char* what, long a = 0, long b = 0) {
    std::fprintf(stderr, "mix_harq_check: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: mix_harq_check FILE");
    std::ifstream in(argv[1]);
    int32_t n = -1;
    in >> n;
    if (!in || n < 0) return fail("bad n");
    std::vector<Cfg> cfg(n);
    for (auto& c : cfg) {
        in >> c.n_tb >> c.C >> c.G >> c.Z >> c.K >> c.Kp >> c.N >> c.N_cb >> c.B;
        if (!in || c.C < 1) return fail("short file");
        for (int r = 0; r < c.C; ++r) { int32_t e; in >> e; }
        for (int k = 0; k < MIX_FIELDS; ++k) in >> c.lib_off[k];
        if (!in) return fail("short file");
    }
    int64_t lib_tot[MIX_FIELDS];
    for (int k = 0; k < MIX_FIELDS; ++k) in >> lib_tot[k];
    if (!in) return fail("short file (totals)");

    // the tables the plan uploads: records, the two prefix tables, and the tb offsets of the rate-recovery flag addressing
    std::vector<MixRmRec> recs(n);
    std::vector<int32_t> rm_prefix(n + 1, 0), tb_prefix(n + 1, 0);
    std::vector<int64_t> tb_offs(n, 0), cb_offs(n, 0);
    int64_t tb_cur = 0, cb_cur = 0;
    for (int i = 0; i < n; ++i) {
        const Cfg& c = cfg[i];
        const int32_t ncwz = 2 * c.Z + c.N;
        int64_t s[MIX_FIELDS];
        mix_sizes(c.n_tb, c.C, c.G, c.N_cb, ncwz, c.K, c.B, s);
        if (tb_cur != c.lib_off[MIX_TB] || cb_cur != c.lib_off[MIX_CB]) return fail("library offset differs from the header's rule", i);
        tb_offs[i] = tb_cur; cb_offs[i] = cb_cur;
        tb_cur = mix_round_up(tb_cur + s[MIX_TB]);
        cb_cur = mix_round_up(cb_cur + s[MIX_CB]);
        MixRmRec& r = recs[i];
        r = MixRmRec{};
        r.n_tb = c.n_tb; r.C = c.C; r.G = c.G; r.Z = c.Z; r.K = c.K; r.Kp = c.Kp; r.N = c.N; r.N_cb = c.N_cb;
        r.wg_per_cb = mix_rm_wg_per_cb(ncwz);
        rm_prefix[i + 1] = rm_prefix[i] + c.n_tb * c.C * r.wg_per_cb;
        tb_prefix[i + 1] = tb_prefix[i] + c.n_tb;
    }
    if (tb_cur != lib_tot[MIX_TB] || cb_cur != lib_tot[MIX_CB]) return fail("library totals differ from the header's rule");

    // flag arrays of exactly the packed sizes, and one read counter per element
    const std::vector<uint8_t> d_new(tb_cur, 1), d_cbgti(cb_cur, 1);
    std::vector<int32_t> new_rm(tb_cur, 0), new_crc(tb_cur, 0), cbgti_crc(cb_cur, 0);
    long sum = 0;

    // ---- the rate-recovery grid: one flag read per workgroup (nrldpc_mix_rate_recover_kernel<..., true>)
    for (int32_t wg = 0; wg < rm_prefix[n]; ++wg) {
        const MixRmWork w = mix_rm_work(rm_prefix.data(), recs.data(), n, wg);
        if (w.cfg < 0 || w.cfg >= n) return fail("configuration out of range", wg, w.cfg);
        const MixRmRec& c = recs[w.cfg];
        if (c.n_tb <= 0) return fail("a workgroup landed on an empty configuration", wg, w.cfg);
        if (w.blk < 0 || w.blk >= c.n_tb * c.C) return fail("code block out of range", wg, w.blk);
        const int64_t k = mix_rm_new_index(tb_offs.data(), recs.data(), w);
        if (k < tb_offs[w.cfg] || k >= tb_offs[w.cfg] + c.n_tb) return fail("d_new index leaves its segment (rate recovery)", wg, (long)k);
        if (k != tb_offs[w.cfg] + w.blk / c.C) return fail("d_new index is not the workgroup's transport block", wg, (long)k);
        sum += d_new.at(k);
        ++new_rm.at(k);
    }
    // ---- the CRC grid: one d_new read per workgroup, one d_cbgti read per code block (nrldpc_mix_crc_check_kernel<true>)
    for (int32_t wg = 0; wg < tb_prefix[n]; ++wg) {
        const int32_t i = mix_find(tb_prefix.data(), n, wg);
        if (i < 0 || i >= n) return fail("configuration out of range (CRC)", wg, i);
        const Cfg& c = cfg[i];
        const int32_t tb = wg - tb_prefix[i];
        if (tb < 0 || tb >= c.n_tb) return fail("transport block out of range", wg, tb);
        const int64_t k = mix_new_index(tb_offs[i], tb);
        if (k < tb_offs[i] || k >= tb_offs[i] + c.n_tb) return fail("d_new index leaves its segment (CRC)", wg, (long)k);
        sum += d_new.at(k);
        ++new_crc.at(k);
        for (int waves = 1; waves <= 4; ++waves) { // every workgroup shape the launch may pick: wave w takes r = w, w + waves, ...
            for (int wave = 0; wave < waves; ++wave)
                for (int r = wave; r < c.C; r += waves) {
                    const int64_t q = mix_cbgti_index(cb_offs[i], c.C, tb, r);
                    if (q < cb_offs[i] || q >= cb_offs[i] + (int64_t)c.n_tb * c.C) return fail("d_cbgti index leaves its segment", wg, (long)q);
                    if (q != cb_offs[i] + (int64_t)tb * c.C + r) return fail("d_cbgti index is not the wave's code block", wg, (long)q);
                    sum += d_cbgti.at(q);
                    if (waves == 1) ++cbgti_crc.at(q);
                }
        }
    }
    // ---- readers per element: segments exactly as stated above, gaps never
    std::vector<int32_t> want_rm(tb_cur, 0), want_tb(tb_cur, 0), want_cb(cb_cur, 0);
    for (int i = 0; i < n; ++i)
        for (int32_t tb = 0; tb < cfg[i].n_tb; ++tb) {
            want_rm.at(tb_offs[i] + tb) = cfg[i].C * recs[i].wg_per_cb;
            want_tb.at(tb_offs[i] + tb) = 1;
            for (int r = 0; r < cfg[i].C; ++r) want_cb.at(cb_offs[i] + (int64_t)tb * cfg[i].C + r) = 1;
        }
    for (int64_t k = 0; k < tb_cur; ++k) {
        if (new_rm[k] != want_rm[k]) return fail("d_new readers in the rate-recovery grid", (long)k, new_rm[k]);
        if (new_crc[k] != want_tb[k]) return fail("d_new readers in the CRC grid", (long)k, new_crc[k]);
    }
    for (int64_t k = 0; k < cb_cur; ++k)
        if (cbgti_crc[k] != want_cb[k]) return fail("d_cbgti readers", (long)k, cbgti_crc[k]);
    std::printf("mix_harq_check ok: %d configurations, %d + %d workgroups, %ld flag reads\n", n, rm_prefix[n], tb_prefix[n], sum);
    return 0;
}

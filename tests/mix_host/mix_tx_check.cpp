// mix_tx_check.cpp -- stand-alone host check of the transmit-side mixed-batch stages' layout arithmetic and workgroup mapping
// (ldpc-3gpp-matlab_amd/csrc/nrldpc_mix_tx.h), meant to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_mix_tx_api.py does that): an out-of-range index in a table-driven kernel is a fault on the device.
//
// Input (a text file, argv[1]): n, then per configuration
//     n_tb C G Z K Kp N N_cb A B Lcb k0 Qm   E_r[0..C)   and the four offsets the library gave for it (a, c = c_hat, cw, g),
// then the four totals (entry [n]).  The program rebuilds the offsets, the records and the two prefix tables with the header's
// functions, walks EVERY workgroup, wave and thread of both grids exactly as nrldpc_mix_tx_rate_match_kernel and
// nrldpc_mix_tx_crc_attach_kernel map them, touches arrays of exactly the packed sizes at the addresses the kernels would form, and
// checks:
//   rate matching  every byte of a g segment has exactly one writer, no gap byte is touched, every read lies inside its code block's
//                  [2Z, 2Z + N_cb) range, a workgroup past a block's own rows does nothing;
//   attach         every byte of a c segment has exactly one writer, every byte of an `a` segment is read once and inside its own
//                  row, every LDS row index (whatever the 16-byte phase of the source) lies inside the wave's plan-wide stride,
//                  part[] indices are below the plan's largest C and inside the workgroup's LDS, the last block is finished by the
//                  wave that staged it;
//   layout         the library's offsets are the header's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "nrldpc_mix_tx.h"
#include "nrldpc_rm_core.h"

using namespace nrldpc;

struct Cfg {
    int32_t n_tb, C, G, Z, K, Kp, N, N_cb, A, B, Lcb, k0, Qm;
    std::vector<int32_t> E, off;
    int64_t lib_off[4]; // a, c, cw, g
};

static int fail(const char* what, long a = 0, long b = 0) {
    std::fprintf(stderr, "mix_tx_check: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: mix_tx_check FILE");
    std::ifstream in(argv[1]);
    int32_t n = -1;
    in >> n;
    if (!in || n < 0) return fail("bad n");
    std::vector<Cfg> cfg(n);
    for (auto& c : cfg) {
        in >> c.n_tb >> c.C >> c.G >> c.Z >> c.K >> c.Kp >> c.N >> c.N_cb >> c.A >> c.B >> c.Lcb >> c.k0 >> c.Qm;
        if (!in || c.C < 1 || c.Qm < 1) return fail("short file");
        c.E.resize(c.C); c.off.resize(c.C);
        int32_t o = 0;
        for (int r = 0; r < c.C; ++r) { in >> c.E[r]; c.off[r] = o; o += c.E[r]; }
        for (int k = 0; k < 4; ++k) in >> c.lib_off[k];
        if (!in) return fail("short file");
        if (o != c.G) return fail("sum(E_r) != G");
    }
    int64_t lib_tot[4];
    for (int k = 0; k < 4; ++k) in >> lib_tot[k];
    if (!in) return fail("short file (totals)");

    // ---- layout and tables, by the header's rules, against what the library reported
    std::vector<int64_t> a_off(n + 1, 0), c_off(n + 1, 0), cw_off(n + 1, 0), g_off(n + 1, 0);
    std::vector<MixTxRmRec> rm(n);
    std::vector<MixTxCrcGeom> crc(n);
    std::vector<int32_t> rm_prefix(n + 1, 0), tb_prefix(n + 1, 0), e_tab, off_tab;
    int32_t k_max = 0, c_max = 0;
    for (int i = 0; i < n; ++i) {
        const Cfg& c = cfg[i];
        const int32_t ncwz = 2 * c.Z + c.N;
        int64_t s[MIX_FIELDS];
        mix_sizes(c.n_tb, c.C, c.G, c.N_cb, ncwz, c.K, c.B, s);
        const int64_t here[4] = {a_off[i], c_off[i], cw_off[i], g_off[i]};
        for (int k = 0; k < 4; ++k) {
            if (here[k] != c.lib_off[k]) return fail("library offset differs from the header's rule", i, k);
            if (here[k] % MIX_ALIGN) return fail("segment not aligned", i, k);
        }
        a_off[i + 1] = mix_tx_a_next(a_off[i], c.n_tb, c.A);
        c_off[i + 1] = mix_round_up(c_off[i] + s[MIX_C_HAT]);
        cw_off[i + 1] = mix_round_up(cw_off[i] + s[MIX_CW]);
        g_off[i + 1] = mix_round_up(g_off[i] + s[MIX_G]);
        MixTxRmRec& r = rm[i];
        r = MixTxRmRec{};
        r.cw_off = cw_off[i]; r.g_off = g_off[i];
        r.n_tb = c.n_tb; r.C = c.C; r.G = c.G; r.Z = c.Z; r.K = c.K; r.Kp = c.Kp; r.N = c.N; r.N_cb = c.N_cb; r.k0 = c.k0; r.Qm = c.Qm;
        r.e_base = (int32_t)e_tab.size();
        int32_t e_max = 0;
        for (int b = 0; b < c.C; ++b) { e_tab.push_back(c.E[b]); off_tab.push_back(c.off[b]); e_max = c.E[b] > e_max ? c.E[b] : e_max; }
        r.wg_per_cb = mix_tx_rm_wg_per_cb(e_max, c.Qm);
        rm_prefix[i + 1] = rm_prefix[i] + c.n_tb * c.C * r.wg_per_cb;
        tb_prefix[i + 1] = tb_prefix[i] + c.n_tb;
        MixTxCrcGeom& q = crc[i];
        q = MixTxCrcGeom{};
        q.a_off = a_off[i]; q.c_off = c_off[i];
        q.C = c.C; q.K = c.K; q.Kp = c.Kp; q.Lcb = c.Lcb; q.A = c.A; q.B = c.B;
        if (c.n_tb > 0) { k_max = c.K > k_max ? c.K : k_max; c_max = c.C > c_max ? c.C : c_max; }
    }
    const int64_t tot[4] = {a_off[n], c_off[n], cw_off[n], g_off[n]};
    for (int k = 0; k < 4; ++k)
        if (tot[k] != lib_tot[k]) return fail("library totals differ from the header's rule", k);

    // arrays of exactly the packed sizes: one counter per element
    std::vector<uint8_t> a(tot[0], 0), cb(tot[1], 0), cw(tot[2], 0), g(tot[3], 0);

    // ---- the rate-matching grid, as nrldpc_mix_tx_rate_match_kernel maps it
    long idle_wg = 0, live_threads = 0;
    for (int32_t wg = 0; wg < rm_prefix[n]; ++wg) {
        const MixTxRmWork w = mix_tx_rm_work(rm_prefix.data(), rm.data(), n, wg);
        if (w.cfg < 0 || w.cfg >= n) return fail("configuration out of range", wg, w.cfg);
        const MixTxRmRec& c = rm[w.cfg];
        if (c.n_tb <= 0 || c.G <= 0) return fail("a workgroup landed on a configuration without bits", wg, w.cfg);
        if (w.blk < 0 || w.blk >= c.n_tb * c.C) return fail("code block out of range", wg, w.blk);
        if (w.j_wg < 0 || w.j_wg % MIX_TX_RM_WG) return fail("bad first column", wg, w.j_wg);
        const int32_t tb = w.blk / c.C, r = w.blk - tb * c.C;
        const int32_t E = e_tab.at(c.e_base + r), QM = c.Qm, rows = E / QM;
        const RmGeom geo(c.Z, c.K, c.Kp, c.N_cb, c.k0);
        const int64_t cw0 = mix_tx_rm_cw_index(c, w.blk);            // position 0 of d
        const int64_t blk_lo = c.cw_off + (int64_t)w.blk * (2 * c.Z + c.N);
        if (cw0 != blk_lo + 2 * c.Z) return fail("d does not start behind the punctured columns", wg);
        const int64_t g0 = mix_tx_rm_g_index(c, tb, off_tab.at(c.e_base + r));
        if (g0 < c.g_off + (int64_t)tb * c.G || g0 + E > c.g_off + (int64_t)(tb + 1) * c.G) return fail("g block leaves its row", wg);
        bool any = false;
        for (int thread = 0; thread < 256; ++thread) {
            const int32_t j0 = mix_tx_rm_j0(w, thread);
            if (j0 >= rows) continue; // the thread returns
            any = true;
            ++live_threads;
            const int nj = rows - j0 < 4 ? rows - j0 : 4;
            const bool rep = E > geo.P;
            auto read = [&](int64_t d) -> int { // one byte of d
                if (d < 0 || d >= c.N_cb) return fail("read outside the circular buffer", wg, (long)d);
                (void)cw.at(cw0 + d);
                return 0;
            };
            for (int i = 0; i < QM; ++i) {
                const int k = i * rows + j0;
                int q, kend;
                if (rep) { const int d = k / geo.P; q = k - d * geo.P + geo.nfk0; kend = geo.P * (d + 1); }
                else { q = k + geo.nfk0; kend = geo.P; }
                if (q >= geo.P) q -= geo.P;
                if (nj == 4 && k + 3 < kend && q + 3 < geo.P && (q >= geo.lo_f || q + 3 < geo.lo_f)) {
                    const int d0 = q < geo.lo_f ? q : q + geo.F;
                    for (int t = 0; t < 4; ++t)
                        if (read(d0 + t)) return 1;
                } else {
                    for (int t = 0; t < nj; ++t) {
                        const int kk = k + t;
                        int qq = (rep ? kk % geo.P : kk) + geo.nfk0;
                        if (qq >= geo.P) qq -= geo.P;
                        if (read(qq < geo.lo_f ? qq : qq + geo.F)) return 1;
                    }
                }
            }
            const int64_t gt = g0 + (int64_t)j0 * QM;
            for (int ob = 0; ob < nj * QM; ++ob) ++g.at(gt + ob);
        }
        if (!any) {
            ++idle_wg;
            if (w.j_wg < rows) return fail("an idle workgroup inside the block's rows", wg);
        }
    }
    // ---- the attach grid, as nrldpc_mix_tx_crc_attach_kernel maps it
    const int32_t nw = mix_tx_waves(c_max), cap = mix_tx_row_capacity(k_max);
    const int64_t lds_bytes = mix_tx_lds_bytes(nw, k_max, c_max);
    if (cap % 16) return fail("LDS row stride not 16-byte aligned", cap);
    for (int32_t wg = 0; wg < tb_prefix[n]; ++wg) {
        const int32_t i = mix_find(tb_prefix.data(), n, wg);
        if (i < 0 || i >= n) return fail("configuration out of range (attach)", wg, i);
        const MixTxCrcGeom& c = crc[i];
        const int32_t tb = wg - tb_prefix[i];
        if (tb < 0 || tb >= cfg[i].n_tb) return fail("transport block out of range", wg, tb);
        const int32_t pay = mix_tx_pay(c), Ltb = c.B - c.A;
        if (pay < Ltb || c.C * pay != c.B) return fail("payload sizes", wg);
        int32_t staged_last = -1;
        for (int wave = 0; wave < nw; ++wave) {
            for (int r = wave; r < c.C; r += nw) {
                const int32_t seg = mix_tx_seg(c, r);
                const int64_t src = mix_tx_a_index(c, tb, r);
                if (seg < 0 || src < c.a_off + (int64_t)tb * c.A || src + seg > c.a_off + (int64_t)(tb + 1) * c.A) return fail("read of `a` leaves its row", wg, r);
                for (int k = 0; k < seg; ++k) ++a.at(src + k);
                // the LDS row: stage_row places it at the source's 16-byte phase (any base address: every phase), the row grows to K
                // bytes (CRC bits, fillers) and store_row reads up to 4 bytes past byte K - 1
                for (int sh = 0; sh < 16; ++sh)
                    if ((int64_t)wave * cap + sh + c.K + 4 > (int64_t)(wave + 1) * cap) return fail("LDS row leaves the wave's stride", wg, sh);
                if (r >= c_max || mix_tx_part_byte(nw, k_max, r) + 4 > lds_bytes || mix_tx_part_byte(nw, k_max, r) < (int64_t)nw * cap) return fail("part[] index", wg, r);
                const int64_t dst = mix_tx_c_index(c, tb, r);
                for (int k = 0; k < c.K; ++k) ++cb.at(dst + k);
                if (r == c.C - 1) staged_last = wave;
            }
        }
        if (staged_last != mix_tx_last_wave(c, nw)) return fail("the last block is not finished by the wave that staged it", wg, staged_last);
    }
    // ---- every element of every segment exactly once, no gap element at all (cw is only read: in range is what counts)
    auto owned = [&](const std::vector<uint8_t>& v, const std::vector<int64_t>& off, int which, const char* name) -> int {
        std::vector<uint8_t> want(v.size(), 0);
        for (int i = 0; i < n; ++i) {
            const Cfg& c = cfg[i];
            const int64_t size = which == 0 ? (int64_t)c.n_tb * c.A : which == 1 ? (int64_t)c.n_tb * c.C * c.K : (int64_t)c.n_tb * c.G;
            for (int64_t k = 0; k < size; ++k) want.at(off[i] + k) = 1;
        }
        for (size_t k = 0; k < v.size(); ++k)
            if (v[k] != want[k]) { std::fprintf(stderr, "mix_tx_check: %s element %zu touched %d times, expected %d\n", name, k, v[k], want[k]); return 1; }
        return 0;
    };
    if (owned(a, a_off, 0, "a") || owned(cb, c_off, 1, "c") || owned(g, g_off, 2, "g")) return 1;
    std::printf("mix_tx_check ok: %d configurations, %d + %d workgroups, %ld live threads, %ld idle workgroups, %d waves, LDS %ld\n", n, rm_prefix[n],
                tb_prefix[n], live_threads, idle_wg, nw, (long)lds_bytes);
    return 0;
}

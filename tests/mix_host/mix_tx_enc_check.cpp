// mix_tx_enc_check.cpp -- stand-alone host check of the one-launch mixed encoder's records, workgroup mapping and LDS carve-up
// (ldpc-3gpp-matlab_amd/csrc/nrldpc_mix_tx.h), meant to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_mix_tx_encode_api.py does that): an out-of-range index in a table-driven kernel is a fault on the device.
//
// Input (a text file, argv[1]): n, then per configuration
//     n_tb C BG Z K N   and the two offsets the library gave for it (c = c_hat, cw),
// then the two totals (entry [n]), then a count and that many (info, out) byte offsets of the two base pointers above a 16-byte
// boundary.  The program rebuilds the records, the table placement, the workgroup prefix and the launch's LDS size with the header's
// functions, walks EVERY workgroup and wave of the grid exactly as nrldpc_mix_tx_encode_kernel maps them -- and every thread of the
// three phases that store to the output, with the alignment decisions of the kernel taken on the real addresses -- on arrays of
// exactly the packed sizes, and checks:
//   mapping   every codeword of every configuration is served exactly once (by one wave, or by the four waves of one workgroup), a
//             wave without a codeword occurs only in the last workgroup of its configuration;
//   reads     the K = kb*Z bytes read lie inside the codeword's own code block;
//   writes    the ncols*Z bytes written are the codeword's own, each byte by exactly one thread, no gap byte touched;
//   LDS       the table fits its words, each slot's region -- carved with its own configuration's layout -- lies inside the launch's
//             size, the regions inside a slot do not overlap, every 32-bit window of the doubled ring lies inside its column;
//   tables    the offsets of every (BG, Z_c) lie inside the table bytes, 16-byte aligned, shared by configurations of the same
//             (BG, Z_c) and disjoint otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "nr_bg_tables.h"
#include "nrldpc_mix_tx.h"

using namespace nrldpc;

struct Cfg {
    int32_t n_tb, C, bg, Z, K, N;
    int64_t lib_off[2]; // c, cw
};

static int fail(const char* what, long a = 0, long b = 0) {
    std::fprintf(stderr, "mix_tx_enc_check: %s (%ld, %ld)\n", what, a, b);
    return 1;
}

static int set_index(int Z) {
    for (int s = 0; s < 8; ++s)
        for (int k = 0; k < 9 && nr_lifting_sets[s][k]; ++k)
            if (nr_lifting_sets[s][k] == Z) return s;
    return -1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: mix_tx_enc_check FILE");
    std::ifstream in(argv[1]);
    int32_t n = -1;
    in >> n;
    if (!in || n < 0) return fail("bad n");
    std::vector<Cfg> cfg(n);
    for (auto& c : cfg) {
        in >> c.n_tb >> c.C >> c.bg >> c.Z >> c.K >> c.N >> c.lib_off[0] >> c.lib_off[1];
        if (!in || c.C < 1 || (c.bg != 1 && c.bg != 2) || c.n_tb < 0) return fail("short file");
    }
    int64_t lib_tot[2];
    in >> lib_tot[0] >> lib_tot[1];
    int32_t n_pairs = 0;
    in >> n_pairs;
    if (!in || n_pairs < 1) return fail("short file (totals, offsets)");
    std::vector<int32_t> io(n_pairs), oo(n_pairs);
    for (int k = 0; k < n_pairs; ++k) in >> io[k] >> oo[k];
    if (!in) return fail("short file (offsets)");

    // ---- records, tables, prefix and the LDS size by the header's rules
    std::vector<int64_t> c_off(n + 1, 0), cw_off(n + 1, 0);
    std::vector<MixTxEncRec> rec(n);
    std::vector<int32_t> prefix(n + 1, 0), first; // first: the first configuration of each distinct (BG, Z_c)
    int32_t tab_bytes = 0;
    int64_t lds_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const Cfg& c = cfg[i];
        const bool b1 = c.bg == 1;
        const int32_t kb = b1 ? 22 : 10, nrows = b1 ? NR_BG1_ROWS : NR_BG2_ROWS, ncols = b1 ? NR_BG1_COLS : NR_BG2_COLS, nnz = b1 ? NR_BG1_NNZ : NR_BG2_NNZ;
        if (c.K != kb * c.Z || 2 * c.Z + c.N != ncols * c.Z) return fail("K or N is not the base graph's", i);
        if (c_off[i] != c.lib_off[0] || cw_off[i] != c.lib_off[1]) return fail("library offset differs from the header's rule", i);
        if (c_off[i] % MIX_ALIGN || cw_off[i] % MIX_ALIGN) return fail("segment not aligned", i);
        int64_t s[MIX_FIELDS];
        mix_sizes(c.n_tb, c.C, 0, 0, 2 * c.Z + c.N, c.K, 0, s);
        c_off[i + 1] = mix_round_up(c_off[i] + s[MIX_C_HAT]);
        cw_off[i + 1] = mix_round_up(cw_off[i] + s[MIX_CW]);
        MixTxEncRec& r = rec[i];
        r = MixTxEncRec{};
        r.c_off = c_off[i]; r.cw_off = cw_off[i];
        r.n_cw = c.n_tb * c.C;
        r.nwc = mix_tx_enc_nwc(c.bg, c.Z);
        prefix[i + 1] = prefix[i] + mix_tx_enc_wgs(r.n_cw, r.nwc);
        if (r.n_cw == 0) continue; // no workgroup: the record is never read
        r.Z = c.Z; r.kb = kb; r.nrows = nrows; r.ncols = ncols; r.nnz = nnz;
        const MixTxEncLayout L = mix_tx_enc_layout(r.Z, r.kb, r.nrows, r.nnz);
        const int64_t lds = mix_tx_enc_lds_bytes(L, r.nwc);
        lds_bytes = lds > lds_bytes ? lds : lds_bytes;
        bool shared = false;
        for (int32_t k : first)
            if (rec[k].kb == r.kb && rec[k].Z == r.Z) { r.row_ptr_off = rec[k].row_ptr_off; r.shift_off = rec[k].shift_off; r.col_off = rec[k].col_off; shared = true; }
        if (!shared) {
            mix_tx_enc_tab_place(tab_bytes, r);
            tab_bytes += mix_tx_enc_tab_bytes(r.nrows, r.nnz);
            first.push_back(i);
        }
    }
    if (c_off[n] != lib_tot[0] || cw_off[n] != lib_tot[1]) return fail("library totals differ from the header's rule");
    if (lds_bytes > 64 * 1024) return fail("the launch's LDS exceeds a workgroup's", (long)lds_bytes);

    // ---- tables: inside the bytes, aligned, disjoint between distinct (BG, Z_c)
    std::vector<uint8_t> tab(tab_bytes, 0);
    for (int32_t k : first) {
        const MixTxEncRec& r = rec[k];
        if (r.row_ptr_off % 16 || r.shift_off % 16 || r.col_off % 16) return fail("table not 16-byte aligned", k);
        for (int b = 0; b < 2 * (r.nrows + 1); ++b) ++tab.at(r.row_ptr_off + b);
        for (int b = 0; b < 2 * r.nnz; ++b) ++tab.at(r.shift_off + b);
        for (int b = 0; b < r.nnz; ++b) ++tab.at(r.col_off + b);
    }
    for (size_t b = 0; b < tab.size(); ++b)
        if (tab[b] > 1) return fail("two tables overlap", (long)b);
    for (int i = 0; i < n; ++i) {
        const MixTxEncRec& r = rec[i];
        if (r.n_cw == 0) continue;
        (void)tab.at(r.row_ptr_off + 2 * (r.nrows + 1) - 1); (void)tab.at(r.shift_off + 2 * r.nnz - 1); (void)tab.at(r.col_off + r.nnz - 1);
    }

    // ---- LDS of every non-empty configuration, inside the plan-wide size
    for (int i = 0; i < n; ++i) {
        const MixTxEncRec& r = rec[i];
        if (r.n_cw == 0) continue;
        const MixTxEncLayout L = mix_tx_enc_layout(r.Z, r.kb, r.nrows, r.nnz);
        if (r.nnz + r.nrows + 1 > L.tab || L.tab % 4) return fail("the table leaves its LDS words", i);
        if (L.D != 0 || L.D + (r.kb + 4) * L.DW > L.lam || L.lam + 4 * L.W > L.PP || L.PP + (r.nrows - 4) * L.W > L.xc) return fail("regions of a slot overlap", i);
        // xc: 4*Z bytes, and store_row reads up to 4 bytes past its last one
        if (4 * (int64_t)L.xc + 4 * r.Z + 4 > 4 * (int64_t)L.wave_words || L.wave_words % 4) return fail("xc leaves the slot", i);
        for (int slot = 0; slot < mix_tx_enc_per_wg(r.nwc); ++slot)
            if (mix_tx_enc_slot_word(L, slot) < L.tab || 4 * (mix_tx_enc_slot_word(L, slot) + L.wave_words) > lds_bytes) return fail("a slot's region leaves the launch's LDS", i, slot);
        // every 32-bit window of the doubled ring: words (s >> 5) and (s >> 5) + 1 of a column, s = 32 m + shift mod Z
        const int ils = set_index(r.Z);
        if (ils < 0) return fail("not a lifting size", i);
        for (int e = 0; e < r.nnz; ++e) {
            const int sh = (cfg[i].bg == 1 ? nr_bg1_shift[ils][e] : nr_bg2_shift[ils][e]) % r.Z;
            const int s = 32 * (L.W - 1) + sh;
            if ((s >> 5) + 1 >= L.DW) return fail("a ring window leaves its column", i, e);
        }
        // the ballots of a column fill DW / 2 pairs of words; the word build fills words m, m + W, ... < DW: every word a window reads
        if (L.DW % 2 || 32 * L.DW < 2 * r.Z + 32) return fail("doubled ring too short", i);
    }

    // ---- the grid
    std::vector<uint8_t> cb(c_off[n], 0), cw(cw_off[n], 0);
    std::vector<std::vector<int32_t>> served(n);
    for (int i = 0; i < n; ++i) served[i].assign(rec[i].n_cw, 0);
    long idle_waves = 0;
    for (int32_t wg = 0; wg < prefix[n]; ++wg) {
        int32_t cw0 = -2;
        for (int wave = 0; wave < MIX_TX_ENC_WAVES; ++wave) {
            const MixTxEncWork w = mix_tx_enc_work(prefix.data(), rec.data(), n, wg, wave);
            if (w.cfg < 0 || w.cfg >= n) return fail("configuration out of range", wg, w.cfg);
            const MixTxEncRec& r = rec[w.cfg];
            if (r.n_cw <= 0) return fail("a workgroup landed on a configuration without codewords", wg, w.cfg);
            if (w.cw < 0) {
                if (wg != prefix[w.cfg + 1] - 1) return fail("a wave without a codeword before the configuration's last workgroup", wg, wave);
                if (r.nwc == MIX_TX_ENC_WAVES) return fail("a whole workgroup without a codeword", wg);
                ++idle_waves;
                continue;
            }
            if (w.cw >= r.n_cw) return fail("codeword out of range", wg, w.cw);
            const int NWC = r.nwc, GT = 64 * NWC, wv = wave % NWC;
            if (wv == 0) { cw0 = w.cw; ++served[w.cfg][w.cw]; }
            else if (w.cw != cw0) return fail("the waves of a workgroup-wide codeword disagree", wg, wave);
            const int Z = r.Z, kb = r.kb;
            const int64_t info = mix_tx_enc_info_index(r, w.cw), out = mix_tx_enc_out_index(r, w.cw);
            if (info < r.c_off + (int64_t)w.cw * cfg[w.cfg].K || info + kb * Z > r.c_off + (int64_t)(w.cw + 1) * cfg[w.cfg].K) return fail("the read leaves the code block", wg, wave);
            if (out != r.cw_off + (int64_t)w.cw * (2 * Z + cfg[w.cfg].N)) return fail("the output is not the codeword's", wg, wave);
            for (int pair = 0; pair < n_pairs; ++pair) {
                const int64_t ia = io[pair] + info, oa = oo[pair] + out; // the real addresses modulo 16
                for (int lane = 0; lane < 64; ++lane) {
                    const int gl = wv * 64 + lane;
                    // 1. systematic copy
                    const int nsys = kb * Z;
                    const int64_t al = ia | oa;
                    int done = 0;
                    if ((al & 15) == 0) {
                        for (int i = gl; i < (nsys >> 4); i += GT)
                            for (int b = 0; b < 16; ++b) { (void)cb.at(info + 16 * i + b); ++cw.at(out + 16 * i + b); }
                        done = nsys & ~15;
                    } else if ((al & 3) == 0) {
                        for (int i = gl; i < (nsys >> 2); i += GT)
                            for (int b = 0; b < 4; ++b) { (void)cb.at(info + 4 * i + b); ++cw.at(out + 4 * i + b); }
                        done = nsys & ~3;
                    }
                    for (int i = done + gl; i < nsys; i += GT) { (void)cb.at(info + i); ++cw.at(out + i); }
                    // 4. extension parity
                    const int next = r.nrows - 4;
                    const int64_t ext = out + (int64_t)(kb + 4) * Z;
                    if ((Z & 3) == 0 && ((oo[pair] + ext) & 3) == 0) {
                        for (int o = 4 * gl; o < next * Z; o += 4 * GT)
                            for (int b = 0; b < 4; ++b) ++cw.at(ext + o + b);
                    } else {
                        for (int o = gl; o < next * Z; o += GT) ++cw.at(ext + o);
                    }
                }
                // the core parity: store_row writes exactly its n bytes (head, 16-byte body, tail), a wave per call
                if (NWC == 1) for (int b = 0; b < 4 * Z; ++b) ++cw.at(out + (int64_t)kb * Z + b);
                else for (int b = 0; b < Z; ++b) ++cw.at(out + (int64_t)(kb + wv) * Z + b);
            }
        }
    }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < rec[i].n_cw; ++k)
            if (served[i][k] != 1) return fail("a codeword is not served exactly once", i, k);
    // every byte of every codeword segment once per offset pair, no gap byte at all
    std::vector<uint8_t> want(cw.size(), 0);
    for (int i = 0; i < n; ++i)
        for (int64_t k = 0; k < (int64_t)rec[i].n_cw * (2 * cfg[i].Z + cfg[i].N); ++k) want.at(cw_off[i] + k) = (uint8_t)n_pairs;
    for (size_t k = 0; k < cw.size(); ++k)
        if (cw[k] != want[k]) { std::fprintf(stderr, "mix_tx_enc_check: cw element %zu written %d times, expected %d\n", k, cw[k], want[k]); return 1; }
    std::printf("mix_tx_enc_check ok: %d configurations, %d workgroups, %ld idle waves, %zu tables in %d bytes, LDS %ld\n", n, prefix[n], idle_waves,
                first.size(), tab_bytes, (long)lds_bytes);
    return 0;
}

// mix_chan_check.cpp -- stand-alone host check of the mixed-batch channel leg's layout arithmetic and workgroup mappings
// (ldpc-3gpp-matlab_amd/csrc/nrldpc_mix_chan.h), meant to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_mix_chan_api.py does that): an out-of-range index in a table-driven kernel is a fault on the device.
//
// Input (a text file, argv[1]): n, then per configuration
//     n_tb G Qm first_symbol   and the two offsets the library gave for it (g of nrldpc_mix_layout, sym of nrldpc_mix_chan_layout),
// then the two totals (entry [n]).  The program rebuilds the offsets, the records and the two prefix tables with the header's functions,
// walks EVERY workgroup and thread of both grids exactly as the four kernels map them, touches arrays of exactly the packed sizes at
// the indices the kernels dereference, and checks:
//   modem grid  (mapper, demapper) every bit / output element of a g segment, every symbol and every per-symbol variance has exactly
//               one owner, no gap element and no index outside the arrays is touched, a thread's symbols are consecutive and a
//               surplus thread of a configuration's last workgroup owns nothing;
//   pair grid   (fused stage, stand-alone noise) the same for symbols, variances and the fused stage's bits / LLRs, for the given
//               first_symbol of every configuration AND for the other parity (first_symbol ^ 1): the symbol with global index x is
//               served by Philox counter x >> 1 and word pair x & 1, also where the counter crosses 2^32; surplus threads -- the
//               plan sizes a configuration for n_sym / 2 + 1 pairs, whatever the parity -- own nothing;
//   layout      the library's offsets are the header's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "nrldpc_mix_chan.h"

using namespace nrldpc;

struct Cfg {
    int64_t n_tb, G;
    int32_t Qm;
    uint64_t first;
    int64_t lib_g, lib_sym;
};

static int fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "mix_chan_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

// one owner more of element i of an array of exactly the packed size (heap memory: the address sanitizer sees a stray index too)
static bool own(std::vector<uint8_t>& a, int64_t i) {
    if (i < 0 || i >= (int64_t)a.size()) return false;
    if (a[(size_t)i] == 255) return false;
    ++a[(size_t)i];
    return true;
}

// every element of every segment has exactly one owner, every gap element none
static int exactly_once(const std::vector<uint8_t>& a, const std::vector<int64_t>& off, const std::vector<int64_t>& len, const char* what) {
    std::vector<uint8_t> want(a.size(), 0);
    for (size_t i = 0; i < len.size(); ++i)
        for (int64_t k = 0; k < len[i]; ++k) want[(size_t)(off[i] + k)] = 1;
    for (size_t k = 0; k < a.size(); ++k)
        if (a[k] != want[k]) return fail(what, (long long)k, a[k]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: mix_chan_check FILE");
    std::ifstream in(argv[1]);
    int32_t n = -1;
    in >> n;
    if (!in || n < 0) return fail("bad n");
    std::vector<Cfg> cfg(n);
    for (auto& c : cfg) {
        in >> c.n_tb >> c.G >> c.Qm >> c.first >> c.lib_g >> c.lib_sym;
        if (!in || c.Qm < 1 || c.n_tb < 0 || c.G < 0) return fail("short file");
        if ((c.n_tb * c.G) % c.Qm) return fail("bits are no multiple of Q_m");
    }
    int64_t lib_tot_g = 0, lib_tot_sym = 0;
    in >> lib_tot_g >> lib_tot_sym;
    if (!in) return fail("short file (totals)");

    // ---- layout and tables, by the header's rules, against what the library reported
    std::vector<int64_t> g_off(n + 1, 0), sym_off(n + 1, 0), bits(n), syms(n);
    std::vector<MixChanRec> recs(n);
    std::vector<int32_t> modem_prefix(n + 1, 0), pair_prefix(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const Cfg& c = cfg[i];
        if (g_off[i] != c.lib_g || sym_off[i] != c.lib_sym) return fail("library offset differs from the header's rule", i);
        if (g_off[i] % MIX_ALIGN || sym_off[i] % MIX_ALIGN) return fail("segment not aligned", i);
        bits[i] = c.n_tb * c.G;
        syms[i] = bits[i] / c.Qm;
        MixChanRec& r = recs[i];
        r = MixChanRec{};
        r.g_off = g_off[i]; r.sym_off = sym_off[i]; r.n_sym = syms[i]; r.Qm = c.Qm; r.inv_norm = 1.0f;
        g_off[i + 1] = mix_round_up(g_off[i] + bits[i]);
        sym_off[i + 1] = mix_chan_sym_next(sym_off[i], syms[i]);
        modem_prefix[i + 1] = modem_prefix[i] + (int32_t)mix_chan_modem_wgs(syms[i], c.Qm);
        pair_prefix[i + 1] = pair_prefix[i] + (int32_t)mix_chan_pair_wgs(syms[i]);
        // the grids are as small as the single kernels': ceil(ceil(n_sym / S) / 256) and ceil((n_sym / 2 + 1) / 256) workgroups
        const int64_t S = mix_chan_spt(c.Qm), thr = (syms[i] + S - 1) / S;
        if (mix_chan_modem_wgs(syms[i], c.Qm) != (thr + 255) / 256) return fail("modem grid size", i);
        if (mix_chan_pair_wgs(syms[i]) != (syms[i] ? (syms[i] / 2 + 1 + 255) / 256 : 0)) return fail("pair grid size", i);
    }
    if (g_off[n] != lib_tot_g || sym_off[n] != lib_tot_sym) return fail("library totals differ from the header's rule");
    const std::vector<int64_t> g_start(g_off.begin(), g_off.end() - 1), s_start(sym_off.begin(), sym_off.end() - 1);

    // ---- the modem grid: mapper (reads bits, writes symbols) and demapper (reads symbols and variances, writes field g)
    {
        std::vector<uint8_t> g((size_t)g_off[n], 0), sym((size_t)sym_off[n], 0);
        std::vector<int64_t> threads_with_work(n, 0);
        for (int32_t wg = 0; wg < modem_prefix[n]; ++wg)
            for (int32_t t = 0; t < MIX_CHAN_BLOCK; ++t) {
                const MixChanWork w = mix_chan_work(modem_prefix.data(), n, wg, t);
                if (w.cfg < 0 || w.cfg >= n || w.t < 0) return fail("modem grid: configuration out of range", wg, t);
                const MixChanRec& c = recs[w.cfg];
                if (c.n_sym == 0) return fail("modem grid: a configuration without symbols was found", wg, w.cfg);
                const int32_t S = mix_chan_spt(c.Qm);
                const MixChanModemThread th = mix_chan_modem_thread(c.n_sym, S, w.t);
                if (th.nv < 0 || th.nv > S) return fail("modem grid: nv out of range", wg, t);
                if (th.nv == 0) { // a surplus thread: only behind the configuration's last symbol, only in its last workgroup
                    if (th.s0 < c.n_sym || wg + 1 != modem_prefix[w.cfg + 1]) return fail("modem grid: an idle thread inside a configuration", wg, t);
                    continue;
                }
                ++threads_with_work[w.cfg];
                for (int32_t s = 0; s < th.nv; ++s) {
                    if (th.s0 + s >= c.n_sym) return fail("modem grid: symbol past the segment", wg, t);
                    if (!own(sym, mix_chan_sym_index(c, th.s0 + s))) return fail("modem grid: symbol index", wg, t);
                    for (int32_t k = 0; k < c.Qm; ++k)
                        if (!own(g, mix_chan_g_index(c, th.s0 + s) + k)) return fail("modem grid: bit index", wg, t);
                }
                // a full thread's wide accesses: S symbols = 2S floats, S*Q_m bits, all inside the segment (checked element by element above)
                if (th.nv == S && mix_chan_g_index(c, th.s0) + (int64_t)S * c.Qm > c.g_off + c.n_sym * c.Qm) return fail("modem grid: wide access past the segment", wg, t);
            }
        for (int i = 0; i < n; ++i) {
            const int64_t S = mix_chan_spt(cfg[i].Qm);
            if (threads_with_work[i] != (syms[i] + S - 1) / S) return fail("modem grid: thread count", i, threads_with_work[i]);
        }
        if (exactly_once(sym, s_start, syms, "modem grid: a symbol without exactly one owner, or a gap touched")) return 1;
        if (exactly_once(g, g_start, bits, "modem grid: a bit without exactly one owner, or a gap touched")) return 1;
    }

    // ---- the pair grid: fused stage (reads bits, writes LLRs in field g) and stand-alone noise (symbols, variances), either parity
    for (int flip = 0; flip < 2; ++flip) {
        std::vector<uint8_t> g((size_t)g_off[n], 0), sym((size_t)sym_off[n], 0);
        for (int32_t wg = 0; wg < pair_prefix[n]; ++wg)
            for (int32_t t = 0; t < MIX_CHAN_BLOCK; ++t) {
                const MixChanWork w = mix_chan_work(pair_prefix.data(), n, wg, t);
                if (w.cfg < 0 || w.cfg >= n || w.t < 0) return fail("pair grid: configuration out of range", wg, t);
                const MixChanRec& c = recs[w.cfg];
                if (c.n_sym == 0) return fail("pair grid: a configuration without symbols was found", wg, w.cfg);
                const uint64_t first = cfg[w.cfg].first ^ (uint64_t)flip;
                const MixChanPairThread th = mix_chan_pair_thread(c.n_sym, first, w.t);
                if (th.s0 < -1) return fail("pair grid: s0 below -1", wg, t);
                if (!th.v0 && !th.v1) { // a surplus thread: behind the last symbol
                    if (th.s0 < c.n_sym) return fail("pair grid: an idle thread inside a configuration", wg, t);
                    continue;
                }
                for (int h = 0; h < 2; ++h) {
                    if (!(h ? th.v1 : th.v0)) continue;
                    const int64_t s = th.s0 + h;
                    if (s < 0 || s >= c.n_sym) return fail("pair grid: symbol outside the segment", wg, t);
                    const uint64_t x = first + (uint64_t)s; // the global index: counter x >> 1, words 2 (x & 1) and 2 (x & 1) + 1
                    if ((x >> 1) != th.c || (int)(x & 1) != h) return fail("pair grid: Philox counter or word pair", wg, t);
                    if (!own(sym, mix_chan_sym_index(c, s))) return fail("pair grid: symbol index", wg, t);
                    for (int32_t k = 0; k < c.Qm; ++k)
                        if (!own(g, mix_chan_g_index(c, s) + k)) return fail("pair grid: bit index", wg, t);
                }
            }
        if (exactly_once(sym, s_start, syms, "pair grid: a symbol without exactly one owner, or a gap touched")) return 1;
        if (exactly_once(g, g_start, bits, "pair grid: a bit without exactly one owner, or a gap touched")) return 1;
    }
    // the counter's high word really changes inside a segment somewhere when the caller says so (argv[2] = "cross")
    if (argc > 2) {
        bool crosses = false;
        for (int i = 0; i < n; ++i)
            if (syms[i] > 0 && (cfg[i].first >> 33) != ((cfg[i].first + (uint64_t)syms[i] - 1) >> 33)) crosses = true;
        if (!crosses) return fail("no configuration whose pair counter crosses 2^32");
    }
    std::printf("mix_chan_check ok: %d configurations, %lld bits, %lld symbols, %d + %d workgroups\n", n, (long long)g_off[n],
                (long long)sym_off[n], modem_prefix[n], pair_prefix[n]);
    return 0;
}

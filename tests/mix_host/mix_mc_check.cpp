// mix_mc_check.cpp -- stand-alone host check of the mixed-batch Monte-Carlo stages (ldpc-3gpp-matlab_amd/csrc/nrldpc_mix_mc.h and the
// shared chunk rule nrldpc_payload_bits.h), meant to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_mix_mc_api.py does that): an out-of-range index in a table-driven kernel is a fault on the device.
//
// Input (a text file, argv[1]): n, then per configuration
//     n_tb A B seed first_block   and the three offsets the library gave for it (a of nrldpc_mix_tx_layout; b_hat, tb of nrldpc_mix_layout),
// then the three totals (entry [n]), then per configuration its expected payload as n_tb * A characters '0' / '1' (harness.payload_bits_np;
// "-" for an empty configuration).  The program rebuilds the offsets, the records and both prefix tables with the headers' functions and
//   payload  walks EVERY workgroup and thread of the payload grid at base addresses +0 ... +3 of a 16-byte aligned buffer, storing real
//            bytes through mix_mc_pay_store: every byte of every segment has exactly one owner and holds the expected bit, whichever of
//            the two store forms the address picked; no gap or guard byte is touched; a surplus thread sits behind its configuration's
//            last chunk, in its last workgroup;
//   outcome  walks every workgroup, wave and lane of the outcome grid and of the left grid over three attempts of hand-made ok / b_hat
//            patterns, the first with first = 1 on buffers poisoned with 0xFF, against the reference loop below (the per-block
//            bookkeeping of harness.simulate_point_device); gaps keep their poison;
//   layout   the library's offsets are the headers'.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "nrldpc_mix_mc.h"
#include "nrldpc_mix_tx.h"

using namespace nrldpc;

struct Cfg {
    int64_t n_tb;
    int32_t A, B;
    uint64_t seed, first;
    int64_t lib_a, lib_b_hat, lib_tb;
    std::string bits;
};

static int fail(const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "mix_mc_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: mix_mc_check FILE");
    std::ifstream in(argv[1]);
    int32_t n = -1;
    in >> n;
    if (!in || n < 0) return fail("bad n");
    std::vector<Cfg> cfg(n);
    for (auto& c : cfg) {
        in >> c.n_tb >> c.A >> c.B >> c.seed >> c.first >> c.lib_a >> c.lib_b_hat >> c.lib_tb;
        if (!in || c.n_tb < 0 || c.A < 1 || c.B <= c.A) return fail("short file");
    }
    int64_t lib_tot_a = 0, lib_tot_b_hat = 0, lib_tot_tb = 0;
    in >> lib_tot_a >> lib_tot_b_hat >> lib_tot_tb;
    for (auto& c : cfg) {
        in >> c.bits;
        if (!in || (c.n_tb == 0 ? c.bits != "-" : (int64_t)c.bits.size() != c.n_tb * c.A)) return fail("short file (expected bits)");
    }

    // ---- layout and tables, by the headers' rules, against what the library reported
    std::vector<int64_t> a_off(n + 1, 0), b_off(n + 1, 0), tb_off(n + 1, 0);
    std::vector<MixMcRec> recs(n);
    std::vector<int32_t> pay_prefix(n + 1, 0), tb_prefix(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const Cfg& c = cfg[i];
        if (a_off[i] != c.lib_a || b_off[i] != c.lib_b_hat || tb_off[i] != c.lib_tb) return fail("library offset differs from the header's rule", i);
        MixMcRec& r = recs[i];
        r = MixMcRec{};
        r.a_off = a_off[i]; r.b_hat_off = b_off[i]; r.tb_off = tb_off[i];
        r.n_tb = (int32_t)c.n_tb; r.A = c.A; r.B = c.B;
        a_off[i + 1] = mix_tx_a_next(a_off[i], c.n_tb, c.A);
        b_off[i + 1] = mix_round_up(b_off[i] + c.n_tb * c.B);
        tb_off[i + 1] = mix_round_up(tb_off[i] + c.n_tb);
        pay_prefix[i + 1] = pay_prefix[i] + (int32_t)mix_mc_pay_wgs(c.n_tb, c.A);
        tb_prefix[i + 1] = tb_prefix[i] + (int32_t)c.n_tb;
        // the grid is as small as the single kernel's: ceil(n_tb * ceil(A / 4) / 256) workgroups
        if (mix_mc_pay_wgs(c.n_tb, c.A) != (c.n_tb * ((c.A + 3) / 4) + 255) / 256) return fail("payload grid size", i);
    }
    if (a_off[n] != lib_tot_a || b_off[n] != lib_tot_b_hat || tb_off[n] != lib_tot_tb) return fail("library totals differ from the header's rule");

    // what every byte of the packed payload array must hold: the expected bit inside a segment, the poison in a gap
    const uint8_t POISON = 0xA5;
    std::vector<uint8_t> want((size_t)a_off[n], POISON);
    for (int i = 0; i < n; ++i)
        for (int64_t k = 0; k < cfg[i].n_tb * cfg[i].A; ++k) want[(size_t)(a_off[i] + k)] = (uint8_t)(cfg[i].bits[(size_t)k] - '0');

    // ---- payload grid, at four byte alignments of the array
    const size_t GUARD = 16;
    for (size_t shift = 0; shift < 4; ++shift) {
        const size_t bytes = GUARD + shift + (size_t)a_off[n] + GUARD;
        uint8_t* buf = static_cast<uint8_t*>(std::aligned_alloc(16, (bytes + 15) / 16 * 16));
        if (!buf) return fail("allocation");
        std::memset(buf, POISON, bytes);
        uint8_t* a = buf + GUARD + shift;
        std::vector<uint8_t> owners((size_t)a_off[n], 0);
        for (int32_t wg = 0; wg < pay_prefix[n]; ++wg)
            for (int32_t t = 0; t < MIX_MC_BLOCK; ++t) {
                const MixMcPayThread th = mix_mc_pay_thread(pay_prefix.data(), recs.data(), n, wg, t);
                if (th.cfg < 0 || th.cfg >= n) return fail("payload grid: configuration out of range", wg, t);
                const MixMcRec& c = recs[th.cfg];
                if (c.n_tb == 0) return fail("payload grid: an empty configuration was found", wg, th.cfg);
                if (th.b < 0) { // a surplus thread: only behind the configuration's last chunk, only in its last workgroup
                    const int64_t local = (int64_t)(wg - pay_prefix[th.cfg]) * MIX_MC_BLOCK + t;
                    if (local < (int64_t)c.n_tb * payload_chunks(c.A) || wg + 1 != pay_prefix[th.cfg + 1]) return fail("payload grid: an idle thread inside a configuration", wg, t);
                    continue;
                }
                if (th.b >= c.n_tb || th.i0 < 0 || th.i0 >= c.A || th.i0 % 4) return fail("payload grid: chunk out of range", wg, t);
                for (int32_t k = 0; k < 4 && th.i0 + k < c.A; ++k) {
                    const int64_t idx = mix_mc_a_index(c, th.b, th.i0 + k);
                    if (idx < a_off[th.cfg] || idx >= a_off[th.cfg] + (int64_t)c.n_tb * c.A) return fail("payload grid: byte outside the segment", wg, t);
                    ++owners[(size_t)idx];
                }
                mix_mc_pay_store(c, th, cfg[th.cfg].seed, cfg[th.cfg].first, a);
            }
        for (size_t k = 0; k < (size_t)a_off[n]; ++k) {
            if (owners[k] != (want[k] == POISON ? 0 : 1)) return fail("payload grid: a byte without exactly one owner", (long long)k, owners[k]);
            if (a[k] != want[k]) return fail("payload grid: wrong bit, or a gap byte written", (long long)k, (long long)shift);
        }
        for (size_t k = 0; k < GUARD + shift; ++k)
            if (buf[k] != POISON) return fail("payload grid: guard byte written in front", (long long)k, (long long)shift);
        for (size_t k = 0; k < GUARD; ++k)
            if (a[(size_t)a_off[n] + k] != POISON) return fail("payload grid: guard byte written behind", (long long)k, (long long)shift);
        std::free(buf);
    }

    // ---- outcome and left grids: three attempts of hand-made patterns against the reference loop
    {
        std::vector<uint8_t> a(want), a_hat((size_t)a_off[n], 0xFF), ref_a_hat(a_hat), b_hat((size_t)b_off[n], POISON);
        std::vector<uint8_t> done((size_t)tb_off[n], 0xFF), good((size_t)tb_off[n], 0xFF), ref_done(done), ref_good(good);
        std::vector<int32_t> ok((size_t)tb_off[n], -1), left(n, -7);
        for (int attempt = 0; attempt < 3; ++attempt) {
            const int32_t first = attempt == 0 ? 1 : 0;
            // the patterns: by packed index j a block is acknowledged on attempt 1 only, on attempts 0 and 2 (with another b_hat the
            // second time: the first must stay), on one attempt, or never (j % 11 == 10, with b_hat equal to a: good stays 0);
            // j % 3 == 1: b_hat differs from a in the last payload byte only
            for (int i = 0; i < n; ++i)
                for (int32_t t = 0; t < recs[i].n_tb; ++t) {
                    const int64_t j = mix_mc_tb_index(recs[i], t);
                    ok[(size_t)j] = j % 11 == 10 ? 0 : ((j * 7 + attempt * 3) % 5 < 2 ? (j % 2 ? 1 : 0x100) : 0);
                    uint8_t* row = &b_hat[(size_t)mix_mc_b_hat_index(recs[i], t)];
                    std::memcpy(row, &a[(size_t)mix_mc_a_index(recs[i], t, 0)], (size_t)recs[i].A);
                    std::memset(row + recs[i].A, 1, (size_t)(recs[i].B - recs[i].A));
                    if (j % 3 == 1) row[recs[i].A - 1] ^= 1;
                    if (attempt == 2) row[0] ^= 1;
                }
            // the reference: lines 236-245 of harness.simulate_point_device per transport block
            for (int i = 0; i < n; ++i)
                for (int32_t t = 0; t < recs[i].n_tb; ++t) {
                    const size_t j = (size_t)(tb_off[i] + t), row = (size_t)(a_off[i] + (int64_t)t * cfg[i].A);
                    const bool was = first ? false : ref_done[j] != 0, now = ok[j] != 0;
                    if (now && !was) std::memcpy(&ref_a_hat[row], &b_hat[(size_t)(b_off[i] + (int64_t)t * cfg[i].B)], (size_t)cfg[i].A);
                    ref_done[j] = was || now;
                    ref_good[j] = ref_done[j] && std::memcmp(&ref_a_hat[row], &a[row], (size_t)cfg[i].A) == 0;
                }
            // the outcome grid
            std::vector<uint8_t> seen((size_t)tb_off[n], 0);
            for (int32_t wg = 0; wg < mix_mc_out_wgs(tb_prefix[n]); ++wg)
                for (int32_t wave = 0; wave < MIX_MC_WAVES; ++wave) {
                    const MixMcOutWave w = mix_mc_out_wave(tb_prefix.data(), n, wg, wave);
                    if (w.cfg < 0) {
                        if (wg * MIX_MC_WAVES + wave < tb_prefix[n]) return fail("outcome grid: an idle wave inside the grid", wg, wave);
                        continue;
                    }
                    if (w.cfg >= n || w.t < 0 || w.t >= recs[w.cfg].n_tb) return fail("outcome grid: block out of range", wg, wave);
                    const MixMcRec& c = recs[w.cfg];
                    if (seen[(size_t)mix_mc_tb_index(c, w.t)]++) return fail("outcome grid: a block with two waves", wg, wave);
                    const MixMcOutState s = mix_mc_out_state(c, w.t, first, ok.data(), done.data());
                    bool any = false;
                    for (int32_t lane = 0; lane < MIX_MC_WAVE; ++lane) any = mix_mc_out_lane(c, w.t, lane, s, a.data(), b_hat.data(), a_hat.data()) || any;
                    mix_mc_out_finish(c, w.t, s, any, done.data(), good.data());
                }
            if (a_hat != ref_a_hat) return fail("outcome: a_hat differs from the reference loop (or a gap byte was written)", attempt);
            if (done != ref_done || good != ref_good) return fail("outcome: done / good differ from the reference loop", attempt);
            // the left grid
            for (int32_t wg = 0; wg < mix_mc_left_wgs(n); ++wg)
                for (int32_t wave = 0; wave < MIX_MC_WAVES; ++wave) {
                    const int32_t i = mix_mc_left_cfg(n, wg, wave);
                    if (i < 0) continue;
                    if (i >= n) return fail("left grid: configuration out of range", wg, wave);
                    int32_t cnt = 0;
                    for (int32_t k = 0; k < mix_mc_left_sweeps(recs[i]); ++k)
                        for (int32_t lane = 0; lane < MIX_MC_WAVE; ++lane) cnt += mix_mc_left_lane(recs[i], k, lane, done.data()) ? 1 : 0;
                    left[(size_t)i] = cnt;
                }
            for (int i = 0; i < n; ++i) {
                int32_t cnt = 0;
                for (int32_t t = 0; t < recs[i].n_tb; ++t) cnt += ref_done[(size_t)(tb_off[i] + t)] == 0;
                if (left[(size_t)i] != cnt) return fail("left grid: count differs", i, left[(size_t)i]);
            }
        }
        // the patterns did what they are for: some block acknowledged late, some never, some acknowledged yet not good
        int64_t late = 0, never = 0, wrong = 0;
        for (int i = 0; i < n; ++i)
            for (int32_t t = 0; t < recs[i].n_tb; ++t) {
                const size_t j = (size_t)(tb_off[i] + t);
                never += ref_done[j] == 0; wrong += ref_done[j] && !ref_good[j]; late += ref_done[j] && ref_good[j];
            }
        if (tb_prefix[n] >= 12 && (!late || !never || !wrong)) return fail("outcome: the patterns cover too little", late, never);
    }
    std::printf("mix_mc_check ok: %d configurations, %d payload workgroups, %d transport blocks\n", n, pay_prefix[n], tb_prefix[n]);
    return 0;
}

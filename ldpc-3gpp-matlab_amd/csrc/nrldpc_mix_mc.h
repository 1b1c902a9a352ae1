// nrldpc_mix_mc.h -- mixed transport-block batches, the two Monte-Carlo stages on the transmit plan: the record, the workgroup mappings
// and every index of nrldpc_mix_tx_payload_dev (the payload draw) and nrldpc_mix_tx_outcome_dev (the per-block outcome latch and the
// per-configuration "still retransmitting" count); kernels: nrldpc_mix_mc.hip; semantics: include/nrldpc.h, DESIGN.md section 4.21.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// The first part is plain C++ that a host compiler reads too: tests/mix_host/mix_mc_check.cpp walks every workgroup, wave and thread
// of the three grids on the CPU (address and undefined-behaviour sanitizers on), storing and loading real bytes through the same
// functions the kernels call.  An out-of-range index in a table-driven kernel is a fault.
//
// The payload array is the transmit plan's a (nrldpc_mix_tx.h: mix_tx_a_next); b_hat and the per-transport-block arrays (ok, done, good)
// reuse fields b_hat and tb of nrldpc_mix_layout element for element (nrldpc_mix.h: MIX_B_HAT, MIX_TB).
#pragma once
#include <stdint.h>

#include "nrldpc_mix.h"
#include "nrldpc_payload_bits.h"

namespace nrldpc {

constexpr int MIX_MC_BLOCK = 256;                 // threads per workgroup of all three grids
constexpr int MIX_MC_WAVE = 64;                   // lanes of a wave (gfx950)
constexpr int MIX_MC_WAVES = MIX_MC_BLOCK / MIX_MC_WAVE;

// One configuration of both stages.  40 bytes.
struct MixMcRec {
    int64_t a_off, b_hat_off, tb_off; // element offsets of the segment in the payload array, in b_hat and in the per-transport-block arrays
    int32_t n_tb, A, B;
    int32_t pad_;
};

// ---- payload grid: thread t of a configuration owns chunk (t mod q4) of block (t div q4), q4 = ceil(A/4): nrldpc_payload_bits_kernel's
// mapping inside the segment ------------------------------------------------------------------------------------------------------------
NRLDPC_MIX_HD int64_t mix_mc_pay_wgs(int64_t n_tb, int32_t A) { return (n_tb * payload_chunks(A) + MIX_MC_BLOCK - 1) / MIX_MC_BLOCK; }

struct MixMcPayThread {
    int32_t cfg; // configuration
    int32_t b;   // transport block inside the configuration, or -1: a surplus thread of the configuration's last workgroup
    int32_t i0;  // first bit of the chunk
};
// workgroup wg, thread `thread` of the payload grid.  prefix as for mix_find: a configuration without transport blocks shares its
// prefix with the next one and is never found.
NRLDPC_MIX_HD MixMcPayThread mix_mc_pay_thread(const int32_t* prefix, const MixMcRec* recs, int32_t n, int32_t wg, int32_t thread) {
    MixMcPayThread th;
    th.cfg = mix_find(prefix, n, wg);
    const MixMcRec& c = recs[th.cfg];
    const int32_t q4 = payload_chunks(c.A);
    const int64_t t = (int64_t)(wg - prefix[th.cfg]) * MIX_MC_BLOCK + thread;
    if (t >= (int64_t)c.n_tb * q4) { th.b = -1; th.i0 = 0; return th; }
    th.b = (int32_t)(t / q4);
    th.i0 = 4 * (int32_t)(t - (int64_t)th.b * q4);
    return th;
}
// element of the payload array that holds bit i of transport block b
NRLDPC_MIX_HD int64_t mix_mc_a_index(const MixMcRec& c, int32_t b, int32_t i) { return c.a_off + (int64_t)b * c.A + i; }
// what a payload thread with work does (seed, first_block: the configuration's nrldpc_mix_draw)
NRLDPC_MIX_HD void mix_mc_pay_store(const MixMcRec& c, const MixMcPayThread& th, uint64_t seed, uint64_t first_block, uint8_t* a) {
    const uint32_t nib = payload_nibble(seed, first_block + (uint64_t)th.b, payload_words(c.A), th.i0);
    payload_store_chunk(a + mix_mc_a_index(c, th.b, th.i0), nib, th.i0, c.A);
}

// ---- outcome grid: a wave is one transport block (x = wg * 4 + wave in the order of the plan's transport-block prefix), lane l owns
// bytes l, l + 64, ... of its rows ------------------------------------------------------------------------------------------------------
NRLDPC_MIX_HD int32_t mix_mc_out_wgs(int32_t n_tb_total) { return (n_tb_total + MIX_MC_WAVES - 1) / MIX_MC_WAVES; }

struct MixMcOutWave {
    int32_t cfg; // configuration, or -1: a surplus wave of the last workgroup
    int32_t t;   // transport block inside the configuration
};
NRLDPC_MIX_HD MixMcOutWave mix_mc_out_wave(const int32_t* tb_prefix, int32_t n, int32_t wg, int32_t wave) {
    MixMcOutWave w;
    const int32_t x = wg * MIX_MC_WAVES + wave;
    if (x >= tb_prefix[n]) { w.cfg = -1; w.t = 0; return w; }
    w.cfg = mix_find(tb_prefix, n, x);
    w.t = x - tb_prefix[w.cfg];
    return w;
}
NRLDPC_MIX_HD int64_t mix_mc_tb_index(const MixMcRec& c, int32_t t) { return c.tb_off + t; }                     // ok, done, good
NRLDPC_MIX_HD int64_t mix_mc_b_hat_index(const MixMcRec& c, int32_t t) { return c.b_hat_off + (int64_t)t * c.B; } // byte 0 of the block's b_hat row

// the wave-uniform state of a block: was = acknowledged before this call (never read with `first`), now = this attempt's CRC holds
struct MixMcOutState {
    bool was, now;
};
NRLDPC_MIX_HD MixMcOutState mix_mc_out_state(const MixMcRec& c, int32_t t, int32_t first, const int32_t* ok, const uint8_t* done) {
    MixMcOutState s;
    s.was = first ? false : done[mix_mc_tb_index(c, t)] != 0;
    s.now = ok[mix_mc_tb_index(c, t)] != 0;
    return s;
}
// One lane's share of a block: latches a_hat from b_hat where the block is newly acknowledged, and returns whether any of the lane's
// bytes of a_hat differs from a.  A block that is neither acknowledged now nor before touches no row (its `good` is 0 whatever they hold).
NRLDPC_MIX_HD bool mix_mc_out_lane(const MixMcRec& c, int32_t t, int32_t lane, const MixMcOutState& s, const uint8_t* a, const uint8_t* b_hat,
                                   uint8_t* a_hat) {
    if (!s.was && !s.now) return true;
    const int64_t row = mix_mc_a_index(c, t, 0), src = mix_mc_b_hat_index(c, t);
    bool differs = false;
    for (int32_t k = lane; k < c.A; k += MIX_MC_WAVE) {
        uint8_t v;
        if (s.was) v = a_hat[row + k];
        else a_hat[row + k] = v = b_hat[src + k];
        differs = differs || v != a[row + k];
    }
    return differs;
}
// what lane 0 writes once the wave knows whether any lane saw a difference
NRLDPC_MIX_HD void mix_mc_out_finish(const MixMcRec& c, int32_t t, const MixMcOutState& s, bool any_differs, uint8_t* done, uint8_t* good) {
    const bool d = s.was || s.now;
    done[mix_mc_tb_index(c, t)] = d ? 1 : 0;
    good[mix_mc_tb_index(c, t)] = d && !any_differs ? 1 : 0;
}

// ---- left grid: a wave is one configuration; sweep k of a wave looks at blocks 64 k + lane, the wave adds up how many are not done ------
NRLDPC_MIX_HD int32_t mix_mc_left_wgs(int32_t n) { return (n + MIX_MC_WAVES - 1) / MIX_MC_WAVES; }
NRLDPC_MIX_HD int32_t mix_mc_left_cfg(int32_t n, int32_t wg, int32_t wave) { // -1: a surplus wave of the last workgroup
    const int32_t i = wg * MIX_MC_WAVES + wave;
    return i < n ? i : -1;
}
NRLDPC_MIX_HD int32_t mix_mc_left_sweeps(const MixMcRec& c) { return (c.n_tb + MIX_MC_WAVE - 1) / MIX_MC_WAVE; }
// whether this lane's block of sweep k exists and is still retransmitting
NRLDPC_MIX_HD bool mix_mc_left_lane(const MixMcRec& c, int32_t k, int32_t lane, const uint8_t* done) {
    const int32_t t = k * MIX_MC_WAVE + lane;
    return t < c.n_tb && done[mix_mc_tb_index(c, t)] == 0;
}

} // namespace nrldpc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "nrldpc.h" // nrldpc_mix_draw

namespace nrldpc {

struct MixMcPayLaunch {
    const MixMcRec* recs;        // device, [n]
    const int32_t* prefix;       // device, [n + 1] workgroups
    int32_t n, n_wg;
    const nrldpc_mix_draw* draw; // device, [n]: the caller's records
    uint8_t* a;
};
hipError_t launch_mix_mc_payload(const MixMcPayLaunch& a, hipStream_t stream);

struct MixMcOutLaunch {
    const MixMcRec* recs;        // device, [n]
    const int32_t* tb_prefix;    // device, [n + 1] transport blocks
    int32_t n, n_tb_total;
    int32_t first;
    const uint8_t* a;
    const uint8_t* b_hat;
    const int32_t* ok;
    uint8_t* a_hat;
    uint8_t* done;
    uint8_t* good;
    int32_t* left;               // nullable: no second launch
};
hipError_t launch_mix_mc_outcome(const MixMcOutLaunch& a, hipStream_t stream);

} // namespace nrldpc
#endif

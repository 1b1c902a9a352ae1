// nrldpc_mix_tx.h -- mixed transport-block batches, transmit side: the payload layout, the device-side tables and the workgroup mapping
// of nrldpc_mix_tx_crc_attach_dev / nrldpc_mix_tx_rate_match_dev (nrldpc_mix_tx.hip; semantics: include/nrldpc.h).
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// The first part -- the layout rule of the payload array, the table records, the workgroup -> work mapping of both grids and every
// index the two kernels form from them -- is plain C++ that a host compiler reads too: tests/mix_host/mix_tx_check.cpp walks every
// workgroup, wave and thread of both grids on the CPU (address and undefined-behaviour sanitizers on).  An out-of-range index in a
// table-driven kernel is a fault.
//
// Every transmit array but the payload reuses a field of nrldpc_mix_layout element for element: code blocks = c_hat, codeword bytes = cw,
// rate-matched bits = g (nrldpc_mix.h: MIX_C_HAT, MIX_CW, MIX_G).
#pragma once
#include <stdint.h>

#include "nrldpc_mix.h"

namespace nrldpc {

constexpr int MIX_TX_RM_COLS = 4;                       // interleaver columns j per thread (nrldpc_rate_match_kernel)
constexpr int MIX_TX_RM_WG = 256 * MIX_TX_RM_COLS;      // columns per workgroup of 256 threads

// the payload array a [n_tb][A]: a_off[i + 1] from a_off[i]
NRLDPC_MIX_HD int64_t mix_tx_a_next(int64_t a_off, int64_t n_tb, int64_t A) { return mix_round_up(a_off + n_tb * A); }

// ---- rate matching: a workgroup is 256 threads x 4 columns of one code block of one transport block -------------------------------------
struct MixTxRmRec {
    int64_t cw_off, g_off;  // element offsets of the segment in the codeword bytes and in the rate-matched bits
    int32_t n_tb, C, G, Z, K, Kp, N, N_cb, k0, Qm;
    int32_t e_base;         // E_r[r] = e_tab[e_base + r], offset of block r inside a row of g = off_tab[e_base + r]
    int32_t wg_per_cb;      // workgroups per code block = ceil(max_r E_r / Q_m / MIX_TX_RM_WG); 0 when G == 0
};

struct MixTxRmWork {
    int32_t cfg;   // configuration
    int32_t blk;   // tb * C + r inside the configuration
    int32_t j_wg;  // first interleaver column of the workgroup
};

NRLDPC_MIX_HD int32_t mix_tx_rm_wg_per_cb(int32_t e_max, int32_t Qm) { return (e_max / Qm + MIX_TX_RM_WG - 1) / MIX_TX_RM_WG; }

// workgroup wg of the rate-matching grid -> its configuration, code block and first column.  prefix as for mix_find: a configuration
// without workgroups (no transport blocks, or G == 0) shares its prefix with the next one and is never found, so `per` is positive.
NRLDPC_MIX_HD MixTxRmWork mix_tx_rm_work(const int32_t* prefix, const MixTxRmRec* recs, int32_t n, int32_t wg) {
    MixTxRmWork w;
    w.cfg = mix_find(prefix, n, wg);
    const int32_t local = wg - prefix[w.cfg];
    const int32_t per = recs[w.cfg].wg_per_cb;
    w.blk = local / per;
    w.j_wg = (local - w.blk * per) * MIX_TX_RM_WG;
    return w;
}

// first column of a thread; it has work when this is below E_r / Q_m
NRLDPC_MIX_HD int32_t mix_tx_rm_j0(const MixTxRmWork& w, int32_t thread) { return w.j_wg + thread * MIX_TX_RM_COLS; }
// element of the codeword array that holds position 0 of the block's d (behind the 2Z punctured columns)
NRLDPC_MIX_HD int64_t mix_tx_rm_cw_index(const MixTxRmRec& c, int32_t blk) { return c.cw_off + (int64_t)blk * (2 * c.Z + c.N) + 2 * c.Z; }
// element of g that takes bit 0 of code block r of transport block tb (off_r = off_tab[e_base + r])
NRLDPC_MIX_HD int64_t mix_tx_rm_g_index(const MixTxRmRec& c, int32_t tb, int32_t off_r) { return c.g_off + (int64_t)tb * c.G + off_r; }

// ---- CRC attach: a workgroup is one transport block, a wave one code block (waves loop when C exceeds the plan's wave count) ----------
struct MixTxCrcGeom {
    int64_t a_off, c_off;   // element offsets of the segment in the payload array and in the code blocks
    int32_t C, K, Kp, Lcb, A, B;
    int32_t pad_[2];
};

NRLDPC_MIX_HD int32_t mix_tx_waves(int32_t c_max) { return c_max < 4 ? (c_max < 1 ? 1 : c_max) : 4; }
// bytes of LDS a wave's row of K bits takes: row_capacity of nrldpc_crc_wave.h (stage_row places the copy at the source's offset
// modulo 16 and store_row reads up to 4 bytes past the end; the device code static_asserts the two agree)
NRLDPC_MIX_HD int32_t mix_tx_row_capacity(int32_t K) { return ((K + 15) & ~15) + 48; }
// the workgroup's LDS: one row per wave at the plan-wide stride, then part[c_max]
NRLDPC_MIX_HD int64_t mix_tx_lds_bytes(int32_t waves, int32_t k_max, int32_t c_max) { return (int64_t)waves * mix_tx_row_capacity(k_max) + 4 * (int64_t)c_max + 16; }
NRLDPC_MIX_HD int64_t mix_tx_part_byte(int32_t waves, int32_t k_max, int32_t r) { return (int64_t)waves * mix_tx_row_capacity(k_max) + 4 * (int64_t)r; }

NRLDPC_MIX_HD int32_t mix_tx_pay(const MixTxCrcGeom& c) { return c.Kp - c.Lcb; }                     // payload bits per code block
NRLDPC_MIX_HD int32_t mix_tx_seg(const MixTxCrcGeom& c, int32_t r) { return r == c.C - 1 ? mix_tx_pay(c) - (c.B - c.A) : mix_tx_pay(c); } // bits of `a` in block r
NRLDPC_MIX_HD int64_t mix_tx_a_index(const MixTxCrcGeom& c, int32_t tb, int32_t r) { return c.a_off + (int64_t)tb * c.A + (int64_t)r * mix_tx_pay(c); }
NRLDPC_MIX_HD int64_t mix_tx_c_index(const MixTxCrcGeom& c, int32_t tb, int32_t r) { return c.c_off + ((int64_t)tb * c.C + r) * c.K; }
// the wave that finishes the last code block once the segment remainders are folded: its row still holds that block's share of `a`
NRLDPC_MIX_HD int32_t mix_tx_last_wave(const MixTxCrcGeom& c, int32_t waves) { return (c.C - 1) % waves; }

} // namespace nrldpc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "nrldpc_kernels.h" // CrcPlan

namespace nrldpc {

// One configuration of the attach launch.  The two plans are built the way nrldpc_crc_attach_dev builds them (the transport-block plan
// with horner_tail for the shorter last segment, the code-block plan over K' - L_cb bits): they are NOT the receive plan's.
struct MixTxCrcRec {
    MixTxCrcGeom g;
    CrcPlan cb, tb;
};

struct MixTxCrcLaunch {
    const MixTxCrcRec* recs;  // device, [n]
    const int32_t* prefix;    // device, [n + 1] transport blocks
    int32_t n, n_tb_total;
    int32_t waves;            // waves per workgroup: min(4, largest C of the plan)
    int32_t k_max, c_max;     // largest K and C of the plan: the LDS a workgroup needs
    const uint8_t* a;
    uint8_t* c;
};
hipError_t launch_mix_tx_crc_attach(const MixTxCrcLaunch& a, hipStream_t stream);

struct MixTxRmLaunch {
    const MixTxRmRec* recs;   // device, [n]
    const int32_t* prefix;    // device, [n + 1] workgroups
    const int32_t* e_tab;     // device: E_r of every configuration
    const int32_t* off_tab;   // device: offsets of the code blocks inside a row of g
    int32_t n, n_wg;
    const uint8_t* cw;
    uint8_t* g;
};
hipError_t launch_mix_tx_rate_match(const MixTxRmLaunch& a, hipStream_t stream);

} // namespace nrldpc
#endif

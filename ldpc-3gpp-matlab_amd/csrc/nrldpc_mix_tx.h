// nrldpc_mix_tx.h -- mixed transport-block batches, transmit side: the payload layout, the device-side tables and the workgroup mapping
// of nrldpc_mix_tx_crc_attach_dev / nrldpc_mix_tx_rate_match_dev (nrldpc_mix_tx.hip; semantics: include/nrldpc.h)
// and of the one-launch encoder nrldpc_mix_tx_encode_all_dev (nrldpc_mix_tx_enc.hip).
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// The first part -- the layout rule of the payload array, the table records, the workgroup -> work mapping of both grids and every
// index the two kernels form from them -- is plain C++ that a host compiler reads too: tests/mix_host/mix_tx_check.cpp walks every
// workgroup, wave and thread of both grids on the CPU (address and undefined-behaviour sanitizers on), tests/mix_host/mix_tx_enc_check.cpp
// the encoder's.  An out-of-range index in a table-driven kernel is a fault.
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

// ---- encode in one launch (nrldpc_mix_tx_encode_all_dev; kernel: nrldpc_mix_tx_enc.hip) -------------------------
// A workgroup is four waves.  A configuration's codewords take one wave each (four codewords per workgroup) or the whole workgroup,
// by launch_encode's rule (nrldpc_encode.hip) restated; tests/mix_host/mix_tx_enc_check.cpp walks the grid on the CPU.
constexpr int MIX_TX_ENC_WAVES = 4;

// Substitution order of the four core-parity blocks, derived on the host from (base graph, shifts mod Z): what an encoder handle
// stores and what EncArgs carries (nrldpc_kernels.h), as one plain struct.
struct EncSolveOrder {
    int32_t p0_shift;          // rot(p0, p0_shift) = lam0+lam1+lam2+lam3
    int32_t step_row[3];       // row that yields the next block
    int32_t step_col[3];       // unknown block solved at each step (0..3 relative to kb)
    int32_t step_shift[3];     // shift of the unknown block in that row
    int32_t step_nk[3];        // core-parity blocks of that row already known at that step ...
    int32_t step_kcol[3][3];   // ... their columns (0..3 relative to kb) ...
    int32_t step_kshift[3][3]; // ... and shifts
};

// EncLayout (nrldpc_encode.hip) restated for host and device: LDS words; the shared table first, then one region per codeword slot
struct MixTxEncLayout {
    int32_t W, DW, tab, D, lam, PP, xc, wave_words;
};
NRLDPC_MIX_HD MixTxEncLayout mix_tx_enc_layout(int32_t Z, int32_t kb, int32_t nrows, int32_t nnz) {
    MixTxEncLayout L;
    L.W = (Z + 31) >> 5;                      // packed words per column
    L.DW = 2 * ((2 * Z + 32 + 63) >> 6);      // words of a doubled ring (whole ballots)
    L.tab = ((nnz + nrows + 1 + 3) & ~3);     // table: nnz edge words + nrows+1 row pointers
    L.D = 0;
    L.lam = L.D + (kb + 4) * L.DW;
    L.PP = L.lam + 4 * L.W;
    L.xc = L.PP + (nrows - 4) * L.W;
    L.wave_words = ((L.xc + Z + 2 + 3) & ~3); // xc: 4*Z bytes + slack
    return L;
}

// waves per codeword: launch_encode's rule (the plan does not read the NRLDPC_ENC_NWC A/B knob)
NRLDPC_MIX_HD int32_t mix_tx_enc_nwc(int32_t bg, int32_t Z) { return bg == 1 && Z >= 128 ? 4 : 1; }
NRLDPC_MIX_HD int32_t mix_tx_enc_per_wg(int32_t nwc) { return MIX_TX_ENC_WAVES / nwc; }
NRLDPC_MIX_HD int32_t mix_tx_enc_wgs(int32_t n_cw, int32_t nwc) { return (n_cw + mix_tx_enc_per_wg(nwc) - 1) / mix_tx_enc_per_wg(nwc); }
// LDS bytes one configuration's workgroup needs; the launch takes the largest over the plan's non-empty configurations
NRLDPC_MIX_HD int64_t mix_tx_enc_lds_bytes(const MixTxEncLayout& L, int32_t nwc) { return 4 * ((int64_t)L.tab + (int64_t)mix_tx_enc_per_wg(nwc) * L.wave_words); }
// first LDS word of a codeword slot's region
NRLDPC_MIX_HD int64_t mix_tx_enc_slot_word(const MixTxEncLayout& L, int32_t slot) { return (int64_t)L.tab + (int64_t)slot * L.wave_words; }

// The base-graph tables of one (BG, Z_c) inside the plan's table bytes: row_ptr (uint16 [nrows + 1]), shift reduced mod Z (uint16 [nnz]),
// col (uint8 [nnz]), each at a multiple of 16 bytes.  Configurations that share (BG, Z_c) share one copy.
NRLDPC_MIX_HD int32_t mix_tx_enc_pad16(int32_t x) { return (x + 15) & ~15; }
NRLDPC_MIX_HD int32_t mix_tx_enc_tab_bytes(int32_t nrows, int32_t nnz) { return mix_tx_enc_pad16(2 * (nrows + 1)) + mix_tx_enc_pad16(2 * nnz) + mix_tx_enc_pad16(nnz); }

struct MixTxEncRec {
    int64_t c_off, cw_off;  // element offsets of the segment in the code blocks and in the codeword bytes
    int32_t n_cw;           // codewords of the configuration = n_tb * C
    int32_t Z, kb, nrows, ncols, nnz;
    int32_t row_ptr_off, shift_off, col_off; // byte offsets of the (BG, Z_c) tables in the plan's table bytes
    int32_t nwc;            // waves per codeword: 1 or 4
    EncSolveOrder ord;
    int32_t pad_;
};
NRLDPC_MIX_HD void mix_tx_enc_tab_place(int32_t base, MixTxEncRec& r) {
    r.row_ptr_off = base;
    r.shift_off = r.row_ptr_off + mix_tx_enc_pad16(2 * (r.nrows + 1));
    r.col_off = r.shift_off + mix_tx_enc_pad16(2 * r.nnz);
}

struct MixTxEncWork {
    int32_t cfg;  // configuration
    int32_t cw;   // codeword inside the configuration, or -1: this wave has none (the ragged last workgroup of a configuration)
};

// workgroup wg, wave `wave` of the encode grid -> its configuration and codeword.  prefix as for mix_find: a configuration without
// codewords shares its prefix with the next one and is never found.  With four waves per codeword the four waves of a workgroup
// get the same answer.
NRLDPC_MIX_HD MixTxEncWork mix_tx_enc_work(const int32_t* prefix, const MixTxEncRec* recs, int32_t n, int32_t wg, int32_t wave) {
    MixTxEncWork w;
    w.cfg = mix_find(prefix, n, wg);
    const int32_t nwc = recs[w.cfg].nwc;
    w.cw = (wg - prefix[w.cfg]) * mix_tx_enc_per_wg(nwc) + wave / nwc;
    if (w.cw >= recs[w.cfg].n_cw) w.cw = -1;
    return w;
}
// first element of codeword cw's code block and of its codeword bytes (on the record's fields: the kernel holds them as scalars)
NRLDPC_MIX_HD int64_t mix_tx_enc_info_index(int64_t c_off, int32_t kb, int32_t Z, int32_t cw) { return c_off + (int64_t)cw * kb * Z; }
NRLDPC_MIX_HD int64_t mix_tx_enc_out_index(int64_t cw_off, int32_t ncols, int32_t Z, int32_t cw) { return cw_off + (int64_t)cw * ncols * Z; }
NRLDPC_MIX_HD int64_t mix_tx_enc_info_index(const MixTxEncRec& r, int32_t cw) { return mix_tx_enc_info_index(r.c_off, r.kb, r.Z, cw); }
NRLDPC_MIX_HD int64_t mix_tx_enc_out_index(const MixTxEncRec& r, int32_t cw) { return mix_tx_enc_out_index(r.cw_off, r.ncols, r.Z, cw); }

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

struct MixTxEncLaunch {
    const MixTxEncRec* recs;  // device, [n]
    const int32_t* prefix;    // device, [n + 1] workgroups
    const uint8_t* tab;       // device: the base-graph tables of every distinct (BG, Z_c) (MixTxEncRec::*_off)
    int32_t n, n_wg;
    int32_t lds_bytes;        // the largest mix_tx_enc_lds_bytes of the plan's non-empty configurations
    const uint8_t* c;
    uint8_t* cw;
};
hipError_t launch_mix_tx_encode(const MixTxEncLaunch& a, hipStream_t stream);

} // namespace nrldpc
#endif

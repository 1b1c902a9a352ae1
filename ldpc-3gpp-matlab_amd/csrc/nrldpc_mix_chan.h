// nrldpc_mix_chan.h -- mixed transport-block batches, the channel leg: the symbol layout, the device-side table and the two workgroup
// mappings of nrldpc_mix_chan_modulate_dev / _awgn_dev / _demodulate_dev (nrldpc_mix_modem.hip) and of the fused
// nrldpc_mix_chan_awgn_llr_dev (nrldpc_mix_chan.hip); semantics: include/nrldpc.h, DESIGN.md section 4.20.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// The first part -- the layout rule of the symbol array, the table record, the workgroup -> (configuration, thread) mapping of both
// grids and every index the four kernels form from them -- is plain C++ that a host compiler reads too:
// tests/mix_host/mix_chan_check.cpp walks every thread of both grids on the CPU (address and undefined-behaviour sanitizers on).  An
// out-of-range index in a table-driven kernel is a fault.
//
// Bits and LLRs reuse field g of nrldpc_mix_layout element for element (nrldpc_mix.h: MIX_G); only the symbol array is new.
#pragma once
#include <stdint.h>

#include "nrldpc_mix.h"

namespace nrldpc {

constexpr int MIX_CHAN_BLOCK = 256; // threads per workgroup of both grids (= MODEM_BLOCK, AWGN_BLOCK and the fused kernel's 256)

// the symbol array: sym_off[i + 1] from sym_off[i], in SYMBOLS.  Symbol s of configuration i is the float pair at 2 * (sym_off[i] + s),
// its entry in a per-symbol variance array the float at sym_off[i] + s.
NRLDPC_MIX_HD int64_t mix_chan_sym_next(int64_t sym_off, int64_t n_sym) { return mix_round_up(sym_off + n_sym); }

// One configuration of all four launches.  32 bytes.
struct MixChanRec {
    int64_t g_off, sym_off; // element offsets of the segment in the bits / LLRs (field g) and in the symbol array
    int64_t n_sym;          // n_tb * G / Q_m
    int32_t Qm;
    float inv_norm;         // 1 / sqrt(2 mean(level^2)) of one rail, as the single calls form it
};

// symbols per thread of the mapper and the demapper: SymbolsPerThread of the single kernels (nrldpc_modem_sym.h)
NRLDPC_MIX_HD constexpr int32_t mix_chan_spt(int32_t Qm) { return Qm == 1 ? 4 : 2; }

// ---- mapper / demapper grid: thread t of a configuration owns local symbols [t*S, t*S + S) --------------------------------------------
NRLDPC_MIX_HD int64_t mix_chan_modem_wgs(int64_t n_sym, int32_t Qm) {
    const int64_t S = mix_chan_spt(Qm);
    return ((n_sym + S - 1) / S + MIX_CHAN_BLOCK - 1) / MIX_CHAN_BLOCK;
}
// ---- noise grids (fused and stand-alone): thread t owns the aligned pair (2c, 2c+1) of the GLOBAL symbol count, c = (first_symbol >> 1) + t.
// The parity of first_symbol is only known on the device: n_sym / 2 + 1 pairs serve either (an even first_symbol touches
// ceil(n_sym / 2) pairs, an odd one n_sym / 2 + 1), and a thread without a symbol in range leaves.
NRLDPC_MIX_HD int64_t mix_chan_pair_wgs(int64_t n_sym) {
    return n_sym > 0 ? (n_sym / 2 + 1 + MIX_CHAN_BLOCK - 1) / MIX_CHAN_BLOCK : 0;
}

struct MixChanWork {
    int32_t cfg; // configuration
    int64_t t;   // thread of the configuration
};
// workgroup wg, thread `thread` of either grid -> its configuration and its thread index there.  prefix as for mix_find: a
// configuration without symbols shares its prefix with the next one and is never found.
NRLDPC_MIX_HD MixChanWork mix_chan_work(const int32_t* prefix, int32_t n, int32_t wg, int32_t thread) {
    MixChanWork w;
    w.cfg = mix_find(prefix, n, wg);
    w.t = (int64_t)(wg - prefix[w.cfg]) * MIX_CHAN_BLOCK + thread;
    return w;
}

// a mapper / demapper thread: its first local symbol and how many of its S symbols exist (0: a surplus thread of the last workgroup)
struct MixChanModemThread {
    int64_t s0;
    int32_t nv;
};
NRLDPC_MIX_HD MixChanModemThread mix_chan_modem_thread(int64_t n_sym, int32_t S, int64_t t) {
    MixChanModemThread th;
    th.s0 = t * S;
    const int64_t left = n_sym - th.s0;
    th.nv = left <= 0 ? 0 : (int32_t)(left < S ? left : S);
    return th;
}

// a noise thread: its Philox counter, the local index of the pair's even symbol (-1 for the first pair of an odd first_symbol) and
// which of the two symbols lie in the segment (neither: a surplus thread)
struct MixChanPairThread {
    uint64_t c;
    int64_t s0;
    bool v0, v1;
};
NRLDPC_MIX_HD MixChanPairThread mix_chan_pair_thread(int64_t n_sym, uint64_t first_symbol, int64_t t) {
    MixChanPairThread th;
    th.c = (first_symbol >> 1) + (uint64_t)t;
    th.s0 = (int64_t)(2 * th.c - first_symbol);
    th.v0 = th.s0 >= 0 && th.s0 < n_sym;
    th.v1 = th.s0 + 1 < n_sym; // (s0 >= -1)
    return th;
}

// element of the bit / LLR arrays (field g) that holds value 0 of local symbol s; symbol index in the symbol / variance arrays
NRLDPC_MIX_HD int64_t mix_chan_g_index(const MixChanRec& c, int64_t s) { return c.g_off + s * c.Qm; }
NRLDPC_MIX_HD int64_t mix_chan_sym_index(const MixChanRec& c, int64_t s) { return c.sym_off + s; }

} // namespace nrldpc

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "nrldpc.h" // nrldpc_mix_chan_point

namespace nrldpc {

// the tables of one grid: the records are shared, each grid has its prefix
struct MixChanTables {
    const MixChanRec* recs;  // device, [n]
    const int32_t* prefix;   // device, [n + 1] workgroups
    int32_t n, n_wg;
};

struct MixChanLlrLaunch { // the fused stage (pair grid)
    MixChanTables t;
    const nrldpc_mix_chan_point* pt; // device, [n]: sigma, inv_n0, seed, first_symbol are read
    const uint8_t* g;
    float* llr;
};
hipError_t launch_mix_chan_awgn_llr(const MixChanLlrLaunch& a, hipStream_t stream);

struct MixChanModLaunch { // mapper (modem grid)
    MixChanTables t;
    const uint8_t* g;
    float* tx;
};
hipError_t launch_mix_chan_modulate(const MixChanModLaunch& a, hipStream_t stream);

struct MixChanAwgnLaunch { // stand-alone noise (pair grid)
    MixChanTables t;
    const nrldpc_mix_chan_point* pt; // device, [n]: variance (without `var`), seed, first_symbol are read
    const float* tx;
    const float* var;                // packed symbol layout, or null
    float* rx;                       // may equal tx
};
hipError_t launch_mix_chan_awgn(const MixChanAwgnLaunch& a, hipStream_t stream);

struct MixChanDemodLaunch { // demapper (modem grid)
    MixChanTables t;
    const nrldpc_mix_chan_point* pt; // device, [n]: variance; not read for the hard decision or with `var`
    const float* rx;
    const float* var;                // packed symbol layout, or null
    void* out;                       // field g: f32 / f16 LLRs or hard-bit bytes
    int32_t method, out_dtype;
};
hipError_t launch_mix_chan_demodulate(const MixChanDemodLaunch& a, hipStream_t stream);

} // namespace nrldpc
#endif

/*
 * nrldpc.h -- C ABI of the MI355X-native NR LDPC codec core (libnrldpc_hip.so).
 *
 * Drop-in boundary for the one hot path of robmaunder/ldpc-3gpp-matlab: the LDPC coding core that
 * the reference's System objects delegate to MathWorks toolbox objects.
 *
 *   nrldpc_create   replaces  comm.LDPCDecoder('ParityCheckMatrix',H,'MaximumIterationCount',it,
 *                             'IterationTerminationCondition','Parity check satisfied')
 *                             NRLDPCDecoder.m:120 (and the commented-out comm.gpu.LDPCDecoder seam at
 *                             :117-121), and comm.LDPCEncoder('ParityCheckMatrix',H) NRLDPCEncoder.m:49.
 *                             H is never materialised: (bg, Z) identify it (NRLDPC.m:433-440,
 *                             get_3gpp_base_graph.m, get_pcm.m).
 *   nrldpc_decode   replaces  step(obj.hLDPCDecoder, cw_tilde)   NRLDPCDecoder.m:265
 *   nrldpc_encode   replaces  step(obj.hLDPCEncoder, c)          NRLDPCEncoder.m:158
 *   nrldpc_destroy  replaces  release() of those toolbox objects
 *
 * Plain pointers and sizes only.  Host-pointer entry points are synchronous; *_dev entry points take
 * device pointers plus a hipStream_t (passed as void*) and are asynchronous on that stream.
 * A handle is not thread-safe; use one handle per GPU / host thread.
 *
 * Error convention (NRLDPC.m / NRLDPCDecoder.m use two MATLAB identifiers; the MEX gateway maps
 * return codes onto exactly those):
 *   NRLDPC_ERR_UNSUPPORTED -> 'ldpc_3gpp_matlab:UnsupportedParameters'  (callers catch and skip:
 *                             plot_BLER_vs_SNR.m:173, testbench.m:51)
 *   NRLDPC_ERR_ARG / _HIP  -> 'ldpc_3gpp_matlab:Error'                  (e.g. NRLDPCDecoder.m:149)
 */
#ifndef NRLDPC_H
#define NRLDPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRLDPC_OK 0
#define NRLDPC_ERR_UNSUPPORTED 1 /* invalid BG / lifting size / layer count / parameter combination */
#define NRLDPC_ERR_ARG 2         /* shape or pointer violation */
#define NRLDPC_ERR_HIP 3         /* HIP runtime failure (text via nrldpc_last_error) */
#define NRLDPC_ERR_NOMEM 4

/* LLR element types accepted at the boundary.  Codeword-contiguous layout [batch][ncols*Z], which
 * is MATLAB's column-major (ncols*Z) x batch.  Positive LLR <=> bit 0 (NRLDPCDecoder.m:262-266):
 * 0 = punctured / untransmitted, +inf = filler bit (known 0). */
#define NRLDPC_LLR_F32 0
#define NRLDPC_LLR_F16 1
#define NRLDPC_LLR_F64 2 /* host entry point only (MATLAB double); narrowed to f32 -- large batches: quantised to the
                            kernels' int8 grid, see nrldpc_quantise_llr -- on the host */

typedef struct nrldpc_codec* nrldpc_handle;

/* ABI revision of this header.  Revision 3 put `struct_size` in front of nrldpc_cfg and nrldpc_dims (revision 2 had
 * grown both at the tail -- beta; alpha, beta -- with nothing a caller built against revision 1 could be told apart by).
 * nrldpc_abi_version() returns the revision the loaded library was built with (the library is loaded by path and has
 * no SONAME; a binding checks this number at load time, as ldpc-3gpp-matlab_amd/_capi.py does).
 * Revision 4 adds nrldpc_decode_packed and the CRC-aided stop (early_term = 2; crc_poly, crc_len, crc_bits at the tail of
 * nrldpc_cfg).
 * Revision 5 makes the active layer count a property of the CALL, not of the handle: nrldpc_set_layers / nrldpc_last_layers /
 * nrldpc_count_layers / nrldpc_pool_set_layers / nrldpc_set_llr_dtype and the value NRLDPC_LAYERS_AUTO (-1) for nrldpc_cfg.n_layers -- see "Active
 * layers" below; and adds nrldpc_pool_decode_packed.  nrldpc_cfg and nrldpc_dims keep their revision-4 layout and size.
 * Revision 6 adds nrldpc_decode_packed_layers (the layer count as an ARGUMENT of one call: nothing sticks to the handle) and
 * nrldpc_pool_set_timing / nrldpc_pool_last_kernel_ms (event-pair kernel times of every shard of a pool) and
 * nrldpc_last_host_phases (the phase times of a large host-pointer call) and nrldpc_payload_bits_dev (the Monte-Carlo loop's payload
 * draw as one kernel); nothing a revision-5 caller uses changed meaning. */
#define NRLDPC_ABI_VERSION 6

/* Active layers.  The reference always decodes the full H (NRLDPCDecoder.m:120).  A base-graph row i >= 4 owns the degree-1
 * extension-parity column kb + i; when every codeword of a call holds LLR 0 in that column (not transmitted: rate matching
 * stopped below it, NRLDPCDecoder.m:216-234) the row's check-to-variable messages are identically zero and the row can be left
 * out -- exactly, for sum-product and min-sum alike -- as can every row above it that is in the same
 * state.  At the reference's own defaults (plot_BLER_vs_SNR.m:29-41: BG2, R = 1/3) that is 21 of 42 rows, at R = 8/9 on BG1 5 of 46.
 *   n_layers = 0 (NRLDPC_LAYERS_ALL): every row;  4..46 / 4..42: that many rows, the caller vouches for the zeros;
 *   NRLDPC_LAYERS_AUTO: read off the data, per call -- n = max(4, c - kb + 1) for the highest base-graph column c of the call's
 *   codewords that holds a value other than +-0 and NaN (NaN is ingested as 0).  Exact for any rv_id, repetition, LBRM or
 *   HARQ-combined buffer because nothing is assumed about how the zeros came about.  Host-pointer entry points scan the caller's
 *   array from the top column down on the copy threads (a column block that is all zero is read once and never quantised or
 *   sent); device-pointer entry points run a pre-pass kernel and read one integer back, i.e. they synchronise `stream` once
 *   before the launch.  With cfg.alpha == 0 the check-node rule follows the count in use (nrldpc_default_rule).
 *   The count under AUTO is ONE number per call -- the maximum over the call's codewords -- so with cfg.alpha == 0 the rule,
 *   and through it a codeword's hard decisions and iteration count, can depend on which other codewords share the call
 *   (leaving rows out is exact; changing the rule is not).  A caller that needs batch-independent results gives the count
 *   (nrldpc_set_layers / nrldpc_decode_packed_layers: what the patched NRLDPCDecoder.m does, from E_r, k_0 and N_cb) or a
 *   fixed rule (cfg.alpha != 0). */
#define NRLDPC_LAYERS_ALL 0
#define NRLDPC_LAYERS_AUTO (-1)

typedef struct nrldpc_cfg {
    uint32_t struct_size; /* = sizeof(nrldpc_cfg); nrldpc_create refuses any other value (NRLDPC_ERR_ARG)      */
    int32_t bg;         /* 1 or 2                                     (NRLDPC.m:28)               */
    int32_t Z;          /* lifting size Z_c, one of the 51 of Table 5.3.2-1 (NRLDPC.m:409-411)    */
    int32_t n_layers;   /* base rows to decode, 4..46 (BG1) / 4..42 (BG2); 0 = all (reference: all); NRLDPC_LAYERS_AUTO = read
                           off each call's LLRs ("Active layers" above); nrldpc_set_layers changes it between calls */
    int32_t max_iter;   /* 'MaximumIterationCount' (NRLDPCDecoder.m:41,120); 1..2000              */
    int32_t early_term; /* 0 = always max_iter iterations; 1 = stop a codeword when all active parity checks hold (the
                           reference: 'Parity check satisfied', NRLDPCDecoder.m:120); 2 = that, or when the CRC of the
                           code block holds on the hard decisions (crc_* below) -- see "CRC-aided stop"              */
    float alpha;        /* min-sum normalisation factor, 0 < alpha <= 1; 0 = choose alpha AND beta by code rate
                           (nrldpc_default_rule: the rule whose BLER sits closest to the reference's sum-product) */
    int32_t llr_scale;  /* fixed-point units per unit LLR: power of two 1..32; 0 = default 8 */
    int32_t llr_dtype;  /* NRLDPC_LLR_*                                                            */
    int32_t device_id;  /* HIP device ordinal                                                      */
    int32_t max_batch;  /* staging capacity of the host entry points; 0 = grow on demand          */
    float beta;         /* min-sum offset in LLR units (>= 0), read only when alpha != 0: message magnitude =
                           max(alpha*min - beta, 0) on the fixed-point grid; 0 = plain normalised min-sum; rounded to
                           the nearest 1/(2*llr_scale) LLR (nrldpc_get_dims reports the value in use)               */
    /* CRC-aided stop, read only when early_term == 2 (else leave 0).  The reference checks a code block's CRC AFTER decoding
     * (CRC24B per code block when C > 1, else the transport block's CRC24A / CRC16: NRLDPCDecoder.m:298-301, 336;
     * get_3gpp_crc_polynomial.m:3-14); here the same check also ends the iterations of a codeword whose information bits are
     * already right while a parity bit is not: after an iteration a codeword is done when its active parity checks hold, OR
     * when the first crc_bits hard decisions (payload followed by its CRC, K' of NRLDPC.m) leave remainder 0 under crc_poly and
     * are not all zero (an all-zero block has remainder 0 whatever was sent; with rv_id 2 / 3 the punctured systematic bits
     * start at a-posteriori 0, i.e. hard decision 0).  Hard decisions and iteration counts are those of the oracle's
     * orc_decode_onmsq_crc.  Measured against the parity-check stop: profiles/r04_crc_stop.json. */
    uint32_t crc_poly;  /* generator polynomial with its x^crc_len term, e.g. CRC24B 0x1800063, CRC24A 0x1864CFB, CRC16 0x11021 */
    int32_t crc_len;    /* L: 24 or 16 for TS 38.212 (6..24 accepted)                                   */
    int32_t crc_bits;   /* K' = payload + CRC bits of the code block, crc_len < crc_bits <= K            */
} nrldpc_cfg;

/* Dimensions implied by (bg, Z): ncols*Z LLRs in, K = kb*Z hard bits out. */
typedef struct nrldpc_dims {
    uint32_t struct_size;     /* in: = sizeof(nrldpc_dims), set by the caller before nrldpc_get_dims */
    int32_t nrows, ncols, kb; /* 46,68,22 or 42,52,10 */
    int32_t i_ls;             /* set index (get_3gpp_set_index.m) */
    int32_t K, N_cw;          /* kb*Z, ncols*Z */
    int32_t n_layers;         /* active layer count of the next call: 4..rows, or NRLDPC_LAYERS_AUTO */
    float alpha, beta;        /* resolved check-node rule (beta in LLR units); under NRLDPC_LAYERS_AUTO with cfg.alpha == 0:
                                 the rule of the last call's count (before the first call: of all rows) */
} nrldpc_dims;

int nrldpc_abi_version(void); /* NRLDPC_ABI_VERSION of the library's build */
int nrldpc_create(const nrldpc_cfg* cfg, nrldpc_handle* out);
void nrldpc_destroy(nrldpc_handle h);
int nrldpc_get_dims(nrldpc_handle h, nrldpc_dims* out);

/* Active layer count of the calls that follow (every decode entry point, nrldpc_decode_multi_dev included): NRLDPC_LAYERS_ALL,
 * 4..rows of the base graph, or NRLDPC_LAYERS_AUTO.  No device work, no reallocation: the kernels take the count as a launch
 * argument.  With cfg.alpha == 0 the check-node rule becomes nrldpc_default_rule(bg, count) -- a call gives bit for bit what a
 * handle created with that n_layers gives.  NRLDPC_ERR_UNSUPPORTED for any other value.
 * (A System object's rate is tunable between step() calls -- G, rv_id: NRLDPC.m:51-85 -- so the count is too.) */
int nrldpc_set_layers(nrldpc_handle h, int32_t n_layers);
/* Decoding algorithm of the calls that follow (every decode entry point of the handle, nrldpc_decode_multi_dev and the pool
 * paths included).  No device work.  These entry points were added without a revision bump (NRLDPC_ABI_VERSION stays 6,
 * nrldpc_cfg keeps its size): a binding detects them by symbol.
 *   NRLDPC_ALG_MIN_SUM (default): the layered offset-normalised min-sum kernels on the int8 grid, unchanged.
 *   NRLDPC_ALG_SUM_PRODUCT: flooding sum-product with the parity-check stop -- the reference's comm.LDPCDecoder
 *     (NRLDPCDecoder.m:120) -- with the semantics of orc_decode_bp_flood_app in oracle/nrldpc_oracle.c, computed in fp32:
 *     - ingest: f32 / f16 as given, host f64 narrowed to f32; NOT quantised (no int8 grid, no llr_scale, no clamp); NaN -> 0,
 *       +inf kept (filler bits).  cfg.alpha, cfg.beta and cfg.llr_scale are not read.  Host-pointer calls never take the
 *       int8 route of large batches (nrldpc_quantise_llr); they send the caller's format.
 *     - messages r (check to variable) start at 0; a sweep: APP = lambda + sum r; q = APP - r_old (an infinite APP stays
 *       infinite); r_new = 2 atanh(prod over the other edges of tanh(q/2)) with the product clamped to +-(1 - 1e-15), i.e.
 *       |r| <= 35.23; every q of a sweep from the same APP (flooding); APP recomputed from r_new.
 *     - stop: early_term = 1 after the first sweep in which every ACTIVE check holds on APP < 0 (the count reported is that
 *       sweep's number); early_term = 0 exactly max_iter sweeps; early_term = 2 is refused (NRLDPC_ERR_UNSUPPORTED, here and
 *       by nrldpc_set_algorithm on such a handle).  Active layers ("Active layers" above) leave rows out as the oracle's
 *       n_layers does; NRLDPC_LAYERS_AUTO finds the count as for min-sum.
 *     - app_out: the a-posteriori LLRs after the last sweep.  Results are bit-identical from run to run and independent of the
 *       batch, its split and its neighbours (no atomics; one fixed order of operations per codeword).
 *     - tolerance against orc_decode_bp_flood_app (double): |APP - APP_ref| <= 1e-3 * max(1, |APP_ref|) on every finite entry,
 *       infinite entries equal, signs equal wherever |APP_ref| > 1e-3.  Measured on an MI355X over BG1 / BG2, 13 lifting sizes
 *       (2 ... 384), all / 4 / an intermediate layer count, 1..3 sweeps at Es/N0 = -3 dB with punctured and filler columns
 *       (234 cases, 1.04e7 entries; tests/test_sum_product_gpu.py): at most 2.9e-6 absolute, 1.6e-6 relative to max(1, |APP_ref|).
 *       The check node runs in the phi domain (phi(x) = -ln tanh(x/2)) with prefix and suffix sums, so fp32 reaches the
 *       oracle's cap; DESIGN.md section 4.10 holds the derivation.
 * NRLDPC_ERR_UNSUPPORTED for any other value. */
#define NRLDPC_ALG_MIN_SUM 0     /* default: the layered offset-normalised min-sum kernels (unchanged) */
#define NRLDPC_ALG_SUM_PRODUCT 1 /* flooding sum-product, the reference's comm.LDPCDecoder (NRLDPCDecoder.m:120) */
int nrldpc_set_algorithm(nrldpc_handle h, int32_t algorithm);
int nrldpc_get_algorithm(nrldpc_handle h, int32_t* algorithm);
/* LLR element type of the calls that follow (NRLDPC_LLR_*; NRLDPC_LLR_F64 for host pointers only): a gateway whose caller holds
 * `single` or `double` arrays hands each over as it is, through one handle (staging buffers grow on demand). */
int nrldpc_set_llr_dtype(nrldpc_handle h, int32_t llr_dtype);
/* The count the most recent decode call of this handle ran with (what NRLDPC_LAYERS_AUTO found); 0 before the first call. */
int nrldpc_last_layers(nrldpc_handle h, int32_t* n_layers);
/* What NRLDPC_LAYERS_AUTO finds for `batch` codewords at the HOST address llr ([batch][ncols*Z] of llr_dtype, NRLDPC_LLR_*):
 * the layer count, 4..rows; -1 on invalid arguments (text via nrldpc_last_error).  Host function, no device needed. */
int nrldpc_count_layers(int32_t bg, int32_t Z, const void* llr, int32_t batch, int32_t llr_dtype);

/* Decode `batch` codewords.  llr: [batch][ncols*Z] of cfg.llr_dtype.  hard: [batch][K] bytes in
 * {0,1} (the K x 1 logical of comm.LDPCDecoder).  iters_out (nullable): iterations executed per
 * codeword.  app_out (nullable): a-posteriori LLRs [batch][ncols*Z] float. */
int nrldpc_decode(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out,
                  float* app_out);
int nrldpc_decode_dev(nrldpc_handle h, const void* d_llr, int32_t batch, uint8_t* d_hard,
                      int32_t* d_iters_out, float* d_app_out, void* stream);
/* nrldpc_decode with BIT-PACKED hard decisions: hard_packed: [batch][ceil(K/8)] bytes, bit k of a codeword in byte k/8 at bit
 * k%8 (least significant first; the unused bits of a codeword's last byte are 0).  The bits are packed on the device, so an
 * eighth of the bytes crosses PCIe and the copy into the caller's array: the form a MEX gateway uses (matlab/nrldpc_mex.cpp
 * unpacks into the K x C logical array the reference's comm.LDPCDecoder returns, NRLDPCDecoder.m:265). */
int nrldpc_decode_packed(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard_packed, int32_t* iters_out);
/* nrldpc_decode_packed with the active layer count of THIS call as an argument (0 all / 4..rows / NRLDPC_LAYERS_AUTO): the
 * handle's own count (cfg.n_layers, nrldpc_set_layers) is neither read nor changed, so a HARQ caller that gives the count for
 * one transmission and omits it for the next gets the handle's default back (ABI revision 6).  The reference's
 * seam is one call per step: step(obj.hLDPCDecoder, cw_tilde), NRLDPCDecoder.m:265 -- the patched LDPC_coding passes the
 * count it derives from E_r, k_0 and N_cb (NRLDPC.m:463-543) here. */
int nrldpc_decode_packed_layers(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard_packed, int32_t* iters_out,
                                int32_t n_layers);

/* ---- whole-codeword hard decisions and final parity checks --------------------------------------------------------------
 * comm.LDPCDecoder's OutputValue = 'Whole codeword' and FinalParityChecksOutputPort: nrldpc_decode[_dev] plus up to three more
 * outputs per codeword, each left out by a null pointer (at least one must be given, else NRLDPC_ERR_ARG).  These entry points
 * were added without a revision bump (NRLDPC_ABI_VERSION stays 6): a binding detects them by symbol, as nrldpc_set_algorithm.
 *   - cw_packed: bit v is APP_v < 0 after the last iteration / sweep, for all N_cw = ncols*Z columns -- the rule the K
 *     information bits follow (+inf and +-0 give 0, -inf gives 1), so the first K bits of cw_packed equal `hard`.  Columns above
 *     the active rows carry the hard decision of what app_out reports for them.
 *   - unsatisfied / checks_packed: the ACTIVE checks on those bits.  "Active" is the layer count the call ran with, which
 *     nrldpc_last_layers reports: given (nrldpc_set_layers), taken from the handle, or found by NRLDPC_LAYERS_AUTO -- once per
 *     call, over the whole batch.  unsatisfied == 0 says the codeword converged on the active rows, whatever the iteration count
 *     (iters < max_iter under early_term = 1 implies it; iters == max_iter alone says nothing).
 *   - hard, iters and every output are bit-identical to what nrldpc_decode_dev with app_out would give (the outputs derived from
 *     app_out by the rule above); they do not depend on the batch or on how it is split.
 *   - early_term == 2 (the CRC-aided stop) is refused with NRLDPC_ERR_UNSUPPORTED, as app_out is.
 *   - NRLDPC_ALG_SUM_PRODUCT: the sum-product kernel writes the outputs itself (no scratch, no second kernel).
 *     NRLDPC_ALG_MIN_SUM: the call runs the soft-output route of the decoder (app_out) into a scratch owned by the handle, then a
 *     finish kernel on the same stream; the scratch holds at most NRLDPC_CW_SCRATCH_BYTES, so the call walks the batch in chunks
 *     of floor(NRLDPC_CW_SCRATCH_BYTES / (4 * N_cw)) codewords (the NRLDPC_LAYERS_AUTO count and the check-node rule are resolved
 *     once, before the first chunk).  This is slower than a plain decode: DESIGN.md section 4.11.  A second call on the same handle
 *     is ordered behind the previous one, whatever its stream.
 * Pool (nrldpc_pool_*) and nrldpc_decode_multi_dev variants do not exist: out of scope.
 * sizeof(nrldpc_cw_out) == 32 on LP64 (the library static_asserts it; a binding can compare its own structure's size). */
#define NRLDPC_CW_SCRATCH_BYTES (64u << 20) /* 64 MiB: bound of the handle-owned scratch of nrldpc_decode_cw[_dev] (min-sum) */
typedef struct nrldpc_cw_out {
    uint32_t struct_size;    /* = sizeof(nrldpc_cw_out); any other value: NRLDPC_ERR_ARG */
    uint8_t* cw_packed;      /* [batch][ceil(N_cw/8)]: bit v of a codeword in byte v/8 at bit v%8 (LSB first); N_cw = ncols*Z is a multiple of
                                4, not of 8, when Z is odd: the unused bits of a codeword's last byte are 0; nullable */
    int32_t* unsatisfied;    /* [batch]: number of ACTIVE checks that fail on the final hard decisions; 0 = converged; nullable */
    uint8_t* checks_packed;  /* [batch][ceil(nrows*Z/8)]: check (l*Z+z) as one bit, same packing; rows >= the active count are 0; nullable */
} nrldpc_cw_out;
/* d_out is a HOST structure whose three pointers are device memory; asynchronous on `stream` (under NRLDPC_LAYERS_AUTO the stream is
 * synchronised once, as by nrldpc_decode_dev).  d_llr: F32 / F16. */
int nrldpc_decode_cw_dev(nrldpc_handle h, const void* d_llr, int32_t batch, uint8_t* d_hard, int32_t* d_iters_out,
                         const nrldpc_cw_out* d_out, void* stream);
/* Host memory throughout; llr in cfg.llr_dtype (F32 / F16 / F64, F64 narrowed to F32 on the host).  The caller's array is staged in
 * its own format: never the int8 wire route of large nrldpc_decode batches.  Synchronous. */
int nrldpc_decode_cw(nrldpc_handle h, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out,
                     const nrldpc_cw_out* out);

/* The quantisation nrldpc_decode applies to large host batches while it copies them into its pinned staging
 * buffers (so that 1 byte per LLR crosses PCIe instead of 4): dst[i] = NaN ? 0 : rint(clamp(float(src[i]) * llr_scale,
 * +-127)) as int8 -- the kernels' own ingest arithmetic, operation for operation -- with +inf (filler bits,
 * NRLDPCDecoder.m:264) as -128.  src: n values of llr_dtype (NRLDPC_LLR_*).  Returns 1 when a -inf was met (int8 has
 * no code for it; nrldpc_decode then sends that chunk in its own format), else 0.  Host function, no device needed. */
int nrldpc_quantise_llr(int8_t* dst, const void* src, int64_t n, int32_t llr_dtype, int32_t llr_scale);

/* Mixed batches: n configurations (handles of one device that may differ in base graph, lifting size, layer
 * count, iteration cap, ...) decoded with one launch per base graph and LLR type instead of n launches --
 * a small bucket alone is a one-workgroup kernel that leaves the GPU idle.  For i < n: batch[i] codewords at
 * d_llr[i] (dtype of h[i]) -> d_hard[i], iteration counts to d_iters[i] when d_iters and d_iters[i] are
 * non-null.  Results are those of n nrldpc_decode_dev calls.  The launch tables go through a ring of four
 * (pinned, device, event) slots owned by h[0], so calls in flight on different streams never share one; asynchronous on
 * `stream`.  (The reference decodes one code block per step(), NRLDPCDecoder.m:257-266; a receiver serving many
 * users holds exactly such a mix of (BG, Z_c).)  A handle set to NRLDPC_ALG_SUM_PRODUCT is decoded by a launch of its own on
 * `stream` -- the result of nrldpc_decode_dev -- while the min-sum handles of the call keep their shared launches. */
int nrldpc_decode_multi_dev(int32_t n, const nrldpc_handle* h, const void* const* d_llr, const int32_t* batch,
                            uint8_t* const* d_hard, int32_t* const* d_iters, void* stream);

/* ---- one node, several GPUs: codeword batches shard with no collective --------------------
 * A pool owns one codec handle and one host thread per entry of device_ids (an ordinal may repeat: several logical
 * shards on one GPU).  nrldpc_pool_decode cuts the batch into n_devices * chunks_per_device contiguous chunks and the
 * threads pull them from a queue, so that shards which finish early under early termination (BASELINE.json
 * configs[4]) take more chunks; results land in place, identical to one nrldpc_decode call.  cfg->device_id is
 * ignored.  The reference decodes one code block at a time on one thread (NRLDPCDecoder.m:257-266). */
typedef struct nrldpc_pool* nrldpc_pool_handle;
int nrldpc_pool_create(const nrldpc_cfg* cfg, const int32_t* device_ids, int32_t n_devices, int32_t chunks_per_device,
                       nrldpc_pool_handle* out);
int nrldpc_pool_decode(nrldpc_pool_handle p, const void* llr, int32_t batch, uint8_t* hard, int32_t* iters_out);
/* nrldpc_pool_decode with bit-packed hard decisions ([batch][ceil(K/8)], as nrldpc_decode_packed): what a MEX gateway calls */
int nrldpc_pool_decode_packed(nrldpc_pool_handle p, const void* llr, int32_t batch, uint8_t* hard_packed, int32_t* iters_out);
/* nrldpc_set_layers for every handle of the pool.  Under NRLDPC_LAYERS_AUTO the count is found ONCE per call over the whole
 * batch (host form: before the chunks are dealt; device form: every shard scans its slice, the maximum is taken, then every
 * shard launches), so the result does not depend on how the batch is cut. */
int nrldpc_pool_set_layers(nrldpc_pool_handle p, int32_t n_layers);
/* nrldpc_set_algorithm for every handle of the pool (added without a revision bump, as nrldpc_set_algorithm) */
int nrldpc_pool_set_algorithm(nrldpc_pool_handle p, int32_t algorithm);
/* The same for data that is already ON the devices: shard i (entry i of device_ids) decodes batch[i] codewords from
 * d_llr[i] into d_hard[i] (and d_iters[i] when d_iters and d_iters[i] are non-null); every pointer of shard i is
 * device memory of device_ids[i], in cfg.llr_dtype (F32 / F16).  One host thread per shard launches on the shard's
 * own stream; the call returns when every shard's stream is idle.  Ordering: the shard streams are private, so each shard
 * first waits (hipDeviceSynchronize on its device) for everything the caller has ALREADY submitted to that device -- LLRs a
 * kernel of the caller's is still writing when the call is made are complete before the decoder reads them; work submitted
 * from another thread DURING the call is not ordered against it.  No host copy, no collective: this is the form that
 * scales with the number of GPUs (the host-pointer form above is bounded by the host's copy bandwidth). */
int nrldpc_pool_decode_dev(nrldpc_pool_handle p, const void* const* d_llr, const int32_t* batch, uint8_t* const* d_hard,
                           int32_t* const* d_iters);
/* Kernel timing for a pool (nrldpc_set_timing for every shard's handle): when enabled, each shard records a HIP event pair
 * around its decode kernel on the shard's own launch stream; nrldpc_pool_last_kernel_ms writes the duration of every shard's
 * last launch to ms[0 .. n_devices-1] (0 for a shard that had no work).  This is how a one-process, N-GPU caller -- bench.py
 * --in-process -- gets per-GPU kernel times without a process group. */
int nrldpc_pool_set_timing(nrldpc_pool_handle p, int32_t enabled);
int nrldpc_pool_last_kernel_ms(nrldpc_pool_handle p, float* ms);
int nrldpc_pool_size(nrldpc_pool_handle p); /* number of shards (n_devices of nrldpc_pool_create) */
/* codewords each shard (entry of device_ids) decoded in the last nrldpc_pool_decode call; counts: [n_devices] */
int nrldpc_pool_last_split(nrldpc_pool_handle p, int32_t* counts);
void nrldpc_pool_destroy(nrldpc_pool_handle p);

/* Systematic encode.  info: [batch][K] bytes {0,1}; cw: [batch][ncols*Z] bytes {0,1} = [info;parity]
 * with H*cw = 0 (NRLDPCEncoder.m:158).  Only bit 0 of an input byte is read: a byte b encodes as b & 1, and
 * every output byte, the systematic copy included, is 0 or 1.  Neither pointer needs any alignment. */
int nrldpc_encode(nrldpc_handle h, const uint8_t* info, int32_t batch, uint8_t* cw);
int nrldpc_encode_dev(nrldpc_handle h, const uint8_t* d_info, int32_t batch, uint8_t* d_cw, void* stream);

/* ---- stages either side of the core; stateless, current HIP device ---- */
#define NRLDPC_MAX_C 160 /* code blocks per transport block */

/* Parameters of one transport block as the reference derives them (NRLDPC.m:297-543). */
typedef struct nrldpc_tb_params {
    int32_t bg, Z;           /* BG, Z_c */
    int32_t A, B, C;         /* payload, payload + TB CRC, code blocks */
    int32_t K, K_prime, N;   /* per code block: K, K', N */
    int32_t N_cb, k_0;       /* circular buffer length and start (NRLDPC.m:463-469, 510-543) */
    int32_t Q_m, G;          /* bits per symbol, total rate-matched bits */
    int32_t tb_crc_len;      /* 16 or 24 (CRC16 / CRC24A, NRLDPC.m:297-303) */
    int32_t cb_crc_len;      /* 0 or 24 (CRC24B when C > 1, NRLDPC.m:347-353) */
    int32_t E_r[NRLDPC_MAX_C]; /* NRLDPC.m:485-507 */
} nrldpc_tb_params;

/* Rate recovery: replaces code_block_concatenation + bit_interleaving + bit_selection (NRLDPCDecoder.m:143-242)
 * and the 2Z-zero prefix / NaN->+inf of LDPC_coding (:262-264).  d_g_tilde: [n_tb][G] f32 LLRs.
 * d_harq (nullable = I_HARQ 0): [n_tb][C][N_cb] f32 soft buffer, accumulated in place (:236-239).
 * d_cw_llr: [n_tb*C][ncols*Z] of out_dtype (NRLDPC_LLR_F32 / _F16): the decoder core's input.
 * For f16 demodulator LLRs or an f16 soft buffer see nrldpc_rate_recover_ex_dev below. */
int nrldpc_rate_recover_dev(const nrldpc_tb_params* p, const float* d_g_tilde, int32_t n_tb, float* d_harq,
                            void* d_cw_llr, int32_t out_dtype, void* stream);

/* The same stage with the element type of every array chosen per call: in_dtype (d_g_tilde), harq_dtype (d_harq; not read when
 * d_harq is null) and out_dtype (d_cw_llr) each take NRLDPC_LLR_F32 or NRLDPC_LLR_F16.  Added without a revision bump
 * (NRLDPC_ABI_VERSION stays 6): a binding finds it by symbol.  nrldpc_rate_recover_dev itself is unchanged.
 *   f16 input   is widened to f32, which is exact; the same sums then run in the same order as in nrldpc_rate_recover_dev:
 *               repetitions in ascending k, then the buffer.
 *   f16 buffer  for a non-filler position p inside the circular buffer: val = (f32 sum of what this transmission delivers to p) +
 *               float(buffer[p]), one f32 add; buffer[p] = half(clamp(val, +-65504)), round to nearest even; the decoder's LLR at p
 *               is the stored value widened.  The decoder always sees exactly what the buffer holds, so a later call that delivers
 *               nothing to p reproduces it.  Filler positions of the buffer are never touched; their output is +inf, as ever.
 *   clamp rule  this entry point clamps a finite value to +-65504 before ANY conversion to f16, for the buffer and for the output --
 *               the demapper's rule for the same reason: +inf means "filler bit, known 0" to the decoder, and soft combining over
 *               retransmissions is where magnitudes grow.  With (in_dtype, harq_dtype) = (F32, F32) the call equals
 *               nrldpc_rate_recover_dev bit for bit, buffer included, wherever that call's output is finite or a filler; where that
 *               call overflows an f16 output to +-inf, this one gives +-65504.
 *   addresses   any address the element types allow is served: an f16 array may sit at an odd multiple of 2 bytes (rows of
 *               d_g_tilde do when G is odd, rows of the buffer when N_cb is odd -- limited-buffer rate matching), and a sub-range
 *               of a larger allocation works.
 *   Non-finite input LLRs: unspecified (the demapper never produces them).
 * Errors, all before any device call: a dtype other than F32 / F16 -> NRLDPC_ERR_UNSUPPORTED; null p, negative n_tb, null d_cw_llr
 * or null d_g_tilde (with G > 0) when n_tb > 0 -> NRLDPC_ERR_ARG; the parameter checks of nrldpc_rate_recover_dev with the same
 * texts.  n_tb == 0 returns NRLDPC_OK without a launch. */
int nrldpc_rate_recover_ex_dev(const nrldpc_tb_params* p, const void* d_g_tilde, int32_t in_dtype, int32_t n_tb,
                               void* d_harq, int32_t harq_dtype, void* d_cw_llr, int32_t out_dtype, void* stream);

/* CRC stages: replaces code_block_segmentation + crc_calculation of the decoder (NRLDPCDecoder.m:271-340).
 * d_c_hat: [n_tb*C][K] hard bits from nrldpc_decode_dev.  d_b_hat: [n_tb][B] bytes (a_hat = first A of a row).
 * d_ok: [n_tb], 0 where the reference returns [] (TB CRC or any CB CRC failed).  d_cb_pass (nullable):
 * [n_tb][C] per-code-block CRC flags (code_block_CRC_passed, :95). */
int nrldpc_crc_check_dev(const nrldpc_tb_params* p, const uint8_t* d_c_hat, int32_t n_tb, uint8_t* d_b_hat,
                         int32_t* d_ok, int32_t* d_cb_pass, void* stream);

/* The same stage with the reference's state machine (NRLDPCDecoder.m:283-316,337), for incremental redundancy
 * (I_HARQ ~= 0) and code-block-group retransmission (CBGTI):
 *   cbgti_flags (host, C bytes, nullable = all 1): CBGTI_flags of NRLDPC.m:471-477; a code block is taken over --
 *       payload written to d_b_hat, pass flag set -- only when its CRC holds (C > 1) AND its flag is 1 (:304);
 *   keep_b_hat != 0 (I_HARQ ~= 0): d_b_hat is in/out, the b_hat_buffer of :286-287,311-313 -- segments of blocks
 *       not taken over keep what an earlier step stored; 0: those segments are zeroed (:289);
 *   d_cb_pass (required): in/out, the sticky code_block_CRC_passed of :280,305,315 -- the caller zeroes it at
 *       reset() (:355); d_ok[tb] = TB CRC of the resulting b_hat holds and every flag is set (:337).
 * nrldpc_crc_check_dev is this call with no CBGTI, keep_b_hat = 0 and d_cb_pass as a plain output. */
int nrldpc_crc_check_harq_dev(const nrldpc_tb_params* p, const uint8_t* d_c_hat, int32_t n_tb, uint8_t* d_b_hat,
                              int32_t* d_ok, int32_t* d_cb_pass, const uint8_t* cbgti_flags, int32_t keep_b_hat,
                              void* stream);

/* ---- mixed transport-block batches: rate recovery and the CRC stage in one launch each -------------------------------------
 * nrldpc_decode_multi_dev decodes a mix of (BG, Z_c) in a handful of launches; these entry points do the same for the stages either
 * side of it, for a batch whose transport blocks differ in (BG, A, G, Q_m, rv_id, LBRM, C).  A MIX PLAN is built once from n
 * parameter blocks and n transport-block counts, is immutable, owns the device-side tables and defines ONE packed layout for every
 * array of the receive chain; the stage calls take the plan and base pointers only.  nrldpc_decode_multi_dev sits between them
 * unchanged: its d_llr[i], d_hard[i], d_iters[i] are base + off[i].cw / .c_hat / .cb of the same packed arrays.
 * Added without a revision bump (NRLDPC_ABI_VERSION stays 6): a binding finds the functions by symbol.
 *
 * Layout.  Configuration i's segment of each array is exactly the array the single-configuration call takes; segments follow in the
 * caller's order; off[0] is 0 in every field; off[i+1].x = round_up(off[i].x + size_i.x, 16) ELEMENTS, so every segment starts 16-byte
 * aligned for every element type; entry [n] holds the totals (what to allocate).  Rows inside a segment keep whatever alignment G,
 * N_cb and N_cw give them (odd G with f16 input: rows at odd multiples of 2 bytes).  n_tb[i] == 0 takes no room and does no work;
 * G == 0 is legal (testbench.m:35).  Gap elements are never read or written.
 *
 * Semantics, by equality.  nrldpc_mix_rate_recover_dev leaves in every segment -- output and soft buffer -- bit for bit what
 *   nrldpc_rate_recover_ex_dev(&p[i], g + off[i].g, in_dtype, n_tb[i], harq ? harq + off[i].harq : NULL, harq_dtype, cw + off[i].cw,
 *   out_dtype, stream) leaves: the same f32 sums in the same order (repetitions in ascending k, then the buffer), the same clamp
 *   before any conversion to f16, fillers +inf, filler positions of the buffer untouched; with (F32, F32) it therefore equals
 *   nrldpc_rate_recover_dev too.  (The environment knobs of the single-configuration launch rule are not read.)
 * nrldpc_mix_crc_check_dev leaves in b_hat, ok and cb_pass what nrldpc_crc_check_dev leaves per configuration.
 * One launch per stage call, whatever n; exactly one thread reads and writes each buffer position, no atomics: results are the same
 * from run to run and do not depend on which configurations share the plan or on how a mix is split into plans.
 *
 * Refusals.  nrldpc_mix_layout and nrldpc_mix_create refuse before any device call: for a parameter block the code and text the
 * single-configuration calls give for it (their parameter checks, E_r / G checks and the CRC length / B checks) with
 * " (configuration i)" appended; a negative n or n_tb[i], or null arrays with n > 0: NRLDPC_ERR_ARG.  n == 0 is a valid empty plan:
 * both stage calls on it return NRLDPC_OK without a launch.  Stage calls: a dtype other than F32 / F16 -> NRLDPC_ERR_UNSUPPORTED
 * (harq_dtype is not read when d_harq is null); a null base pointer whose array is not empty -> NRLDPC_ERR_ARG.
 *
 * Concurrency.  The plan's tables are uploaded synchronously by nrldpc_mix_create and never written again: calls in flight on several
 * streams may share one plan (each with its own arrays).  The stage calls only enqueue: no allocation, copy or synchronisation.
 *
 * HARQ and CBGTI.  nrldpc_mix_rate_recover_harq_dev and nrldpc_mix_crc_check_harq_dev (below the plain calls, which are unchanged in
 * bits and in code path) carry the reference decoder's state machine -- d_tilde_buffer, b_hat_buffer, the sticky
 * code_block_CRC_passed, CBGTI_flags and reset (NRLDPCDecoder.m:236-239, 286-316, 337, 343-356) -- per TRANSPORT BLOCK of the mix.
 * Added without a revision bump as well.  Two flag arrays, both on the device (per-configuration host arrays do not fit a kernel
 * argument block at n ~ 100), both nullable:
 *   d_new    one byte per transport block in the packed `tb` layout (configuration i's flags start at element off[i].tb); non-zero =
 *            this transport block starts a new HARQ process in this step; NULL = none does.
 *   d_cbgti  one byte per code block in the packed `cb` layout (at off[i].cb + tb*C + r): the CBGTI_flags of NRLDPC.m:471-477, per
 *            transport block; NULL = all 1.
 * Rate recovery: a transport block whose flag is 0 gets, in every segment, bit for bit what nrldpc_mix_rate_recover_dev leaves with the
 *   same buffer.  For a flagged one, output and buffer at every non-filler position are bit for bit what nrldpc_rate_recover_ex_dev
 *   leaves on a buffer that held +0.0 in every position of that block's [C][N_cb] rows: a position that receives nothing ends as +0,
 *   a delivered -0.0 ends as +0 too (-0 + +0), the same clamp before any conversion to f16.  The old contents of a flagged block's
 *   rows are never read (NaN or stale data there reaches nothing), so starting a new process costs no memset pass and no second
 *   launch.  Filler positions of the buffer are never touched, flagged or not.  d_new == NULL equals nrldpc_mix_rate_recover_dev bit
 *   for bit.  d_harq is required whenever the plan's harq total is non-zero.
 * CRC stage: for a transport block with new = 0, b_hat, ok and cb_pass are what nrldpc_crc_check_harq_dev(&p[i], ..., n_tb = 1,
 *   cbgti_flags = that block's C flags, keep_b_hat = 1) leaves on that block's rows -- a code block is taken over only when its CRC
 *   holds (C > 1) and its flag is 1; segments not taken over keep what they held and enter the transport-block CRC with those bits;
 *   cb_pass is ORed with its old value.  For new = 1: the same call with keep_b_hat = 0 on a cb_pass row zeroed first -- the
 *   reference's reset() followed by a step, for that transport block alone.  When all transport blocks of a configuration share flags
 *   and new, the call equals one nrldpc_crc_check_harq_dev per configuration.  d_cb_pass is required (in/out): a null one with a
 *   non-empty cb array -> NRLDPC_ERR_ARG with the single call's text.
 * Both: one launch per call whatever n, one thread per buffer position, no atomics, results independent of how a mix is split into
 *   plans, gap elements never read or written, enqueue only; null base pointers of non-empty arrays and bad dtypes are refused as in
 *   the plain calls (harq_dtype always: the buffer is required), before any device call; on the empty plan both return NRLDPC_OK
 *   without a launch.
 * rv_id.  A plan stays immutable.  rv_id only moves k_0, and no field of nrldpc_mix_layout depends on it: a HARQ receiver holds one
 *   plan per redundancy version (per distinct tuple of rv_ids, at most a handful) over the SAME packed arrays.
 *
 * Out of scope: pool variants, a one-launch mixed encoder (the transmit side itself is nrldpc_mix_tx_*, below), the MEX gateway, a G
 * that changes between retransmissions. */
typedef struct nrldpc_mix* nrldpc_mix_handle;

/* element offsets of configuration i inside the packed arrays; entry [n] holds the totals */
typedef struct nrldpc_mix_offsets {
    int64_t g;      /* g_tilde        [n_tb][G]              */
    int64_t harq;   /* soft buffer    [n_tb][C][N_cb]        */
    int64_t cw;     /* codeword LLRs  [n_tb*C][ncols*Z]   = d_llr[i]  of nrldpc_decode_multi_dev */
    int64_t c_hat;  /* hard decisions [n_tb*C][K]         = d_hard[i]                            */
    int64_t cb;     /* one value per code block [n_tb*C]: d_iters[i], cb_pass                    */
    int64_t b_hat;  /* [n_tb][B]                                                                 */
    int64_t tb;     /* one value per transport block [n_tb]: ok                                  */
} nrldpc_mix_offsets;                       /* sizeof == 56 (the library static_asserts it) */

/* host function, no device: off has n + 1 entries */
int nrldpc_mix_layout(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, nrldpc_mix_offsets* off);

int nrldpc_mix_create(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int32_t device_id, nrldpc_mix_handle* out);
void nrldpc_mix_destroy(nrldpc_mix_handle m);

int nrldpc_mix_rate_recover_dev(nrldpc_mix_handle m, const void* d_g_tilde, int32_t in_dtype,
                                void* d_harq /* nullable */, int32_t harq_dtype,
                                void* d_cw_llr, int32_t out_dtype, void* stream);
int nrldpc_mix_crc_check_dev(nrldpc_mix_handle m, const uint8_t* d_c_hat, uint8_t* d_b_hat,
                             int32_t* d_ok, int32_t* d_cb_pass /* nullable */, void* stream);

/* the HARQ / CBGTI forms ("HARQ and CBGTI" above) */
int nrldpc_mix_rate_recover_harq_dev(nrldpc_mix_handle m, const void* d_g_tilde, int32_t in_dtype,
                                     void* d_harq, int32_t harq_dtype, void* d_cw_llr, int32_t out_dtype,
                                     const uint8_t* d_new /* nullable */, void* stream);
int nrldpc_mix_crc_check_harq_dev(nrldpc_mix_handle m, const uint8_t* d_c_hat, uint8_t* d_b_hat, int32_t* d_ok,
                                  int32_t* d_cb_pass /* required, in/out */, const uint8_t* d_cbgti /* nullable */,
                                  const uint8_t* d_new /* nullable */, void* stream);

/* ---- mixed HARQ steps that decode only the code blocks still pending -------------------------------------------------------------
 * Between nrldpc_mix_rate_recover_harq_dev and nrldpc_mix_crc_check_harq_dev the decoder decodes every code block of every transport
 * block, also those whose hard decisions the CRC stage then throws away (CBGTI flag 0, NRLDPCDecoder.m:304) and those acknowledged
 * rounds ago.  These three calls turn the HARQ state into a DENSE batch and back: nrldpc_mix_pending_dev compacts the pending code
 * blocks of every configuration into an index list and a count, nrldpc_mix_gather_cw_dev copies their LLR rows to the front of each
 * configuration's segment of a second packed array, nrldpc_decode_multi_dev decodes batch[i] = count[i] rows there (it accepts
 * batch[i] == 0), and nrldpc_mix_scatter_hard_dev puts the hard decisions back at their rows.  Added without a revision bump
 * (NRLDPC_ABI_VERSION stays 6): a binding finds the functions by symbol.  The plain and HARQ stage calls above are unchanged.
 *
 * The rule.  For code block r of transport block tb of configuration i (packed index cb = off[i].cb + tb*C + r) let
 *   f = d_cbgti ? d_cbgti[cb] != 0 : 1      w = d_new ? d_new[off[i].tb + tb] != 0 : 0
 *   p = d_cb_pass[cb] != 0                  o = d_ok[off[i].tb + tb] != 0          allp = all C blocks of the transport block have p
 * NRLDPC_MIX_SKIP_UNSCHEDULED: pending = f.  Reads neither d_cb_pass nor d_ok.  The CRC stage never takes a block with f = 0 over, so
 *   b_hat, ok and cb_pass of a step are bit for bit what the step that decodes everything leaves, always.
 * NRLDPC_MIX_SKIP_SETTLED: pending = f && (w || (!o && (C == 1 || !p || allp))): a scheduled block is decoded when its transport block
 *   starts a new process; otherwise when the transport block is not yet acknowledged and the block is its only one (C == 1: there is
 *   no code-block CRC, cb_pass says nothing), or has not passed, or all blocks passed and the transport-block CRC still fails (the
 *   whole transport block is decoded again).  d_ok is the PREVIOUS step's ok array: that makes it state, zero after a reset.
 *   DEVIATION from the reference: a settled block keeps the hard decisions of the step in which it settled (its row of d_c_hat) instead
 *   of being decoded again on the combined buffer.  The two differ only when the re-decode would pass its CRC with other bits, or,
 *   for C == 1, when the re-decode of an acknowledged block would fail.
 *
 * nrldpc_mix_pending_dev: d_index[off[i].cb + j], j < d_count[i], is the local row tb*C + r of the j-th pending block of configuration
 *   i, in ascending order; entries from d_count[i] on and gap elements are not written; d_count has n entries.
 * Dense arrays use the SAME packed layout and totals as the full ones: configuration i's dense rows start at off[i].cw / .c_hat / .cb and
 *   there are d_count[i] of them, so the base pointers given to nrldpc_decode_multi_dev do not depend on the counts.
 * nrldpc_mix_gather_cw_dev: dense row j of configuration i = row d_index[off[i].cb + j] of d_cw_llr, bit for bit (f32 or f16; NaN
 *   payloads, infinities and -0.0 survive); dense rows from d_count[i] on are not written, the source is not written.
 * nrldpc_mix_scatter_hard_dev: row d_index[off[i].cb + j] of d_c_hat = dense row j (K bytes).  Rows of blocks that are not pending are
 *   NOT written: d_c_hat is in/out and keeps their earlier decisions.  With d_iters: the count of a block that is not pending
 *   becomes 0, that of a pending block is d_iters_dense's (left as it is when d_iters_dense is null).
 * All three: the counts are read on the device; one launch per call whatever n, enqueue only (no allocation, copy or
 *   synchronisation); one writer per position, no atomics; results independent of how a mix is split into plans; gap elements never
 *   read or written; the plan stays immutable and shareable between streams.  d_index and d_count must be what nrldpc_mix_pending_dev
 *   left for the same plan (an index outside its configuration is not followed).
 * Refusals, before any device call: a rule other than the two -> NRLDPC_ERR_UNSUPPORTED; a dtype other than F32 / F16 ->
 *   NRLDPC_ERR_UNSUPPORTED; a null pointer of a required array of a non-empty plan -> NRLDPC_ERR_ARG (SETTLED requires d_cb_pass and
 *   d_ok); on a plan without transport blocks all three return NRLDPC_OK without a launch and write nothing, d_count included.
 * Out of scope: pool variants, the MEX gateway, the single-configuration chain (a plan with n = 1 serves it), rate recovery writing
 *   dense rows directly (it would save the gather, but changes an existing kernel). */
#define NRLDPC_MIX_SKIP_UNSCHEDULED 1
#define NRLDPC_MIX_SKIP_SETTLED 2
int nrldpc_mix_pending_dev(nrldpc_mix_handle m, int32_t rule,
                           const int32_t* d_cb_pass, const int32_t* d_ok, /* SETTLED: required; UNSCHEDULED: not read */
                           const uint8_t* d_cbgti /* nullable */, const uint8_t* d_new /* nullable */,
                           int32_t* d_index /* packed cb layout */, int32_t* d_count /* [n] */, void* stream);
int nrldpc_mix_gather_cw_dev(nrldpc_mix_handle m, const void* d_cw_llr, int32_t dtype,
                             const int32_t* d_index, const int32_t* d_count, void* d_cw_dense, void* stream);
int nrldpc_mix_scatter_hard_dev(nrldpc_mix_handle m, const uint8_t* d_c_hat_dense, const int32_t* d_iters_dense /* nullable */,
                                const int32_t* d_index, const int32_t* d_count,
                                uint8_t* d_c_hat /* in/out */, int32_t* d_iters /* nullable */, void* stream);

/* Transmit-side counterparts (vector generation for the Monte-Carlo harness, plot_BLER_vs_SNR.m:129):
 * nrldpc_crc_attach_dev replaces crc_calculation + code_block_segmentation of the encoder
 * (NRLDPCEncoder.m:70-124): d_a [n_tb][A] bits -> d_c [n_tb*C][K] code blocks (fillers 0), ready for
 * nrldpc_encode_dev.  nrldpc_rate_match_dev replaces bit_selection + bit_interleaving +
 * code_block_concatenation (NRLDPCEncoder.m:168-256): d_cw [n_tb*C][ncols*Z] -> d_g [n_tb][G]. */
int nrldpc_crc_attach_dev(const nrldpc_tb_params* p, const uint8_t* d_a, int32_t n_tb, uint8_t* d_c, void* stream);
int nrldpc_rate_match_dev(const nrldpc_tb_params* p, const uint8_t* d_cw, int32_t n_tb, uint8_t* d_g, void* stream);

/* ---- mixed transport-block batches, transmit side: CRC attach and rate matching in one launch each ----------------------------
 * The transmit mirror of nrldpc_mix_*: for a batch whose transport blocks differ in (BG, A, G, Q_m, rv_id, LBRM, C), a TRANSMIT PLAN
 * is built once from n parameter blocks and n transport-block counts, is immutable, owns its device-side tables, and serves three
 * stage calls that take the plan and base pointers only.  nrldpc_mix_tx_handle is a type of its own; the receive plan, its layout
 * and nrldpc_mix_create are unchanged.  Added without a revision bump (NRLDPC_ABI_VERSION stays 6): a binding finds the functions by
 * symbol.
 *
 * Layout.  Only the payload array a ([n_tb][A] bytes per configuration) is new: a_off[0] = 0, a_off[i+1] = round_up(a_off[i] +
 *   n_tb[i]*A_i, 16), entry [n] = the total (nrldpc_mix_tx_layout; host only).  Every other transmit array reuses a field of
 *   nrldpc_mix_layout element for element: code blocks c [n_tb*C][K] = field c_hat, codeword bytes [n_tb*C][ncols*Z] = field cw,
 *   rate-matched bits g [n_tb][G] = field g -- a loop-back hands g to a channel and on to the receive plan of the same (p, n_tb).
 *
 * Semantics, by equality.  In every segment
 *   nrldpc_mix_tx_crc_attach_dev leaves in c  what nrldpc_crc_attach_dev(&p[i], a + a_off[i], n_tb[i], c + off[i].c_hat, stream) leaves,
 *   nrldpc_mix_tx_encode_dev     leaves in cw what nrldpc_encode_dev(h[i], c + off[i].c_hat, n_tb[i]*C_i, cw + off[i].cw, stream) leaves,
 *   nrldpc_mix_tx_rate_match_dev leaves in g  what nrldpc_rate_match_dev(&p[i], cw + off[i].cw, n_tb[i], g + off[i].g, stream) leaves,
 *   bit for bit.  Only bit 0 of an input byte is read and every output byte is 0 or 1.  Gap elements are never read or written; one
 *   thread writes each output byte, no atomics: results are the same from run to run and do not depend on which configurations share
 *   the plan or on how a mix is split into plans.  These are byte arrays: any byte address of the base pointers is served.
 *   Attach and rate matching are ONE launch each whatever n.  The encode stage has no kernel of its own: it launches the existing
 *   encoder once per non-empty configuration, in configuration order, on the caller's stream; h[i] may repeat for configurations that
 *   share (BG, Z_c) and is not read for an empty one.
 *
 * Refusals.  nrldpc_mix_tx_layout and nrldpc_mix_tx_create refuse what nrldpc_mix_layout / nrldpc_mix_create refuse, with the same
 *   codes and texts (" (configuration i)" appended to the single-configuration call's text; NRLDPC_ERR_ARG for negative counts or null
 *   arrays; "too large for one launch"), and add the transmit stages' own per block: a code block shorter than the transport-block CRC
 *   (nrldpc_crc_attach_dev's text) and a Q_m outside {1, 2, 4, 6, 8} -> NRLDPC_ERR_UNSUPPORTED.  The first broken block is the one
 *   reported.  n == 0 or all counts zero is a valid empty plan that needs no device: every stage call on it returns NRLDPC_OK without
 *   a launch.  Stage calls refuse, before any device call: a null plan; a null base pointer whose array is not empty; for the encode
 *   stage, naming the configuration, a null handle of a non-empty configuration, a handle whose (BG, Z) differs from the
 *   configuration's, a handle on another device than the plan -> NRLDPC_ERR_ARG.
 *
 * Concurrency.  The plan's tables are one device allocation, uploaded synchronously by nrldpc_mix_tx_create and never written again:
 *   calls in flight on several streams may share one plan (each with its own arrays).  The stage calls only enqueue.
 *
 * Out of scope: a one-launch mixed encoder, pool variants, the MEX gateway, a mixed-batch channel stage. */
typedef struct nrldpc_mix_tx* nrldpc_mix_tx_handle;

/* host function, no device: a_off has n + 1 entries (elements = bytes of the payload array) */
int nrldpc_mix_tx_layout(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int64_t* a_off);

int nrldpc_mix_tx_create(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int32_t device_id, nrldpc_mix_tx_handle* out);
void nrldpc_mix_tx_destroy(nrldpc_mix_tx_handle m);

int nrldpc_mix_tx_crc_attach_dev(nrldpc_mix_tx_handle m, const uint8_t* d_a, uint8_t* d_c, void* stream);
int nrldpc_mix_tx_encode_dev(nrldpc_mix_tx_handle m, const nrldpc_handle* h /* [n] */, const uint8_t* d_c, uint8_t* d_cw, void* stream);
int nrldpc_mix_tx_rate_match_dev(nrldpc_mix_tx_handle m, const uint8_t* d_cw, uint8_t* d_g, void* stream);

/* ---- the transmit plan's encode stage in ONE launch -------------------------------------------------------------------------------
 * Added after the block above was written, again without a revision bump (a binding finds the function by symbol).  The
 * per-configuration call nrldpc_mix_tx_encode_dev remains and behaves as described there; this call is the same stage with a kernel
 * of its own, table driven like attach and rate matching, and takes no handle array: the base-graph tables and the solve order of
 * every distinct (BG, Z_c) among the non-empty configurations are built by nrldpc_mix_tx_create and live in the plan's one device
 * allocation, uploaded once and never written again -- streams may share a plan as before.
 *
 * Semantics, by equality.  nrldpc_mix_tx_encode_all_dev(m, c, cw, stream) leaves cw as nrldpc_mix_tx_encode_dev(m, h, c, cw, stream)
 *   leaves it: in every segment what nrldpc_encode_dev(h[i], c + off[i].c_hat, n_tb[i]*C_i, cw + off[i].cw, stream) leaves, bit for
 *   bit.  Only bit 0 of an input byte is read and every output byte is 0 or 1.  Gap bytes are never read or written; one thread
 *   writes each output byte, no atomics.  Any byte address of the base pointers is served: every codeword takes, at its real
 *   addresses, the copy, ring-build and store forms the single call takes there.  ONE launch whatever n; the call only enqueues.
 *   Waves per codeword follow the single call's rule (four for BG1 from Z = 128 on, else one); the NRLDPC_ENC_NWC experiment knob is
 *   not read.
 *
 * Refusals, before any device call: a null plan; a null base pointer whose array is not empty -> NRLDPC_ERR_ARG.  The empty plan
 *   returns NRLDPC_OK without a launch and without a device.
 *
 * Which to call: DESIGN.md section 4.18 holds the measurement (a mix of many configurations against a uniform batch). */
int nrldpc_mix_tx_encode_all_dev(nrldpc_mix_tx_handle m, const uint8_t* d_c, uint8_t* d_cw, void* stream);

/* Channel leg of the Monte-Carlo loop, fused: replaces step(hMod,g), step(hChan,tx),
 * step(hDemod,rx) of plot_BLER_vs_SNR.m:130-132 -- NRModulator.m:73-81 (TS 38.211 maps, unit average power),
 * comm.AWGNChannel at EsN0_dB (:50,105), NRDemodulator.m:76-84 (exact LLRs, Variance = 10^(-EsN0/10), :106).
 * d_g: n_bits rate-matched bits (bytes {0,1}), n_bits a multiple of Q_m in {1,2,4,6,8}; d_g_tilde: n_bits f32 LLRs,
 * positive = bit 0.  Noise: Philox-4x32-10 keyed by `seed`, counter = first_symbol + symbol index, Box-Muller --
 * the same (seed, symbol) always sees the same noise, whatever the batch split.  Current HIP device. */
int nrldpc_awgn_llr_dev(const uint8_t* d_g, int64_t n_bits, int32_t Q_m, float EsN0_dB, uint64_t seed,
                        uint64_t first_symbol, float* d_g_tilde, void* stream);
/* Payload of the Monte-Carlo loop: replaces `a = round(rand(A,1))` of plot_BLER_vs_SNR.m:118 for n_tb transport blocks at once.
 * d_a: [n_tb][A] bytes {0,1}; bit i of the block with GLOBAL index first_block + b is bit (i mod 64) of
 * splitmix64(seed + ((first_block + b) * ceil(A/64) + i div 64 + 1) * 0x9E3779B97F4A7C15) -- the same (seed, block) always draws the
 * same payload, whatever the batch split (MATLAB's Mersenne-Twister stream cannot be replicated outside MATLAB: SURVEY.md 8c; curves
 * are compared statistically).  Current HIP device.  (ABI revision 6.) */
int nrldpc_payload_bits_dev(uint64_t seed, uint64_t first_block, int32_t n_tb, int32_t A, uint8_t* d_a, void* stream);

/* The channel leg's two ends on their own, for a caller whose channel is not the library's (a capture, an equaliser's output, a
 * fading model): the mirrors of NRModulator.m and NRDemodulator.m.  Stateless, current HIP device, asynchronous on `stream`.
 * Added without a revision bump (a binding finds them by symbol); nothing an earlier caller uses changed.
 *
 * nrldpc_modulate_dev: d_g, n_bits bits (bytes {0,1}, the rate-matching stage's output), n_bits a multiple of Q_m in {1,2,4,6,8}
 * -> d_tx, n_bits/Q_m symbols as interleaved float (re, im) pairs (complex64), unit average power.  Maps of NRModulator.m:73-81:
 * BPSK +-e^{j pi/4}; QPSK and the QAMs one Gray-coded PAM rail per axis (TS 38.211 5.1.3-5.1.5), even bits on I, odd bits on Q,
 * sign bit first, scaled by 1/sqrt(2 mean(level^2)).  Within two float roundings of the float64 map (tested: 4e-7 per component).
 *
 * nrldpc_demodulate_dev: d_rx, n_sym symbols (re, im) -> n_sym*Q_m values in d_out, by `method` (DecisionMethod, NRDemodulator.m:10):
 *   NRLDPC_DEMOD_LLR         exact: per rail the log-sum-exp over its 2^(Q_m/2) levels, maximum subtracted -- the arithmetic of the
 *                            fused kernel; LLR = log P(bit 0) - log P(bit 1), positive = bit 0, as everywhere in the library;
 *   NRLDPC_DEMOD_APPROX_LLR  max-log: (min over the levels with bit 1 of d^2 - min over those with bit 0 of d^2) / N0; equal to the
 *                            exact value for BPSK and QPSK (one level per bit value);
 *   NRLDPC_DEMOD_HARD        bit = 1 exactly when the max-log LLR is < 0: the nearest constellation point, a tie gives 0 (so the
 *                            sign bit of the max-log f32 LLR of the same input is the hard bit).  d_out: bytes {0,1}; out_dtype and the
 *                            variance are not read.
 * N0 is the complex noise variance (Variance, NRDemodulator.m:14,94-96): `variance` for every symbol, or, when d_variance is not
 * null, d_variance[s] for symbol s (device, n_sym floats; replaces the scalar) -- equalised symbols, fading.  An array filled with
 * one value gives the scalar call's bits.  Non-finite symbols and non-positive array entries: unspecified.
 * out_dtype NRLDPC_LLR_F32 or NRLDPC_LLR_F16; an f16 LLR is clamped to +-65504 before conversion (a strong symbol must not become
 * +inf, which the decoder reads as a filler bit: LLR conventions above).  Any address the element types allow and any n_sym >= 0
 * are served, sub-ranges of a buffer included, and a call over a buffer equals calls over its parts bit for bit.
 * Accuracy of both LLR methods against float64 (tests/test_modem_gpu.py, the fused kernel's operating points, BPSK -2 dB to
 * 256QAM 45 dB): |dLLR| <= 5e-4 * max(1, |LLR|) for f32 (measured maximum: DESIGN.md section 4.12), plus 2^-11 |LLR| for f16.
 * Errors, all before any device call: Q_m not in {1,2,4,6,8} ("Unsupported modulation", NRModulator.m:83), unknown method,
 * out_dtype other than F32 / F16 -> NRLDPC_ERR_UNSUPPORTED; n_bits no multiple of Q_m, a negative size, a null pointer with a
 * non-zero size, d_variance == NULL and `variance` not positive and finite -> NRLDPC_ERR_ARG.  A zero size returns NRLDPC_OK without
 * a launch. */
#define NRLDPC_DEMOD_LLR 0         /* 'Log-likelihood ratio'             (NRDemodulator.m:10) */
#define NRLDPC_DEMOD_APPROX_LLR 1  /* 'Approximate log-likelihood ratio' */
#define NRLDPC_DEMOD_HARD 2        /* 'Hard decision' */
int nrldpc_modulate_dev(const uint8_t* d_g, int64_t n_bits, int32_t Q_m, float* d_tx /* [n_bits/Q_m][2] */, void* stream);
int nrldpc_demodulate_dev(const float* d_rx /* [n_sym][2] */, int64_t n_sym, int32_t Q_m, int32_t method,
                          float variance, const float* d_variance /* [n_sym], nullable */,
                          void* d_out /* [n_sym*Q_m]: out_dtype for the two LLR methods, uint8 {0,1} for HARD */,
                          int32_t out_dtype /* NRLDPC_LLR_F32 / _F16; not read for HARD */, void* stream);

/* The middle of the channel leg on its own: step(hChan, tx) of plot_BLER_vs_SNR.m:131, the mirror of comm.AWGNChannel.
 * rx[s] = tx[s] + w[s] for n_sym symbols as interleaved float (re, im) pairs (complex64).  Stateless, current HIP device,
 * asynchronous on `stream`.  Added without a revision bump (a binding finds it by symbol); nothing an earlier caller uses changed.
 *
 * Noise: w is exactly the noise nrldpc_awgn_llr_dev draws for the same (seed, first_symbol).  The global index of local symbol s is
 * first_symbol + s; the aligned pair (2c, 2c+1) of the global index shares one Philox-4x32-10 block, key = seed, counter
 * (c, c >> 32, 0, 0); words 0,1 feed the even symbol, words 2,3 the odd one; a word becomes the 24-bit uniform
 * ((w >> 8) + 0.5) / 2^24; Box-Muller on the two uniforms of a symbol (the hardware's log2 / sqrt / sin / cos) gives its two rails,
 * each scaled by sigma = sqrt(N0 / 2).  Each noise component is rounded to f32 and added to the symbol with one f32 add.
 * N0 is the complex noise variance: `variance` for every symbol, or, when d_variance is not null, d_variance[s] for symbol s (device,
 * n_sym floats; replaces the scalar) -- what nrldpc_demodulate_dev accepts.  sigma is formed from the f32 N0 on the device in both
 * cases: an array filled with one value gives the scalar call's bits.  variance == 0 gives rx == tx as numbers.
 * A call over a buffer equals calls over its parts bit for bit at any split, given each part's own first_symbol.  Any float-aligned
 * address and any n_sym >= 0 are served.  d_rx == d_tx (in place) is allowed; any other overlap is unspecified.
 * nrldpc_demodulate_dev(NRLDPC_DEMOD_LLR, variance = N0) of nrldpc_awgn_dev(nrldpc_modulate_dev(g), N0, seed, first_symbol) agrees with
 * nrldpc_awgn_llr_dev(g, EsN0_dB, seed, first_symbol) for N0 = 10^(-EsN0_dB/10) within |dLLR| <= 1e-3 * max(1, |LLR|)
 * (tests/test_awgn_gpu.py; measured maximum: DESIGN.md section 4.14).
 * Errors, all before any device call, NRLDPC_ERR_ARG: a negative n_sym; a null d_tx or d_rx with n_sym > 0; d_variance == NULL and
 * `variance` negative or not finite; first_symbol + n_sym overflowing 64 bits.  n_sym == 0 returns NRLDPC_OK without a launch.
 * Non-positive or non-finite array entries, and non-finite symbols: unspecified. */
int nrldpc_awgn_dev(const float* d_tx /* [n_sym][2] */, int64_t n_sym,
                    float variance, const float* d_variance /* [n_sym], nullable */,
                    uint64_t seed, uint64_t first_symbol,
                    float* d_rx /* [n_sym][2]; may equal d_tx */, void* stream);

/* ---- mixed transport-block batches, the channel leg: one launch per stage ------------------------------------------------------------
 * The leg between the transmit plan (nrldpc_mix_tx_*) and the receive plan (nrldpc_mix_*) for a batch whose transport blocks differ
 * in modulation order and operating point: the four calls above -- nrldpc_awgn_llr_dev, nrldpc_modulate_dev, nrldpc_awgn_dev,
 * nrldpc_demodulate_dev -- over every configuration of a mix in ONE launch each.  (The transmit-plan block above lists "a mixed-batch
 * channel stage" as out of scope; this block, added after it, is that stage.)  A CHANNEL PLAN is built from the same (n, p[], n_tb[])
 * as the other two plans, is immutable and owns one device allocation of tables, uploaded synchronously by nrldpc_mix_chan_create and
 * never written again: calls in flight on several streams may share one plan.  nrldpc_mix_chan_handle is a type of its own; the
 * receive and transmit plans are unchanged.  Added without a revision bump (NRLDPC_ABI_VERSION stays 6): a binding finds the
 * functions by symbol.
 *
 * Layout.  Bits and LLRs use field g of nrldpc_mix_layout element for element: the transmit plan's packed g goes in, the receive
 *   plan's packed g_tilde comes out.  Only the symbol array is new: configuration i holds n_sym_i = n_tb[i]*G_i/Q_m_i symbols (a
 *   symbol never straddles transport blocks: E_r is a multiple of Q_m); sym_off[0] = 0, sym_off[i+1] = round_up(sym_off[i] + n_sym_i,
 *   16) in SYMBOLS, entry [n] = the total (nrldpc_mix_chan_layout; host only).  Symbol s of configuration i is the float pair at
 *   2*(sym_off[i] + s), its entry in a per-symbol variance array the float at sym_off[i] + s.  Gap elements are never read or
 *   written.  nrldpc_mix_offsets keeps its 56 bytes.
 *
 * Operating points vary per call and are not part of the plan: one 32-byte nrldpc_mix_chan_point per configuration in a caller-owned
 *   DEVICE array of n records (host arrays do not fit a kernel argument block at n ~ 100).  nrldpc_mix_chan_point_set (host only) does
 *   the host arithmetic of nrldpc_awgn_llr_dev: n0 = pow(10, -EsN0_dB/10) in double, then variance = (float)n0, sigma =
 *   (float)sqrt(n0/2), inv_n0 = (float)(1/n0), each narrowed once; "EsN0_dB out of range" outside (-60, 80) dB.  A caller with its own
 *   noise figure writes variance, seed and first_symbol directly (the stand-alone stages read no other field).  Records are read on
 *   the device and not validated there: non-positive or non-finite values, and first_symbol + n_sym_i past 2^64, are unspecified, as
 *   for the per-symbol arrays of the single calls.
 *
 * Semantics, by equality.  In every segment
 *   nrldpc_mix_chan_awgn_llr_dev   leaves what nrldpc_awgn_llr_dev(g + off[i].g, n_tb[i]*G_i, Q_m_i, EsN0_i, seed_i, first_symbol_i,
 *                                  g_tilde + off[i].g, stream) leaves, for the EsN0_i the record was set from,
 *   nrldpc_mix_chan_modulate_dev   leaves what nrldpc_modulate_dev(g + off[i].g, n_tb[i]*G_i, Q_m_i, tx + 2*sym_off[i], stream) leaves,
 *   nrldpc_mix_chan_awgn_dev       leaves what nrldpc_awgn_dev(tx + 2*sym_off[i], n_sym_i, pt[i].variance, d_variance ? d_variance +
 *                                  sym_off[i] : NULL, seed_i, first_symbol_i, rx + 2*sym_off[i], stream) leaves; d_rx == d_tx is allowed,
 *   nrldpc_mix_chan_demodulate_dev leaves what nrldpc_demodulate_dev(rx + 2*sym_off[i], n_sym_i, Q_m_i, method, pt[i].variance,
 *                                  d_variance ? d_variance + sym_off[i] : NULL, out + off[i].g (in elements of the output type),
 *                                  out_dtype, stream) leaves: all three methods, f32 or clamped f16 LLRs, hard-bit bytes; d_pt is not
 *                                  read for NRLDPC_DEMOD_HARD, nor when d_variance is given,
 *   bit for bit.  The mapper, the noise stage and the demapper are compiled without floating-point contraction, as their single forms
 *   are: every operation is one IEEE operation or one deterministic hardware instruction.  The fused stage is compiled with
 *   contraction allowed, as nrldpc_awgn_llr_dev's kernel is; its equality with that kernel rests on the compiler fusing the same
 *   multiply-adds in the shared per-symbol code, which it does (the floating-point instruction sequences of the two code objects are
 *   equal, profiles/r10_mix_chan_isa.txt, and tests/test_mix_chan_gpu.py holds the two to bit equality on the device): the contract
 *   of the fused stage is BIT EQUALITY as well, not the fall-back tolerance.
 *   Each call is one launch whatever n and only enqueues (no allocation, copy or synchronisation); one writer per element, no atomics;
 *   results do not depend on which configurations share a plan or on how a mix is split into plans.  Any address the element types
 *   allow is served: any byte address for bit and hard-bit arrays, 2-byte for f16, 4-byte for floats.
 *
 * Refusals, all before any device call.  nrldpc_mix_chan_layout and nrldpc_mix_chan_create refuse what nrldpc_mix_layout /
 *   nrldpc_mix_create refuse, with the same codes and texts and " (configuration i)" appended, and a Q_m outside {1, 2, 4, 6, 8} with
 *   "Unsupported modulation (configuration i)", NRLDPC_ERR_UNSUPPORTED; a mix too large for one launch gets the existing text.  n == 0
 *   or all counts zero is a valid empty plan that needs no device: every stage call on it returns NRLDPC_OK without a launch.  Stage
 *   calls refuse a null plan, a null base pointer of a non-empty array and a null d_pt where it is read with NRLDPC_ERR_ARG, an unknown
 *   method or a dtype other than F32 / F16 with NRLDPC_ERR_UNSUPPORTED and the single calls' texts.
 *
 * Out of scope: pool variants, the MEX gateway, a mixed payload draw, f16 output of the fused stage, a fused form with per-symbol
 *   variance.  (Of these, a mixed payload draw has been supplied since: nrldpc_mix_tx_payload_dev, in the Monte-Carlo block below.)
 *   Measurements against the loop of single calls: DESIGN.md section 4.20. */
typedef struct nrldpc_mix_chan* nrldpc_mix_chan_handle;

typedef struct nrldpc_mix_chan_point {
    float variance;               /* N0: read by the stand-alone noise and demapper stages */
    float sigma, inv_n0;          /* sqrt(N0/2), 1/N0 as nrldpc_awgn_llr_dev forms them: read by the fused stage */
    uint32_t reserved;            /* 0 */
    uint64_t seed, first_symbol;  /* Philox key; global index of the configuration's local symbol 0 */
} nrldpc_mix_chan_point;          /* sizeof == 32 (the library static_asserts it) */

/* host functions, no device: sym_off has n + 1 entries (in symbols) */
int nrldpc_mix_chan_layout(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int64_t* sym_off);
int nrldpc_mix_chan_point_set(float EsN0_dB, uint64_t seed, uint64_t first_symbol, nrldpc_mix_chan_point* out);

int nrldpc_mix_chan_create(int32_t n, const nrldpc_tb_params* p, const int32_t* n_tb, int32_t device_id, nrldpc_mix_chan_handle* out);
void nrldpc_mix_chan_destroy(nrldpc_mix_chan_handle m);

int nrldpc_mix_chan_awgn_llr_dev(nrldpc_mix_chan_handle m, const uint8_t* d_g, const nrldpc_mix_chan_point* d_pt,
                                 float* d_g_tilde, void* stream);
int nrldpc_mix_chan_modulate_dev(nrldpc_mix_chan_handle m, const uint8_t* d_g, float* d_tx, void* stream);
int nrldpc_mix_chan_awgn_dev(nrldpc_mix_chan_handle m, const float* d_tx, const nrldpc_mix_chan_point* d_pt,
                             const float* d_variance /* nullable, packed symbol layout */, float* d_rx /* may equal d_tx */, void* stream);
int nrldpc_mix_chan_demodulate_dev(nrldpc_mix_chan_handle m, const float* d_rx, int32_t method, const nrldpc_mix_chan_point* d_pt,
                                   const float* d_variance /* nullable */, void* d_out /* field g */, int32_t out_dtype, void* stream);

/* ---- mixed transport-block batches, the Monte-Carlo loop's own two stages: payload draw and outcome latch ----------------------------
 * What plot_BLER_vs_SNR.m:118-137 does around the encoder, the channel and the decoder, for every configuration of a mix at once: the
 * payload draw (nrldpc_payload_bits_dev per configuration, in ONE launch) and the per-block bookkeeping of the HARQ loop -- latch a_hat
 * on the first attempt whose transport-block CRC holds, OR the acknowledgements, compare with the payload, count who still
 * retransmits -- which the single-configuration harness writes as tensor expressions.  Both calls hang off the TRANSMIT plan
 * (nrldpc_mix_tx_handle), which already owns the payload layout a_off, A_i, n_tb[i] and the receive layout's offsets; the plan's
 * tables grow by one 40-byte record per configuration and one prefix table.  Added without a revision bump (NRLDPC_ABI_VERSION stays
 * 6): a binding finds the functions by symbol.  With the transmit, channel and receive stages above, a Monte-Carlo point on a mix is a
 * number of launches that does not depend on n (harness.simulate_point_mixed).
 *
 * nrldpc_mix_tx_payload_dev.  d_draw: a caller-owned DEVICE array of n 16-byte records, read on the device and not validated there (a
 *   per-call operating point, as nrldpc_mix_chan_point is).  Semantics, by equality: segment i of d_a is bit for bit what
 *     nrldpc_payload_bits_dev(d_draw[i].seed, d_draw[i].first_block, n_tb[i], A_i, d_a + a_off[i], stream)
 *   leaves, first_block >= 2^32 included.  One launch whatever n; gap bytes are never written; any byte address of d_a is served (a
 *   chunk of four bits is one 4-byte store where it is whole and its real address is a multiple of four, a byte loop otherwise -- the
 *   rule, and the hash, are one shared copy with the single kernel: csrc/nrldpc_payload_bits.h).
 *
 * nrldpc_mix_tx_outcome_dev.  d_a, d_a_hat: the packed payload layout (a_off); d_b_hat: field b_hat; d_ok, d_done, d_good: field tb
 *   (d_ok is what the CRC stage wrote: int32; d_done and d_good are bytes).  With j = off[i].tb + t the packed index of transport block
 *   t of configuration i:
 *     was = first ? 0 : d_done[j] != 0;   now = d_ok[j] != 0;
 *     if (now && !was)  the A_i bytes at d_a_hat + a_off[i] + t*A_i become the first A_i bytes of the b_hat row at off[i].b_hat + t*B_i;
 *     d_done[j] = was || now;
 *     d_good[j] = d_done[j] && the a_hat row equals the a row byte for byte;
 *     d_left[i] = the number of t < n_tb[i] with d_done == 0 after the call (0 for an empty configuration); nullable.
 *   A block with neither `was` nor `now` has none of its rows read or written.  With first != 0 the old contents of d_done and d_a_hat
 *   are never read: stale bytes there reach nothing, and a new batch costs no memset pass (as d_new in the HARQ stages).  Exactly
 *   harness.simulate_point_device's bookkeeping per transport block.  Integers only, one writer per byte, no atomics; d_left is summed
 *   in block order by one wave per configuration in a second small launch: at most two launches whatever n, one when d_left is null.
 *
 * Both calls only enqueue (no allocation, copy or synchronisation); calls in flight on several streams may share the plan.
 * Refusals, all before any device call: a null plan, a null base pointer of a non-empty array, a null d_draw with a non-empty plan ->
 *   NRLDPC_ERR_ARG.  The empty plan returns NRLDPC_OK without a launch and writes nothing, d_left included.
 * Out of scope: pool and multi-GPU variants, the MEX gateway.  Measurements: DESIGN.md section 4.21. */
typedef struct nrldpc_mix_draw {
    uint64_t seed, first_block;   /* splitmix64 seed; global index of the configuration's transport block 0 */
} nrldpc_mix_draw;                /* sizeof == 16 (the library static_asserts it) */

int nrldpc_mix_tx_payload_dev(nrldpc_mix_tx_handle m, const nrldpc_mix_draw* d_draw /* [n], device */,
                              uint8_t* d_a /* packed a layout */, void* stream);
int nrldpc_mix_tx_outcome_dev(nrldpc_mix_tx_handle m, const uint8_t* d_a, const uint8_t* d_b_hat /* field b_hat */,
                              const int32_t* d_ok /* field tb */, int32_t first,
                              uint8_t* d_a_hat /* in/out, a layout */, uint8_t* d_done /* in/out, tb layout */,
                              uint8_t* d_good /* out, tb layout */, int32_t* d_left /* out, [n], nullable */, void* stream);

/* Kernel timing: when enabled, every *_dev / host call records HIP events around its kernel on the
 * launch stream; nrldpc_last_kernel_ms synchronises on the stop event and returns the duration. */
int nrldpc_set_timing(nrldpc_handle h, int32_t enabled);
int nrldpc_last_kernel_ms(nrldpc_handle h, float* ms);
/* Where the handle's last LARGE host-pointer call (nrldpc_decode / nrldpc_decode_packed[_layers] above 8 MB: the chunked pipeline)
 * spent its time -- what NRLDPC_HOST_TRACE=1 prints, as numbers (ABI revision 6): out10[0] chunks, [1] codewords per chunk, [2] layers
 * decoded, then milliseconds of the CALLER's thread: [3] NRLDPC_LAYERS_AUTO scan, [4] copy / quantise into pinned memory incl. the
 * H2D enqueue, [5] kernel launch + D2H enqueue, [6] waiting for the device, [7] copying results out; [8] NUMA node the copy
 * threads are pinned to, [9] CPU the caller ran on.  NRLDPC_ERR_ARG when no such call has been made on the handle. */
int nrldpc_last_host_phases(nrldpc_handle h, double* out10);

/* Check-node rule nrldpc_create applies when cfg.alpha == 0, by base graph and active layer count (0 = all):
 * the (alpha, beta) pair measured closest to flooding sum-product (the reference's comm.LDPCDecoder,
 * NRLDPCDecoder.m:120) at equal iteration caps; DESIGN.md section 6 holds the measurements.  beta in LLR units. */
int nrldpc_default_rule(int32_t bg, int32_t n_layers, float* alpha, float* beta);

/* Parameter helpers shared with the host-side chain (no device work). */
int nrldpc_set_index(int32_t Z);                        /* get_3gpp_set_index.m:5-11; -1 if invalid  */
int nrldpc_lifting_size(int32_t K_b, int32_t K_prime);  /* get_3gpp_lifting_size.m:5-16; -1 if none */

const char* nrldpc_strerror(int code);
const char* nrldpc_last_error(void); /* text of the most recent failure on this thread */
const char* nrldpc_version(void);
const char* nrldpc_build_id(void);   /* hash of the sources this binary was built from (build.py: source_id) */
const char* nrldpc_kernel_id(void);  /* hash of the decoder kernels' sources alone (build.py: kernel_id): ties a rocprofv3
                                        summary under profiles/ to the kernels it measured */

#ifdef __cplusplus
}
#endif
#endif /* NRLDPC_H */

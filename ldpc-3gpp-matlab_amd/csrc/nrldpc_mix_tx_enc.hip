// nrldpc_mix_tx_enc.hip -- the encoder for a MIX of transport-block configurations in ONE launch (nrldpc_mix_tx_encode_all_dev;
// semantics: include/nrldpc.h): the stage between nrldpc_mix_tx_crc_attach_dev and nrldpc_mix_tx_rate_match_dev
// (nrldpc_mix_tx.hip).  nrldpc_mix_tx_encode_dev, which launches nrldpc_encode_kernel once per configuration, remains.
//
// Table driven like the other mixed kernels.  A record per configuration (segment offsets, codeword count, Z and the base graph's
// sizes, where its (BG, Z_c) tables lie, the solve order, waves per codeword), a prefix table over workgroups and the base-graph
// tables of every distinct (BG, Z_c) live in the plan's device allocation, uploaded once by nrldpc_mix_tx_create and never written
// again.  Every thread finds its workgroup's configuration by a binary search of the prefix (nrldpc_mix_tx.h: mix_tx_enc_work); the
// record is read through workgroup-uniform addresses in the CONSTANT address space -- nothing writes the plan's tables while a kernel
// runs, so every load of a field is a scalar load wherever it stands, as the single-configuration kernel reads EncArgs from its kernel
// arguments (a copy of the record taken up front held 31 words of solve order in SGPRs throughout: 106 SGPRs, 8 spilled, 7 waves per
// SIMD; this form: 86, none, 8) -- and one switch on its waves per codeword picks the NWC-templated body.
//
// The body is nrldpc_encode_kernel<NWC>'s (nrldpc_encode.hip) with the EncArgs fields taken from the record and its phases unchanged:
// table into LDS, systematic copy, ring build, the four core rows, the byte-domain dual-diagonal solve, extension rows, expansion.  The
// info and output pointers are formed per codeword from the segment offsets, and every alignment decision of that kernel -- the
// 16 / 4 / 1-byte copy, the word or ballot ring build, the dword or byte extension store -- is taken per codeword on the real
// addresses in the same order: a codeword of a packed segment runs the path it runs in the single call at the same address, and is
// left bit for bit the same.  One thread writes each output byte; no atomics.
//
// Why a copy and not a function both units call: as for nrldpc_mix_tx.hip -- sharing a body with a single-configuration kernel changed
// that kernel's instructions.  nrldpc_encode.hip is untouched; tests/test_mix_tx_encode_gpu.py holds the two
// to equality on every path class of tests/tx_cases.py.
//
// The workgroup's LDS is the plan-wide maximum; each codeword slot's region is carved with its OWN configuration's layout inside it.
// The one __syncthreads() behind the table load stands in the kernel, before the switch: all four waves reach it, whichever of them
// have a codeword (the ragged last workgroup of a configuration).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "nrldpc_mix_tx.h"
#include "nrldpc_wave.h"

namespace nrldpc {

static_assert(sizeof(MixTxEncRec) % 8 == 0, "records are laid out as an array with int64 members");

__device__ __forceinline__ int mix_tx_enc_rotz(int z, int p, int Z) {
    int v = z + p;
    return v >= Z ? v - Z : v;
}

// a record of the plan's device tables, read-only for the lifetime of the plan
typedef const MixTxEncRec __attribute__((address_space(4))) MixTxEncRecC;

// one codeword: wave `wave` of the workgroup (NWC = 1: alone; NWC = 4: with the other three).  tw: the table in LDS (edge words, row
// pointers), already complete.
template <int NWC>
__device__ __forceinline__ void mix_tx_encode_codeword(MixTxEncRecC& r, const MixTxEncLayout& L, uint32_t* tw, const uint8_t* c_base,
                                                       uint8_t* cw_base, int cw, int wave, int lane) {
    static_assert(NWC == 1 || NWC == 4, "a codeword is served by one wave or by the whole workgroup");
    constexpr int GT = 64 * NWC; // threads that serve one codeword
    // what separates two phases of a codeword: its own wave's LDS order, or the workgroup's barrier
    auto group_sync = [] {
        if constexpr (NWC == 1) wave_lds_sync();
        else __syncthreads();
    };
    const int Z = r.Z, kb = r.kb, nrows = r.nrows;
    const int W = L.W, DW = L.DW;
    const uint32_t* rp = tw + r.nnz;                // row pointers
    const int slot = wave / NWC, wv = wave % NWC;   // codeword of the workgroup, wave within its group
    const int gl = wv * 64 + lane;                  // thread within the group
    if (cw < 0) return;                             // (NWC = 4: the whole workgroup, together)
    uint32_t* wbase = tw + mix_tx_enc_slot_word(L, slot);
    uint32_t* D = wbase + L.D;
    uint32_t* lamP = wbase + L.lam;
    uint32_t* PP = wbase + L.PP;
    uint8_t* xc = reinterpret_cast<uint8_t*>(wbase + L.xc);
    const uint8_t* info = c_base + mix_tx_enc_info_index(r.c_off, r.kb, r.Z, cw);
    uint8_t* out = cw_base + mix_tx_enc_out_index(r.cw_off, r.ncols, r.Z, cw);

    // 1. systematic part straight to the output, widest copies both alignments allow
    {
        const int n = kb * Z;
        const uintptr_t al = reinterpret_cast<uintptr_t>(info) | reinterpret_cast<uintptr_t>(out);
        int done = 0;
        if ((al & 15) == 0) {
            for (int i = gl; i < (n >> 4); i += GT) {
                uint4 v = reinterpret_cast<const uint4*>(info)[i];
                v.x &= 0x01010101u; v.y &= 0x01010101u; v.z &= 0x01010101u; v.w &= 0x01010101u;
                reinterpret_cast<uint4*>(out)[i] = v;
            }
            done = n & ~15;
        } else if ((al & 3) == 0) {
            for (int i = gl; i < (n >> 2); i += GT)
                reinterpret_cast<uint32_t*>(out)[i] = reinterpret_cast<const uint32_t*>(info)[i] & 0x01010101u;
            done = n & ~3;
        }
        for (int i = done + gl; i < n; i += GT) out[i] = info[i] & 1u;
    }

    // 2. doubled bit rings of `ncol` byte columns at src -> D[c0 ..]; the byte reads of a batch of ballots are
    // issued together (global loads for the systematic part, LDS reads for the core parity)
    const int idx0 = lane % Z, step = 64 % Z;
    auto pack_b = [&](auto src, int c0, int ncol, auto batch) {
        constexpr int PB = decltype(batch)::value;
        for (int c = wv; c < ncol; c += NWC) { // a ballot is a wave's: whole columns per wave
            int idx = idx0;
            for (int w0 = 0; w0 < DW / 2; w0 += PB) {
                uint8_t b[PB];
#pragma unroll
                for (int k = 0; k < PB; ++k) {
                    b[k] = src[c * Z + idx];
                    idx += step;
                    if (idx >= Z) idx -= Z;
                }
#pragma unroll
                for (int k = 0; k < PB; ++k) {
                    const unsigned long long m = __ballot(b[k] & 1u);
                    if (w0 + k < DW / 2 && lane < 2) D[(c0 + c) * DW + 2 * (w0 + k) + lane] = (uint32_t)(m >> (32 * lane));
                }
            }
        }
    };
    auto pack = [&](auto src, int c0, int ncol) { // batch size: 2 ballots cover Z <= 48, 7 + 6 cover Z = 384
        if (DW <= 4) pack_b(src, c0, ncol, std::integral_constant<int, 2>{});
        else pack_b(src, c0, ncol, std::integral_constant<int, 7>{});
    };
    // XOR over the edges of base row i with column < col_limit of the 32-bit windows starting at ring bit 32m;
    // edge words and windows are read in batches so that their LDS latencies overlap
    constexpr int EB = 5;
    auto row_word = [&](int i, int m, int col_limit) {
        uint32_t acc = 0;
        const int e1 = rp[i + 1];
        for (int e0 = rp[i]; e0 < e1; e0 += EB) {
            uint32_t t[EB], lo[EB], hi[EB];
#pragma unroll
            for (int k = 0; k < EB; ++k) t[k] = tw[e0 + k < e1 ? e0 + k : e1 - 1];
#pragma unroll
            for (int k = 0; k < EB; ++k) {
                const int s = 32 * m + (int)(t[k] >> 8);
                const uint32_t* d = D + (t[k] & 0xff) * DW + (s >> 5);
                const bool on = (e0 + k < e1) && (int)(t[k] & 0xff) < col_limit;
                lo[k] = on ? d[0] : 0u;
                hi[k] = on ? d[1] : 0u;
                t[k] = s & 31;
            }
#pragma unroll
            for (int k = 0; k < EB; ++k) acc ^= __builtin_amdgcn_alignbit(hi[k], lo[k], t[k]);
        }
        return acc;
    };
    auto bit_of = [&](const uint32_t* P, int z) { return (P[z >> 5] >> (z & 31)) & 1u; };

    // Z a multiple of 32: a ring word is 32 consecutive bytes of a column, so a lane builds whole words from two 16-byte loads
    // -- ((w & 0x01010101) * 0x01020408) >> 24 squeezes 4 byte-bits into a nibble -- instead of one byte load and one ballot per bit
    const bool words32 = (Z & 31) == 0;
    auto squeeze = [](uint32_t w) { return ((w & 0x01010101u) * 0x01020408u) >> 24; };
    auto put_word = [&](int c, int m, uint32_t v) { // ring word m of column c into every slot of the doubled ring it fills
        for (int w = m; w < DW; w += W) D[c * DW + w] = v;
    };
    if (words32 && (reinterpret_cast<uintptr_t>(info) & 15) == 0) {
        for (int it = gl; it < kb * W; it += GT) {
            const int c = it / W, m = it - c * W;
            const uint4* s4 = reinterpret_cast<const uint4*>(info + (size_t)c * Z + 32 * m);
            const uint4 lo = s4[0], hi = s4[1];
            put_word(c, m, squeeze(lo.x) | squeeze(lo.y) << 4 | squeeze(lo.z) << 8 | squeeze(lo.w) << 12 |
                               squeeze(hi.x) << 16 | squeeze(hi.y) << 20 | squeeze(hi.z) << 24 | squeeze(hi.w) << 28);
        }
    } else {
        pack(info, 0, kb);
    }
    group_sync();
    // 3a. lambda_i = systematic part of core row i
    for (int it = gl; it < 4 * W; it += GT) {
        const int i = it / W, m = it - i * W;
        lamP[it] = row_word(i, m, kb);
    }
    group_sync();
    // 3b. dual-diagonal core in the byte domain: the sum of the four rows isolates p0, the other three
    // blocks follow by substitution
    for (int z = gl; z < Z; z += GT) {
        const uint32_t tot = bit_of(lamP, z) ^ bit_of(lamP + W, z) ^ bit_of(lamP + 2 * W, z) ^ bit_of(lamP + 3 * W, z);
        xc[mix_tx_enc_rotz(z, r.ord.p0_shift, Z)] = (uint8_t)tot;
    }
    group_sync();
    // (unrolled: every index into the solve order is a constant)
#pragma unroll
    for (int st = 0; st < 3; ++st) {
        const int i = r.ord.step_row[st], u = r.ord.step_col[st], nk = r.ord.step_nk[st];
        for (int z = gl; z < Z; z += GT) {
            uint32_t s = bit_of(lamP + i * W, z);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < nk) s ^= xc[r.ord.step_kcol[st][k] * Z + mix_tx_enc_rotz(z, r.ord.step_kshift[st][k], Z)];
            xc[u * Z + mix_tx_enc_rotz(z, r.ord.step_shift[st], Z)] = (uint8_t)s;
        }
        group_sync();
    }
    if constexpr (NWC == 1) store_row(out + (size_t)kb * Z, xc, 4 * Z);
    else store_row(out + (size_t)(kb + wv) * Z, xc + wv * Z, Z); // one core-parity column per wave
    if (words32) { // xc starts on a dword boundary
        const uint32_t* x32 = reinterpret_cast<const uint32_t*>(xc);
        for (int it = gl; it < 4 * W; it += GT) {
            const int c = it / W, m = it - c * W;
            const uint32_t* q = x32 + (c * Z + 32 * m) / 4;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v |= squeeze(q[k]) << (4 * k);
            put_word(kb + c, m, v);
        }
    } else {
        pack(xc, kb, 4);
    }
    group_sync();
    // 3c. extension rows
    const int next = nrows - 4;
    for (int it = gl; it < next * W; it += GT) {
        const int i = it / W, m = it - i * W;
        PP[it] = row_word(4 + i, m, kb + 4);
    }
    group_sync();
    // 4. expand the extension parity to bytes
    uint8_t* ext = out + (size_t)(kb + 4) * Z;
    if ((Z & 3) == 0 && (reinterpret_cast<uintptr_t>(ext) & 3) == 0) {
        const int o0 = 4 * gl;
        int i = o0 / Z, z = o0 - i * Z;
        const int qi = (4 * GT) / Z, qz = 4 * GT - qi * Z;
        for (int o = o0; o < next * Z; o += 4 * GT) {
            const uint32_t nib = (PP[i * W + (z >> 5)] >> (z & 31)) & 0xFu;
            *reinterpret_cast<uint32_t*>(ext + o) = (nib * 0x00204081u) & 0x01010101u;
            i += qi; z += qz;
            if (z >= Z) { z -= Z; ++i; }
        }
    } else {
        int i = gl / Z, z = gl - i * Z;
        const int qi = GT / Z, qz = GT - qi * Z;
        for (int o = gl; o < next * Z; o += GT) {
            ext[o] = (uint8_t)bit_of(PP + i * W, z);
            i += qi; z += qz;
            if (z >= Z) { z -= Z; ++i; }
        }
    }
}

__global__ __launch_bounds__(64 * MIX_TX_ENC_WAVES) void nrldpc_mix_tx_encode_kernel(const MixTxEncLaunch a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // the same in every lane of a wave: say so
    // configuration and codeword: blockIdx and the prefix table only, so cfg and everything read through it is workgroup-uniform
    const MixTxEncWork w = mix_tx_enc_work(a.prefix, a.recs, a.n, (int)blockIdx.x, wave);
    MixTxEncRecC& r = *(MixTxEncRecC*)(a.recs + w.cfg);
    const MixTxEncLayout L = mix_tx_enc_layout(r.Z, r.kb, r.nrows, r.nnz);
    uint32_t* tw = reinterpret_cast<uint32_t*>(lds); // col | shift << 8 per edge
    uint32_t* rp = tw + r.nnz;                       // row pointers
    const uint16_t* row_ptr = reinterpret_cast<const uint16_t*>(a.tab + r.row_ptr_off);
    const uint16_t* shift = reinterpret_cast<const uint16_t*>(a.tab + r.shift_off);
    const uint8_t* col = a.tab + r.col_off;
    for (int e = threadIdx.x; e < r.nnz; e += 64 * MIX_TX_ENC_WAVES) tw[e] = (uint32_t)col[e] | ((uint32_t)shift[e] << 8);
    for (int i = threadIdx.x; i <= r.nrows; i += 64 * MIX_TX_ENC_WAVES) rp[i] = row_ptr[i];
    __syncthreads(); // every wave of the workgroup, with or without a codeword
    // waves per codeword is workgroup-uniform: one switch to the NWC-templated body
    if (r.nwc == 4) mix_tx_encode_codeword<4>(r, L, tw, a.c, a.cw, w.cw, wave, lane);
    else mix_tx_encode_codeword<1>(r, L, tw, a.c, a.cw, w.cw, wave, lane);
}

hipError_t launch_mix_tx_encode(const MixTxEncLaunch& a, hipStream_t stream) {
    if (a.n_wg <= 0) return hipSuccess;
    if (a.lds_bytes <= 0 || a.lds_bytes > 64 * 1024) return hipErrorInvalidValue; // (nrldpc_mix_tx_create refuses such a plan)
    hipLaunchKernelGGL(nrldpc_mix_tx_encode_kernel, dim3(a.n_wg), dim3(64 * MIX_TX_ENC_WAVES), (size_t)a.lds_bytes, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

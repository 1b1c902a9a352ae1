// nrldpc_mix.hip -- rate recovery and the CRC stage for a MIX of transport-block configurations in one launch each
// (nrldpc_mix_rate_recover_dev, nrldpc_mix_crc_check_dev; semantics: include/nrldpc.h), and their HARQ forms
// (nrldpc_mix_rate_recover_harq_dev, nrldpc_mix_crc_check_harq_dev): the same two kernels instantiated with
// HARQ = true, which adds a per-transport-block "starts a new HARQ process" flag to both and the sticky code-block flags, CBGTI and
// the kept b_hat segments of nrldpc_crc_check_kernel to the CRC stage.  The HARQ = false instantiations compile to the code they
// were before the parameter existed (every addition sits under if constexpr, the argument block is a structure of its own).
//
// Both kernels are table driven.  The per-configuration records (scalar parameters, E_r and its offsets, the two CRC plans) and a
// prefix table over the work items live in device memory, uploaded once by nrldpc_mix_create and never written again; a
// workgroup finds its configuration by a binary search of the prefix table (nrldpc_mix.h: mix_find, mix_rm_work), so everything
// that selects a code path -- configuration, form, element types, Q_m -- is workgroup-uniform.  The number of launches does not
// depend on the number of configurations: one per stage.
//
// Rate recovery is the gather of nrldpc_ratematch_ex.hip -- four neighbouring positions of a code block's decoder input per lane,
// through the same gather bodies, element rules and tail (nrldpc_rm_core.h: repetitions in ascending k, then the buffer, the clamp
// before any conversion to f16) -- and leaves bit for bit what nrldpc_rate_recover_ex_dev leaves in every segment.  A segment of
// a packed array starts 16 elements aligned, its rows do not (odd G, odd N_cb): every access wider than one element is taken by
// a test on the address it would use.  Every buffer position is read and written by exactly one thread; no atomics.
//
// The CRC stage is the wave-per-code-block kernel of nrldpc_crc.hip (LDS staging, then the per-lane bit-serial register, the GF(2)
// combine tree and the Horner fold of the segment remainders of nrldpc_crc_wave.h) with the plans read from the record.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "nrldpc_crc_wave.h"
#include "nrldpc_mix.h"
#include "nrldpc_rm_core.h"
#include "nrldpc_wave.h"

namespace nrldpc {
using namespace rm_dev;

// ---- rate recovery ---------------------------------------------------------------------------------------------------------------
template <bool HARQ> struct MixRmArgs { typedef MixRmLaunch type; };
template <> struct MixRmArgs<true> { typedef MixRmHarqLaunch type; };
__host__ __device__ __forceinline__ const MixRmLaunch& base_of(const MixRmLaunch& a) { return a; }
__host__ __device__ __forceinline__ const MixRmLaunch& base_of(const MixRmHarqLaunch& a) { return a.b; }

template <typename InT, typename HbT, typename OutT, bool HARQ>
__global__ __launch_bounds__(256) void nrldpc_mix_rate_recover_kernel(const typename MixRmArgs<HARQ>::type args) {
    const MixRmLaunch& a = base_of(args);
    const MixRmWork w = mix_rm_work(a.prefix, a.recs, a.n, (int)blockIdx.x);
    const MixRmRec& c = a.recs[w.cfg];
    const int blk = w.blk; // tb * C + r
    const int C = c.C, Z = c.Z, N_cb = c.N_cb, Qm = c.Qm;
    const int tb = blk / C, r = blk - tb * C;
    const int ncwz = 2 * Z + c.N;
    const int lane = threadIdx.x & 63;
    const int tile0 = w.tile0 + ((int)threadIdx.x >> 6) * MIX_RM_TILE;
    if (tile0 >= ncwz) return;
    const RmGeom geo(Z, c.K, c.Kp, N_cb, c.k0);
    const int E = a.e_tab[c.e_base + r];
    const int rows = E > 0 ? E / Qm : 1;
    const InT* f = static_cast<const InT*>(a.g) + c.g_off + (int64_t)tb * c.G + a.off_tab[c.e_base + r];
    HbT* hb = a.harq ? static_cast<HbT*>(a.harq) + c.harq_off + (int64_t)blk * N_cb : nullptr;
    OutT* out = static_cast<OutT*>(a.out) + c.cw_off + (int64_t)blk * ncwz;
    const bool echo = hb && c.echo;
    bool fresh = false; // workgroup-uniform: a workgroup is one code block of one transport block
    if constexpr (HARQ) fresh = args.is_new[mix_rm_new_index(args.tb_offs, a.recs, w)] != 0;
    if (c.form == RM_GENERAL) {
        // the general gather: repetitions summed in ascending k (:229-231), then the buffer
        const int Pq = geo.P / rows, Pr = geo.P - Pq * rows;
#pragma unroll
        for (int s = 0; s < MIX_RM_SWEEPS; ++s) {
            const int pos0 = tile0 + s * 256 + 4 * lane;
            if (pos0 >= ncwz) break;
            float val[4];
            bool fill[4], inb[4];
            const bool keep[4] = {false, false, false, false};
            gather_general(geo, f, pos0 - 2 * Z, N_cb, E, rows, Qm, Pq, Pr, val, fill, inb);
            finish4<HARQ>(hb, out, pos0, pos0 - 2 * Z, ncwz, val, fill, inb, keep, fresh);
        }
        return;
    }
    // no repetition: a position takes exactly one e(k) or none
#pragma unroll
    for (int s = 0; s < MIX_RM_SWEEPS; ++s) {
        const int pos0 = tile0 + s * 256 + 4 * lane;
        if (pos0 >= ncwz) break;
        float val[4];
        bool fill[4], inb[4], live[4], keep[4];
        int idx[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = pos0 + t - 2 * Z;
            fill[t] = geo.filler(p);
            inb[t] = p >= 0 && p < N_cb && !fill[t];
            const int q = geo.q_of(p);
            int i = 0;
            for (int m = 1; m < Qm; ++m) i += (q >= m * rows);
            const int j = q - i * rows;
            live[t] = inb[t] && q < E;
            keep[t] = echo && inb[t] && !live[t];
            idx[t] = live[t] ? j * Qm + i : 0;
        }
        // predicated: a position that receives nothing must not touch g_tilde at all -- for a trailing code block with E_r == 0
        // f already points one past the transport block's LLRs
#pragma unroll
        for (int t = 0; t < 4; ++t) val[t] = live[t] ? (float)f[idx[t]] : 0.0f;
        finish4<HARQ>(hb, out, pos0, pos0 - 2 * Z, ncwz, val, fill, inb, keep, fresh);
    }
}

template <bool HARQ> static hipError_t launch_mix_rm(const typename MixRmArgs<HARQ>::type& args, hipStream_t stream) {
    const MixRmLaunch& a = base_of(args);
    if (a.n_wg <= 0) return hipSuccess;
    rm_with_types(a.in_f16, a.harq && a.harq_f16, a.out_f16, [&](auto in, auto hb, auto out) {
        hipLaunchKernelGGL((nrldpc_mix_rate_recover_kernel<decltype(in), decltype(hb), decltype(out), HARQ>), dim3(a.n_wg), dim3(256), 0, stream, args);
    });
    return hipGetLastError();
}

hipError_t launch_mix_rate_recover(const MixRmLaunch& a, hipStream_t stream) { return launch_mix_rm<false>(a, stream); }

hipError_t launch_mix_rate_recover_harq(const MixRmHarqLaunch& a, hipStream_t stream) {
    if (a.b.n_wg <= 0) return hipSuccess;
    if (!a.b.harq || !a.is_new || !a.tb_offs) return hipErrorInvalidValue; // (the C ABI never gets here: it launches the plain kernel)
    return launch_mix_rm<true>(a, stream);
}

// ---- CRC stage -------------------------------------------------------------------------------------------------------------------
template <bool HARQ> struct MixCrcArgs { typedef MixCrcLaunch type; };
template <> struct MixCrcArgs<true> { typedef MixCrcHarqLaunch type; };
__device__ __forceinline__ const MixCrcLaunch& base_of(const MixCrcLaunch& a) { return a; }
__device__ __forceinline__ const MixCrcLaunch& base_of(const MixCrcHarqLaunch& a) { return a.b; }

// one workgroup per transport block, one wave per code block (waves loop when C exceeds the workgroup's waves).
// HARQ: the state machine of nrldpc_crc_check_kernel (NRLDPCDecoder.m:286-316, 337) with keep_b_hat = sticky = !new[tb] and the CBGTI
// flag read per code block -- a transport block that starts a new HARQ process is reset() followed by a step, for that block alone.
template <bool HARQ>
__global__ __launch_bounds__(256) void nrldpc_mix_crc_check_kernel(const typename MixCrcArgs<HARQ>::type args) {
    const MixCrcLaunch& a = base_of(args);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int cfg = mix_find(a.prefix, a.n, (int)blockIdx.x);
    const MixCrcRec& c = a.recs[cfg];
    const int tb = (int)blockIdx.x - a.prefix[cfg];
    const int C = c.C, K = c.K, Kp = c.Kp;
    const int cap = row_capacity(a.k_max); // one stride for every configuration: the carve-up below stays 16-byte aligned
    uint8_t* base = reinterpret_cast<uint8_t*>(lds) + (size_t)wave * cap;
    int* cb_fail = reinterpret_cast<int*>(lds + (size_t)nw * cap);  // [c_max]
    uint32_t* part = reinterpret_cast<uint32_t*>(cb_fail + a.c_max); // [c_max] TB-polynomial remainder per segment
    const uint8_t* chat = a.c_hat + c.c_hat_off + (int64_t)tb * C * K;
    uint8_t* b_hat = a.b_hat + c.b_hat_off + (int64_t)tb * c.B;
    const int pay = Kp - c.Lcb; // payload bits per code block
    bool keep = false; // workgroup-uniform: the transport block continues a HARQ process (b_hat and cb_pass are in/out)
    if constexpr (HARQ) keep = !(args.is_new && args.is_new[mix_new_index(c.tb_off, tb)] != 0);
    for (int r = wave; r < C; r += nw) {
        wave_lds_sync(); // previous round's readers are done with the row
        const uint8_t* row = stage_row(base, chat + (size_t)r * K, Kp);
        wave_lds_sync();
        int fail = 0;
        if (C > 1) fail = wave_crc(row, Kp, c.cb) != 0; // NRLDPCDecoder.m:298-301
        if constexpr (HARQ) {                            // :304: CRC holds AND the block was (re)transmitted
            if (args.cbgti) fail |= args.cbgti[mix_cbgti_index(c.cb_off, C, tb, r)] == 0;
        }
        uint32_t p;
        if (!fail) {
            p = wave_crc(row, pay, c.tb);
            store_row(b_hat + (size_t)r * pay, row, pay); // :303-309 payload copy
        } else if (HARQ && keep) {                        // :286-287: the segment keeps what an earlier step stored
            wave_lds_sync();
            row = stage_row(base, b_hat + (size_t)r * pay, pay);
            wave_lds_sync();
            p = wave_crc(row, pay, c.tb);
        } else {                                          // :289: b_hat = zeros(B,1)
            p = 0;
            uint8_t* z = b_hat + (size_t)r * pay;
            for (int i = lane; i < pay; i += 64) z[i] = 0;
        }
        if (lane == 0) { cb_fail[r] = fail; part[r] = p; }
    }
    __syncthreads();
    if (wave == 0) {
        uint32_t reg = 0; // :336 over b_hat = segment 0 || ... || segment C-1
        for (int r = 0; r < C; ++r) reg = gf2_apply(c.tb.horner, reg) ^ part[r];
        int any_cb = 0;   // :337 any(~code_block_CRC_passed)
        for (int r = lane; r < C; r += 64) {
            int pass = cb_fail[r] ? 0 : 1;
            if constexpr (HARQ) {                         // flags sticky (:305, 315) unless the block starts anew (:355)
                int32_t* f = a.cb_pass + c.cb_off + (int64_t)tb * C + r;
                if (keep) pass |= (*f != 0);
                *f = pass;
            } else {
                if (a.cb_pass) a.cb_pass[c.cb_off + (int64_t)tb * C + r] = pass;
            }
            any_cb |= !pass;
        }
        any_cb = __any(any_cb);
        if (lane == 0) a.ok[c.tb_off + tb] = (reg != 0 || any_cb) ? 0 : 1; // :337-339
    }
}

hipError_t launch_mix_crc_check(const MixCrcLaunch& a, hipStream_t stream) {
    if (a.n_tb_total <= 0) return hipSuccess;
    const size_t lds = (size_t)a.waves * row_capacity(a.k_max) + 8 * (size_t)a.c_max + 16;
    hipLaunchKernelGGL(nrldpc_mix_crc_check_kernel<false>, dim3(a.n_tb_total), dim3(64 * a.waves), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_mix_crc_check_harq(const MixCrcHarqLaunch& a, hipStream_t stream) {
    if (a.b.n_tb_total <= 0) return hipSuccess;
    if (!a.b.cb_pass) return hipErrorInvalidValue; // (refused by the C ABI before it gets here)
    const size_t lds = (size_t)a.b.waves * row_capacity(a.b.k_max) + 8 * (size_t)a.b.c_max + 16;
    hipLaunchKernelGGL(nrldpc_mix_crc_check_kernel<true>, dim3(a.b.n_tb_total), dim3(64 * a.b.waves), lds, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

// nrldpc_mix_tx.hip -- CRC attach and rate matching for a MIX of transport-block configurations in one launch each
// (nrldpc_mix_tx_crc_attach_dev, nrldpc_mix_tx_rate_match_dev; semantics: include/nrldpc.h): the transmit mirror
// of nrldpc_mix.hip.  The encoder between them is not here: nrldpc_mix_tx_encode_dev launches the existing kernel once per
// configuration at the plan's offsets, and the one-launch form nrldpc_mix_tx_encode_all_dev has a unit of its own (nrldpc_mix_tx_enc.hip).
//
// Both kernels are table driven, like the receive side's.  The per-configuration records (sizes, E_r and its offsets, the two CRC
// plans) and a prefix table over the work items live in device memory, uploaded once by nrldpc_mix_tx_create and never written
// again; a workgroup finds its configuration by a binary search of the prefix table (nrldpc_mix.h: mix_find; nrldpc_mix_tx.h:
// mix_tx_rm_work), so everything that selects a code path -- configuration, Q_m, repetition -- is workgroup-uniform.
//
// Rate matching is nrldpc_rate_match_kernel (nrldpc_ratematch.hip) with its arguments read from the record: the same RmGeom, the same
// repetition split, the same four-byte run test in the same order, the same dword-or-byte store rule, so it leaves bit for bit what
// nrldpc_rate_match_dev leaves in every segment.  One thread writes each byte of g; no atomics.
//
// The CRC stage is nrldpc_crc_attach_kernel (nrldpc_crc.hip): a wave per code block stages its share of the payload into LDS
// (stage_row), takes both remainders (wave_crc, nrldpc_crc_wave.h) and stores the finished row (store_row); the last code block is
// finished after the segment remainders are folded.
//
// Why the two bodies are this unit's own copies and not functions both units call: moved into a header -- as a
// template <int QM> __device__ __forceinline__ function taking the geometry, the two pointers and (E, rows, j0), with the row pointer
// of g passed as a value and as a callable evaluated where the kernel forms it -- all five nrldpc_rate_match_kernel<QM> came out with
// other instructions than the parent commit's (+6 .. +72 lines of assembly per kernel); and nrldpc_crc_attach_kernel through a device
// function taking the sizes and the two plans by reference came out 7 lines shorter, not the same.  The existing kernels therefore
// keep their text and profiles/r09_mix_tx_isa.txt shows them identical; the price is the ~90 lines below, which change whenever
// theirs do (tests/test_mix_tx_gpu.py holds the two sides to equality on every path of either).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>

#include "nrldpc_crc_wave.h"
#include "nrldpc_mix_tx.h"
#include "nrldpc_rm_core.h"
#include "nrldpc_wave.h"

namespace nrldpc {

static_assert(sizeof(MixTxCrcRec) % 8 == 0 && sizeof(MixTxRmRec) % 8 == 0, "records are laid out as arrays with int64 members");

// ---- rate matching ---------------------------------------------------------------------------------------------------------------
template <class F, int... I> __device__ __forceinline__ void mix_tx_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void mix_tx_static_for(F&& f) { mix_tx_static_for_impl(f, std::make_integer_sequence<int, N>{}); }

typedef uint32_t __attribute__((aligned(1))) mix_tx_u32_unaligned;

// one thread: four interleaver columns j0 .. j0+3 of all QM rows of code block r of transport block tb (the body of
// nrldpc_rate_match_kernel<QM>, index arithmetic unchanged)
template <int QM>
__device__ __forceinline__ void mix_tx_rate_match_thread(const MixTxRmLaunch& a, const MixTxRmRec& c, const MixTxRmWork& w) {
    static_assert(MIX_TX_RM_COLS == 4, "the body below handles four columns per thread");
    const int blk = w.blk;
    const int tb = blk / c.C, r = blk - tb * c.C;
    const int E = a.e_tab[c.e_base + r];
    const int rows = E / QM;
    const int j0 = mix_tx_rm_j0(w, (int)threadIdx.x);
    if (j0 >= rows) return;
    const RmGeom geo(c.Z, c.K, c.Kp, c.N_cb, c.k0);
    const uint8_t* cw = a.cw + mix_tx_rm_cw_index(c, blk);
    const int nj = rows - j0 < 4 ? rows - j0 : 4; // j of this thread that exist
    uint32_t run[QM]; // byte t of run[i] = e(i*rows + j0 + t)
    const bool rep = E > geo.P; // uniform over the workgroup
#pragma unroll
    for (int i = 0; i < QM; ++i) {
        const int k = i * rows + j0;
        int q, kend; // q: position among the buffer's non-filler bits; kend: first k of the next repetition
        if (rep) { const int d = k / geo.P; q = k - d * geo.P + geo.nfk0; kend = geo.P * (d + 1); }
        else { q = k + geo.nfk0; kend = geo.P; }
        if (q >= geo.P) q -= geo.P;
        // four consecutive e indices are four consecutive bytes when the run stays below P in k (no repetition wrap) and
        // in q (no buffer wrap) and on one side of the filler gap
        if (nj == 4 && k + 3 < kend && q + 3 < geo.P && (q >= geo.lo_f || q + 3 < geo.lo_f)) {
            run[i] = *reinterpret_cast<const mix_tx_u32_unaligned*>(cw + (q < geo.lo_f ? q : q + geo.F)) & 0x01010101u;
        } else {
            uint32_t v = 0;
            for (int t = 0; t < nj; ++t) {
                const int kk = k + t;
                int qq = (rep ? kk % geo.P : kk) + geo.nfk0;
                if (qq >= geo.P) qq -= geo.P;
                v |= (uint32_t)(cw[qq < geo.lo_f ? qq : qq + geo.F] & 1u) << (8 * t);
            }
            run[i] = v;
        }
    }
    // interleave: output byte t*QM + i = byte t of run[i], with v_perm_b32 (see nrldpc_rate_match_kernel)
    uint32_t out[QM];
    mix_tx_static_for<QM>([&](auto oc) {
        constexpr int o = decltype(oc)::value;
        constexpr int t0 = (4 * o) / QM, i0 = (4 * o) % QM, t1 = (4 * o + 1) / QM, i1 = (4 * o + 1) % QM;
        constexpr int t2 = (4 * o + 2) / QM, i2 = (4 * o + 2) % QM, t3 = (4 * o + 3) / QM, i3 = (4 * o + 3) % QM;
        if constexpr (QM == 1) {
            out[o] = run[0];
        } else if constexpr (QM == 2) { // bytes (run0.t0, run1.t1, run0.t2, run1.t3)
            out[o] = __builtin_amdgcn_perm(run[1], run[0], (uint32_t)(t0 | ((4 + t1) << 8) | (t2 << 16) | ((4 + t3) << 24)));
        } else {
            const uint32_t p01 = __builtin_amdgcn_perm(run[i1], run[i0], (uint32_t)(t0 | ((4 + t1) << 8) | 0x0c0c0000u));
            const uint32_t p23 = __builtin_amdgcn_perm(run[i3], run[i2], (uint32_t)(t2 | ((4 + t3) << 8) | 0x0c0c0000u));
            out[o] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
        }
    });
    uint8_t* g = a.g + mix_tx_rm_g_index(c, tb, a.off_tab[c.e_base + r]) + (size_t)j0 * QM;
    if (nj == 4 && (reinterpret_cast<uintptr_t>(g) & 3) == 0) {
#pragma unroll
        for (int o = 0; o < QM; ++o) reinterpret_cast<uint32_t*>(g)[o] = out[o];
    } else {
        for (int ob = 0; ob < nj * QM; ++ob) g[ob] = (uint8_t)(out[ob >> 2] >> (8 * (ob & 3)));
    }
}

// Q_m is workgroup-uniform: one switch to the QM-templated body (the v_perm_b32 selectors and the run[QM] registers need a
// compile-time QM).  nrldpc_mix_tx_create admits no other Q_m than these five.
__global__ __launch_bounds__(256) void nrldpc_mix_tx_rate_match_kernel(const MixTxRmLaunch a) {
    const MixTxRmWork w = mix_tx_rm_work(a.prefix, a.recs, a.n, (int)blockIdx.x);
    const MixTxRmRec& c = a.recs[w.cfg];
    switch (c.Qm) {
        case 1: mix_tx_rate_match_thread<1>(a, c, w); break;
        case 2: mix_tx_rate_match_thread<2>(a, c, w); break;
        case 4: mix_tx_rate_match_thread<4>(a, c, w); break;
        case 6: mix_tx_rate_match_thread<6>(a, c, w); break;
        case 8: mix_tx_rate_match_thread<8>(a, c, w); break;
        default: break;
    }
}

hipError_t launch_mix_tx_rate_match(const MixTxRmLaunch& a, hipStream_t stream) {
    if (a.n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_tx_rate_match_kernel, dim3(a.n_wg), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ---- CRC attach ------------------------------------------------------------------------------------------------------------------
// One workgroup per transport block, one wave per code block: the state machine of nrldpc_crc_attach_kernel (NRLDPCEncoder.m:70-124)
// with the sizes and both plans read from the configuration's record (workgroup-uniform addresses).  The wave count and the LDS row
// stride are the PLAN's: a wave whose r never falls below this configuration's C skips the loop and still reaches the barrier, and
// the last block is finished by wave (C - 1) % nw with nw the plan's count -- the wave that staged it.
__global__ __launch_bounds__(256) void nrldpc_mix_tx_crc_attach_kernel(const MixTxCrcLaunch a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int cfg = mix_find(a.prefix, a.n, (int)blockIdx.x);
    const MixTxCrcRec& rec = a.recs[cfg];
    const MixTxCrcGeom& c = rec.g;
    const int tb = (int)blockIdx.x - a.prefix[cfg];
    const int C = c.C, K = c.K, Kp = c.Kp, Lcb = c.Lcb;
    const int cap = mix_tx_row_capacity(a.k_max); // one stride for every configuration: the carve-up below stays 16-byte aligned
    uint8_t* base = reinterpret_cast<uint8_t*>(lds) + (size_t)wave * cap;
    uint8_t* row = base;
    uint32_t* part = reinterpret_cast<uint32_t*>(lds + mix_tx_part_byte(nw, a.k_max, 0)); // [c_max]
    const int pay = mix_tx_pay(c), Ltb = c.B - c.A;
    auto finish = [&](int r) { // payload complete in row[0..pay): CB CRC (:113-118), fillers (:120-122), store
        if (C > 1) {
            const uint32_t cr = wave_crc(row, pay, rec.cb);
            if (lane < Lcb) row[pay + lane] = (uint8_t)((cr >> (Lcb - 1 - lane)) & 1u);
        }
        for (int i = Kp + lane; i < K; i += 64) row[i] = 0;
        wave_lds_sync();
        store_row(a.c + mix_tx_c_index(c, tb, r), row, K);
    };
    for (int r = wave; r < C; r += nw) {
        const bool last = (r == C - 1);
        const int seg = mix_tx_seg(c, r); // bits of `a` in this code block (:104-112)
        wave_lds_sync();
        row = stage_row(base, a.a + mix_tx_a_index(c, tb, r), seg);
        wave_lds_sync();
        const uint32_t p = wave_crc(row, seg, rec.tb);
        if (lane == 0) part[r] = p;
        if (!last) finish(r);
    }
    __syncthreads();
    if (wave == mix_tx_last_wave(c, nw)) { // this wave's row still holds the last code block's share of `a`
        uint32_t reg = 0;                  // NRLDPCEncoder.m:80-81 over a = segment 0 || ... || tail
        for (int r = 0; r + 1 < C; ++r) reg = gf2_apply(rec.tb.horner, reg) ^ part[r];
        reg = gf2_apply(rec.tb.horner_tail, reg) ^ part[C - 1];
        if (lane < Ltb) row[pay - Ltb + lane] = (uint8_t)((reg >> (Ltb - 1 - lane)) & 1u);
        wave_lds_sync();
        finish(C - 1);
    }
}

hipError_t launch_mix_tx_crc_attach(const MixTxCrcLaunch& a, hipStream_t stream) {
    if (a.n_tb_total <= 0) return hipSuccess;
    if (mix_tx_row_capacity(a.k_max) != row_capacity(a.k_max)) return hipErrorInvalidValue; // (the header's restatement for the host walk)
    const size_t lds = (size_t)mix_tx_lds_bytes(a.waves, a.k_max, a.c_max);
    hipLaunchKernelGGL(nrldpc_mix_tx_crc_attach_kernel, dim3(a.n_tb_total), dim3(64 * a.waves), lds, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

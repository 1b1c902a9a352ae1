// nrldpc_mix_skip.hip -- mixed HARQ steps that decode only the code blocks still pending: the three launches between rate recovery
// and the CRC stage of a mix (nrldpc_mix_pending_dev, nrldpc_mix_gather_cw_dev, nrldpc_mix_scatter_hard_dev; semantics:
// include/nrldpc.h).  The rule, the partition, the mapping and the row copy are the host/device functions of
// nrldpc_mix_skip.h; the kernels below are those functions on a grid.
//
// pending: one workgroup per configuration.  A thread counts the pending blocks of its contiguous run, an inclusive scan over the
// thread counts in LDS gives its base, and it walks the run again to write its indices from there: ascending, one writer per
// position, no atomics, no scratch.  Thread 0 writes the count.
//
// gather / scatter: HBM-bound row copies.  The grid holds a workgroup per (configuration, row, chunk of the row) for EVERY row; a
// workgroup whose dense slot is at or above the count the pending kernel left on the device leaves at once.  The access width is
// chosen by a test on the two addresses (workgroup-uniform): 16 bytes per lane wherever both rows allow it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_mix_skip.h"

namespace nrldpc {

__global__ __launch_bounds__(MIX_SKIP_THREADS) void nrldpc_mix_pending_kernel(const MixSkipRec* recs, int32_t rule, const MixSkipState s, int32_t* index,
                                                                               int32_t* count) {
    __shared__ int32_t scan[2][MIX_SKIP_THREADS];
    const int t = threadIdx.x;
    const MixSkipRec c = recs[blockIdx.x];
    const auto pend = [&](int32_t blk) { return mix_skip_block_pending(rule, s, c, blk); };
    int32_t lo, hi;
    mix_skip_run(c.n_cb, MIX_SKIP_THREADS, t, lo, hi);
    const int32_t own = mix_skip_count_run(lo, hi, pend);
    scan[0][t] = own;
    __syncthreads();
    int from = 0;
#pragma unroll
    for (int k = 0; k < MIX_SKIP_SCAN_STEPS; ++k) {
        scan[from ^ 1][t] = mix_skip_scan_step(scan[from], t, 1 << k);
        from ^= 1;
        __syncthreads();
    }
    mix_skip_write_run(lo, hi, scan[from][t] - own, pend, index + c.cb_off);
    if (t == 0) count[blockIdx.x] = scan[from][MIX_SKIP_THREADS - 1];
}

// SCATTER = false: dense row `slot` <- full row index[slot] (the LLRs); true: full row index[slot] <- dense row `slot` (the hard bits),
// and the iteration counts
template <bool SCATTER>
__global__ __launch_bounds__(MIX_SKIP_COPY_THREADS) void nrldpc_mix_skip_copy_kernel(const MixSkipLaunch a, const uint8_t* from, uint8_t* to, const int32_t* index,
                                                                                      const int32_t* count, const int32_t* iters_dense, int32_t* iters) {
    const MixSkipWork w = mix_skip_work(a.prefix, a.recs, a.n, a.esize, (int)blockIdx.x);
    const MixSkipRec& c = a.recs[w.cfg];
    const int32_t cnt = count[w.cfg];
    const int t = threadIdx.x;
    const int32_t* idx = index + c.cb_off;
    // (an index outside the configuration can only come from a caller that did not take it from the pending kernel: such a row is
    // left alone rather than followed out of the arrays)
    const int32_t row = w.slot < cnt ? idx[w.slot] : -1;
    const bool valid = row >= 0 && row < c.n_cb;
    if constexpr (SCATTER) {
        if (iters && w.chunk == 0 && (valid || (w.slot == 0 && cnt == 0))) {
            int32_t lo, hi, lo2, hi2;
            mix_skip_zero_range(idx, cnt, c.n_cb, w.slot, lo, hi, lo2, hi2);
            int32_t* it = iters + c.cb_off;
            for (int32_t b = (lo < 0 ? 0 : lo) + t; b < hi && b < c.n_cb; b += MIX_SKIP_COPY_THREADS) it[b] = 0;
            for (int32_t b = (lo2 < 0 ? 0 : lo2) + t; b < hi2 && b < c.n_cb; b += MIX_SKIP_COPY_THREADS) it[b] = 0;
            if (valid && iters_dense && t == 0) it[row] = iters_dense[c.cb_off + w.slot];
        }
    }
    if (!valid) return;
    const int64_t row_bytes = mix_skip_row_bytes(c, a.esize);
    const int64_t seg = (SCATTER ? c.c_hat_off : c.cw_off) * a.esize;
    int64_t lo;
    int32_t len;
    mix_skip_span(row_bytes, w.chunk, lo, len);
    const int64_t full = seg + (int64_t)row * row_bytes + lo, dense = seg + (int64_t)w.slot * row_bytes + lo;
    mix_skip_copy(from + (SCATTER ? dense : full), to + (SCATTER ? full : dense), len, t, MIX_SKIP_COPY_THREADS);
}

hipError_t launch_mix_skip_pending(const MixSkipLaunch& a, int32_t rule, const MixSkipState& s, int32_t* index, int32_t* count, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_pending_kernel, dim3(a.n), dim3(MIX_SKIP_THREADS), 0, stream, a.recs, rule, s, index, count);
    return hipGetLastError();
}

hipError_t launch_mix_skip_gather(const MixSkipLaunch& a, const void* cw, const int32_t* index, const int32_t* count, void* dense, hipStream_t stream) {
    if (a.n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_skip_copy_kernel<false>, dim3(a.n_wg), dim3(MIX_SKIP_COPY_THREADS), 0, stream, a, static_cast<const uint8_t*>(cw),
                       static_cast<uint8_t*>(dense), index, count, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_mix_skip_scatter(const MixSkipLaunch& a, const uint8_t* dense, const int32_t* iters_dense, const int32_t* index, const int32_t* count,
                                   uint8_t* c_hat, int32_t* iters, hipStream_t stream) {
    if (a.n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_skip_copy_kernel<true>, dim3(a.n_wg), dim3(MIX_SKIP_COPY_THREADS), 0, stream, a, dense, c_hat, index, count, iters_dense, iters);
    return hipGetLastError();
}

} // namespace nrldpc

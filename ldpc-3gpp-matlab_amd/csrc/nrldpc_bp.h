// nrldpc_bp.h -- launch interface of the flooding sum-product decoder (nrldpc_decode_bp.hip), shared with nrldpc_capi.hip.
// Kept apart from nrldpc_kernels.h: that header is part of the min-sum kernels' identity (nrldpc_kernel_id).
#ifndef NRLDPC_BP_H
#define NRLDPC_BP_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nrldpc {

constexpr int BP_MAX_DEG = 19;          // largest row degree of either base graph (BG1 row 0)
constexpr int BP_MAX_THREADS = 1024;    // workgroup size cap (__launch_bounds__)
constexpr size_t BP_TAB_BYTES = 2176;   // LDS bytes of the graph tables in front of APP

struct BpArgs {
    const void* llr;    // [batch][ncols*Z] f32, or f16 when llr_f16
    uint8_t* hard;      // [batch][kb*Z]
    int32_t* iters;     // [batch], nullable
    float* app;         // [batch][ncols*Z], nullable
    // nrldpc_cw_out (include/nrldpc.h), each nullable; with any of them the launch carries CW_LDS_BYTES (nrldpc_cwout.h) more LDS
    uint8_t* cw_packed;     // [batch][ceil(ncols*Z/8)]
    int32_t* unsatisfied;   // [batch]
    uint8_t* checks_packed; // [batch][ceil(nrows*Z/8)]
    const uint16_t* row_ptr; // base graph, row-ordered edges (the handle's d_row_ptr / d_col / d_shift: shifts mod Z)
    const uint8_t* col;
    const uint16_t* shift;
    const uint16_t* col_ptr;  // [ncols+1]: the edges of column c are col_edge[col_ptr[c] .. col_ptr[c+1]), ascending
    const uint16_t* col_edge; // [nnz]
    float* ws;          // per-workgroup slices of ws_stride floats: r [nnz*Z], then lambda [ncols*Z]
    size_t ws_stride;
    int batch, Z, nrows, ncols, kb, nnz, n_layers, max_iter, early_term, llr_f16;
    float r_cap;        // largest |r|: 2*atanh(1 - 1e-15), the oracle's clamp of the tanh product
};

int bp_threads(int ncols, int Z);
size_t bp_lds_bytes(int ncols, int Z);
// workgroups the device holds at once (current device); *what names the call that failed
hipError_t bp_resident(int threads, size_t lds, int* out, const char** what);
hipError_t launch_bp_flood(const BpArgs& a, int grid, int threads, size_t lds, hipStream_t stream);

} // namespace nrldpc
#endif

// nrldpc_cwout.hip -- the finish kernel behind nrldpc_decode_cw[_dev] on a min-sum handle: whole-codeword hard decisions, bit-packed,
// and the final parity checks, from the fp32 a-posteriori LLRs the soft-output route of the decoder kernels wrote.
//
// One workgroup per codeword, grid-stride over the batch.  The codeword's hard decisions live in LDS as a bit image (at most
// 26112 bits); both passes are in cw_finish_codeword (nrldpc_cwout.h), which the sum-product kernel's output stage calls too.
// The kernel reads 4 bytes per bit once and writes an eighth of a byte per bit: it is bound by that read and nothing else.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "nrldpc_cwout.h"

namespace nrldpc {

__global__ __launch_bounds__(1024) void nrldpc_cw_finish_kernel(const CwFinishArgs a) {
    __shared__ uint16_t rp[CW_T_RP], ecol[CW_T_E], esh[CW_T_E];
    __shared__ __align__(8) unsigned long long bits[CW_BIT_WORDS];
    __shared__ int red[CW_MAX_WAVES];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = a.ncols * a.Z;
    for (int i = tid; i <= a.nrows; i += nt) rp[i] = a.row_ptr[i];
    for (int i = tid; i < a.nnz; i += nt) { ecol[i] = a.col[i]; esh[i] = a.shift[i]; }
    __syncthreads();
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        cw_finish_codeword(a.app + (size_t)b * N, b, N, a.Z, a.nrows, a.n_layers, rp, ecol, esh, bits, red, a.cw_packed, a.unsatisfied,
                           a.checks_packed);
        __syncthreads(); // the image and the counts belong to the next codeword from here on
    }
}

int cw_finish_threads(int ncols, int Z) {
    const int n = ((ncols * Z + 63) / 64) * 64;
    return n < 1024 ? n : 1024;
}

hipError_t launch_cw_finish(const CwFinishArgs& a, hipStream_t stream) {
    if (a.batch < 1 || a.Z < 1 || a.ncols < 1 || a.ncols * a.Z > CW_MAX_N || a.nrows + 1 > CW_T_RP || a.nnz < 1 ||
        a.nnz > CW_T_E || a.n_layers < 0 || a.n_layers > a.nrows || !a.app || !a.row_ptr || !a.col || !a.shift)
        return hipErrorInvalidValue;
    const int grid = a.batch < 4096 ? a.batch : 4096;
    hipLaunchKernelGGL(nrldpc_cw_finish_kernel, dim3(grid), dim3(cw_finish_threads(a.ncols, a.Z)), 0, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

// nrldpc_decode_bp.hip -- flooding sum-product with the parity-check stop (NRLDPC_ALG_SUM_PRODUCT): the algorithm of the
// reference's comm.LDPCDecoder (NRLDPCDecoder.m:120), with the semantics of orc_decode_bp_flood_app / bp_one in
// oracle/nrldpc_oracle.c, in fp32.
//
// Layout: one workgroup per codeword, persistent over the batch (the grid is the device's resident capacity).  The a-posteriori
// LLRs APP [ncols*Z] live in LDS; the check-to-variable messages r [active edges][Z] and the channel LLRs [ncols*Z] live in a
// per-workgroup slice of a device workspace (474 KiB of messages at BG1 Z = 384 do not fit the 160 KiB of LDS).  The channel
// LLRs are read from the caller's array ONCE per codeword (zero-copy callers hand over pinned host memory).  A sweep:
//   A. threads over (row, z): q_j = APP - r_old (an infinite APP stays infinite), r_new written over r_old (coalesced along z);
//   B. threads over (column, z): APP = lambda + sum of r_new over the column's active edges (column-ordered edge list);
//   stop: threads over (row, z) test the active checks on APP < 0, one __syncthreads_or for the workgroup.
// Every codeword follows one fixed order of operations, whatever workgroup takes it: no atomics, no batch dependence.
//
// Check node in the phi domain, phi(x) = -ln tanh(x/2) = log1p(2 / expm1(x)) (its own inverse; phi(0) = inf, phi(inf) = 0):
// |r_j| = min(phi(sum_{k != j} phi(|q_k|)), r_cap), sign = product of the other signs.  The sum over the others is a prefix sum
// plus a suffix sum -- terms are positive and nothing is subtracted, so it keeps its relative accuracy from phi = 1e-15 (r at the
// oracle's cap 2*atanh(1 - 1e-15) = 35.23) to phi = inf (a q of 0) -- where fp32 tanh(x/2) rounds to 1 from |x| ~ 17 on.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>

#include "nrldpc_bp.h"
#include "nrldpc_cwout.h"

namespace nrldpc {

static constexpr int T_RP = 48, T_E = 320, T_CP = 72; // LDS table capacities (uint16): row_ptr, per-edge tables, col_ptr
static_assert(BP_TAB_BYTES >= (T_RP + 3 * T_E + T_CP) * 2, "LDS table bytes");

// phi(x) = -ln tanh(x/2) for x >= 0: log1pf keeps relative accuracy where the argument is small (x large, phi ~ 2 e^-x) and
// expm1f where x is small (phi ~ ln(2/x)); expm1f overflows to inf above x ~ 88.7, where phi is 0 in fp32 anyway
static __device__ __forceinline__ float bp_phi(float x) { return log1pf(2.0f / expm1f(x)); }

__global__ __launch_bounds__(BP_MAX_THREADS) void nrldpc_bp_flood_kernel(const BpArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    uint16_t* rp = reinterpret_cast<uint16_t*>(lds);
    uint16_t* ecol = rp + T_RP;
    uint16_t* esh = ecol + T_E;
    uint16_t* ce = esh + T_E;
    uint16_t* cp = ce + T_E;
    float* app = reinterpret_cast<float*>(lds + BP_TAB_BYTES);
    const int Z = a.Z, N = a.ncols * Z, K = a.kb * Z, nl = a.n_layers;
    // whole-codeword bits and final parity checks (nrldpc_cw_out): the bit image and the wave counts sit behind APP (N is a
    // multiple of 4, so the offset is a multiple of 16 bytes); the launch carries those bytes only when an output is wanted
    const bool cw_out = a.cw_packed || a.unsatisfied || a.checks_packed;
    unsigned long long* cw_bits = reinterpret_cast<unsigned long long*>(lds + BP_TAB_BYTES + (size_t)N * 4);
    int* cw_red = reinterpret_cast<int*>(cw_bits + CW_BIT_WORDS);
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i <= a.nrows; i += nt) rp[i] = a.row_ptr[i];
    for (int i = tid; i < a.nnz; i += nt) { ecol[i] = a.col[i]; esh[i] = a.shift[i]; ce[i] = a.col_edge[i]; }
    for (int i = tid; i <= a.ncols; i += nt) cp[i] = a.col_ptr[i];
    __syncthreads();
    const int ne = rp[nl];          // edges of the active rows: the first ne of the row-ordered list
    const int nchk = nl * Z;        // active checks
    float* r = a.ws + (size_t)blockIdx.x * a.ws_stride; // [ne][Z]
    float* lam = r + (size_t)a.nnz * Z;                  // [N]
    const float cap = a.r_cap;
    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        // ingest: unquantised; NaN -> 0, +-inf kept (+inf: filler bits)
        if (a.llr_f16) {
            const __half* src = static_cast<const __half*>(a.llr) + (size_t)b * N;
            for (int v = tid; v < N; v += nt) { float x = __half2float(src[v]); if (x != x) x = 0.0f; lam[v] = x; app[v] = x; }
        } else {
            const float* src = static_cast<const float*>(a.llr) + (size_t)b * N;
            for (int v = tid; v < N; v += nt) { float x = src[v]; if (x != x) x = 0.0f; lam[v] = x; app[v] = x; }
        }
        for (int i = tid; i < ne * Z; i += nt) r[i] = 0.0f;
        __syncthreads();
        int it = 1;
        for (;; ++it) {
            // A: check nodes, every q from the same APP snapshot (flooding)
            for (int t = tid; t < nchk; t += nt) {
                const int l = t / Z, z = t - l * Z;
                const int e0 = rp[l], deg = rp[l + 1] - e0;
                float ph[BP_MAX_DEG];
                uint32_t sg = 0;
#pragma unroll
                for (int j = 0; j < BP_MAX_DEG; ++j) {
                    ph[j] = 0.0f;
                    if (j < deg) {
                        const int e = e0 + j;
                        int zz = z + esh[e];
                        if (zz >= Z) zz -= Z;
                        const float A = app[ecol[e] * Z + zz];
                        const float q = __builtin_isinf(A) ? A : A - r[(size_t)e * Z + z];
                        ph[j] = bp_phi(fabsf(q));
                        sg |= (uint32_t)__builtin_signbit(q) << j;
                    }
                }
                const uint32_t par = (uint32_t)__builtin_popcount(sg) & 1u;
                float suf[BP_MAX_DEG + 1]; // suf[j] = ph[j] + ... + ph[deg-1], summed right to left
                suf[BP_MAX_DEG] = 0.0f;
#pragma unroll
                for (int j = BP_MAX_DEG - 1; j >= 0; --j) suf[j] = j < deg ? ph[j] + suf[j + 1] : 0.0f;
                float pre = 0.0f; // ph[0] + ... + ph[j-1], summed left to right
#pragma unroll
                for (int j = 0; j < BP_MAX_DEG; ++j) {
                    if (j < deg) {
                        const float m = fminf(bp_phi(pre + suf[j + 1]), cap);
                        r[(size_t)(e0 + j) * Z + z] = (par ^ ((sg >> j) & 1u)) ? -m : m;
                        pre += ph[j];
                    }
                }
            }
            __syncthreads();
            // B: variable nodes, APP = lambda + r_new over the column's active edges (ascending edge order)
            for (int v = tid; v < N; v += nt) {
                const int c = v / Z, zv = v - c * Z;
                float s = lam[v];
                for (int k = cp[c]; k < cp[c + 1]; ++k) {
                    const int e = ce[k];
                    if (e >= ne) break;
                    int z = zv - esh[e];
                    if (z < 0) z += Z;
                    s += r[(size_t)e * Z + z];
                }
                app[v] = s;
            }
            __syncthreads();
            if (a.early_term) { // parity-check stop over the active rows, on the hard decisions APP < 0
                int bad = 0;
                for (int t = tid; t < nchk && !bad; t += nt) {
                    const int l = t / Z, z = t - l * Z;
                    int p = 0;
                    for (int e = rp[l]; e < rp[l + 1]; ++e) {
                        int zz = z + esh[e];
                        if (zz >= Z) zz -= Z;
                        p ^= app[ecol[e] * Z + zz] < 0.0f;
                    }
                    bad |= p;
                }
                if (!__syncthreads_or(bad)) break;
            }
            if (it >= a.max_iter) break;
        }
        for (int k = tid; k < K; k += nt) a.hard[(size_t)b * K + k] = app[k] < 0.0f;
        if (a.app)
            for (int v = tid; v < N; v += nt) a.app[(size_t)b * N + v] = app[v];
        if (a.iters && tid == 0) a.iters[b] = it;
        if (cw_out) // from the APP in LDS: the routine the finish kernel runs on app_out, so the bits are the same
            cw_finish_codeword(app, b, N, Z, a.nrows, nl, rp, ecol, esh, cw_bits, cw_red, a.cw_packed, a.unsatisfied, a.checks_packed);
        __syncthreads(); // APP, r and lambda belong to the next codeword from here on
    }
}

int bp_threads(int ncols, int Z) {
    const int n = ((ncols * Z + 63) / 64) * 64;
    return n < BP_MAX_THREADS ? n : BP_MAX_THREADS;
}

size_t bp_lds_bytes(int ncols, int Z) { return BP_TAB_BYTES + (size_t)ncols * Z * 4; }

hipError_t bp_resident(int threads, size_t lds, int* out, const char** what) {
    static size_t attr_lds[64] = {}; // dynamic LDS the kernel is allowed on each device so far (raised to what a launch needs)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) { *what = "hipGetDevice"; return e; }
    const void* k = reinterpret_cast<const void*>(nrldpc_bp_flood_kernel);
    if (lds > attr_lds[dev & 63]) {
        e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { (void)hipGetLastError(); *what = "hipFuncSetAttribute(sum-product kernel, dynamic LDS)"; return e; }
        attr_lds[dev & 63] = lds;
    }
    int per_cu = 0, cus = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, threads, lds);
    if (e != hipSuccess) { *what = "hipOccupancyMaxActiveBlocksPerMultiprocessor(sum-product kernel)"; return e; }
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) { *what = "hipDeviceGetAttribute(multiprocessor count)"; return e; }
    *out = per_cu * cus > 0 ? per_cu * cus : 1;
    return hipSuccess;
}

hipError_t launch_bp_flood(const BpArgs& a, int grid, int threads, size_t lds, hipStream_t stream) {
    if (a.nrows + 1 > T_RP || a.nnz > T_E || a.ncols + 1 > T_CP || threads > BP_MAX_THREADS || lds > 160 * 1024 || grid < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nrldpc_bp_flood_kernel, dim3(grid), dim3(threads), lds, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

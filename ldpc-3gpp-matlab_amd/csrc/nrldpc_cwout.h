// nrldpc_cwout.h -- whole-codeword hard decisions and final parity checks (nrldpc_cw_out of include/nrldpc.h): the launch interface
// of the finish kernel (nrldpc_cwout.hip) and the device routine it shares with the sum-product kernel's output stage
// (nrldpc_decode_bp.hip), so that both produce the same bits from the same a-posteriori LLRs.
// Kept apart from nrldpc_kernels.h: that header is part of the min-sum kernels' identity (nrldpc_kernel_id).
#ifndef NRLDPC_CWOUT_H
#define NRLDPC_CWOUT_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace nrldpc {

constexpr int CW_MAX_N = 68 * 384;             // longest codeword (BG1, Z = 384): 26112 bits
constexpr int CW_BIT_WORDS = CW_MAX_N / 64;    // 64-bit words of the LDS bit image: 408 (3264 bytes)
constexpr int CW_MAX_WAVES = 16;               // waves of a workgroup (1024 threads)
constexpr int CW_T_RP = 48, CW_T_E = 320;      // table capacities of the finish kernel (uint16): row_ptr, per-edge tables
// LDS bytes cw_finish_codeword needs: the bit image, then one count per wave
constexpr size_t CW_LDS_BYTES = (size_t)CW_BIT_WORDS * 8 + (size_t)CW_MAX_WAVES * 4;

struct CwFinishArgs {
    const float* app;        // [batch][ncols*Z] a-posteriori LLRs
    uint8_t* cw_packed;      // [batch][ceil(ncols*Z/8)], nullable
    int32_t* unsatisfied;    // [batch], nullable
    uint8_t* checks_packed;  // [batch][ceil(nrows*Z/8)], nullable
    const uint16_t* row_ptr; // base graph, row-ordered edges (the handle's d_row_ptr / d_col / d_shift: shifts mod Z)
    const uint8_t* col;
    const uint16_t* shift;
    int batch, Z, nrows, ncols, nnz, n_layers;
};

int cw_finish_threads(int ncols, int Z);
hipError_t launch_cw_finish(const CwFinishArgs& a, hipStream_t stream);

#if defined(__HIPCC__)
// The outputs of codeword b from its a-posteriori LLRs `app` (global memory or LDS), by the whole workgroup (blockDim.x a multiple
// of 64, at most 1024; every thread calls it).  Bit v = app[v] < 0: NaN, +-0 and +inf give 0, -inf gives 1.
//   pass 1: a wave takes 64 consecutive v, __ballot goes into the LDS image as one 64-bit word (bits past N -- N is a multiple of
//           4, not of 8 or 64 -- are 0 because the predicate includes v < N); cw_packed is written from the image, a byte per
//           thread, ceil(N/8) of them;
//   pass 2: a wave takes 64 consecutive checks t = l*Z + z over ALL rows, the parity of an active one is the XOR of the image's
//           bits at col*Z + (z + shift) mod Z, an inactive one is 0; the ballot's bytes go to checks_packed from lanes 0..7, its
//           population count into the wave's count; the counts are added in wave order by thread 0.  No atomics.
// rp / ecol / esh: the graph tables in LDS; bits / red: CW_LDS_BYTES of LDS, 8-byte aligned.  Ends with the image still in use by
// no one: the caller's next __syncthreads() frees it.
static __device__ __forceinline__ void cw_finish_codeword(const float* app, int b, int N, int Z, int nrows, int nl,
                                                          const uint16_t* rp, const uint16_t* ecol, const uint16_t* esh,
                                                          unsigned long long* bits, int* red, uint8_t* cw_packed,
                                                          int32_t* unsatisfied, uint8_t* checks_packed) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w0 = tid - lane;
    for (int v0 = w0; v0 < N; v0 += nt) { // v0 is the same for the 64 lanes of a wave: the ballot sees whole waves
        const int v = v0 + lane;
        const unsigned long long m = __ballot(v < N && app[v] < 0.0f);
        if (lane == 0) bits[v0 >> 6] = m;
    }
    __syncthreads();
    if (cw_packed) {
        const unsigned char* img = reinterpret_cast<const unsigned char*>(bits); // little-endian: byte i holds bits 8i .. 8i+7
        const int nbytes = (N + 7) >> 3;
        uint8_t* dst = cw_packed + (size_t)b * (size_t)nbytes;
        for (int i = tid; i < nbytes; i += nt) dst[i] = img[i];
    }
    if (!unsatisfied && !checks_packed) return;
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(bits);
    const int nchk = nrows * Z, nact = nl * Z, cbytes = (nchk + 7) >> 3;
    int cnt = 0;
    for (int t0 = w0; t0 < nchk; t0 += nt) {
        const int t = t0 + lane;
        uint32_t p = 0;
        if (t < nact) {
            const int l = t / Z, z = t - l * Z;
            for (int e = rp[l]; e < rp[l + 1]; ++e) {
                int zz = z + esh[e];
                if (zz >= Z) zz -= Z;
                const int v = ecol[e] * Z + zz;
                p ^= bw[v >> 5] >> (v & 31);
            }
            p &= 1u;
        }
        const unsigned long long m = __ballot(p != 0);
        cnt += __popcll(m);
        if (checks_packed && lane < 8) {
            const int i = (t0 >> 3) + lane; // t0 is a multiple of 64: byte i holds checks 8i .. 8i+7
            if (i < cbytes) checks_packed[(size_t)b * (size_t)cbytes + i] = (uint8_t)(m >> (8 * lane));
        }
    }
    if (unsatisfied) {
        if (lane == 0) red[tid >> 6] = cnt;
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int w = 0; w < (nt >> 6); ++w) s += red[w];
            unsatisfied[b] = s;
        }
    }
}
#endif

} // namespace nrldpc
#endif

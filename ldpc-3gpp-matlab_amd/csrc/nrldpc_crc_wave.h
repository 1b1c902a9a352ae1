// nrldpc_crc_wave.h -- the wave-parallel CRC the CRC stages share (nrldpc_crc.hip, nrldpc_mix.hip): one wave64 takes the remainder
// of a message staged in LDS.  Each lane runs the bit-serial CRC register over its own contiguous chunk and the 64 chunk remainders
// are combined pairwise in a log2(64) tree with
//     crc(A || B) = crc(A) * x^|B| mod g  xor  crc(B),
// the multiplication by x^(chunk * 2^s) being a precomputed 24x24 GF(2) matrix per tree level (CrcPlan, made on the host from the
// polynomial of get_3gpp_crc_polynomial.m:3-14).  Zero initial state => leading zeros are free.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_kernels.h" // CrcPlan

namespace nrldpc {

// v * M over GF(2), M = 24 columns (zero beyond the CRC length) in kernel-argument or device memory.  Every lane calls
// this (wave-uniform control flow): lane b fetches column b once and the 24 columns are then broadcast with
// v_readlane, so no scalar-load latency sits inside the loop.
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t* M, uint32_t v) {
    const int lane = threadIdx.x & 63;
    const uint32_t mine = M[lane < 24 ? lane : 0];
    uint32_t o = 0;
#pragma unroll
    for (int b = 0; b < 24; ++b) o ^= (0u - ((v >> b) & 1u)) & (uint32_t)__builtin_amdgcn_readlane((int)mine, b);
    return o;
}

// CRC remainder of `len` bits (one per byte, in LDS) by one wave; every lane returns the result.
// pl.chunk bits per lane with 64 * chunk >= len; the shortfall acts as leading zeros.
__device__ __forceinline__ uint32_t wave_crc(const uint8_t* bits, int len, const CrcPlan& pl) {
    const int lane = threadIdx.x & 63;
    const int chunk = pl.chunk;
    const int pad = 64 * chunk - len;
    const uint32_t top = 1u << (pl.L - 1), mask = (1u << pl.L) - 1u, poly = pl.poly & mask;
    uint32_t reg = 0;
    const int i0 = lane * chunk - pad;
#pragma unroll 4
    for (int i = i0 < 0 ? 0 : i0; i < i0 + chunk; ++i) {
        const uint32_t fb = ((reg & top) ? 1u : 0u) ^ (bits[i] & 1u);
        reg = (reg << 1) & mask;
        reg ^= fb ? poly : 0u;
    }
    // tree: after level s, lanes that are multiples of 2^(s+1) hold the CRC of 2^(s+1) chunks
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const uint32_t right = __shfl_down(reg, 1 << s, 64);
        reg = gf2_apply(pl.shiftmat[s], reg) ^ right;
    }
    return __shfl(reg, 0, 64);
}

// bytes of LDS a wave's row of K bits takes (stage_row, nrldpc_wave.h)
__host__ __device__ __forceinline__ int row_capacity(int K) { return ((K + 15) & ~15) + 48; }

} // namespace nrldpc

// nrldpc_noise.h -- the library's complex Gaussian noise, shared by the fused channel kernel (nrldpc_channel.hip) and the stand-alone
// AWGN stage (nrldpc_awgn.hip): the two draw the same sample for the same (seed, global symbol index).  The test oracle restates it in
// float64 (channel_oracle.noise).  (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// Pair c of the global symbol count -- symbols 2c and 2c+1 -- owns one Philox-4x32-10 block, counter (c, c>>32, 0, 0), key = seed:
// words 0,1 feed the even symbol, words 2,3 the odd one.  A symbol's two words become one Box-Muller sample.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrldpc {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// Box-Muller from the two uniform words of one symbol, in polar form: the radius of a complex sample with deviation sigma = sqrt(N0/2)
// per rail, and its direction (cos, sin); the sample is (rad * cs, rad * sn).  The RADIUS takes the scale, before the direction is
// applied, in both kernels: (r * sigma) * cos and (r * cos) * sigma round differently.  (sigma is an argument, not a factor the caller
// applies afterwards, so that the fused kernel compiles to the instructions it had when these lines stood in it.)
__device__ __forceinline__ void box_muller(uint32_t w1, uint32_t w2, float sigma, float& rad, float& cs, float& sn) {
    // 24-bit uniforms in (0,1): exact in f32
    const float u1 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f), u2 = ((float)(w2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    // The hardware's own transcendentals: v_sin_f32 / v_cos_f32 take their argument in REVOLUTIONS, so sin(2 pi u2) is one
    // instruction on u2 itself -- no range reduction (the library sincosf carries a Payne-Hanek path for arguments it never gets
    // here); v_log_f32 is log2, v_sqrt_f32 is within 1 ulp.  Results move by ~1e-6 relative against the float64 definition.
    rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1)) * sigma; // -2 ln u1 = -2 ln2 log2 u1
    sn = __builtin_amdgcn_sinf(u2);
    cs = __builtin_amdgcn_cosf(u2);
}

} // namespace nrldpc

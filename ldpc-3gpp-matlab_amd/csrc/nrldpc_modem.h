// nrldpc_modem.h -- what the fused channel kernel (nrldpc_channel.hip) and the stand-alone symbol mapper / soft demapper
// (nrldpc_modem.hip) share: the TS 38.211 rail arithmetic, and the launch arguments of the stand-alone kernels, the stand-alone AWGN
// stage (nrldpc_awgn.hip) among them.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrldpc {

// amplitude of one I/Q rail from its NB bits, most significant (sign) first: TS 38.211 5.1.3-5.1.5,
// 16QAM (1-2b0)(2-(1-2b2)), 64QAM (1-2b0)(4-(1-2b2)(2-(1-2b4))), 256QAM one level more
template <int NB> __device__ __forceinline__ float pam_level(uint32_t code) {
    float x = 1.0f;
#pragma unroll
    for (int j = 1; j < NB; ++j) {
        const uint32_t b = (code >> (j - 1)) & 1u; // innermost (last) bit first
        x = (float)(1 << j) - (b ? -x : x);
    }
    return ((code >> (NB - 1)) & 1u) ? -x : x;
}

template <int NB> __device__ __forceinline__ void rail_llr(float y, float inv_n0, float inv_norm, float (&llr)[NB]) {
    if constexpr (NB == 1) { // two points +-p: log-sum-exp of one term each, ((y+p)^2 - (y-p)^2)/N0 = 4 p y / N0
        llr[0] = 4.0f * inv_norm * y * inv_n0;
        return;
    }
    float mx[NB][2], sm[NB][2];
#pragma unroll
    for (int k = 0; k < NB; ++k) { mx[k][0] = mx[k][1] = -3.0e38f; sm[k][0] = sm[k][1] = 0.0f; }
    float met[1 << NB];
#pragma unroll
    for (uint32_t c = 0; c < (1u << NB); ++c) {
        const float d = y - pam_level<NB>(c) * inv_norm;
        met[c] = -d * d * inv_n0;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int bit = (c >> (NB - 1 - k)) & 1u;
            mx[k][bit] = fmaxf(mx[k][bit], met[c]);
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < (1u << NB); ++c)
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int bit = (c >> (NB - 1 - k)) & 1u;
            sm[k][bit] += __builtin_amdgcn_exp2f((met[c] - mx[k][bit]) * 1.4426950408889634f); // e^x = 2^(x log2 e): v_exp_f32
        }
#pragma unroll
    for (int k = 0; k < NB; ++k) // (sums lie in [1, 2^NB]: v_log_f32 needs no denormal care)
        llr[k] = (mx[k][0] - mx[k][1]) + 0.6931471805599453f * (__builtin_amdgcn_logf(sm[k][0]) - __builtin_amdgcn_logf(sm[k][1]));
}

// N dwords at an address that is dword-aligned and no more: the compiler picks dwordx4 / x3 / x2 pieces
template <int N> __device__ __forceinline__ void load_words(const void* p, uint32_t (&w)[N]) {
    __builtin_memcpy(w, __builtin_assume_aligned(p, 4), 4 * N);
}
template <int N> __device__ __forceinline__ void store_words(void* p, const uint32_t (&w)[N]) {
    __builtin_memcpy(__builtin_assume_aligned(p, 4), w, 4 * N);
}

// ---- stand-alone mapper / demapper (nrldpc_modem.hip) ----------------------------------------------------------------------------
struct ModArgs {
    const uint8_t* g; // [n_sym * Qm] bits, one byte each
    float* tx;        // [n_sym][2] (re, im)
    int64_t n_sym;
    int32_t Qm;
    float inv_norm;   // 1 / sqrt(2 mean(level^2))
};
struct DemodArgs {
    const float* rx;  // [n_sym][2] (re, im)
    const float* var; // [n_sym] complex noise variance per symbol, or null: `variance` for every symbol
    void* out;        // [n_sym * Qm]: f32 / f16 LLRs, or bytes {0,1} (method 2)
    int64_t n_sym;
    int32_t Qm, method, out_dtype; // NRLDPC_DEMOD_*, NRLDPC_LLR_F32 / _F16 (not read for method 2)
    float variance, inv_norm;
};
hipError_t launch_modulate(const ModArgs& a, hipStream_t stream);
hipError_t launch_demodulate(const DemodArgs& a, hipStream_t stream);

// ---- stand-alone AWGN stage (nrldpc_awgn.hip) ------------------------------------------------------------------------------------
struct AwgnArgs {
    const float* tx;  // [n_sym][2] (re, im)
    const float* var; // [n_sym] complex noise variance per symbol, or null: `variance` for every symbol
    float* rx;        // [n_sym][2]; may equal tx
    int64_t n_sym;
    uint64_t seed, first_symbol; // Philox key; global index of local symbol 0
    float variance;
};
hipError_t launch_awgn(const AwgnArgs& a, hipStream_t stream);

} // namespace nrldpc

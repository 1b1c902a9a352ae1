// nrldpc_payload_bits.h -- the payload draw of the Monte-Carlo loop (plot_BLER_vs_SNR.m:118: a = round(rand(A,1)) per block), per
// four-bit chunk: one copy for nrldpc_payload_bits_kernel (nrldpc_channel.hip) and the mixed-batch draw nrldpc_mix_tx_payload_kernel
// (nrldpc_mix_mc.hip), as nrldpc_channel_sym.h is for the fused channel stage.
// (Not in nrldpc_kernels.h: that header is part of the decoder kernels' identity, nrldpc_kernel_id.)
//
// Bit i of the transport block with GLOBAL index `block` = bit (i mod 64) of splitmix64(seed + (block*W + i div 64 + 1) * golden),
// W = ceil(A/64) (harness.payload_bits_np is the definition): a function of the global block index alone, so any split of a batch over
// devices, launches or configurations of a mix draws the same payloads.  A thread writes four consecutive bits of a block as four
// bytes (64 % 4 == 0: they never straddle a hash word).
//
// Plain C++ that a host compiler reads too: tests/mix_host/mix_mc_check.cpp runs the chunk rule on the CPU against payload_bits_np.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NRLDPC_PAYLOAD_HD __host__ __device__ __forceinline__
#else
#define NRLDPC_PAYLOAD_HD inline
#endif

namespace nrldpc {

NRLDPC_PAYLOAD_HD uint64_t splitmix64(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// four-bit chunks per block
NRLDPC_PAYLOAD_HD int32_t payload_chunks(int32_t A) { return (A + 3) >> 2; }

// hash words per block
NRLDPC_PAYLOAD_HD int32_t payload_words(int32_t A) { return (A + 63) >> 6; }

// bits i0 .. i0+3 (i0 a multiple of 4) of the block with global index `block`, bit k of the result = bit i0 + k; W = payload_words(A)
NRLDPC_PAYLOAD_HD uint32_t payload_nibble(uint64_t seed, uint64_t block, int32_t W, int32_t i0) {
    const uint64_t h = splitmix64(seed + ((block * (uint64_t)W + (uint64_t)(i0 >> 6)) + 1ull) * 0x9E3779B97F4A7C15ull);
    return (uint32_t)(h >> (i0 & 63)) & 0xFu;
}

// the chunk's bytes: o = the address of bit i0 of the block's row.  One 4-byte store where the chunk is whole and its REAL address
// allows it, a byte loop up to the row end otherwise -- the same bytes either way, at any byte address of the array.
NRLDPC_PAYLOAD_HD void payload_store_chunk(uint8_t* o, uint32_t nib, int32_t i0, int32_t A) {
    if (i0 + 4 <= A && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = (nib * 0x00204081u) & 0x01010101u; // bit k of the nibble -> byte k
    } else {
        for (int k = 0; k < 4 && i0 + k < A; ++k) o[k] = (uint8_t)((nib >> k) & 1u);
    }
}

} // namespace nrldpc

// nrldpc_mix_mc.hip -- the two Monte-Carlo stages of a MIX of transport-block configurations on the transmit plan: the payload draw
// nrldpc_mix_tx_payload_dev (one launch) and the outcome latch nrldpc_mix_tx_outcome_dev (one launch, and a second small one when the
// caller asks for the per-configuration count of blocks still retransmitting); semantics: include/nrldpc.h, DESIGN.md section 4.21.
//
// Table driven, like the other mixed stages: the per-configuration records and the prefix tables live in device memory, uploaded once by
// nrldpc_mix_tx_create and never written again; a workgroup (payload) or a wave (outcome) finds its configuration by a binary search of
// a prefix table (nrldpc_mix.h: mix_find), so everything that selects a code path is wave-uniform.  Every index and every byte moved is
// formed by nrldpc_mix_mc.h, which tests/mix_host/mix_mc_check.cpp runs on the CPU; what is left here is the launch geometry and the
// wave votes.
//
// Payload: nrldpc_payload_bits_kernel's thread (nrldpc_channel.hip) inside each segment -- the shared chunk rule of
// nrldpc_payload_bits.h, seed and first block read from the caller's device record of the configuration.
// Outcome: integers only, one writer per byte, no atomics -- a wave owns a transport block, its lanes the bytes l, l + 64, ... of the
// block's rows; "does any byte differ" is one wave vote, and lane 0 writes done and good.  The count of blocks not yet done is summed by
// one wave per configuration from votes over 64 blocks at a time, in block order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nrldpc_mix_mc.h"

namespace nrldpc {

static_assert(sizeof(MixMcRec) == 40, "records are laid out as an array with int64 members");
static_assert(sizeof(nrldpc_mix_draw) == 16, "nrldpc_mix_draw: the size include/nrldpc.h states");

__global__ __launch_bounds__(MIX_MC_BLOCK) void nrldpc_mix_tx_payload_kernel(const MixMcPayLaunch l) {
    const MixMcPayThread th = mix_mc_pay_thread(l.prefix, l.recs, l.n, (int)blockIdx.x, (int)threadIdx.x);
    if (th.b < 0) return;
    const MixMcRec c = l.recs[th.cfg];
    const nrldpc_mix_draw d = l.draw[th.cfg];
    mix_mc_pay_store(c, th, d.seed, d.first_block, l.a);
}

__global__ __launch_bounds__(MIX_MC_BLOCK) void nrldpc_mix_tx_outcome_kernel(const MixMcOutLaunch l) {
    const int wave = (int)threadIdx.x / MIX_MC_WAVE, lane = (int)threadIdx.x % MIX_MC_WAVE;
    const MixMcOutWave w = mix_mc_out_wave(l.tb_prefix, l.n, (int)blockIdx.x, wave);
    if (w.cfg < 0) return;
    const MixMcRec c = l.recs[w.cfg];
    const MixMcOutState s = mix_mc_out_state(c, w.t, l.first, l.ok, l.done);
    const bool differs = mix_mc_out_lane(c, w.t, lane, s, l.a, l.b_hat, l.a_hat);
    const bool any_differs = __any(differs) != 0; // (every lane of the wave is here: the exits above are wave-uniform)
    if (lane == 0) mix_mc_out_finish(c, w.t, s, any_differs, l.done, l.good);
}

__global__ __launch_bounds__(MIX_MC_BLOCK) void nrldpc_mix_tx_left_kernel(const MixMcOutLaunch l) {
    const int wave = (int)threadIdx.x / MIX_MC_WAVE, lane = (int)threadIdx.x % MIX_MC_WAVE;
    const int32_t i = mix_mc_left_cfg(l.n, (int)blockIdx.x, wave);
    if (i < 0) return;
    const MixMcRec c = l.recs[i];
    int32_t left = 0;
    for (int32_t k = 0; k < mix_mc_left_sweeps(c); ++k) left += __popcll(__ballot(mix_mc_left_lane(c, k, lane, l.done)));
    if (lane == 0) l.left[i] = left;
}

hipError_t launch_mix_mc_payload(const MixMcPayLaunch& a, hipStream_t stream) {
    if (a.n_wg <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_tx_payload_kernel, dim3(a.n_wg), dim3(MIX_MC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mix_mc_outcome(const MixMcOutLaunch& a, hipStream_t stream) {
    if (a.n_tb_total <= 0) return hipSuccess;
    hipLaunchKernelGGL(nrldpc_mix_tx_outcome_kernel, dim3(mix_mc_out_wgs(a.n_tb_total)), dim3(MIX_MC_BLOCK), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.left) return e;
    hipLaunchKernelGGL(nrldpc_mix_tx_left_kernel, dim3(mix_mc_left_wgs(a.n)), dim3(MIX_MC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

} // namespace nrldpc

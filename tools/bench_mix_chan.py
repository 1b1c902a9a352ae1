"""The channel leg of a mixed batch: one launch per stage against the loop of single calls.

Two workloads: the mix of tools/bench_mix_tx.py (DESIGN.md sections 4.15 - 4.18: one configuration per (BG, lifting size) that a
parameter object reaches with C = 1, R = 1/3, QPSK; 80 transport blocks each) and a UNIFORM plan (one configuration, the headline
transport block x 4096), where the table-driven form buys nothing and only its cost shows.  For each of the four stages -- the fused
nrldpc_mix_chan_awgn_llr_dev, and nrldpc_mix_chan_modulate_dev / _awgn_dev / _demodulate_dev -- two versions, alternated in one process:
  (a) the loop: the single call once per configuration at the plan's offsets (what a caller did before);
  (b) the one mix launch.
Both write the same packed layout, so their outputs are compared equal, bit for bit, in the same run.  A repetition is GROUP
invocations of the stage back to back between one pair of device events (a single launch of a few microseconds would measure the event
pair); reported is the time per invocation: median, minimum and maximum over the repetitions, spread = (max - min) / median, and the host
time to enqueue.  For the two memory-bound stages (mapper, demapper) the bytes read plus written are set against
tools/ubench/hbm_copy.hip at the same traffic when its binary is given.

    python tools/bench_mix_chan.py [--out profiles/mix_chan_vs_loop.json] [--reps 20] [--warmup 3] [--hbm-copy tools/ubench/hbm_copy.bin]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
import torch  # noqa: E402
from bench_mix_chain import ALL_Z, one_block_params  # noqa: E402  (the mix of section 4.15, from its own tool)
from bench_mix_skip import hbm_copy  # noqa: E402

STAGES = ("awgn_llr", "modulate", "awgn", "demodulate")
vp, i32, i64, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "spread": float((x.max() - x.min()) / np.median(x))}


def workload(ps, n_tb, args):
    """Time the four stages of one plan both ways; returns the result record."""
    lib = pkg.load()
    n = len(ps)
    plan = pkg.MixChanPlan(ps, n_tb)
    tot, goff, soff = plan.totals(), [o.g for o in plan.off], plan.sym_off
    bits = [k * p.G for p, k in zip(ps, n_tb)]
    syms = [b // p.Q_m for b, p in zip(bits, ps)]
    first = [int(x) for x in np.concatenate([[0], np.cumsum(syms)[:-1]])]  # one symbol stream, configuration after configuration
    seeds = [1234 + i for i in range(n)]
    pts = plan.points(args.esn0, seeds, first)
    d_pt = torch.from_numpy(np.frombuffer(pts, np.uint8).copy()).cuda()
    n0 = [float(pts[i].variance) for i in range(n)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randint(0, 2, (tot["g"],), generator=gen, device="cuda", dtype=torch.uint8)
    tx = torch.zeros(2 * tot["sym"], dtype=torch.float32, device="cuda")
    rx = torch.zeros_like(tx)
    out = {v: {"awgn_llr": torch.zeros(tot["g"], dtype=torch.float32, device="cuda"), "modulate": torch.zeros_like(tx), "awgn": torch.zeros_like(tx),
               "demodulate": torch.zeros(tot["g"], dtype=torch.float32, device="cuda")} for v in ("a", "b")}
    s = vp(torch.cuda.current_stream().cuda_stream)
    h = plan._h
    # the inputs of the later stages, made once by the mix calls
    plan.modulate(g.data_ptr(), tx.data_ptr(), stream=s.value)
    plan.awgn(tx.data_ptr(), d_pt.data_ptr(), rx.data_ptr(), stream=s.value)
    torch.cuda.synchronize()
    live = [i for i in range(n) if bits[i]]

    def loop_args(stage, dst):
        """the argument tuples of the single calls, made once: the timed loop only calls"""
        o = dst.data_ptr()
        if stage == "awgn_llr":
            return [(vp(g.data_ptr() + goff[i]), i64(bits[i]), i32(ps[i].Q_m), f32(args.esn0), u64(seeds[i]), u64(first[i]), vp(o + 4 * goff[i]), s) for i in live]
        if stage == "modulate":
            return [(vp(g.data_ptr() + goff[i]), i64(bits[i]), i32(ps[i].Q_m), vp(o + 8 * soff[i]), s) for i in live]
        if stage == "awgn":
            return [(vp(tx.data_ptr() + 8 * soff[i]), i64(syms[i]), f32(n0[i]), None, u64(seeds[i]), u64(first[i]), vp(o + 8 * soff[i]), s) for i in live]
        return [(vp(rx.data_ptr() + 8 * soff[i]), i64(syms[i]), i32(ps[i].Q_m), i32(0), f32(n0[i]), None, vp(o + 4 * goff[i]), i32(0), s) for i in live]

    single = {"awgn_llr": lib.nrldpc_awgn_llr_dev, "modulate": lib.nrldpc_modulate_dev, "awgn": lib.nrldpc_awgn_dev, "demodulate": lib.nrldpc_demodulate_dev}
    pt = vp(d_pt.data_ptr())

    def mix_call(stage, dst):
        o = vp(dst.data_ptr())
        if stage == "awgn_llr":
            return lambda: lib.nrldpc_mix_chan_awgn_llr_dev(h, vp(g.data_ptr()), pt, o, s)
        if stage == "modulate":
            return lambda: lib.nrldpc_mix_chan_modulate_dev(h, vp(g.data_ptr()), o, s)
        if stage == "awgn":
            return lambda: lib.nrldpc_mix_chan_awgn_dev(h, vp(tx.data_ptr()), pt, None, o, s)
        return lambda: lib.nrldpc_mix_chan_demodulate_dev(h, vp(rx.data_ptr()), 0, pt, None, o, 0, s)

    res = {}
    for stage in STAGES:
        tuples, fn_a = loop_args(stage, out["a"][stage]), single[stage]

        def run_a():
            for t in tuples:
                if fn_a(*t):
                    raise RuntimeError(lib.nrldpc_last_error())

        call_b = mix_call(stage, out["b"][stage])

        def run_b():
            if call_b():
                raise RuntimeError(lib.nrldpc_last_error())

        rec = {v: {"device": [], "host": []} for v in ("a", "b")}
        for it in range(args.warmup + args.reps):
            for v, fn in (("a", run_a), ("b", run_b)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.group):
                    fn()
                e1.record()
                host = (time.perf_counter() - t0) * 1e3 / args.group
                torch.cuda.synchronize()
                if it >= args.warmup:
                    rec[v]["device"].append(e0.elapsed_time(e1) / args.group)
                    rec[v]["host"].append(host)
        a, b = out["a"][stage], out["b"][stage]
        equal = bool((a.view(torch.int32) == b.view(torch.int32)).all()) and bool(b.any())
        r = {"a_loop": {k: stats(x) for k, x in rec["a"].items()}, "b_one_launch": {k: stats(x) for k, x in rec["b"].items()},
             "launches": {"a_loop": len(live), "b_one_launch": 1}, "outputs_equal_bit_for_bit": equal}
        r["loop_over_one_launch_median"] = r["a_loop"]["device"]["median"] / r["b_one_launch"]["device"]["median"]
        r["b_range_wholly_below_a_range"] = bool(r["b_one_launch"]["device"]["max"] < r["a_loop"]["device"]["min"])
        r["bytes_read_plus_written"] = {"awgn_llr": 5 * sum(bits), "modulate": sum(bits) + 8 * sum(syms), "awgn": 16 * sum(syms), "demodulate": 8 * sum(syms) + 4 * sum(bits)}[stage]
        r["TB_s_b"] = r["bytes_read_plus_written"] / (r["b_one_launch"]["device"]["median"] * 1e-3) / 1e12
        res[stage] = r
    plan.close()
    return {"configurations": n, "non_empty": len(live), "transport_blocks": sum(n_tb), "bits": sum(bits), "symbols": sum(syms),
            "Q_m": sorted({p.Q_m for p in ps}), "EsN0_dB": args.esn0, "stages": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_chan_vs_loop.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--group", type=int, default=8, help="invocations back to back between one event pair")
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--uniform-n", type=int, default=4096)
    ap.add_argument("--esn0", type=float, default=0.0)
    ap.add_argument("--hbm-copy", default=None, help="the binary built from tools/ubench/hbm_copy.hip")
    args = ap.parse_args()
    mix = [p for bg in (1, 2) for Z in ALL_Z for p in [one_block_params(bg, Z)] if p is not None]
    head = pkg.NRLDPC(BG=1, A=8424, G=25272, Q_m=2)
    head.validate()
    res = {"tool": "tools/bench_mix_chan.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(), "reps": args.reps, "warmup": args.warmup,
           "invocations_per_event_pair": args.group, "unit": "ms per invocation of the stage (device events unless said otherwise)",
           "mixed": workload(mix, [args.n_tb] * len(mix), args),
           "uniform": dict(workload([head], [args.uniform_n], args), configuration="BG1, Z = 384, A = 8424, G = 25272, QPSK, C = 1"),
           "not_measured": ["mixes whose configurations differ in Q_m (this mix is QPSK throughout: the register count of the 256QAM body is carried, its "
                            "arithmetic is not run)", "per-symbol variance arrays", "f16 and hard-bit outputs, the max-log method", "hardware counters of the new kernels",
                            "MixedChannel.step end to end with its copy of the operating points", "several streams sharing one plan"]}
    if args.hbm_copy:
        mbs = sorted({round(res[w]["stages"][st]["bytes_read_plus_written"] / 1e6, 3) for w in ("mixed", "uniform") for st in ("modulate", "demodulate")})
        got, raw = hbm_copy(args.hbm_copy, mbs)
        res["hbm_copy_at_the_same_traffic"] = [{"traffic_MB": mb, **v} for mb, v in sorted(got.items())]
        res["hbm_copy_output"] = raw.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not all(res[w]["stages"][st]["outputs_equal_bit_for_bit"] for w in ("mixed", "uniform") for st in STAGES):
        print("OUTPUTS DIFFER between the loop and the one launch", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

"""The Monte-Carlo loop's own stages on a mixed batch, and the mixed sweep: one launch against the loop, and plot_SNR_vs_A both ways.

(a) Stages.  Two workloads: the mix of tools/bench_mix_tx.py (DESIGN.md sections 4.15 - 4.20: one configuration per (BG, lifting size)
    that a parameter object reaches with C = 1, R = 1/3, QPSK; 80 transport blocks each) and a UNIFORM plan (one configuration, the
    headline transport block x 4096), where the table-driven form buys nothing and only its cost shows.
      payload  nrldpc_mix_tx_payload_dev against nrldpc_payload_bits_dev once per configuration at the plan's offsets;
      outcome  nrldpc_mix_tx_outcome_dev (with d_left: two launches) against the tensor expressions of harness.simulate_point_device per
               configuration (newly / where / or, the final compare, and ok.all() as the "still retransmitting" question, left on the
               device: no read-back on either side).
    Both versions are alternated in one process; a repetition is GROUP invocations back to back between one pair of device events;
    reported per invocation: median, minimum, maximum, spread = (max - min) / median over the repetitions, and the host time to enqueue.
    Outputs are compared equal in the same run.
(b) Sweep.  Wall time of harness.plot_SNR_vs_A at the reference's defaults (device=True) with mixed=True against mixed=False, alternated,
    result files compared byte for byte.

    python tools/bench_mix_montecarlo.py [--out profiles/mix_montecarlo_vs_loop.json] [--reps 7] [--warmup 2] [--no-sweep]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
H = importlib.import_module("ldpc-3gpp-matlab_amd.harness")
import torch  # noqa: E402
from bench_mix_chain import ALL_Z, one_block_params  # noqa: E402  (the mix of section 4.15, from its own tool)

vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "spread": float((x.max() - x.min()) / np.median(x))}


def timed(versions, args):
    """Alternate the versions; device and host milliseconds per invocation."""
    rec = {v: {"device": [], "host": []} for v, _ in versions}
    for it in range(args.warmup + args.reps):
        for v, fn in versions:
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
    return {v: {k: stats(x) for k, x in r.items()} for v, r in rec.items()}


def compare(r, launches_a, launches_b, equal):
    r["launches"] = {"a_loop": launches_a, "b_one_launch": launches_b}
    r["outputs_equal"] = equal
    r["loop_over_one_launch_median"] = r["a_loop"]["device"]["median"] / r["b_one_launch"]["device"]["median"]
    r["b_range_wholly_below_a_range"] = bool(r["b_one_launch"]["device"]["max"] < r["a_loop"]["device"]["min"])
    return r


def workload(ps, n_tb, args):
    lib = pkg.load()
    n = len(ps)
    plan = pkg.MixTxPlan(ps, n_tb)
    a_off, off, tot = plan.a_off, plan.off, plan.totals()
    live = [i for i in range(n) if n_tb[i]]
    seeds, first = [77 + i for i in range(n)], [1000 * i for i in range(n)]
    s = vp(torch.cuda.current_stream().cuda_stream)
    h = plan._h
    # ---- payload
    d_draw = torch.from_numpy(np.frombuffer(plan.draws(seeds, first), np.uint8)[:16 * n].copy()).cuda()
    a = {v: torch.zeros(tot["a"], dtype=torch.uint8, device="cuda") for v in ("a", "b")}
    tuples = [(u64(seeds[i]), u64(first[i]), i32(n_tb[i]), i32(ps[i].A), vp(a["a"].data_ptr() + a_off[i]), s) for i in live]

    def pay_loop():
        for t in tuples:
            if lib.nrldpc_payload_bits_dev(*t):
                raise RuntimeError(lib.nrldpc_last_error())

    def pay_mix():
        if lib.nrldpc_mix_tx_payload_dev(h, vp(d_draw.data_ptr()), vp(a["b"].data_ptr()), s):
            raise RuntimeError(lib.nrldpc_last_error())

    res = {"payload": compare(timed((("a_loop", pay_loop), ("b_one_launch", pay_mix)), args), len(live), 1,
                              bool(torch.equal(a["a"], a["b"])) and bool(a["b"].any()))}
    res["payload"]["bytes_written"] = int(sum(n_tb[i] * ps[i].A for i in live))
    # ---- outcome: b_hat = the payload with every seventh block spoiled, three quarters of the blocks acknowledged
    gen = torch.Generator(device="cuda").manual_seed(9)
    b_hat = torch.zeros(off[n].b_hat, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(off[n].tb, dtype=torch.int32, device="cuda")
    for i in live:
        rows = a["b"][a_off[i]: a_off[i] + n_tb[i] * ps[i].A].view(n_tb[i], ps[i].A).clone()
        rows[::7, -1] ^= 1
        b_hat[off[i].b_hat: off[i].b_hat + n_tb[i] * ps[i].B].view(n_tb[i], ps[i].B)[:, :ps[i].A] = rows
        ok[off[i].tb: off[i].tb + n_tb[i]] = (torch.rand(n_tb[i], generator=gen, device="cuda") < 0.75).to(torch.int32)
    a_hat = torch.zeros(tot["a"], dtype=torch.uint8, device="cuda")
    done = torch.zeros(off[n].tb, dtype=torch.uint8, device="cuda")
    good = torch.zeros(off[n].tb, dtype=torch.uint8, device="cuda")
    left = torch.zeros(n, dtype=torch.int32, device="cuda")
    views = [dict(a=a["b"][a_off[i]: a_off[i] + n_tb[i] * ps[i].A].view(n_tb[i], ps[i].A),
                  dec=b_hat[off[i].b_hat: off[i].b_hat + n_tb[i] * ps[i].B].view(n_tb[i], ps[i].B)[:, :ps[i].A],
                  good=ok[off[i].tb: off[i].tb + n_tb[i]]) for i in live]
    ref = {}

    def out_loop():
        """one attempt of simulate_point_device's bookkeeping per configuration, from a fresh state (as `first` below)"""
        outs, alls = [], []
        for v in views:
            okv = torch.zeros(v["good"].shape[0], dtype=torch.bool, device="cuda")
            a_hat_v = torch.zeros_like(v["a"])
            g = v["good"] != 0
            newly = g & ~okv
            a_hat_v = torch.where(newly[:, None], v["dec"], a_hat_v)
            okv = okv | g
            alls.append(okv.all())
            outs.append(okv & (a_hat_v == v["a"]).all(dim=1))
        ref["good"], ref["all"] = outs, alls

    def out_mix():
        if lib.nrldpc_mix_tx_outcome_dev(h, vp(a["b"].data_ptr()), vp(b_hat.data_ptr()), vp(ok.data_ptr()), 1, vp(a_hat.data_ptr()),
                                         vp(done.data_ptr()), vp(good.data_ptr()), vp(left.data_ptr()), s):
            raise RuntimeError(lib.nrldpc_last_error())

    r = timed((("a_loop", out_loop), ("b_one_launch", out_mix)), args)
    equal = all(bool(torch.equal(good[off[i].tb: off[i].tb + n_tb[i]] != 0, ref["good"][k])) and bool(ref["all"][k]) == (int(left[i]) == 0)
                for k, i in enumerate(live))
    res["outcome"] = compare(r, "9 tensor operations per configuration: %d" % (9 * len(live)), 2, equal)
    res["outcome"]["bytes_read_plus_written_at_most"] = int(sum(n_tb[i] * (3 * ps[i].A + 6) for i in live))
    plan.close()
    return {"configurations": n, "non_empty": len(live), "transport_blocks": int(sum(n_tb)), "payload_bits": int(sum(n_tb[i] * ps[i].A for i in live)), "stages": res}


def sweep(args):
    """plot_SNR_vs_A at the reference's defaults, both ways, alternated; wall seconds."""
    wall = {False: [], True: []}
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(args.sweep_warmup + args.sweep_reps):
            files = {}
            for mixed in (False, True):
                d = os.path.join(tmp, "%d_%d" % (it, mixed))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                H.plot_SNR_vs_A(results_dir=d, device=True, mixed=mixed)
                torch.cuda.synchronize()
                if it >= args.sweep_warmup:
                    wall[mixed].append(time.perf_counter() - t0)
                files[mixed] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
            same = same and files[False] == files[True] and len(files[False]) == 1
    r = {"a_sequential_s": stats(wall[False]), "b_mixed_s": stats(wall[True]), "result_files_byte_identical": bool(same),
         "arguments": "plot_SNR_vs_A(device=True): A = 1000 ... 8000, R = 1/3, BG = 1, QPSK, 50 iterations, 100 block errors, target BLER 1e-2, batch 256",
         "reps": args.sweep_reps, "warmup": args.sweep_warmup}
    r["sequential_over_mixed_median"] = r["a_sequential_s"]["median"] / r["b_mixed_s"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_montecarlo_vs_loop.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group", type=int, default=8, help="invocations back to back between one event pair")
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--uniform-n", type=int, default=4096)
    ap.add_argument("--sweep-reps", type=int, default=7)
    ap.add_argument("--sweep-warmup", type=int, default=2)
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    mix = [p for bg in (1, 2) for Z in ALL_Z for p in [one_block_params(bg, Z)] if p is not None]
    head = pkg.NRLDPC(BG=1, A=8424, G=25272, Q_m=2)
    head.validate()
    res = {"tool": "tools/bench_mix_montecarlo.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(), "reps": args.reps, "warmup": args.warmup,
           "invocations_per_event_pair": args.group, "unit": "ms per invocation of the stage (device events unless said otherwise)",
           "mixed": workload(mix, [args.n_tb] * len(mix), args),
           "uniform": dict(workload([head], [args.uniform_n], args), configuration="BG1, Z = 384, A = 8424, G = 25272, QPSK, C = 1"),
           "not_measured": ["hardware counters of the three new kernels", "later attempts of the outcome stage (first = 0: one more byte read per block)",
                            "simulate_point_mixed on the 101-configuration mix end to end", "several streams sharing one plan",
                            "the sweep with other arguments than the reference's defaults"]}
    if args.no_sweep:
        res["not_measured"].append("the sweep (--no-sweep)")
    else:
        res["sweep"] = sweep(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    bad = not all(res[w]["stages"][st]["outputs_equal"] for w in ("mixed", "uniform") for st in ("payload", "outcome"))
    if bad or not res.get("sweep", {}).get("result_files_byte_identical", True):
        print("OUTPUTS DIFFER between the loop and the one launch", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

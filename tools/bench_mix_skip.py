"""Mixed HARQ retransmission step, demodulator LLRs to b_hat: MixedDecodeChain(I_HARQ=1, skip="settled") against the same chain with
skip=None (the step that decodes every code block), and the three launches the mode adds against a plain copy at the same traffic.

Two workloads (f32 demodulator LLRs, f16 LLRs into the decoder, f16 soft buffer, the parity-check stop, R = 1/3, QPSK, C = 1):
  headline   4096 transport blocks of BG1 Z = 384;
  mix        one configuration per (BG, lifting size) reachable with C = 1 (the mix of tools/bench_mix_chain.py), 80 transport blocks each.
The state every repetition starts from is what one transmission at rv_id = 0 leaves in the soft buffer, with the PENDING SHARE set
directly in the state arrays: in every configuration the first round(share * n_tb) transport blocks get ok = 0, cb_pass = 0 (pending),
the others ok = 1, cb_pass = 1 (settled) -- shares 1.0, 0.5, 0.1, 0.0.  The timed step is the retransmission at rv_id = 2.  The state is
restored before every repetition outside the timed region; the two chains alternate inside one repetition; a step is timed with device
events, and nothing synchronises between repetitions but the read-back the mode itself makes.
Each of the three launches (pending, gather, scatter) is also timed alone -- 8 launches back to back between one event pair, as
tools/ubench/hbm_copy.hip times a copy -- and set against that program's figure for the same bytes when its binary is given.
No acceptance ratio is fixed: the file states what was measured.

    python tools/bench_mix_skip.py [--out profiles/mix_skip_vs_full.json] [--reps 20] [--warmup 3] [--hbm-copy tools/ubench/hbm_copy.bin]
"""
import argparse
import copy
import json
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_mix_chain as B  # noqa: E402  (the mix, transmit(), stats())

pkg, DC, torch, ROOT = B.pkg, B.DC, B.torch, B.ROOT
SHARES = (1.0, 0.5, 0.1, 0.0)


def with_rv(p, rv):
    q = copy.copy(p)
    q.rv_id = rv
    return q


def spread(x):
    x = np.asarray(x, np.float64)
    return float((x.max() - x.min()) / np.median(x))


def group_time(fn, launches=8, groups=11):
    """median over groups of (one event pair around `launches` calls) / launches, in ms; the first group is a warm-up"""
    ms = []
    for rep in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1) / launches)
    return B.stats(ms)


def workload(args, name, ps, n_tb):
    C = pkg._capi
    n = len(ps)
    llr0, _ = B.transmit([with_rv(p, 0) for p in ps], n_tb, args.esn0, seed=7)
    llr2, _ = B.transmit([with_rv(p, 2) for p in ps], n_tb, args.esn0, seed=7)  # (the same payloads: transmit() draws them from its seed)
    kw = dict(iterations=args.iterations, I_HARQ=1, harq_dtype=np.float16)
    full, skip = DC.MixedDecodeChain(ps, n_tb, **kw), DC.MixedDecodeChain(ps, n_tb, skip="settled", **kw)
    res = {"configurations": n, "transport_blocks": sum(n_tb), "code_blocks": sum(k * p.C for p, k in zip(ps, n_tb)), "points": []}
    try:
        assert all(p.C == 1 for p in ps)
        g0, g2 = full.pack(llr0, "g"), full.pack(llr2, "g")
        full.step(g0, rv_id=0)
        torch.cuda.synchronize()
        snap_harq = full.harq.clone()
        res["ok_after_first_transmission"] = int(full.ok.sum())
        for ch in (full, skip):  # the codecs' layer counts for rv_id 2, the plans, the dense arrays: outside the timed region
            ch.harq.copy_(snap_harq)
            ch.step(g2, rv_id=2)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        for share in SHARES:
            flag = full.pack([torch.tensor([0] * round(share * k) + [1] * (k - round(share * k)), dtype=torch.int32, device="cuda") for k in n_tb], "tb")
            cb = full.pack([torch.tensor([0] * round(share * k) + [1] * (k - round(share * k)), dtype=torch.int32, device="cuda").view(k, 1) for k in n_tb], "cb")
            pending = sum(round(share * k) for k in n_tb)

            def restore(ch):
                ch.harq.copy_(snap_harq); ch.ok.copy_(flag); ch.cb_pass.copy_(cb)

            rec = {"full": [], "skip": []}
            evs = []
            for it in range(args.warmup + args.reps):
                for nm, ch in (("full", full), ("skip", skip)) if it % 2 == 0 else (("skip", skip), ("full", full)):
                    restore(ch)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ch.step(g2, rv_id=2)
                    e1.record()
                    if it >= args.warmup:
                        evs.append((nm, e0, e1))
            torch.cuda.synchronize()
            for nm, e0, e1 in evs:
                rec[nm].append(e0.elapsed_time(e1))
            assert skip.last_decoded == [round(share * k) for k in n_tb], (share, skip.last_decoded[:8])
            # the pending blocks end alike in both chains (the settled ones are the unskipped chain's to decode again)
            sel = flag[: full.plan.totals.tb] == 0
            same = bool((full.ok[sel] == skip.ok[sel]).all()) and (share < 1.0 or bool((full.b_hat == skip.b_hat).all()))
            a, b = B.stats(rec["full"]), B.stats(rec["skip"])
            point = {"pending_share": share, "pending_code_blocks": pending, "step_skip_none_ms": a, "step_skip_settled_ms": b,
                     "ratio_settled_over_none_median": b["median"] / a["median"], "spread_skip_none": spread(rec["full"]),
                     "spread_skip_settled": spread(rec["skip"]), "pending_blocks_end_alike": same}
            # ---- the three launches alone, on the state of this share
            restore(skip)
            plan = skip._plan_for(2)[0]
            dense_cw, dense_c, dense_it, _ = skip._dense if skip._dense is not None else (skip.cw_llr, skip.c_hat, skip.iters, None)
            torch.cuda.synchronize()
            t_pend = group_time(lambda: plan.pending(C.MIX_SKIP_SETTLED, skip.cb_pass.data_ptr(), skip.ok.data_ptr(), skip.cbgti.data_ptr(), None,
                                                     skip.index.data_ptr(), skip.count.data_ptr(), stream=stream))
            if skip._dense is not None:
                t_gather = group_time(lambda: plan.gather_cw(skip.cw_llr.data_ptr(), skip.index.data_ptr(), skip.count.data_ptr(), dense_cw.data_ptr(),
                                                             dtype=C.LLR_F16, stream=stream))
                t_scatter = group_time(lambda: plan.scatter_hard(dense_c.data_ptr(), dense_it.data_ptr(), skip.index.data_ptr(), skip.count.data_ptr(),
                                                                 skip.c_hat.data_ptr(), skip.iters.data_ptr(), stream=stream))
                rows = [round(share * k) for k in n_tb]
                point["gather"] = {"ms": t_gather, "traffic_MB": 2 * 2 * sum(r * (2 * p.Z_c + p.N) for r, p in zip(rows, ps)) / 1e6}
                point["scatter"] = {"ms": t_scatter, "traffic_MB": 2 * sum(r * p.K for r, p in zip(rows, ps)) / 1e6}
                for k in ("gather", "scatter"):
                    point[k]["GB_per_s"] = point[k]["traffic_MB"] / point[k]["ms"]["median"] if point[k]["ms"]["median"] else None
            point["pending"] = {"ms": t_pend, "state_bytes_read": sum(k * p.C * 5 + k * 4 for p, k in zip(ps, n_tb))}
            res["points"].append(point)
            print(name, json.dumps(point), flush=True)
        p1 = res["points"][0]
        res["all_pending_overhead_ms"] = p1["step_skip_settled_ms"]["median"] - p1["step_skip_none_ms"]["median"]
        res["all_pending_overhead_accounted_for_ms"] = {"pending_launch": p1["pending"]["ms"]["median"],
                                                        "note": "plus one n-element read-back and a stream synchronisation (not timed apart)"}
        # the pending share below which the mode wins: where the ratio crosses 1 between two measured points (linear in the share)
        cross = None
        pts = sorted(res["points"], key=lambda q: q["pending_share"])
        for lo, hi in zip(pts, pts[1:]):
            rl, rh = lo["ratio_settled_over_none_median"], hi["ratio_settled_over_none_median"]
            if rl < 1.0 <= rh:
                cross = lo["pending_share"] + (1.0 - rl) / (rh - rl) * (hi["pending_share"] - lo["pending_share"])
        res["mode_wins_below_pending_share"] = cross if cross is not None else ("every measured share" if pts[-1]["ratio_settled_over_none_median"] < 1 else None)
    finally:
        full.close()
        skip.close()
    return res


def hbm_copy(path, traffic_mb):
    """tools/ubench/hbm_copy.hip at the given traffic figures (a child process of its own): {MB: GB/s} of its 4 x 16 B per lane copy"""
    out = subprocess.run([path] + ["%.3f" % mb for mb in traffic_mb], capture_output=True, text=True, timeout=120).stdout
    got = {}
    for line in out.splitlines():
        m = re.match(r"copy \(4 x 16 B per lane\)\s+traffic\s+([\d.]+) MB\s+([\d.]+) ms per launch\s+([\d.]+) GB/s", line)
        if m:
            got[float(m.group(1))] = {"ms": float(m.group(2)), "GB_per_s": float(m.group(3))}
    return got, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_skip_vs_full.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--esn0", type=float, default=-1.0)
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--headline-tb", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--hbm-copy", default=None, help="the binary built from tools/ubench/hbm_copy.hip")
    args = ap.parse_args()
    res = {"tool": "tools/bench_mix_skip.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms (device events)", "rate": "1/3", "Q_m": 2, "EsN0_dB": args.esn0, "iterations": args.iterations, "stop": "parity check",
           "state": "soft buffer after one transmission at rv_id 0; ok / cb_pass set to the pending share", "timed_step": "rv_id 2"}
    mix = [p for bg in (1, 2) for Z in B.ALL_Z for p in [B.one_block_params(bg, Z)] if p is not None]
    res["headline"] = workload(args, "headline", [B.one_block_params(1, 384)], [args.headline_tb])
    res["mix"] = workload(args, "mix", mix, [args.n_tb] * len(mix))
    if args.hbm_copy:
        mbs = sorted({round(pt[k]["traffic_MB"], 3) for w in ("headline", "mix") for pt in res[w]["points"] for k in ("gather", "scatter") if k in pt and pt[k]["traffic_MB"] > 0})
        got, raw = hbm_copy(args.hbm_copy, mbs)
        res["hbm_copy_at_the_same_traffic"] = [{"traffic_MB": mb, **v} for mb, v in sorted(got.items())]
        res["hbm_copy_output"] = raw.splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

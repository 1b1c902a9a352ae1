"""The transmit plan's encode stage: one launch per configuration against one launch in all.

The mix is that of tools/bench_mix_tx.py: one configuration per (BG, lifting size) that a parameter object
reaches with C = 1, R = 1/3, QPSK, 80 transport blocks each.  Two versions of the three-stage step, alternated in one process, both
through the plan:
  (a) nrldpc_mix_tx_crc_attach_dev, nrldpc_mix_tx_encode_dev (n encoder launches: the parent's behaviour), nrldpc_mix_tx_rate_match_dev;
  (b) the same with nrldpc_mix_tx_encode_all_dev (one launch) in the middle.
Both write the same packed layout, so their outputs are compared equal in the same run.  Device events around every stage, warm-ups,
median and range; the host time to enqueue.  Criterion, for the encode stage and for the whole step: the range of (b) lies wholly
below the range of (a).  Then, without a threshold, a UNIFORM mix (one configuration, the headline transport block x 4096):
nrldpc_mix_tx_encode_all_dev beside the single nrldpc_encode_dev on the same input -- what the table-driven form costs where it is
not needed.

    python tools/bench_mix_tx_encode.py [--out profiles/mix_tx_encode_vs_loop.json] [--reps 30] [--warmup 5]
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
from bench_mix_chain import ALL_Z, one_block_params, stats  # noqa: E402  (the mix of section 4.15, from its own tool)

STAGES = ("attach", "encode", "rate_match")


def mixed(args):
    lib = pkg.load()
    ps = [p for bg in (1, 2) for Z in ALL_Z for p in [one_block_params(bg, Z)] if p is not None]
    n = len(ps)
    n_tb = [args.n_tb] * n
    plan = pkg.MixTxPlan(ps, n_tb)
    tot = plan.totals()
    codecs = {}
    for p in ps:
        if (p.BG, p.Z_c) not in codecs:
            codecs[(p.BG, p.Z_c)] = pkg.Codec(p.BG, p.Z_c, max_iter=1)
    gen = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(0, 2, (tot["a"],), generator=gen, device="cuda", dtype=torch.uint8)
    arr = {v: {k: torch.zeros(tot[k], dtype=torch.uint8, device="cuda") for k in ("c", "cw", "g")} for v in ("a", "b")}
    vp = ctypes.c_void_p
    s = vp(torch.cuda.current_stream().cuda_stream)
    hs = (vp * n)(*[codecs[(p.BG, p.Z_c)]._h for p in ps])
    h = plan._h
    m_att, m_enc, m_all, m_rm = (lib.nrldpc_mix_tx_crc_attach_dev, lib.nrldpc_mix_tx_encode_dev, lib.nrldpc_mix_tx_encode_all_dev,
                                 lib.nrldpc_mix_tx_rate_match_dev)
    pa = vp(a.data_ptr())
    ptr = {v: {k: vp(arr[v][k].data_ptr()) for k in arr[v]} for v in arr}

    def step(v, e):
        q = ptr[v]
        t0 = time.perf_counter()
        e[0].record()
        assert m_att(h, pa, q["c"], s) == 0
        e[1].record()
        if v == "a":
            assert m_enc(h, hs, q["c"], q["cw"], s) == 0
        else:
            assert m_all(h, q["c"], q["cw"], s) == 0
        e[2].record()
        assert m_rm(h, q["cw"], q["g"], s) == 0
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    rec = {v: {k: [] for k in ("host",) + STAGES + ("total",)} for v in ("a", "b")}
    for it in range(args.warmup + args.reps):
        for v in ("a", "b"):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            host = step(v, e)
            torch.cuda.synchronize()
            if it >= args.warmup:
                r = rec[v]
                r["host"].append(host)
                for k, st in enumerate(STAGES):
                    r[st].append(e[k].elapsed_time(e[k + 1]))
                r["total"].append(e[0].elapsed_time(e[3]))
    equal = all(bool((arr["a"][k] == arr["b"][k]).all()) for k in ("c", "cw", "g"))
    assert bool(arr["b"]["g"].any())
    res = {v: {k: stats(rec[v][k]) for k in rec[v]} for v in ("a", "b")}
    below = {st: bool(res["b"][st]["max"] < res["a"][st]["min"]) for st in ("encode", "total")}
    out = {
        "mix": {"configurations": n, "bg1": sum(p.BG == 1 for p in ps), "bg2": sum(p.BG == 2 for p in ps), "transport_blocks_each": args.n_tb,
                "transport_blocks": sum(n_tb), "rate": "1/3", "Q_m": 2, "distinct_bg_z": len(codecs),
                "workgroup_per_codeword_configurations": sum(p.BG == 1 and p.Z_c >= 128 for p in ps),
                "bytes": {"a": tot["a"], "c": tot["c"], "cw": tot["cw"], "g": tot["g"]}},
        "reps": args.reps, "warmup": args.warmup, "unit": "ms (device events unless said otherwise)",
        "a_per_configuration_encode": dict(res["a"], launches={"attach": 1, "encode": n, "rate_match": 1}),
        "b_one_launch_encode": dict(res["b"], launches={"attach": 1, "encode": 1, "rate_match": 1}),
        "outputs_of_a_and_b_equal": equal,
        "b_range_wholly_below_a_range": below,
        "speedup_median": {st: res["a"][st]["median"] / res["b"][st]["median"] for st in STAGES + ("total", "host")},
        "encode_share_of_b_step": res["b"]["encode"]["median"] / res["b"]["total"]["median"],
        "encode_bytes_read_plus_written": tot["c"] + tot["cw"],
        "encode_TB_s_b": (tot["c"] + tot["cw"]) / (res["b"]["encode"]["median"] * 1e-3) / 1e12,
        "criterion_encode_and_total_below": bool(equal and below["encode"] and below["total"]),
    }
    plan.close()
    for c in codecs.values():
        c.close()
    return out


def uniform(args):
    """One configuration, the headline transport block (BG1, Z = 384, A = 8424, G = 25272, QPSK) x 4096: the one-launch mixed encoder
    beside the single-configuration encoder on the same code blocks."""
    p = pkg.NRLDPC(BG=1, A=8424, G=25272, Q_m=2)
    p.validate()
    n = args.uniform_n
    plan = pkg.MixTxPlan([p], [n])
    codec = pkg.Codec(p.BG, p.Z_c, max_iter=1)
    ncw = 2 * p.Z_c + p.N
    gen = torch.Generator(device="cuda").manual_seed(3)
    c = torch.randint(0, 2, (n * p.C, p.K), generator=gen, device="cuda", dtype=torch.uint8)
    cw = [torch.empty((n * p.C, ncw), dtype=torch.uint8, device="cuda") for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream
    fns = {
        "encode_single": lambda: codec.encode_dev(c.data_ptr(), n * p.C, cw[0].data_ptr(), s),
        "encode_all": lambda: plan.encode_all(c.data_ptr(), cw[1].data_ptr(), stream=s),
    }
    ms = {k: [] for k in fns}
    for it in range(args.warmup + args.reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                ms[k].append(e0.elapsed_time(e1))
    nbytes = n * p.C * (p.K + ncw)
    out = {"configuration": "BG1, Z = 384, A = 8424, G = 25272, QPSK, C = 1", "transport_blocks": n, "outputs_equal": bool((cw[0] == cw[1]).all()),
           "bytes_read_plus_written": nbytes}
    for k, v in ms.items():
        out[k] = stats(v)
        out[k]["TB_s"] = nbytes / (np.median(v) * 1e-3) / 1e12
    out["encode_all_over_single_median"] = out["encode_all"]["median"] / out["encode_single"]["median"]
    plan.close()
    codec.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_tx_encode_vs_loop.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--uniform-n", type=int, default=4096)
    args = ap.parse_args()
    res = {"tool": "tools/bench_mix_tx_encode.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(), "mixed": mixed(args), "uniform": uniform(args),
           "not_measured": ["hardware counters of the new kernel", "mixes with C > 1 or with few configurations", "other transport-block counts than 80 and 4096",
                            "MixedEncodeChain.step end to end", "several streams sharing one plan"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not res["mixed"]["criterion_encode_and_total_below"]:
        print("CRITERION NOT MET: for the encode stage or the whole step the range of (b) does not lie wholly below the range of (a), or the outputs differ",
              file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

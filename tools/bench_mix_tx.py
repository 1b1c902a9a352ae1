"""Mixed transmit step, payload bits to rate-matched bits: the loop the single-configuration stages offer against the transmit plan.

The mix is that of tools/bench_mix_chain.py: one configuration per (BG, lifting size) that a parameter object
reaches with C = 1, R = 1/3, QPSK, 80 transport blocks each.  Two versions, alternated in one process:
  (a) n x nrldpc_crc_attach_dev, n x nrldpc_encode_dev, n x nrldpc_rate_match_dev, argument blocks prebuilt (what a C caller holds);
  (b) nrldpc_mix_tx_crc_attach_dev, nrldpc_mix_tx_encode_dev (the same n encoder launches), nrldpc_mix_tx_rate_match_dev.
Both write the same packed layout, so their outputs are compared equal in the same run.  Device events around every stage, warm-ups,
median and range; the host time to enqueue.  Criterion, per stage, for attach and for rate matching: the range of (b) lies wholly below
the range of (a).  The encode line is the same launches on both sides; its share of (b)'s step is what a one-launch mixed encoder
could still buy.  Then, without a threshold, the two mix kernels at a UNIFORM mix (one configuration, the headline transport block x
4096) beside the single-configuration kernels: what the table-driven form costs where it is not needed.

    python tools/bench_mix_tx.py [--out profiles/mix_tx_vs_loop.json] [--reps 30] [--warmup 5]
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
    C = pkg._capi
    lib = pkg.load()
    ps = [p for bg in (1, 2) for Z in ALL_Z for p in [one_block_params(bg, Z)] if p is not None]
    n = len(ps)
    n_tb = [args.n_tb] * n
    plan = pkg.MixTxPlan(ps, n_tb)
    a_off, off, tot = plan.a_off, plan.off, plan.totals()
    codecs = {}
    for p in ps:
        if (p.BG, p.Z_c) not in codecs:
            codecs[(p.BG, p.Z_c)] = pkg.Codec(p.BG, p.Z_c, max_iter=1)
    cs = [codecs[(p.BG, p.Z_c)] for p in ps]
    gen = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(0, 2, (tot["a"],), generator=gen, device="cuda", dtype=torch.uint8)
    arr = {v: {k: torch.zeros(tot[k], dtype=torch.uint8, device="cuda") for k in ("c", "cw", "g")} for v in ("a", "b")}
    vp = ctypes.c_void_p
    ts = [C.tb_params(p) for p in ps]
    x = arr["a"]
    att_args = [(ctypes.byref(ts[i]), vp(a.data_ptr() + a_off[i]), n_tb[i], vp(x["c"].data_ptr() + off[i].c_hat)) for i in range(n)]
    enc_args = [(cs[i]._h, vp(x["c"].data_ptr() + off[i].c_hat), n_tb[i] * ps[i].C, vp(x["cw"].data_ptr() + off[i].cw)) for i in range(n)]
    rm_args = [(ctypes.byref(ts[i]), vp(x["cw"].data_ptr() + off[i].cw), n_tb[i], vp(x["g"].data_ptr() + off[i].g)) for i in range(n)]
    att, enc, rm = lib.nrldpc_crc_attach_dev, lib.nrldpc_encode_dev, lib.nrldpc_rate_match_dev
    stream = torch.cuda.current_stream().cuda_stream
    s = vp(stream)
    hs = (vp * n)(*[c._h for c in cs])
    y = arr["b"]
    h = plan._h
    m_att, m_enc, m_rm = lib.nrldpc_mix_tx_crc_attach_dev, lib.nrldpc_mix_tx_encode_dev, lib.nrldpc_mix_tx_rate_match_dev
    pa, pc, pcw, pg = vp(a.data_ptr()), vp(y["c"].data_ptr()), vp(y["cw"].data_ptr()), vp(y["g"].data_ptr())

    def ev():
        return [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def loop(e):
        t0 = time.perf_counter()
        e[0].record()
        for q in att_args:
            assert att(*q, s) == 0
        e[1].record()
        for q in enc_args:
            assert enc(*q, s) == 0
        e[2].record()
        for q in rm_args:
            assert rm(*q, s) == 0
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    def step(e):
        t0 = time.perf_counter()
        e[0].record()
        assert m_att(h, pa, pc, s) == 0
        e[1].record()
        assert m_enc(h, hs, pc, pcw, s) == 0
        e[2].record()
        assert m_rm(h, pcw, pg, s) == 0
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    rec = {v: {k: [] for k in ("host",) + STAGES + ("total",)} for v in ("a", "b")}
    for it in range(args.warmup + args.reps):
        for name, fn in (("a", loop), ("b", step)):
            e = ev()
            torch.cuda.synchronize()
            host = fn(e)
            torch.cuda.synchronize()
            if it >= args.warmup:
                r = rec[name]
                r["host"].append(host)
                for k, st in enumerate(STAGES):
                    r[st].append(e[k].elapsed_time(e[k + 1]))
                r["total"].append(e[0].elapsed_time(e[3]))
    equal = all(bool((arr["a"][k] == arr["b"][k]).all()) for k in ("c", "cw", "g"))
    assert bool(arr["b"]["g"].any())
    res = {v: {k: stats(rec[v][k]) for k in rec[v]} for v in ("a", "b")}
    below = {st: bool(res["b"][st]["max"] < res["a"][st]["min"]) for st in STAGES}
    out = {
        "mix": {"configurations": n, "bg1": sum(p.BG == 1 for p in ps), "bg2": sum(p.BG == 2 for p in ps), "transport_blocks_each": args.n_tb,
                "transport_blocks": sum(n_tb), "rate": "1/3", "Q_m": 2, "distinct_codecs": len(codecs),
                "bytes": {"a": tot["a"], "c": tot["c"], "cw": tot["cw"], "g": tot["g"]}},
        "reps": args.reps, "warmup": args.warmup, "unit": "ms (device events unless said otherwise)",
        "a_loop_of_single_configuration_stages": dict(res["a"], launches={"attach": n, "encode": n, "rate_match": n}),
        "b_transmit_plan": dict(res["b"], launches={"attach": 1, "encode": n, "rate_match": 1}),
        "outputs_of_a_and_b_equal": equal,
        "b_range_wholly_below_a_range": below,
        "speedup_median": {st: res["a"][st]["median"] / res["b"][st]["median"] for st in STAGES + ("total",)},
        "encode_share_of_b_step": res["b"]["encode"]["median"] / res["b"]["total"]["median"],
        "criterion_attach_and_rate_match_below": bool(equal and below["attach"] and below["rate_match"]),
    }
    plan.close()
    for c in codecs.values():
        c.close()
    return out


def uniform(args):
    """One configuration, the headline transport block (BG1, Z = 384, A = 8424, G = 25272, QPSK) x 4096: the mix kernels beside the
    single-configuration kernels on the same inputs."""
    C = pkg._capi
    p = pkg.NRLDPC(BG=1, A=8424, G=25272, Q_m=2)
    p.validate()
    n = args.uniform_n
    plan = pkg.MixTxPlan([p], [n])
    t = C.tb_params(p)
    ncw = 2 * p.Z_c + p.N
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randint(0, 2, (n, p.A), generator=gen, device="cuda", dtype=torch.uint8)
    cw = torch.randint(0, 2, (n * p.C, ncw), generator=gen, device="cuda", dtype=torch.uint8)
    c = [torch.empty((n * p.C, p.K), dtype=torch.uint8, device="cuda") for _ in range(2)]
    g = [torch.empty((n, p.G), dtype=torch.uint8, device="cuda") for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream
    fns = {
        "attach_single": lambda: pkg.crc_attach_dev(t, a.data_ptr(), n, c[0].data_ptr(), s),
        "attach_mix": lambda: plan.crc_attach(a.data_ptr(), c[1].data_ptr(), stream=s),
        "rate_match_single": lambda: pkg.rate_match_dev(t, cw.data_ptr(), n, g[0].data_ptr(), s),
        "rate_match_mix": lambda: plan.rate_match(cw.data_ptr(), g[1].data_ptr(), stream=s),
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
    equal = bool((c[0] == c[1]).all()) and bool((g[0] == g[1]).all())
    att_bytes, rm_bytes = n * (p.A + p.C * p.K), n * (p.G + p.G)
    out = {"configuration": "BG1, Z = 384, A = 8424, G = 25272, QPSK, C = 1", "transport_blocks": n, "outputs_equal": equal,
           "attach_bytes": att_bytes, "rate_match_bytes_read_once_plus_written": rm_bytes}
    for k, v in ms.items():
        out[k] = stats(v)
        out[k]["TB_s"] = (att_bytes if k.startswith("attach") else rm_bytes) / (np.median(v) * 1e-3) / 1e12
    out["mix_over_single_median"] = {"attach": out["attach_mix"]["median"] / out["attach_single"]["median"],
                                     "rate_match": out["rate_match_mix"]["median"] / out["rate_match_single"]["median"]}
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_tx_vs_loop.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--uniform-n", type=int, default=4096)
    args = ap.parse_args()
    res = {"tool": "tools/bench_mix_tx.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(), "mixed": mixed(args), "uniform": uniform(args)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not res["mixed"]["criterion_attach_and_rate_match_below"]:
        print("CRITERION NOT MET: for attach or rate matching the range of (b) does not lie wholly below the range of (a), or the outputs differ",
              file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

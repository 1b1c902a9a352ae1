"""Mixed receive step, demodulator LLRs to b_hat: the loop the single-configuration stages offer against MixedDecodeChain.step.

The mix is transport-block level and shaped like BASELINE configs[3] (8192 codewords over 102 (BG, Z) buckets): one configuration
per (BG, lifting size) that a parameter object reaches with C = 1, R = 1/3, QPSK, 80 transport blocks each, f32 demodulator LLRs,
f16 LLRs into the decoder, the parity-check stop, Es/N0 as stated in the output.  Two versions, alternated in one process:
  (a) n x nrldpc_rate_recover_dev, nrldpc_decode_multi_dev, n x nrldpc_crc_check_dev, argument blocks prebuilt (what a C caller holds);
  (b) MixedDecodeChain.step: nrldpc_mix_rate_recover_dev, nrldpc_decode_multi_dev, nrldpc_mix_crc_check_dev.
Both write the same packed layout, so their outputs are compared equal in the same run.  Device events around every stage, warm-ups,
median and range; the host time to enqueue; bytes over time of the two mix kernels against 8 TB/s.  Acceptance: the range of (b)
lies wholly below the range of (a).  Then the two mix kernels at a UNIFORM mix (one configuration, the headline transport block x
4096) beside the single-configuration kernels: what the table-driven form costs where it is not needed (a figure, not a gate).

    python tools/bench_mix_chain.py [--out profiles/mix_chain_vs_loop.json] [--reps 30] [--warmup 5] [--esn0 1.0]
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
pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
import torch  # noqa: E402

ALL_Z = sorted(a * 2 ** j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a * 2 ** j <= 384)
HBM_TB_S = 8.0


def one_block_params(bg, Z):
    """A parameter object with C = 1 that lands on (bg, Z) at R = 1/3 with QPSK, or None when there is none."""
    for kb in ((22,) if bg == 1 else (10, 9, 8, 6)):
        B = kb * Z
        for L in (24, 16):
            A = B - L
            if A < 1:
                continue
            try:
                p = pkg.NRLDPC(BG=bg, A=A, G=2 * ((3 * A + 1) // 2), Q_m=2)
                p.validate()
            except (pkg.UnsupportedParameters, pkg.NRLDPCError):
                continue
            if p.BG == bg and p.Z_c == Z and p.C == 1:
                return p
    return None


def stats(x):
    x = np.asarray(x, np.float64)
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max())}


def transmit(ps, n_tb, esn0, seed=7):
    """f32 demodulator LLRs per configuration through the existing transmit stages and the fused channel kernel."""
    rng = np.random.default_rng(seed)
    out, payload = [], []
    for i, (p, n) in enumerate(zip(ps, n_tb)):
        a = torch.from_numpy(rng.integers(0, 2, (n, p.A), dtype=np.uint8)).cuda()
        enc = DC.DeviceEncodeChain(p)
        g = enc.step(a)
        enc.close()
        llr = torch.empty(g.shape, dtype=torch.float32, device="cuda")
        pkg.awgn_llr_dev(g.data_ptr(), g.numel(), p.Q_m, esn0, seed + i, 0, llr.data_ptr())
        out.append(llr)
        payload.append(a)
    torch.cuda.synchronize()
    return out, payload


def mixed(args):
    C = pkg._capi
    lib = pkg.load()
    ps = [p for bg in (1, 2) for Z in ALL_Z for p in [one_block_params(bg, Z)] if p is not None]
    n = len(ps)
    n_tb = [args.n_tb] * n
    llrs, payload = transmit(ps, n_tb, args.esn0)
    chain = DC.MixedDecodeChain(ps, n_tb, iterations=args.iterations)
    plan, off, tot = chain.plan, chain.plan.offsets, chain.plan.totals
    g = chain.pack(llrs, "g")
    # ---- (a): the loop over the single-configuration stages on packed arrays of its own, argument blocks prebuilt
    cw = torch.zeros(tot.cw, dtype=torch.float16, device="cuda")
    c_hat = torch.zeros(tot.c_hat, dtype=torch.uint8, device="cuda")
    iters = torch.zeros(tot.cb, dtype=torch.int32, device="cuda")
    b_hat = torch.zeros(tot.b_hat, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(tot.tb, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p
    ts = [C.tb_params(p) for p in ps]
    rr_args = [(ctypes.byref(ts[i]), vp(g.data_ptr() + 4 * off[i].g), n_tb[i], None, vp(cw.data_ptr() + 2 * off[i].cw), C.LLR_F16) for i in range(n)]
    crc_args = [(ctypes.byref(ts[i]), vp(c_hat.data_ptr() + off[i].c_hat), n_tb[i], vp(b_hat.data_ptr() + off[i].b_hat), vp(ok.data_ptr() + 4 * off[i].tb), None)
                for i in range(n)]
    multi = C.MultiCall(chain.codecs, [cw.data_ptr() + 2 * off[i].cw for i in range(n)], [n_tb[i] * ps[i].C for i in range(n)],
                        [c_hat.data_ptr() + off[i].c_hat for i in range(n)], [iters.data_ptr() + 4 * off[i].cb for i in range(n)])
    rr, crc = lib.nrldpc_rate_recover_dev, lib.nrldpc_crc_check_dev
    stream = torch.cuda.current_stream().cuda_stream
    s = vp(stream)

    def ev():
        return [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def loop(e):
        t0 = time.perf_counter()
        e[0].record()
        for a in rr_args:
            rc = rr(*a, s)
            assert rc == 0, rc
        e[1].record()
        multi(stream)
        e[2].record()
        for a in crc_args:
            rc = crc(*a, s)
            assert rc == 0, rc
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    def step(e):
        # MixedDecodeChain.step with an event between the stages (the three calls step() makes, in its order)
        t0 = time.perf_counter()
        e[0].record()
        plan.rate_recover(g.data_ptr(), None, chain.cw_llr.data_ptr(), in_dtype=C.LLR_F32, out_dtype=C.LLR_F16, stream=stream)
        e[1].record()
        chain._multi(stream)
        e[2].record()
        plan.crc_check(chain.c_hat.data_ptr(), chain.b_hat.data_ptr(), chain.ok.data_ptr(), None, stream=stream)
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    def whole_step():
        t0 = time.perf_counter()
        chain.step(g)
        return (time.perf_counter() - t0) * 1e3

    rec = {"a": {"host": [], "rr": [], "dec": [], "crc": [], "total": []}, "b": {"host": [], "rr": [], "dec": [], "crc": [], "total": []}}
    step_host, step_wall = [], []
    for it in range(args.warmup + args.reps):
        for name, fn in (("a", loop), ("b", step)):
            e = ev()
            torch.cuda.synchronize()
            host = fn(e)
            torch.cuda.synchronize()
            if it >= args.warmup:
                r = rec[name]
                r["host"].append(host)
                r["rr"].append(e[0].elapsed_time(e[1])); r["dec"].append(e[1].elapsed_time(e[2])); r["crc"].append(e[2].elapsed_time(e[3]))
                r["total"].append(e[0].elapsed_time(e[3]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = whole_step()
        torch.cuda.synchronize()
        if it >= args.warmup:
            step_host.append(h); step_wall.append((time.perf_counter() - t0) * 1e3)
    # ---- the outputs of (a) and (b), compared in this run
    equal = bool((b_hat == chain.b_hat).all()) and bool((ok == chain.ok).all()) and bool((iters == chain.iters).all()) and \
        bool((cw.view(torch.int16) == chain.cw_llr.view(torch.int16)).all())
    n_ok = int(chain.ok.sum())
    right = sum(int((v[:, :p.A] == a).all(dim=1).sum()) for v, p, a in zip(chain.views(chain.b_hat, "b_hat"), ps, payload))
    rr_bytes = sum(k * (4 * p.G + 2 * p.C * (2 * p.Z_c + p.N)) for p, k in zip(ps, n_tb))
    crc_bytes = sum(k * (p.C * int(p.K_prime) + p.B + 4) for p, k in zip(ps, n_tb))
    a_t, b_t = stats(rec["a"]["total"]), stats(rec["b"]["total"])
    out = {
        "mix": {"configurations": n, "bg1": sum(p.BG == 1 for p in ps), "bg2": sum(p.BG == 2 for p in ps), "transport_blocks_each": args.n_tb,
                "codewords": sum(n_tb), "rate": "1/3", "Q_m": 2, "EsN0_dB": args.esn0, "iterations": args.iterations, "stop": "parity check",
                "g_tilde": "f32", "decoder_llr": "f16", "transport_blocks_ok": n_ok, "transport_blocks_right": right,
                "lifting_sizes_without_a_one_block_configuration": [[bg, Z] for bg in (1, 2) for Z in ALL_Z if one_block_params(bg, Z) is None]},
        "reps": args.reps, "warmup": args.warmup, "unit": "ms (device events unless said otherwise)",
        "a_loop_of_single_configuration_stages": {"launches_rate_recovery": n, "launches_crc": n, "rate_recovery": stats(rec["a"]["rr"]),
                                                  "decode_multi": stats(rec["a"]["dec"]), "crc": stats(rec["a"]["crc"]), "total": a_t,
                                                  "host_enqueue": stats(rec["a"]["host"])},
        "b_mixed_decode_chain": {"launches_rate_recovery": 1, "launches_crc": 1, "rate_recovery": stats(rec["b"]["rr"]),
                                 "decode_multi": stats(rec["b"]["dec"]), "crc": stats(rec["b"]["crc"]), "total": b_t,
                                 "host_enqueue": stats(rec["b"]["host"]), "step_host_enqueue": stats(step_host), "step_wall_with_sync": stats(step_wall)},
        "mix_kernels": {"rate_recovery_bytes": rr_bytes, "crc_bytes": crc_bytes,
                        "rate_recovery_TB_s": rr_bytes / (np.median(rec["b"]["rr"]) * 1e-3) / 1e12,
                        "crc_TB_s": crc_bytes / (np.median(rec["b"]["crc"]) * 1e-3) / 1e12, "hbm_peak_TB_s": HBM_TB_S,
                        "rate_recovery_fraction_of_peak": rr_bytes / (np.median(rec["b"]["rr"]) * 1e-3) / 1e12 / HBM_TB_S,
                        "crc_fraction_of_peak": crc_bytes / (np.median(rec["b"]["crc"]) * 1e-3) / 1e12 / HBM_TB_S},
        "outputs_of_a_and_b_equal": equal,
        "speedup_total_median": a_t["median"] / b_t["median"],
        "accepted_b_range_wholly_below_a_range": bool(equal and b_t["max"] < a_t["min"]),
    }
    chain.close()
    return out


def uniform(args):
    """One configuration, the headline transport block (BG1, Z = 384, A = 8424, G = 25272, QPSK) x 4096: the mix kernels beside the
    single-configuration kernels on the same arrays."""
    C = pkg._capi
    lib = pkg.load()
    p = pkg.NRLDPC(BG=1, A=8424, G=25272, Q_m=2)
    p.validate()
    n = args.uniform_n
    plan = pkg.MixPlan([p], [n])
    t = C.tb_params(p)
    ncw = 2 * p.Z_c + p.N
    gen = torch.Generator(device="cuda").manual_seed(3)
    g = 4 * torch.randn((n, p.G), generator=gen, device="cuda", dtype=torch.float32)
    a = torch.randint(0, 2, (n, p.A), generator=gen, device="cuda", dtype=torch.uint8)
    c = torch.empty((n * p.C, p.K), dtype=torch.uint8, device="cuda")
    pkg.crc_attach_dev(p, a.data_ptr(), n, c.data_ptr())
    cw = [torch.empty((n * p.C, ncw), dtype=torch.float16, device="cuda") for _ in range(2)]
    b_hat = [torch.empty((n, p.B), dtype=torch.uint8, device="cuda") for _ in range(2)]
    ok = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream
    fns = {
        "rate_recovery_single": lambda: pkg.rate_recover_dev(t, g.data_ptr(), n, None, cw[0].data_ptr(), out_dtype=C.LLR_F16, stream=s),
        "rate_recovery_mix": lambda: plan.rate_recover(g.data_ptr(), None, cw[1].data_ptr(), in_dtype=C.LLR_F32, out_dtype=C.LLR_F16, stream=s),
        "crc_single": lambda: pkg.crc_check_dev(t, c.data_ptr(), n, b_hat[0].data_ptr(), ok[0].data_ptr(), None, s),
        "crc_mix": lambda: plan.crc_check(c.data_ptr(), b_hat[1].data_ptr(), ok[1].data_ptr(), None, stream=s),
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
    equal = bool((cw[0].view(torch.int16) == cw[1].view(torch.int16)).all()) and bool((b_hat[0] == b_hat[1]).all()) and bool((ok[0] == ok[1]).all())
    assert bool(ok[1].all())
    rr_bytes = n * (4 * p.G + 2 * p.C * ncw)
    crc_bytes = n * (p.C * int(p.K_prime) + p.B + 4)
    out = {"configuration": "BG1, Z = 384, A = 8424, G = 25272, QPSK, C = 1", "transport_blocks": n, "g_tilde": "f32", "decoder_llr": "f16",
           "outputs_equal": equal, "rate_recovery_bytes": rr_bytes, "crc_bytes": crc_bytes}
    for k, v in ms.items():
        out[k] = stats(v)
        out[k]["TB_s"] = (rr_bytes if k.startswith("rate") else crc_bytes) / (np.median(v) * 1e-3) / 1e12
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_chain_vs_loop.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--esn0", type=float, default=1.0)
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--uniform-n", type=int, default=4096)
    args = ap.parse_args()
    res = {"tool": "tools/bench_mix_chain.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(), "mixed": mixed(args), "uniform": uniform(args)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not res["mixed"]["accepted_b_range_wholly_below_a_range"]:
        print("NOT ACCEPTED: the range of (b) does not lie wholly below the range of (a), or the outputs differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

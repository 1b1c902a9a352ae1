#!/usr/bin/env python3
"""Flooding sum-product (NRLDPC_ALG_SUM_PRODUCT) kernel times: the headline shape (BG1 Z = 384 R = 1/3, 4096 codewords) at 25 fixed
sweeps and with the parity stop at -0.5 dB, cfg1 (BG2 Z = 20, 12 rows, 10 sweeps, parity stop), and the 16-thread CPU oracle
(oracle/orc_decode_bp_flood, double) on a sample of the same LLRs.  GPU times are HIP event pairs around the kernel
(nrldpc_set_timing), device-resident inputs, two warm-up launches, median of the next seven.  Prints one JSON line; --out FILE
also writes it, indented, to FILE (profiles/r07_bench_sum_product.json is such a file)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as orc  # noqa: E402

pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
DIMS = {1: (46, 68, 22), 2: (42, 52, 10)}
WARM, REPS = 2, 7


def llrs(bg, Z, B, esn0, E, seed):
    rows, cols, kb = DIMS[bg]
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (256, kb * Z), dtype=np.uint8)
    cw = torch.from_numpy(np.tile(orc.encode(bg, Z, info), (B // 256, 1))).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mu = 2.0 * 10.0 ** (esn0 / 10.0)
    x = (1.0 - 2.0 * cw.float()) * mu + (2.0 * mu) ** 0.5 * torch.randn(cw.shape, generator=g, device="cuda")
    x[:, : 2 * Z] = 0
    x[:, 2 * Z + E:] = 0
    return x.contiguous(), torch.from_numpy(np.tile(info, (B // 256, 1))).cuda()


def gpu_point(name, bg, Z, nl, cap, early, esn0, E, B, seed):
    K = DIMS[bg][2] * Z
    x, truth = llrs(bg, Z, B, esn0, E, seed)
    c = pkg.Codec(bg, Z, max_iter=cap, n_layers=nl, early_term=early, llr_dtype=np.float32, algorithm="sum-product")
    hard = torch.empty((B, K), device="cuda", dtype=torch.uint8)
    it = torch.empty(B, device="cuda", dtype=torch.int32)
    c.set_timing(True)
    ms = []
    for _ in range(WARM + REPS):
        c.decode_dev(x.data_ptr(), B, hard.data_ptr(), it.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        ms.append(c.last_kernel_ms())
    c.close()
    t = sorted(ms[WARM:])
    med = t[len(t) // 2]
    rec = {"point": name, "bg": bg, "Z": Z, "n_layers": nl or DIMS[bg][0], "sweeps_cap": cap, "parity_stop": bool(early),
           "EsN0_dB": esn0, "codewords": B, "kernel_ms_median": med, "kernel_ms_min": t[0], "kernel_ms_max": t[-1],
           "info_Gbit_s": K * B / (med * 1e-3) / 1e9, "mean_sweeps": float(it.float().mean()),
           "block_errors": int((hard != truth).any(1).sum())}
    return rec, x


def cpu_oracle(x, bg, Z, nl, cap, n):
    sample = x[:n].double().cpu().numpy()
    t0 = time.perf_counter()
    _, it = orc.decode_bp_flood(bg, Z, sample, cap, n_layers=nl, nthreads=16)
    dt = time.perf_counter() - t0
    K = DIMS[bg][2] * Z
    return {"threads": 16, "codewords": n, "seconds": dt, "info_Gbit_s": K * n / dt / 1e9, "mean_sweeps": float(it.mean())}


ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--out", metavar="FILE", default=None, help="also write the result, indented, to FILE")
args = ap.parse_args()
out = {"kernel": "nrldpc_bp_flood_kernel", "timing": "HIP event pairs, %d warm-up + median of %d" % (WARM, REPS)}
r, _ = gpu_point("headline BG1 Z=384 R=1/3, 25 fixed sweeps", 1, 384, 0, 25, False, -0.5, 25344, 4096, 11)
out["headline_25_fixed"] = r
print(json.dumps(r), flush=True)
r, x = gpu_point("headline BG1 Z=384 R=1/3, parity stop, cap 25", 1, 384, 0, 25, True, -0.5, 25344, 4096, 12)
out["headline_parity_stop"] = r
print(json.dumps(r), flush=True)
out["headline_parity_stop_cpu_oracle"] = cpu_oracle(x, 1, 384, 0, 25, 64)
del x
r, x = gpu_point("cfg1 BG2 Z=20 (12 rows), parity stop, cap 10", 2, 20, 12, 10, True, 1.0, 300, 65536, 13)
out["cfg1_parity_stop"] = r
out["cfg1_cpu_oracle"] = cpu_oracle(x, 2, 20, 12, 10, 4096)
out["speedup_headline_stop_over_cpu_oracle"] = out["headline_parity_stop"]["info_Gbit_s"] / out["headline_parity_stop_cpu_oracle"]["info_Gbit_s"]
out["speedup_cfg1_over_cpu_oracle"] = out["cfg1_parity_stop"]["info_Gbit_s"] / out["cfg1_cpu_oracle"]["info_Gbit_s"]
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))

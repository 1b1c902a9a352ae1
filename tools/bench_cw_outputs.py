#!/usr/bin/env python3
"""What the whole-codeword / final-parity-check outputs cost: nrldpc_decode_cw_dev against nrldpc_decode_dev at the headline shape
(BG1 Z = 384 R = 1/3, 4096 codewords, 25 fixed iterations), for min-sum (f16 LLRs, as bench.py's headline) and for sum-product
(f32 LLRs).  Each call sits between a HIP event pair on its stream (so the min-sum figure covers the soft-output launch and the
finish kernel of every chunk), device-resident inputs, two warm-up calls, median of the next seven.  Prints one JSON line; --out FILE
also writes it, indented, to FILE.  DESIGN.md section 4.11 quotes it."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle as orc  # noqa: E402

pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
BG, Z, B, ITERS, ESN0, E = 1, 384, 4096, 25, -0.5, 25344
ROWS, COLS, KB = 46, 68, 22
WARM, REPS = 2, 7


def llrs(dtype, seed):
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (256, KB * Z), dtype=np.uint8)
    cw = torch.from_numpy(np.tile(orc.encode(BG, Z, info), (B // 256, 1))).cuda()
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mu = 2.0 * 10.0 ** (ESN0 / 10.0)
    x = (1.0 - 2.0 * cw.float()) * mu + (2.0 * mu) ** 0.5 * torch.randn(cw.shape, generator=g, device="cuda")
    x[:, : 2 * Z] = 0
    x[:, 2 * Z + E:] = 0
    return x.to(dtype).contiguous()


def timed(fn):
    ms = []
    for _ in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = sorted(ms[WARM:])
    return {"ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1]}


def point(algorithm, np_dt, torch_dt, seed):
    x = llrs(torch_dt, seed)
    c = pkg.Codec(BG, Z, max_iter=ITERS, early_term=False, llr_dtype=np_dt, algorithm=algorithm)
    hard = torch.empty((B, KB * Z), device="cuda", dtype=torch.uint8)
    it = torch.empty(B, device="cuda", dtype=torch.int32)
    cw = torch.empty((B, (COLS * Z + 7) // 8), device="cuda", dtype=torch.uint8)
    un = torch.empty(B, device="cuda", dtype=torch.int32)
    ck = torch.empty((B, (ROWS * Z + 7) // 8), device="cuda", dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream
    plain = timed(lambda: c.decode_dev(x.data_ptr(), B, hard.data_ptr(), it.data_ptr(), None, st))
    h0 = hard.clone()
    full = timed(lambda: c.decode_cw_dev(x.data_ptr(), B, hard.data_ptr(), it.data_ptr(), cw.data_ptr(), un.data_ptr(), ck.data_ptr(), st))
    assert torch.equal(hard, h0)
    c.close()
    return {"algorithm": algorithm, "llr_dtype": str(np.dtype(np_dt)), "nrldpc_decode_dev": plain, "nrldpc_decode_cw_dev": full,
            "ratio": full["ms_median"] / plain["ms_median"], "extra_ms": full["ms_median"] - plain["ms_median"],
            "converged_codewords": int((un == 0).sum())}


ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--out", metavar="FILE", default=None, help="also write the result, indented, to FILE")
args = ap.parse_args()
out = {"shape": "BG1 Z=384 R=1/3, %d codewords, %d fixed iterations, Es/N0 %.1f dB" % (B, ITERS, ESN0),
       "timing": "HIP event pair around each call, %d warm-up + median of %d" % (WARM, REPS),
       "min_sum": point("min-sum", np.float16, torch.float16, 21), "sum_product": point("sum-product", np.float32, torch.float32, 22)}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
print(json.dumps(out))

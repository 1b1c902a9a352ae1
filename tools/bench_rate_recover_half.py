#!/usr/bin/env python3
"""Device time of rate recovery on one MI355X for the element types nrldpc_rate_recover_ex_dev adds, at the stage size
tools/bench_chain.py uses (4096 headline transport blocks: BG1, Z = 384, G = 25272, QPSK) plus one 64QAM point and one repetition
point, with and without the HARQ soft buffer.  Per point four combinations of (demodulator LLRs, buffer, codeword LLRs):
(f32, f32, f16) -- nrldpc_rate_recover_dev, today's path, measured in the same build -- and (f16, f32, f16), (f32, f16, f16),
(f16, f16, f16) through the new entry point; beside each a plain device-to-device copy of the same traffic.  HIP event pairs on the
launch stream around 8 launches queued back to back, median of 7 after 2 warm-ups (as tools/bench_modem.py).
Prints one JSON line per measurement; --out FILE also writes them as one JSON list.

Algorithmic bytes per transport block: G x input size + C x (2Z + N) x output size + with the buffer 2 x C x P x buffer size
(P = non-filler positions of the circular buffer: read and written once each).

NRLDPC_RR_SCATTER=0 / 1 forces the gather / the input-driven form (read once per process: one run each); the value is recorded.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
capi = importlib.import_module("ldpc-3gpp-matlab_amd._capi")
N_TB = 4096
WARMUP, REPS, INNER = 2, 7, 8
POINTS = [("headline QPSK", dict(BG=1, A=8424, G=25272, Q_m=2)),
          ("64QAM", dict(BG=1, A=8424, G=25272, Q_m=6)),
          ("repetition (E = 8 N_cb) QPSK", dict(BG=1, A=1000, G=25272, Q_m=2))]
COMBOS = [("f32", "f32", "f16"), ("f16", "f32", "f16"), ("f32", "f16", "f16"), ("f16", "f16", "f16")]
TORCH = {"f32": torch.float32, "f16": torch.float16}
CODE = {"f32": capi.LLR_F32, "f16": capi.LLR_F16}
SIZE = {"f32": 4, "f16": 2}


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1) / INNER)
    return float(np.median(ms))


_copy_ms = {}


def copy_ms(nbytes):
    """A device-to-device copy with `nbytes` of traffic (half read, half written), timed the same way."""
    half = int(nbytes) // 2 // 16 * 16
    if half not in _copy_ms:
        src = torch.randint(0, 255, (half,), device="cuda", dtype=torch.uint8)
        dst = torch.empty_like(src)
        _copy_ms[half] = timed(lambda: dst.copy_(src))
    return _copy_ms[half]


def main(out=None):
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    res = []
    for name, kw in POINTS:
        p = pkg.NRLDPC(**kw)
        p.validate()
        t = capi.tb_params(p)
        ncwz = 2 * p.Z_c + p.N
        lo, hi = max(int(p.K_prime) - 2 * p.Z_c, 0), min(p.K - 2 * p.Z_c, p.N_cb)
        P = p.N_cb - max(hi - lo, 0)
        g32 = 4.0 * torch.randn((N_TB, p.G), generator=gen, device="cuda", dtype=torch.float32)
        g = {"f32": g32, "f16": g32.half()}
        cw = torch.empty((N_TB * p.C, ncwz), device="cuda", dtype=torch.float16)
        for with_buffer in (False, True):
            for i, h, o in COMBOS:
                if not with_buffer and h == "f16":
                    continue  # without a buffer its type is not read
                harq = torch.zeros((N_TB, p.C, p.N_cb), device="cuda", dtype=TORCH[h]) if with_buffer else None
                fn = lambda: capi.rate_recover_dev(t, g[i].data_ptr(), N_TB, harq.data_ptr() if with_buffer else None, cw.data_ptr(),  # noqa: E731
                                                   CODE[o], s, in_dtype=CODE[i], harq_dtype=CODE[h])
                ms = timed(fn)
                nbytes = N_TB * (p.G * SIZE[i] + p.C * ncwz * SIZE[o] + (2 * p.C * P * SIZE[h] if with_buffer else 0))
                c = copy_ms(nbytes)
                r = dict(point=name, kw=kw, n_tb=N_TB, Z=p.Z_c, C=p.C, N_cb=p.N_cb, repeats=bool(max(p.E_r) > P), buffer=with_buffer,
                         input=i, harq=h if with_buffer else None, output=o,
                         entry="nrldpc_rate_recover_dev" if (i, h) == ("f32", "f32") or (i == "f32" and not with_buffer) else "nrldpc_rate_recover_ex_dev",
                         ms=ms, algorithmic_bytes=int(nbytes), GB_s=nbytes / ms / 1e6, copy_ms=c, frac_of_copy=c / ms,
                         NRLDPC_RR_SCATTER=os.environ.get("NRLDPC_RR_SCATTER"))
                print(json.dumps(r), flush=True)
                res.append(r)
                del harq
        del g32, g, cw
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the measurements to this JSON file")
    main(ap.parse_args().out)

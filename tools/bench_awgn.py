#!/usr/bin/env python3
"""Device time of the stand-alone AWGN stage (nrldpc_awgn_dev) on one MI355X at the stage size tools/bench_chain.py and
tools/bench_modem.py use (4096 headline transport blocks: 4096 x 25272 rate-matched bits), for the symbol counts of Q_m = 1, 2, 4, 6, 8,
with a scalar variance and with a per-symbol variance, each beside a plain device-to-device copy of the same traffic; and the
three-stage leg (modulate + awgn + exact f32 demodulate) next to the fused kernel nrldpc_awgn_llr_dev.  HIP event pairs on the launch
stream, median of 7 after 2 warm-ups; an event pair spans 8 launches (of the leg: 8 x 3) queued back to back, so that the host's launch
path hides behind the previous kernel.  Prints one JSON line per measurement; --out FILE also writes them as one JSON list.

Algorithmic bytes:
  awgn                      8 n_sym in + 8 n_sym out (+ 4 n_sym with a per-symbol variance)
  modulate + awgn + demod   (n_bits + 8 n_sym) + 16 n_sym + (8 n_sym + 4 n_bits)
  awgn_llr (fused)          n_bits in + 4 n_bits out
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
capi = importlib.import_module("ldpc-3gpp-matlab_amd._capi")
N_TB, G = 4096, 25272
WARMUP, REPS, INNER = 2, 7, 8


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
    n_bits = N_TB * G
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    g = torch.randint(0, 2, (n_bits,), generator=gen, device="cuda", dtype=torch.uint8)
    out32 = torch.empty(n_bits, device="cuda", dtype=torch.float32)
    res = []

    def rec(kernel, Q_m, ms, nbytes, **kw):
        c = copy_ms(nbytes)
        r = dict(kernel=kernel, Q_m=Q_m, n_sym=n_bits // Q_m, ms=ms, algorithmic_bytes=int(nbytes), GB_s=nbytes / ms / 1e6,
                 copy_ms=c, frac_of_copy=c / ms, **kw)
        print(json.dumps(r), flush=True)
        res.append(r)

    for Q_m, esn0 in ((1, -2.0), (2, 0.0), (4, 8.0), (6, 14.0), (8, 20.0)):
        n_sym = n_bits // Q_m
        N0 = 10.0 ** (-esn0 / 10.0)
        tx = torch.empty(n_sym, device="cuda", dtype=torch.complex64)
        rx = torch.empty(n_sym, device="cuda", dtype=torch.complex64)
        var = torch.full((n_sym,), N0, device="cuda", dtype=torch.float32)
        capi.modulate_dev(g.data_ptr(), n_bits, Q_m, tx.data_ptr(), s)
        rec("awgn, scalar variance", Q_m,
            timed(lambda: capi.awgn_dev(tx.data_ptr(), n_sym, rx.data_ptr(), variance=N0, seed=11, stream=s)), 16 * n_sym, EsN0_dB=esn0)
        rec("awgn, per-symbol variance", Q_m,
            timed(lambda: capi.awgn_dev(tx.data_ptr(), n_sym, rx.data_ptr(), d_variance=var.data_ptr(), seed=11, stream=s)), 20 * n_sym,
            EsN0_dB=esn0)

        def leg():
            capi.modulate_dev(g.data_ptr(), n_bits, Q_m, tx.data_ptr(), s)
            capi.awgn_dev(tx.data_ptr(), n_sym, tx.data_ptr(), variance=N0, seed=11, stream=s)
            capi.demodulate_dev(tx.data_ptr(), n_sym, Q_m, out32.data_ptr(), method="llr", variance=N0, stream=s)

        rec("modulate + awgn (in place) + demodulate llr f32", Q_m, timed(leg), 5 * n_bits + 32 * n_sym, EsN0_dB=esn0)
        rec("awgn_llr (fused: modulate + AWGN + exact LLR)", Q_m,
            timed(lambda: capi.awgn_llr_dev(g.data_ptr(), n_bits, Q_m, esn0, 11, 0, out32.data_ptr(), s)), 5 * n_bits, EsN0_dB=esn0)
        del tx, rx, var
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="also write the measurements to this JSON file")
    main(ap.parse_args().out)

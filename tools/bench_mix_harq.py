"""Mixed receive step WITH HARQ state, demodulator LLRs to b_hat: the loop the single-configuration stages offer against
MixedDecodeChain(I_HARQ=1).step.

The mix is that of tools/bench_mix_chain.py (one configuration per (BG, lifting size) reachable with C = 1, R = 1/3, QPSK; 80 transport
blocks each; f32 demodulator LLRs, f16 LLRs into the decoder, the parity-check stop) with a soft buffer (f32 or f16).  The state every
repetition starts from is what one transmission at rv_id = 0 leaves (restored from a snapshot before every repetition, outside the
timed region, for both versions); the timed step is the retransmission at rv_id = 2.  Two scenarios:
  retransmission   no transport block is new;
  half_new         the first half of every configuration's transport blocks starts a new HARQ process.
Two versions, alternated in one process:
  (a) per configuration: [a fill of the new blocks' buffer rows,] nrldpc_rate_recover_ex_dev with the buffer; nrldpc_decode_multi_dev;
      per configuration: [a fill of the new blocks' cb_pass rows, nrldpc_crc_check_harq_dev(keep_b_hat = 0) on them,]
      nrldpc_crc_check_harq_dev(keep_b_hat = 1) on the rest -- argument blocks prebuilt (what a C caller holds), fills = tensor.zero_();
  (b) nrldpc_mix_rate_recover_harq_dev, nrldpc_decode_multi_dev, nrldpc_mix_crc_check_harq_dev with the flag arrays.
Both work on the same packed layout, so their outputs (buffer, codeword LLRs, iterations, b_hat, ok, cb_pass) are compared equal in
the same run.  Device events around every stage, warm-ups, median and range; the host time to enqueue; and the soft buffer's bytes
per step, flagged against unflagged (computed from the geometry: a continuing block reads and writes every non-filler position of its
circular buffer, a new one only writes).  No acceptance ratio is fixed: the file states what was measured.

    python tools/bench_mix_harq.py [--out profiles/mix_harq_vs_loop.json] [--reps 30] [--warmup 5] [--esn0 -1.0] [--harq-dtype f16]
"""
import argparse
import copy
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_mix_chain as B  # noqa: E402  (the mix, transmit(), stats())

pkg, DC, torch, ROOT = B.pkg, B.DC, B.torch, B.ROOT


def with_rv(p, rv):
    q = copy.copy(p)
    q.rv_id = rv
    return q


def body_positions(p):
    """non-filler positions inside the circular buffer of one code block"""
    lo, hi = max(int(p.K_prime) - 2 * p.Z_c, 0), p.K - 2 * p.Z_c
    return p.N_cb - max(0, min(hi, p.N_cb) - lo)


def scenario(args, name, ps, n_tb, chain, llr0, llr2, hsize):
    C = pkg._capi
    lib = pkg.load()
    n = len(ps)
    vp = ctypes.c_void_p
    plan0, off, tot = chain.plan, chain.plan.offsets, chain.plan.totals
    hdt = torch.float16 if hsize == 2 else torch.float32
    hcode = C.LLR_F16 if hsize == 2 else C.LLR_F32
    # ---- the state before the timed step: one transmission at rv_id = 0
    chain.reset()
    chain.step(chain.pack(llr0, "g"), rv_id=0)
    torch.cuda.synchronize()
    snap = {k: getattr(chain, k).clone() for k in ("harq", "b_hat", "cb_pass")}
    first_ok = int(chain.ok.sum())
    g = chain.pack(llr2, "g")
    plan2, _ = chain._plan_for(2)
    chain.step(g, rv_id=2)  # (sets the codecs' layer counts for this redundancy version: both versions share the codecs)
    k_new = [k // 2 if name == "half_new" else 0 for k in n_tb]
    new = chain.pack([torch.tensor([1] * kn + [0] * (k - kn), dtype=torch.uint8, device="cuda") for k, kn in zip(n_tb, k_new)], "tb")
    d_new = new.data_ptr() if name == "half_new" else None
    # ---- (a): packed arrays of its own, argument blocks prebuilt
    harq = torch.zeros(tot.harq, dtype=hdt, device="cuda")
    cw = torch.zeros(tot.cw, dtype=torch.float16, device="cuda")
    c_hat = torch.zeros(tot.c_hat, dtype=torch.uint8, device="cuda")
    iters = torch.zeros(tot.cb, dtype=torch.int32, device="cuda")
    b_hat = torch.zeros(tot.b_hat, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(tot.tb, dtype=torch.int32, device="cuda")
    cb_pass = torch.zeros(tot.cb, dtype=torch.int32, device="cuda")
    ts = [C.tb_params(with_rv(p, 2)) for p in ps]
    rr_args = [(ctypes.byref(ts[i]), vp(g.data_ptr() + 4 * off[i].g), C.LLR_F32, n_tb[i], vp(harq.data_ptr() + hsize * off[i].harq), hcode,
                vp(cw.data_ptr() + 2 * off[i].cw), C.LLR_F16) for i in range(n)]
    harq_new = [harq[off[i].harq: off[i].harq + k_new[i] * ps[i].C * ps[i].N_cb] for i in range(n) if k_new[i]]
    pass_new = [cb_pass[off[i].cb: off[i].cb + k_new[i] * ps[i].C] for i in range(n) if k_new[i]]

    def crc_block(i, first, count, keep):
        p = ps[i]
        return (ctypes.byref(ts[i]), vp(c_hat.data_ptr() + off[i].c_hat + first * p.C * p.K), count, vp(b_hat.data_ptr() + off[i].b_hat + first * p.B),
                vp(ok.data_ptr() + 4 * (off[i].tb + first)), vp(cb_pass.data_ptr() + 4 * (off[i].cb + first * p.C)), None, keep)

    crc_args = [crc_block(i, 0, k_new[i], 0) for i in range(n) if k_new[i]] + [crc_block(i, k_new[i], n_tb[i] - k_new[i], 1) for i in range(n) if n_tb[i] > k_new[i]]
    multi = C.MultiCall(chain.codecs, [cw.data_ptr() + 2 * off[i].cw for i in range(n)], [n_tb[i] * ps[i].C for i in range(n)],
                        [c_hat.data_ptr() + off[i].c_hat for i in range(n)], [iters.data_ptr() + 4 * off[i].cb for i in range(n)])
    rr, crc = lib.nrldpc_rate_recover_ex_dev, lib.nrldpc_crc_check_harq_dev
    stream = torch.cuda.current_stream().cuda_stream
    s = vp(stream)

    def restore():
        harq.copy_(snap["harq"]); b_hat.copy_(snap["b_hat"]); cb_pass.copy_(snap["cb_pass"])
        chain.harq.copy_(snap["harq"]); chain.b_hat.copy_(snap["b_hat"]); chain.cb_pass.copy_(snap["cb_pass"])

    def loop(e):
        t0 = time.perf_counter()
        e[0].record()
        for v in harq_new:
            v.zero_()
        for a in rr_args:
            rc = rr(*a, s)
            assert rc == 0, rc
        e[1].record()
        multi(stream)
        e[2].record()
        for v in pass_new:
            v.zero_()
        for a in crc_args:
            rc = crc(*a, s)
            assert rc == 0, rc
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    def step(e):
        # MixedDecodeChain._step_harq with an event between the stages (the three calls it makes, in its order)
        t0 = time.perf_counter()
        e[0].record()
        plan2.rate_recover_harq(g.data_ptr(), chain.harq.data_ptr(), chain.cw_llr.data_ptr(), d_new, in_dtype=C.LLR_F32, harq_dtype=hcode,
                                out_dtype=C.LLR_F16, stream=stream)
        e[1].record()
        chain._multi(stream)
        e[2].record()
        plan2.crc_check_harq(chain.c_hat.data_ptr(), chain.b_hat.data_ptr(), chain.ok.data_ptr(), chain.cb_pass.data_ptr(), chain.cbgti.data_ptr(),
                             d_new, stream=stream)
        e[3].record()
        return (time.perf_counter() - t0) * 1e3

    keys = ("host", "rr", "dec", "crc", "total")
    rec = {"a": {k: [] for k in keys}, "b": {k: [] for k in keys}}
    for it in range(args.warmup + args.reps):
        for nm, fn in (("a", loop), ("b", step)):
            restore()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            host = fn(e)
            torch.cuda.synchronize()
            if it >= args.warmup:
                r = rec[nm]
                r["host"].append(host)
                r["rr"].append(e[0].elapsed_time(e[1])); r["dec"].append(e[1].elapsed_time(e[2])); r["crc"].append(e[2].elapsed_time(e[3]))
                r["total"].append(e[0].elapsed_time(e[3]))
    # ---- the outputs of (a) and (b): each is one step from the snapshot
    restore()
    loop([torch.cuda.Event(enable_timing=True) for _ in range(4)])
    step([torch.cuda.Event(enable_timing=True) for _ in range(4)])
    torch.cuda.synchronize()
    hv = torch.int16 if hsize == 2 else torch.int32
    equal = {"buffer": bool((harq.view(hv) == chain.harq.view(hv)).all()), "codeword_llrs": bool((cw.view(torch.int16) == chain.cw_llr.view(torch.int16)).all()),
             "iters": bool((iters == chain.iters).all()), "b_hat": bool((b_hat == chain.b_hat).all()), "ok": bool((ok == chain.ok).all()),
             "cb_pass": bool((cb_pass == chain.cb_pass).all())}
    a_t, b_t = B.stats(rec["a"]["total"]), B.stats(rec["b"]["total"])
    cont = sum((k - kn) * p.C * body_positions(p) for p, k, kn in zip(ps, n_tb, k_new))
    fresh = sum(kn * p.C * body_positions(p) for p, kn in zip(ps, k_new))
    return {
        "new_transport_blocks": sum(k_new), "transport_blocks": sum(n_tb), "ok_after_first_transmission": first_ok, "ok_after_this_step": int(chain.ok.sum()),
        "a_loop_of_single_configuration_stages": {"fills": len(harq_new) + len(pass_new), "launches_rate_recovery": n, "launches_crc": len(crc_args),
                                                  "rate_recovery_with_fills": B.stats(rec["a"]["rr"]), "decode_multi": B.stats(rec["a"]["dec"]),
                                                  "crc_with_fills": B.stats(rec["a"]["crc"]), "total": a_t, "host_enqueue": B.stats(rec["a"]["host"])},
        "b_mixed_decode_chain": {"fills": 0, "launches_rate_recovery": 1, "launches_crc": 1, "rate_recovery": B.stats(rec["b"]["rr"]),
                                 "decode_multi": B.stats(rec["b"]["dec"]), "crc": B.stats(rec["b"]["crc"]), "total": b_t, "host_enqueue": B.stats(rec["b"]["host"])},
        "soft_buffer_bytes_per_step": {"continuing_blocks_read_and_write": 2 * hsize * cont, "new_blocks_write_only": hsize * fresh,
                                       "new_blocks_in_the_loop_fill_read_write": 3 * hsize * fresh, "how": "computed from the geometry, not measured"},
        "outputs_of_a_and_b_equal": equal,
        "speedup_total_median": a_t["median"] / b_t["median"],
        "b_range_wholly_below_a_range": bool(all(equal.values()) and b_t["max"] < a_t["min"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_harq_vs_loop.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--esn0", type=float, default=-1.0)
    ap.add_argument("--n-tb", type=int, default=80)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--harq-dtype", choices=("f32", "f16"), default="f16")
    args = ap.parse_args()
    ps = [p for bg in (1, 2) for Z in B.ALL_Z for p in [B.one_block_params(bg, Z)] if p is not None]
    n_tb = [args.n_tb] * len(ps)
    hsize = 2 if args.harq_dtype == "f16" else 4
    llr0, _ = B.transmit([with_rv(p, 0) for p in ps], n_tb, args.esn0, seed=7)
    llr2, _ = B.transmit([with_rv(p, 2) for p in ps], n_tb, args.esn0, seed=7)  # (the same payloads: transmit() draws them from its seed)
    chain = DC.MixedDecodeChain(ps, n_tb, iterations=args.iterations, I_HARQ=1, harq_dtype=np.float16 if hsize == 2 else np.float32)
    res = {"tool": "tools/bench_mix_harq.py", "device": torch.cuda.get_device_name(0), "nrldpc_build_id": pkg.load().nrldpc_build_id().decode(),
           "nrldpc_kernel_id": pkg.load().nrldpc_kernel_id().decode(),
           "mix": {"configurations": len(ps), "transport_blocks_each": args.n_tb, "rate": "1/3", "Q_m": 2, "EsN0_dB": args.esn0, "iterations": args.iterations,
                   "stop": "parity check", "g_tilde": "f32", "decoder_llr": "f16", "soft_buffer": args.harq_dtype, "state": "one transmission at rv_id 0",
                   "timed_step": "rv_id 2"},
           "reps": args.reps, "warmup": args.warmup, "unit": "ms (device events unless said otherwise)"}
    try:
        for name in ("retransmission", "half_new"):
            res[name] = scenario(args, name, ps, n_tb, chain, llr0, llr2, hsize)
    finally:
        chain.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    if not all(all(res[k]["outputs_of_a_and_b_equal"].values()) for k in ("retransmission", "half_new")):
        print("the outputs of (a) and (b) differ", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

"""Flooding sum-product (NRLDPC_ALG_SUM_PRODUCT) on the GPU against its definition, oracle/orc_decode_bp_flood_app.

The reference's comm.LDPCDecoder (NRLDPCDecoder.m:120) is flooding sum-product with the parity-check stop; the oracle restates it
in double.  These tests hold the product's fp32 kernel to it: the soft output sweep by sweep within a stated tolerance, the parity
stop at every lifting size, the committed sum-product BLER outcomes, the harness at the reference's defaults, every entry point,
determinism, and the refusals.  With NRLDPC_RECORD_DIR set, the measured numbers go to sum_product.json in that directory."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import ALL_Z, BG_DIMS, awgn_llr, rule_kw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3  # |APP_gpu - APP_ref| <= TOL * max(1, |APP_ref|) (include/nrldpc.h)


def _threads():
    n = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return n


def _record(key, value):
    """Adds `value` under `key` to sum_product.json in $NRLDPC_RECORD_DIR (nothing is written when it is unset)."""
    out = os.environ.get("NRLDPC_RECORD_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        p = os.path.join(out, "sum_product.json")
        allr = json.load(open(p)) if os.path.exists(p) else {}
        allr[key] = value
        json.dump(allr, open(p, "w"), indent=1)
    except OSError:
        pass


def _llrs(orc, rng, bg, Z, B, snr, nl=0, n_fill=None, dtype=np.float32):
    """QPSK/AWGN LLRs of B random codewords: first 2Z columns punctured, the last info bits fillers (+inf, bit 0), the extension
    columns of rows >= nl (when given) untransmitted (0)."""
    rows, cols, kb = BG_DIMS[bg]
    K = kb * Z
    info = rng.integers(0, 2, (B, K), dtype=np.uint8)
    nf = (Z // 4 if n_fill is None else n_fill)
    if nf:
        info[:, K - nf:] = 0
    cw = orc.encode(bg, Z, info)
    llr = awgn_llr(rng, cw, snr, np.float64, Z)
    if nf:
        llr[:, K - nf:K] = np.inf
    if nl:
        llr[:, (kb + nl) * Z:] = 0
    return info, cw, llr.astype(dtype)


def _snr_waterfall(Z):
    """Es/N0 near the BLER waterfall of a rate-1/3 code of this lifting size at a few sweeps: +1.5 dB at Z = 2, -1 dB at 384."""
    return 1.5 - 2.5 * np.log(Z / 2.0) / np.log(192.0)


# ---- 1. soft output, sweep by sweep -------------------------------------------------------------------------------------
def test_per_sweep_soft_output_within_the_stated_tolerance(pkg, orc):
    rng = np.random.default_rng(1234)
    zs = [2, 3, 7, 15, 20, 52, 104, 208, 384] + [int(z) for z in rng.choice([z for z in ALL_Z if z not in (2, 3, 7, 15, 20, 52, 104, 208, 384)], 4, replace=False)]
    worst = {"abs_err_max": 0.0, "rel_err_max": 0.0, "compared_entries": 0, "cases": 0}
    for bg in (1, 2):
        rows, cols, kb = BG_DIMS[bg]
        for Z in zs:
            B = 4 if Z >= 200 else 8 if Z >= 64 else 24
            for nl in (0, 4, int(rng.integers(5, rows))):
                for it in (1, 2, 3):
                    codec = pkg.Codec(bg, Z, max_iter=it, n_layers=nl, early_term=False, llr_dtype=np.float32, algorithm="sum-product")
                    _, _, llr = _llrs(orc, rng, bg, Z, B, -3.0, nl=nl)
                    hg, ig, ag = codec.decode(llr, want_iters=True, want_app=True)
                    codec.close()
                    assert (ig == it).all()
                    hr, ir, ar = orc.decode_bp_flood(bg, Z, llr.astype(np.float64), it, n_layers=nl, nthreads=_threads(), want_app=True)
                    full = ir == it
                    if not full.any():
                        continue
                    g, r = ag[full].astype(np.float64), ar[full]
                    inf = np.isinf(r)
                    assert (np.isinf(g) == inf).all() and (g[inf] == r[inf]).all(), (bg, Z, nl, it)
                    f = ~inf
                    big = f & (np.abs(r) > 1e-3)
                    assert (np.signbit(g[big]) == np.signbit(r[big])).all(), (bg, Z, nl, it)
                    err = np.abs(g[f] - r[f])
                    lim = TOL * np.maximum(1.0, np.abs(r[f]))
                    assert (err <= lim).all(), (bg, Z, nl, it, float(err.max()))
                    worst["abs_err_max"] = max(worst["abs_err_max"], float(err.max()))
                    worst["rel_err_max"] = max(worst["rel_err_max"], float((err / np.maximum(1.0, np.abs(r[f]))).max()))
                    worst["compared_entries"] += int(f.sum())
                    worst["cases"] += 1
                    assert (hg[full] == hr[full]).mean() > 0.999
    _record("soft_output_tolerance", worst)
    print(worst)
    assert worst["cases"] > 100


# ---- 2. parity stop, every lifting size ---------------------------------------------------------------------------------
def _compare_stop(tag, hg, ig, hr, ir, cap, stats):
    conv_g, conv_r = ig < cap, ir < cap  # a count below the cap: stopped on the parity check
    # a codeword that converged exactly at the cap is told apart by its checks (hard decisions of the oracle satisfy H)
    agree = (conv_g == conv_r).mean()
    both = conv_g & conv_r
    same_bits = (hg[both] == hr[both]).all(1)
    same_it = ig[both] == ir[both]
    stats.append((tag, float(agree), int(both.sum()), float(same_bits.mean()) if both.any() else 1.0,
                  float(same_it.mean()) if both.any() else 1.0))
    assert agree >= 0.99, (tag, agree)
    if both.any():
        assert same_bits.all(), tag
        assert same_it.mean() >= 0.99, (tag, same_it.mean())


@pytest.mark.parametrize("bg", [1, 2])
def test_parity_stop_against_the_oracle_at_every_lifting_size(pkg, orc, bg):
    rng = np.random.default_rng(77 + bg)
    rows, cols, kb = BG_DIMS[bg]
    stats = []
    for i, Z in enumerate(ALL_Z):
        B = 128 if Z <= 32 else 64 if Z <= 128 else 32
        cap = 8
        dt = np.float16 if i % 3 == 2 else np.float32
        codec = pkg.Codec(bg, Z, max_iter=cap, early_term=True, llr_dtype=dt, algorithm="sum-product")
        info, cw, llr = _llrs(orc, rng, bg, Z, B, _snr_waterfall(Z), dtype=dt)
        hg, ig = codec.decode(llr, want_iters=True)
        hr, ir = orc.decode_bp_flood(bg, Z, llr.astype(np.float64), cap, nthreads=_threads())
        _compare_stop((bg, Z, str(np.dtype(dt))), hg, ig, hr, ir, cap, stats)
        # noise-free codewords: the transmitted bits, in the oracle's sweep count
        q = ((1 - 2.0 * cw[:4]) * 4.0).astype(dt)
        q[:, :2 * Z] = 0
        q[:, kb * Z - Z // 4:kb * Z] = np.inf
        hq, iq = codec.decode(q, want_iters=True)
        _, irq = orc.decode_bp_flood(bg, Z, q.astype(np.float64), cap, nthreads=_threads())
        assert (hq == info[:4]).all() and (iq == irq).all(), (bg, Z)
        codec.close()
    # a random (layers, cap) grid, NRLDPC_LAYERS_AUTO included
    for k in range(12):
        Z = int(rng.choice(ALL_Z))
        nl = int(rng.integers(4, rows + 1))
        cap = int(rng.integers(1, 21))
        auto = k % 3 == 0
        dt = np.float16 if k % 2 else np.float32
        B = 48 if Z <= 64 else 16
        codec = pkg.Codec(bg, Z, max_iter=cap, n_layers=pkg._capi.LAYERS_AUTO if auto else nl, early_term=True, llr_dtype=dt,
                          algorithm="sum-product")
        _, _, llr = _llrs(orc, rng, bg, Z, B, _snr_waterfall(Z) + 3.0 * (rows - nl) / rows, nl=nl, dtype=dt)
        hg, ig = codec.decode(llr, want_iters=True)
        if auto:
            assert codec.last_layers() == pkg._capi.count_layers(bg, Z, llr)
        used = codec.last_layers()
        codec.close()
        hr, ir = orc.decode_bp_flood(bg, Z, llr.astype(np.float64), cap, n_layers=used, nthreads=_threads())
        _compare_stop((bg, Z, used, cap, "auto" if auto else "fixed"), hg, ig, hr, ir, cap, stats)
    _record("parity_stop_bg%d" % bg, {"cases": len(stats), "min_outcome_agreement": min(s[1] for s in stats),
                                      "min_sweep_agreement": min(s[4] for s in stats)})


# ---- 3. the committed sum-product BLER outcomes ---------------------------------------------------------------------------
def test_block_outcomes_match_the_committed_sum_product_results(pkg, orc):
    import bler_cases as BC
    ref = BC.Ref(os.path.join(ROOT, "tests", "golden", "bler_ref.npz"))
    runs = BC.runs()
    by_case = {}
    for key, factory, case, bg, Z, nl, cap, snr in runs:
        by_case.setdefault((factory.__name__, case[0]), []).append((key, factory, case, bg, Z, nl, cap, snr))
    rec, checked = {}, 0
    for group in by_case.values():
        key0, factory, case = group[0][0], group[0][1], group[0][2]
        inp = factory(case, orc.encode)
        codecs = {}
        for key, _, _, bg, Z, nl, cap, snr in group:
            if cap not in codecs:
                codecs[cap] = pkg.Codec(bg, Z, max_iter=cap, n_layers=nl, early_term=True, llr_dtype=np.float64, algorithm="sum-product")
            llr = inp.llr_at(snr)
            nblk = llr.shape[0]
            got = ref.get(key, llr, inp.Kp, inp.info, nblk)
            assert got is not None, "no committed result for %s (or its LLRs differ)" % key
            err_ref, sweeps_ref = got
            hard, it = codecs[cap].decode(llr, want_iters=True)
            err = (hard[:, :inp.Kp] != inp.info[:, :inp.Kp]).any(1)
            diff = int((err != err_ref).sum())
            rec[key] = {"blocks": nblk, "bler": float(err.mean()), "bler_ref": float(err_ref.mean()), "differing_blocks": diff,
                        "mean_sweeps": float(it.mean()), "mean_sweeps_ref": sweeps_ref}
            assert diff <= max(2, 0.01 * nblk), (key, rec[key])
            assert abs(float(it.mean()) - sweeps_ref) <= 0.02 * sweeps_ref, (key, rec[key])
            checked += 1
            del llr, hard
        for c in codecs.values():
            c.close()
        del inp
    _record("bler_runs", rec)
    assert checked == len(runs)


# ---- 4. through the harness, at the reference's defaults ----------------------------------------------------------------
def test_harness_at_the_reference_defaults_reproduces_the_reference_algorithm(pkg, orc):
    import importlib
    from test_bler_gap_gpu import CASES_DEMO, _reference_decoder_class, crossing
    H = importlib.import_module(pkg.__name__ + ".harness")
    Ref = _reference_decoder_class(pkg, orc)
    out = {}
    for name, A, R, BG, mod, rvs, iters, snrs, nblk in CASES_DEMO:
        Q_m = H.Q_M[mod]
        G = int(round(A / R / Q_m) * Q_m)
        res = {}
        for tag, cls, kw in (("gpu", pkg.NRLDPCDecoder, {"algorithm": "sum-product"}), ("ref", Ref, {})):
            hEnc = pkg.NRLDPCEncoder(A=A, BG=BG, G=G, Q_m=Q_m)
            hDec = cls(A=A, BG=BG, G=G, Q_m=Q_m, I_HARQ=1, iterations=iters, **kw)
            oks = []
            for snr in snrs:
                rng = np.random.default_rng(zlib.crc32((name + str(snr)).encode()))
                oks.append(H.simulate_point(hEnc, hDec, Q_m, snr, rvs, nblk, rng))
            hEnc.release(); hDec.release()
            res[tag] = oks
        agree = [float((g == r).mean()) for g, r in zip(res["gpu"], res["ref"])]
        bg_, br_ = [float(1 - o.mean()) for o in res["gpu"]], [float(1 - o.mean()) for o in res["ref"]]
        xg, xr = crossing(snrs, bg_, nblk), crossing(snrs, br_, nblk)
        out[name] = {"EsN0_dB": snrs, "bler_gpu_sum_product": bg_, "bler_reference": br_, "block_agreement": agree,
                     "EsN0_at_bler_0.1_gpu": xg, "EsN0_at_bler_0.1_reference": xr}
        assert min(agree) >= 0.99, out[name]
        assert xg is not None and xr is not None and abs(xg - xr) <= 0.05, out[name]
    _record("harness_reference_defaults", out)


# ---- 5. every entry point agrees ----------------------------------------------------------------------------------------
def test_every_entry_point_agrees(pkg, orc):
    import torch
    rng = np.random.default_rng(5)
    bg, Z, cap = 2, 52, 12
    rows, cols, kb = BG_DIMS[bg]
    K = kb * Z
    B = 96
    info, _, llr = _llrs(orc, rng, bg, Z, B, _snr_waterfall(Z), nl=20)
    c = pkg.Codec(bg, Z, max_iter=cap, n_layers=20, early_term=True, llr_dtype=np.float32, algorithm="sum-product")
    assert c.algorithm == "sum-product"
    h0, i0 = c.decode(llr, want_iters=True)
    hr, ir = orc.decode_bp_flood(bg, Z, llr.astype(np.float64), cap, n_layers=20, nthreads=_threads())
    assert ((i0 < cap) == (ir < cap)).mean() >= 0.99
    pk, ip = c.decode_packed(llr, want_iters=True)
    assert (np.unpackbits(pk, axis=1, bitorder="little")[:, :K] == h0).all() and (ip == i0).all()
    c.set_layers(0)
    pk2, ip2 = c.decode_packed(llr, want_iters=True, n_layers=20)
    assert (np.unpackbits(pk2, axis=1, bitorder="little")[:, :K] == h0).all() and (ip2 == i0).all()
    c.set_layers(20)
    d_llr = torch.from_numpy(llr).cuda()
    d_h = torch.zeros((B, K), dtype=torch.uint8, device="cuda")
    d_i = torch.zeros(B, dtype=torch.int32, device="cuda")
    c.decode_dev(d_llr.data_ptr(), B, d_h.data_ptr(), d_i.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_h.cpu().numpy() == h0).all() and (d_i.cpu().numpy() == i0).all()
    # a pool of two shards on one device
    pool = pkg.CodecPool(bg, Z, [0, 0], max_iter=cap, n_layers=20, early_term=True, llr_dtype=np.float32, algorithm="sum-product")
    hp, ipl = pool.decode(llr, want_iters=True)
    pool.close()
    assert (hp == h0).all() and (ipl == i0).all()
    # f64 host input = f32 input of the narrowed values
    c64 = pkg.Codec(bg, Z, max_iter=cap, n_layers=20, early_term=True, llr_dtype=np.float64, algorithm="sum-product")
    x64 = llr.astype(np.float64) + rng.standard_normal(llr.shape) * 1e-9
    h64, i64 = c64.decode(x64, want_iters=True)
    h32, i32 = c.decode(x64.astype(np.float32), want_iters=True)
    assert (h64 == h32).all() and (i64 == i32).all()
    c64.close()
    # decode_multi_dev: sum-product and min-sum handles in one call, each equal to its own decode_dev
    ms = pkg.Codec(bg, Z, max_iter=cap, n_layers=20, early_term=True, llr_dtype=np.float32)
    sp2 = pkg.Codec(1, 20, max_iter=6, early_term=True, llr_dtype=np.float32, algorithm="sum-product")
    _, _, llr2 = _llrs(orc, rng, 1, 20, 40, 0.5)
    d_llr2 = torch.from_numpy(llr2).cuda()
    outs = [(torch.zeros((B, K), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")) for _ in range(2)]
    o2 = (torch.zeros((40, 22 * 20), dtype=torch.uint8, device="cuda"), torch.zeros(40, dtype=torch.int32, device="cuda"))
    st = torch.cuda.current_stream().cuda_stream
    pkg.decode_multi_dev([c, ms, sp2], [d_llr.data_ptr(), d_llr.data_ptr(), d_llr2.data_ptr()], [B, B, 40],
                         [outs[0][0].data_ptr(), outs[1][0].data_ptr(), o2[0].data_ptr()],
                         [outs[0][1].data_ptr(), outs[1][1].data_ptr(), o2[1].data_ptr()], st)
    torch.cuda.synchronize()
    assert (outs[0][0].cpu().numpy() == h0).all() and (outs[0][1].cpu().numpy() == i0).all()
    ref_ms = (torch.zeros((B, K), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"))
    ms.decode_dev(d_llr.data_ptr(), B, ref_ms[0].data_ptr(), ref_ms[1].data_ptr(), None, st)
    ref_sp2 = (torch.zeros((40, 22 * 20), dtype=torch.uint8, device="cuda"), torch.zeros(40, dtype=torch.int32, device="cuda"))
    sp2.decode_dev(d_llr2.data_ptr(), 40, ref_sp2[0].data_ptr(), ref_sp2[1].data_ptr(), None, st)
    torch.cuda.synchronize()
    assert torch.equal(outs[1][0], ref_ms[0]) and torch.equal(outs[1][1], ref_ms[1])
    assert torch.equal(o2[0], ref_sp2[0]) and torch.equal(o2[1], ref_sp2[1])
    ms.close(); sp2.close(); c.close()
    # a host batch above 8 MB (the chunked pipeline) gives the device call's bits: the int8 route is not taken
    bg, Z, cap = 1, 384, 6
    cb = pkg.Codec(bg, Z, max_iter=cap, early_term=True, llr_dtype=np.float32, algorithm="sum-product")
    _, _, big = _llrs(orc, rng, bg, Z, 24, -1.2)
    big = np.concatenate([big] * 4)  # 96 codewords x 104 KB
    assert big.nbytes > (8 << 20)
    hb, ib = cb.decode(big, want_iters=True)
    d_big = torch.from_numpy(big).cuda()
    d_hb = torch.zeros((big.shape[0], 22 * Z), dtype=torch.uint8, device="cuda")
    d_ib = torch.zeros(big.shape[0], dtype=torch.int32, device="cuda")
    cb.decode_dev(d_big.data_ptr(), big.shape[0], d_hb.data_ptr(), d_ib.data_ptr(), None, st)
    torch.cuda.synchronize()
    assert (d_hb.cpu().numpy() == hb).all() and (d_ib.cpu().numpy() == ib).all()
    cb.close()


# ---- 6. determinism -----------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_batch_split_order_or_streams(pkg, orc):
    import torch
    rng = np.random.default_rng(6)
    for bg, Z, B in ((1, 384, 24), (2, 10, 600)):
        K, N = BG_DIMS[bg][2] * Z, BG_DIMS[bg][1] * Z
        c = pkg.Codec(bg, Z, max_iter=10, early_term=True, llr_dtype=np.float32, algorithm="sum-product")
        _, _, llr = _llrs(orc, rng, bg, Z, B, _snr_waterfall(Z))
        h, i, a = c.decode(llr, want_iters=True, want_app=True)
        h2, i2, a2 = c.decode(llr, want_iters=True, want_app=True)
        assert (h == h2).all() and (i == i2).all() and (a.view(np.uint32) == a2.view(np.uint32)).all()
        k = B // 3
        ha, ia, aa = c.decode(llr[:k], want_iters=True, want_app=True)
        hb, ib, ab = c.decode(llr[k:], want_iters=True, want_app=True)
        assert (np.concatenate([ha, hb]) == h).all() and (np.concatenate([ia, ib]) == i).all()
        assert (np.concatenate([aa, ab]).view(np.uint32) == a.view(np.uint32)).all()
        p = rng.permutation(B)
        hp, ip, ap = c.decode(llr[p], want_iters=True, want_app=True)
        assert (hp == h[p]).all() and (ip == i[p]).all() and (ap.view(np.uint32) == a[p].view(np.uint32)).all()
        # two device calls on one handle, two streams, enqueued back to back
        d_llr = torch.from_numpy(llr).cuda()
        outs = [(torch.zeros((B, K), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
                 torch.zeros((B, N), dtype=torch.float32, device="cuda")) for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        for s, o in ((s1, outs[0]), (s2, outs[1])):
            c.decode_dev(d_llr.data_ptr(), B, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        for o in outs:
            assert (o[0].cpu().numpy() == h).all() and (o[1].cpu().numpy() == i).all()
            assert (o[2].cpu().numpy().view(np.uint32) == a.view(np.uint32)).all()
        c.close()


# ---- 7. refusals, and min-sum untouched ---------------------------------------------------------------------------------
def test_refusals_and_min_sum_unchanged_after_a_round_trip(pkg, orc):
    import ctypes as C
    L = pkg.load()
    c = pkg.Codec(2, 20, max_iter=10, n_layers=12, early_term=True, llr_dtype=np.float32)
    assert c.algorithm == "min-sum"
    assert L.nrldpc_set_algorithm(c._h, 2) == pkg._capi.ERR_UNSUPPORTED
    assert L.nrldpc_set_algorithm(c._h, -1) == pkg._capi.ERR_UNSUPPORTED
    a = C.c_int32(-5)
    assert L.nrldpc_get_algorithm(c._h, C.byref(a)) == 0 and a.value == 0
    with pytest.raises(pkg.UnsupportedParameters):
        pkg.Codec(2, 20, max_iter=10, crc=(0x1800063, 24, 100), algorithm="sum-product")
    crc = pkg.Codec(2, 20, max_iter=10, crc=(0x1800063, 24, 100))
    with pytest.raises(pkg.UnsupportedParameters):
        crc.set_algorithm("sum-product")
    assert crc.algorithm == "min-sum"
    crc.close()
    rng = np.random.default_rng(7)
    _, _, llr = _llrs(orc, rng, 2, 20, 256, 1.0, nl=12)
    c.set_algorithm("sum-product")
    assert c.algorithm == "sum-product"
    c.decode(llr)
    c.set_algorithm("min-sum")
    h, i, app = c.decode(llr, want_iters=True, want_app=True)
    ho, io, ao = orc.decode_nmsq(2, 20, llr.astype(np.float64), 10, n_layers=12, early_term=True, want_app=True, **rule_kw(c))
    assert (h == ho).all() and (i == io).all() and (app == ao).all()
    c.close()

"""Whole-codeword hard decisions and final parity checks (nrldpc_decode_cw / nrldpc_decode_cw_dev, nrldpc_cw_out) on the GPU.

Min-sum: exact against the oracle's soft output (cw_ref = APP_ref < 0 of orc.decode_nmsq), its syndrome weight and a numpy
evaluation of every check -- ragged ballot tails (Z = 2: 136 / 104 bits, Z = 3: 204 / 156), odd Z, the packed, compile-time and
largest geometries, all / 4 / an intermediate layer count, fixed iteration counts and the parity stop, and a batch that crosses the
64 MiB scratch of the min-sum path (two chunks and a ragged tail).  Sum-product: the fused outputs against the same call's
app_out (exact), their own parity (exact) and the oracle's double-precision APP outside the sign clause of the stated tolerance.
Then every entry point, single outputs, two streams of one handle, the refusals, and plain decodes left as they were."""
import ctypes as C

import numpy as np
import pytest

from conftest import BG_DIMS, rule_kw
from test_sum_product_gpu import _llrs, _snr_waterfall, _threads

pytestmark = pytest.mark.gpu

MS_Z = (2, 3, 7, 15, 52, 64, 104, 384)
SP_Z = (2, 3, 15, 52, 104, 384)
MODES = ((0, 1), (0, 2), (0, 3), (1, 8))  # (early_term, iteration cap)
SP_OFF, SP_OFF_FIXED, SP_FLOOR_FIXED = 1.5, 4.0, 6.0
# seeds for which the ORACLE's sum-product output leaves at most 1e-4 of a case's entries within 1e-3 of zero (found on the CPU)
SP_SEED = {(1, 2): 1, (1, 3): 1, (1, 15): 2, (1, 52): 1, (1, 104): 1, (1, 384): 1, (2, 2): 1, (2, 3): 1, (2, 15): 2, (2, 52): 2, (2, 104): 1, (2, 384): 1}
SCRATCH = 64 << 20                        # NRLDPC_CW_SCRATCH_BYTES


def _mid(bg, Z):
    """One intermediate layer count, 5 .. rows - 1, another one for every (BG, Z)."""
    rows = BG_DIMS[bg][0]
    return 5 + (7 * Z + bg) % (rows - 5)


def _snr(bg, Z, nl, et, sp=False):
    """Es/N0 of a case.  Min-sum: fixed iteration counts at the full code's waterfall (nothing converges in one iteration, a pruned
    code hardly in three); the stop near the waterfall of the code the active rows leave -- rate kb / (kb + nl - 2) -- so that a
    batch holds codewords that converge within the cap and codewords that do not.  Sum-product: the stop 1.5 dB above the
    latter, fixed sweep counts 4 dB above it and at 6 dB at least: at the full code's waterfall one a-posteriori LLR in a few
    thousand lies within 1e-3 of zero after one to three sweeps whatever the seed (and, with 4 rows, most of the punctured columns
    do), which is more than the comparison with the oracle may leave out."""
    rows, cols, kb = BG_DIMS[bg]
    if not et and not sp:
        return _snr_waterfall(Z)
    rate = kb / (kb + nl - 2.0)
    snr = _snr_waterfall(Z) + 10.0 * np.log10((2.0 ** (2.0 * rate) - 1.0) / (2.0 ** (2.0 / 3.0) - 1.0))
    if not sp:
        return snr + 0.4
    return snr + SP_OFF if et else max(snr + SP_OFF_FIXED, SP_FLOOR_FIXED)


def _cases(orc, bg, Z, seed, sp=False):
    """(n_layers as configured, rows decoded, early_term, cap, LLRs) of one (BG, Z): the same LLRs whoever asks."""
    rows = BG_DIMS[bg][0]
    rng = np.random.default_rng(seed)
    B = 3 if Z == 384 else 5
    for nl_cfg in (0, 4, _mid(bg, Z)):
        nl = nl_cfg or rows
        for et, cap in MODES:
            _, _, llr = _llrs(orc, rng, bg, Z, B, _snr(bg, Z, nl, et, sp), nl=nl_cfg)
            yield nl_cfg, nl, et, cap, llr


_EDGES = {}


def _checks_np(orc, bg, Z, cw, nl):
    """Every check of H on the bits cw [B][N], [B][rows*Z]: check (l, z) is the XOR of cw[col*Z + (z + shift) mod Z] over the
    edges of row l (get_pcm.m:8); rows >= nl are 0."""
    if (bg, Z) not in _EDGES:
        _EDGES[bg, Z] = orc.graph_edges(bg, Z)
    r, c, s = _EDGES[bg, Z]
    rows = BG_DIMS[bg][0]
    out = np.zeros((cw.shape[0], rows, Z), np.uint8)
    z = np.arange(Z)
    for e in range(len(r)):
        if r[e] < nl:
            out[:, r[e], :] ^= cw[:, c[e] * Z + (z + s[e]) % Z]
    return out.reshape(cw.shape[0], rows * Z)


def _check_exact(orc, bg, Z, nl, got, hard_ref, iters_ref, app_ref, tag):
    """decode_cw's five outputs against a reference decode (hard, iters, APP): bits, syndrome weight, every check."""
    hard, iters, cw, unsat, chk = got
    K = BG_DIMS[bg][2] * Z
    cw_ref = (app_ref < 0).astype(np.uint8)
    assert cw.shape == cw_ref.shape and (cw == cw_ref).all(), tag
    assert (cw[:, :K] == hard).all() and (hard == hard_ref).all() and (iters == iters_ref).all(), tag
    want = np.array([orc.syndrome_weight(bg, Z, cw_ref[b], nl) for b in range(cw_ref.shape[0])])
    assert (unsat == want).all(), (tag, unsat, want)
    chk_ref = _checks_np(orc, bg, Z, cw_ref, nl)
    assert chk.shape == chk_ref.shape and (chk == chk_ref).all(), tag
    assert (chk_ref.sum(1) == want).all(), tag  # the two references agree with each other
    return want


# ---- 1. min-sum, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Z", MS_Z)
@pytest.mark.parametrize("bg", [1, 2])
def test_min_sum_outputs_are_the_oracles(pkg, orc, bg, Z):
    converged = stuck = 0
    for nl_cfg, nl, et, cap, llr in _cases(orc, bg, Z, 4100 + 1000 * bg + Z):
        codec = pkg.Codec(bg, Z, max_iter=cap, n_layers=nl_cfg, early_term=bool(et), llr_dtype=np.float32)
        got = codec.decode_cw(llr, want_checks=True)
        h0, i0 = codec.decode(llr, want_iters=True)
        assert codec.last_layers() == nl
        kw = rule_kw(codec)
        codec.close()
        hr, ir, ar = orc.decode_nmsq(bg, Z, llr.astype(np.float64), cap, n_layers=nl_cfg, early_term=bool(et), want_app=True, **kw)
        tag = (bg, Z, nl, et, cap)
        assert (got[0] == h0).all() and (got[1] == i0).all(), tag
        want = _check_exact(orc, bg, Z, nl, got, hr, ir, ar, tag)
        print(tag, "iters", got[1].tolist(), "unsatisfied", got[3].tolist())
        if et:
            assert (got[3][got[1] < cap] == 0).all(), tag
        converged += int((want == 0).sum())
        stuck += int((want > 0).sum())
    # a case set of converged codewords only (or of none) would show nothing about the count
    assert converged > 0 and stuck > 0, (bg, Z, converged, stuck)


# ---- 2. the chunk boundary of the min-sum scratch -----------------------------------------------------------------------------
def test_min_sum_batch_that_crosses_the_scratch(pkg, orc):
    bg, Z, nl, cap = 2, 384, 4, 1
    rows, cols, kb = BG_DIMS[bg]
    N = cols * Z
    B = SCRATCH // (4 * N) + 3
    assert B == 843  # two chunks: 840 codewords and a tail of 3
    rng = np.random.default_rng(843)
    _, _, llr = _llrs(orc, rng, bg, Z, B, 10.5, nl=nl)
    codec = pkg.Codec(bg, Z, max_iter=cap, n_layers=nl, early_term=False, llr_dtype=np.float32)
    got = codec.decode_cw(llr, want_checks=True)
    h0, i0 = codec.decode(llr, want_iters=True)
    kw = rule_kw(codec)
    codec.close()
    hr, ir, ar = orc.decode_nmsq(bg, Z, llr.astype(np.float64), cap, n_layers=nl, early_term=False, want_app=True, **kw)
    assert (got[0] == h0).all() and (got[1] == i0).all()
    want = _check_exact(orc, bg, Z, nl, got, hr, ir, ar, "chunks")
    assert (want == 0).any() and (want > 0).any() and (want[840:] > 0).any()
    # NRLDPC_LAYERS_AUTO: found once for the whole call (the extension columns above row 4 hold zeros), same rule, same results
    auto = pkg.Codec(bg, Z, max_iter=cap, n_layers=pkg._capi.LAYERS_AUTO, early_term=False, llr_dtype=np.float32)
    ga = auto.decode_cw(llr, want_checks=True)
    assert auto.last_layers() == 4
    auto.close()
    for a, b in zip(ga, got):
        assert (a == b).all()


# ---- 3. sum-product -------------------------------------------------------------------------------------------------------
def _excluded(app_ref):
    """The entries the sign clause of the stated tolerance (include/nrldpc.h) leaves open: 0 < |APP_ref| <= 1e-3."""
    a = np.abs(app_ref)
    return (a > 0) & (a <= 1e-3)


@pytest.mark.parametrize("Z", SP_Z)
@pytest.mark.parametrize("bg", [1, 2])
def test_sum_product_fused_outputs(pkg, orc, bg, Z):
    """Fused outputs = the same call's app_out, hard-decided (exact); parity of the GPU's own bits (exact); against the oracle's
    double-precision APP, bit for bit wherever |APP_ref| > 1e-3 (or APP_ref == 0), on the codewords both ran the same number
    of sweeps on (the oracle always stops on the parity check, so under a fixed count only those it did not stop early)."""
    K = BG_DIMS[bg][2] * Z
    compared = 0
    for nl_cfg, nl, et, cap, llr in _cases(orc, bg, Z, SP_SEED[bg, Z], sp=True):
        tag = (bg, Z, nl, et, cap)
        hr, ir, ar = orc.decode_bp_flood(bg, Z, llr.astype(np.float64), cap, n_layers=nl_cfg, nthreads=_threads(), want_app=True)
        ex = _excluded(ar)
        assert ex.sum() <= 1e-4 * ex.size, (tag, int(ex.sum()))  # the oracle alone: the seeds leave (next to) nothing open
        codec = pkg.Codec(bg, Z, max_iter=cap, n_layers=nl_cfg, early_term=bool(et), llr_dtype=np.float32, algorithm="sum-product")
        hard, iters, cw, unsat, chk = codec.decode_cw(llr, want_checks=True)
        h0, i0, app = codec.decode(llr, want_iters=True, want_app=True)
        assert codec.last_layers() == nl
        codec.close()
        assert (hard == h0).all() and (iters == i0).all(), tag
        assert (cw == (app < 0)).all() and (cw[:, :K] == hard).all(), tag
        own = _checks_np(orc, bg, Z, cw, nl)
        assert (chk == own).all() and (unsat == own.sum(1)).all(), tag
        print(tag, "sweeps", iters.tolist(), "oracle", ir.tolist(), "unsatisfied", unsat.tolist(), "excluded", int(ex.sum()))
        same = iters == ir
        cw_ref = (ar < 0).astype(np.uint8)
        assert ((cw == cw_ref) | ex)[same].all(), tag
        compared += int(same.sum())
        if et:
            assert (unsat[iters < cap] == 0).all(), tag
            for b in np.nonzero((iters == cap) & ~ex.any(1))[0]:
                assert (unsat[b] == 0) == (orc.syndrome_weight(bg, Z, cw_ref[b], nl) == 0), (tag, int(b))
    assert compared > 0


# ---- 4. every entry point -------------------------------------------------------------------------------------------------
def _dev_call(codec, llr, which=(True, True, True), stream=None):
    """decode_cw_dev on torch tensors; returns (hard, iters, cw_packed, unsatisfied, checks_packed) as numpy (None where not asked)."""
    import torch
    B = llr.shape[0]
    nchk8 = (codec.nrows * codec.Z + 7) // 8
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        d_llr = torch.from_numpy(llr).cuda()
        d_h = torch.zeros((B, codec.K), dtype=torch.uint8, device="cuda")
        d_i = torch.zeros(B, dtype=torch.int32, device="cuda")
        d_cw = torch.full((B, (codec.N_cw + 7) // 8), 0xA5, dtype=torch.uint8, device="cuda") if which[0] else None
        d_u = torch.full((B,), -7, dtype=torch.int32, device="cuda") if which[1] else None
        d_c = torch.full((B, nchk8), 0xA5, dtype=torch.uint8, device="cuda") if which[2] else None
    codec.decode_cw_dev(d_llr.data_ptr(), B, d_h.data_ptr(), d_i.data_ptr(), d_cw.data_ptr() if which[0] else None,
                        d_u.data_ptr() if which[1] else None, d_c.data_ptr() if which[2] else None, st.cuda_stream)
    return d_llr, [d_h, d_i, d_cw, d_u, d_c]


def _to_np(outs):
    return [o.cpu().numpy() if o is not None else None for o in outs]


def _packed(got):
    """decode_cw's unpacked (hard, iters, cw, unsat, checks) in the device call's packed form."""
    return [got[0], got[1], np.packbits(got[2], axis=1, bitorder="little"), got[3], np.packbits(got[4], axis=1, bitorder="little")]


@pytest.mark.parametrize("algorithm", ["min-sum", "sum-product"])
def test_entry_points_single_outputs_and_streams(pkg, orc, algorithm):
    import torch
    bg, Z, nl, cap = 1, 15, 13, 6
    rng = np.random.default_rng(99)
    _, _, llr = _llrs(orc, rng, bg, Z, 37, _snr(bg, Z, nl, 1) - 1.0, nl=nl)
    _, _, llr_b = _llrs(orc, rng, bg, Z, 37, _snr(bg, Z, nl, 1) - 1.0, nl=nl)
    kw = dict(max_iter=cap, n_layers=nl, early_term=True, algorithm=algorithm)
    c32 = pkg.Codec(bg, Z, llr_dtype=np.float32, **kw)
    ref = _packed(c32.decode_cw(llr, want_checks=True))
    ref_b = _packed(c32.decode_cw(llr_b, want_checks=True))
    assert (ref[3] == 0).any() and (ref[3] > 0).any()
    # device pointers = host pointers (F32)
    _, outs = _dev_call(c32, llr)
    torch.cuda.synchronize()
    for a, b in zip(_to_np(outs), ref):
        assert a.shape == b.shape and (a == b).all()
    # each single output alone = its part of the all-three call; the others are not touched
    for k in range(3):
        which = tuple(j == k for j in range(3))
        _, outs = _dev_call(c32, llr, which)
        torch.cuda.synchronize()
        got = _to_np(outs)
        assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and (got[2 + k] == ref[2 + k]).all()
        assert all(got[2 + j] is None for j in range(3) if j != k)
    # two calls on two streams of one handle, different inputs, enqueued back to back
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    keep1, o1 = _dev_call(c32, llr, stream=s1)
    keep2, o2 = _dev_call(c32, llr_b, stream=s2)
    torch.cuda.synchronize()
    for a, b in zip(_to_np(o1), ref):
        assert (a == b).all()
    for a, b in zip(_to_np(o2), ref_b):
        assert (a == b).all()
    del keep1, keep2
    c32.close()
    # F16: host = device;  F64: host = F32 of the narrowed values
    l16 = llr.astype(np.float16)
    c16 = pkg.Codec(bg, Z, llr_dtype=np.float16, **kw)
    h16 = _packed(c16.decode_cw(l16, want_checks=True))
    _, outs = _dev_call(c16, l16)
    torch.cuda.synchronize()
    for a, b in zip(_to_np(outs), h16):
        assert (a == b).all()
    c16.close()
    x64 = llr.astype(np.float64) + rng.standard_normal(llr.shape) * 1e-9
    c64 = pkg.Codec(bg, Z, llr_dtype=np.float64, **kw)
    h64 = c64.decode_cw(x64, want_checks=True)
    c64.close()
    c32 = pkg.Codec(bg, Z, llr_dtype=np.float32, **kw)
    h32 = c32.decode_cw(x64.astype(np.float32), want_checks=True)
    c32.close()
    for a, b in zip(h64, h32):
        assert (a == b).all()


# ---- 5. refusals, and plain decodes untouched -------------------------------------------------------------------------------
def test_refusals_and_no_side_effects(pkg, orc):
    L = pkg.load()
    capi = pkg._capi
    bg, Z = 2, 20
    rng = np.random.default_rng(11)
    _, _, llr = _llrs(orc, rng, bg, Z, 16, 1.0, nl=12)
    c = pkg.Codec(bg, Z, max_iter=10, n_layers=12, early_term=True, llr_dtype=np.float32)
    B = llr.shape[0]
    hard, iters, unsat = np.zeros((B, c.K), np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32)
    args = (c._h, llr.ctypes.data_as(C.c_void_p), B, hard.ctypes.data_as(C.c_void_p), iters.ctypes.data_as(C.c_void_p))
    assert L.nrldpc_decode_cw(*args, C.byref(capi.CwOut(None, None, None))) == capi.ERR_ARG
    assert L.nrldpc_decode_cw_dev(*args, C.byref(capi.CwOut(None, None, None)), None) == capi.ERR_ARG
    bad = capi.CwOut(None, unsat.ctypes.data, None)
    bad.struct_size -= 8
    assert L.nrldpc_decode_cw(*args, C.byref(bad)) == capi.ERR_ARG and b"struct_size" in L.nrldpc_last_error()
    assert L.nrldpc_decode_cw_dev(*args, C.byref(bad), None) == capi.ERR_ARG
    assert L.nrldpc_decode_cw(*args, None) == capi.ERR_ARG
    crc = pkg.Codec(bg, Z, max_iter=10, crc=(0x1800063, 24, 100))
    with pytest.raises(pkg.UnsupportedParameters):
        crc.decode_cw(llr)
    ok = capi.CwOut(None, unsat.ctypes.data, None)
    assert L.nrldpc_decode_cw_dev(crc._h, *args[1:], C.byref(ok), None) == capi.ERR_UNSUPPORTED
    crc.close()
    # a plain decode gives what it gave before a decode_cw, for both algorithms
    for alg in ("min-sum", "sum-product"):
        c.set_algorithm(alg)
        before = c.decode(llr, want_iters=True, want_app=True)
        got = c.decode_cw(llr)
        assert len(got) == 4 and (got[0] == before[0]).all() and (got[1] == before[1]).all() and (got[2] == (before[2] < 0)).all()
        after = c.decode(llr, want_iters=True, want_app=True)
        pk = c.decode_packed(llr)
        assert (after[0] == before[0]).all() and (after[1] == before[1]).all()
        assert (after[2].view(np.uint32) == before[2].view(np.uint32)).all()
        assert (np.unpackbits(pk, axis=1, bitorder="little")[:, :c.K] == before[0]).all()
    c.close()

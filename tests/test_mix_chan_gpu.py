"""Mixed transport-block batches on the device, the channel leg: nrldpc_mix_chan_awgn_llr_dev, _modulate_dev, _awgn_dev and
_demodulate_dev against the loop of single-configuration calls, BIT FOR BIT (the fused stage included: its contract ended on bit
equality, not on the fall-back tolerance -- include/nrldpc.h), the fused stage against the float64 oracle,
the separate route against the fused one, split invariance, and MixedEncodeChain -> MixedChannel -> MixedDecodeChain.

The two plans (tests/mix_chan_cases.py; tests/test_mix_chan_api.py walks both grids of both on the CPU):
  main   the nine sets of tests/mix_cases.py, n_tb = (3, 1, 2, 0, 1, 2, 1, 1, 2): every Q_m, an empty configuration, odd symbol counts,
         a BPSK count that is no multiple of four, first symbols even, odd and across the 2^32 crossings;
  tails  one symbol per Q_m, and a configuration with a transport block but no symbol.

Every output array is pre-filled with 0xAA and has guards either side (tx_cases.Slot); the comparison is over the WHOLE packed array,
so gaps must still hold 0xAA after every call, and the guards are checked too.  Input bit bytes carry random bits 1..7 and every input
array has random gaps: only bit 0 of a byte, and no gap element, may be read.  The references are computed once per plan."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

import mix_chan_cases as MC
import tx_cases as T

pytestmark = pytest.mark.gpu

F32, F16 = 0, 1
ESIZE = {"f32": 4, "f16": 2, "hard": 1}


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()  # (a copy: `x` may be read-only)


class Ctx:
    """One test plan: parameter objects, counts, operating points, the channel plan, inputs with random upper bits and gaps."""

    def __init__(self, name, lo=0, hi=None):
        self.pkg = pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
        ps, n_tb, es, seeds, first = MC.plan(pkg, name)
        sl = slice(lo, hi)
        self.ps, self.n_tb, self.es, self.seeds, self.first = ps[sl], n_tb[sl], es[sl], seeds[sl], first[sl]
        self.n = len(self.ps)
        self.plan = pkg.MixChanPlan(self.ps, self.n_tb)
        self.g_off = [o.g for o in self.plan.off]
        self.sym_off = self.plan.sym_off
        self.tot = self.plan.totals()
        self.bits = [k * p.G for p, k in zip(self.ps, self.n_tb)]
        self.syms = MC.n_sym(self.ps, self.n_tb)
        assert self.sym_off == MC.sym_rule(self.ps, self.n_tb) and self.g_off == [o.g for o in pkg.mix_layout(self.ps, self.n_tb)]
        self.pts = self.plan.points(self.es, self.seeds, self.first)
        self.d_pt = dev(np.frombuffer(self.pts, np.uint8))
        self.n0 = [float(self.pts[i].variance) for i in range(self.n)]
        rng = np.random.default_rng(7 + len(name) + lo)
        self.g = [rng.integers(0, 2, b, dtype=np.uint8) | (rng.integers(0, 128, b, dtype=np.uint8) << 1) for b in self.bits]
        self.g_packed = self.pack_in(self.g, self.g_off, self.tot["g"], rng)
        # per-symbol variances: each symbol its own N0, within a factor of two of the configuration's
        self.var = [(n0 * rng.uniform(0.5, 2.0, c)).astype(np.float32) for n0, c in zip(self.n0, self.syms)]
        self.var_packed = self.pack_in(self.var, self.sym_off, self.tot["sym"], rng)
        self.rng = rng

    def pack_in(self, arrays, off, total, rng, per=1):
        """A packed INPUT: the segments, and random bytes in the gaps (finite random floats for float arrays)."""
        dt = arrays[0].dtype if arrays else np.uint8
        out = rng.integers(0, 256, total * per, dtype=np.uint8) if dt == np.uint8 else rng.uniform(-9.0, 9.0, total * per).astype(dt)
        for x, o in zip(arrays, off):
            out[o * per: o * per + x.size] = x.reshape(-1)
        out.setflags(write=False)
        return out

    def pack_out(self, arrays, off, total, per=1):
        """The bytes an OUTPUT array must hold after a call: the segments, and FILL in the gaps."""
        esize = arrays[0].dtype.itemsize
        out = np.full(total * per * esize, T.FILL, np.uint8)
        for x, o in zip(arrays, off):
            out[o * per * esize: o * per * esize + x.nbytes] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        out.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def ctx(name, lo=0, hi=None):
    return Ctx(name, lo, hi)


# ---- the loops of single calls: the references, computed once -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_fused(name):
    """what nrldpc_awgn_llr_dev leaves per configuration: [bits] f32"""
    import torch
    c = ctx(name)
    out = []
    for i in range(c.n):
        o = torch.full((max(c.bits[i], 1),), 7.0, dtype=torch.float32, device="cuda")
        if c.bits[i]:
            c.pkg.awgn_llr_dev(dev(c.g[i]).data_ptr(), c.bits[i], c.ps[i].Q_m, c.es[i], c.seeds[i], c.first[i], o.data_ptr())
        torch.cuda.synchronize()
        out.append(o[:c.bits[i]].cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def ref_tx(name):
    """what nrldpc_modulate_dev leaves per configuration: [n_sym][2] f32"""
    import torch
    c = ctx(name)
    out = []
    for i in range(c.n):
        o = torch.full((max(2 * c.syms[i], 1),), 7.0, dtype=torch.float32, device="cuda")
        if c.bits[i]:
            c.pkg.modulate_dev(dev(c.g[i]).data_ptr(), c.bits[i], c.ps[i].Q_m, o.data_ptr())
        torch.cuda.synchronize()
        out.append(o[:2 * c.syms[i]].cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def ref_rx(name, per_symbol):
    """what nrldpc_awgn_dev leaves per configuration on ref_tx, with the point's variance or the per-symbol array"""
    import torch
    c = ctx(name)
    out = []
    for i, tx in enumerate(ref_tx(name)):
        o = torch.full((max(tx.size, 1),), 7.0, dtype=torch.float32, device="cuda")
        if c.syms[i]:
            v = dev(c.var[i]) if per_symbol else None
            c.pkg.awgn_dev(dev(tx).data_ptr(), c.syms[i], o.data_ptr(), variance=c.n0[i], d_variance=v.data_ptr() if per_symbol else None,
                           seed=c.seeds[i], first_symbol=c.first[i])
        torch.cuda.synchronize()
        out.append(o[:tx.size].cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def ref_demod(name, method, kind, per_symbol):
    """what nrldpc_demodulate_dev leaves per configuration on ref_rx(name, False): kind "f32" / "f16" / "hard" """
    import torch
    c = ctx(name)
    tdt = {"f32": torch.float32, "f16": torch.float16, "hard": torch.uint8}[kind]
    out = []
    for i, rx in enumerate(ref_rx(name, False)):
        o = torch.full((max(c.bits[i], 1),), 7, dtype=tdt, device="cuda")
        if c.syms[i]:
            v = dev(c.var[i]) if per_symbol else None
            c.pkg.demodulate_dev(dev(rx).data_ptr(), c.syms[i], c.ps[i].Q_m, o.data_ptr(), method=method, variance=c.n0[i],
                                 d_variance=v.data_ptr() if per_symbol else None, out_dtype=F16 if kind == "f16" else F32)
        torch.cuda.synchronize()
        out.append(o[:c.bits[i]].cpu().numpy())
    return out


def same_bytes(slot, want, what):
    got = slot.data()
    bad = np.argwhere(got != want)[:4].reshape(-1).tolist()
    assert not bad, (what, "first differing bytes", bad)
    assert slot.guards_intact(), what


# ---- 1. the fused stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "tails"])
def test_fused_stage_equals_the_loop_of_single_calls_bit_for_bit(name):
    """nrldpc_mix_chan_awgn_llr_dev == nrldpc_awgn_llr_dev per configuration, bit for bit (the contract the fused stage ended on: the two
    kernels are compiled with contraction allowed and fuse the same multiply-adds), at an aligned g base and at odd-byte ones, with the
    LLR array 16-byte aligned (QPSK: the float4 store) and not."""
    import torch
    c = ctx(name)
    want = c.pack_out(ref_fused(name), c.g_off, c.tot["g"])
    for go, lo in ((0, 0), (1, 0), (3, 4), (0, 8)):
        src, dst = T.Slot(c.g_packed.size, go, c.g_packed), T.Slot(want.size, lo)
        c.plan.awgn_llr(src.ptr, c.d_pt.data_ptr(), dst.ptr)
        torch.cuda.synchronize()
        same_bytes(dst, want, (name, go, lo))


@pytest.mark.parametrize("name", ["main", "tails"])
def test_fused_stage_against_the_float64_oracle(name):
    """|dLLR| <= 5e-4 * max(1, |LLR|) against oracle/channel_oracle.py per configuration: the single call's own tolerance
    (tests/test_chain_gpu.py), at each configuration's Es/N0, seed and first symbol."""
    import torch
    import channel_oracle as CO
    c = ctx(name)
    dst = T.Slot(4 * c.tot["g"], 0)
    c.plan.awgn_llr(dev(c.g_packed).data_ptr(), c.d_pt.data_ptr(), dst.ptr)
    torch.cuda.synchronize()
    got = dst.data().view(np.float32).astype(np.float64)
    for i in range(c.n):
        if not c.bits[i]:
            continue
        ref = CO.awgn_llr(c.g[i] & 1, c.ps[i].Q_m, c.es[i], c.seeds[i], c.first[i])
        seg = got[c.g_off[i]: c.g_off[i] + c.bits[i]]
        err = np.abs(seg - ref) / np.maximum(1.0, np.abs(ref))
        print("%s configuration %d (Q_m %d, %g dB): max |dLLR| / max(1, |LLR|) = %.3g" % (name, i, c.ps[i].Q_m, c.es[i], err.max()))
        assert np.isfinite(seg).all() and err.max() <= 5e-4, (name, i, float(err.max()))


# ---- 2. the mapper -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "tails"])
def test_mapper_equals_the_loop_of_single_calls_bit_for_bit(name):
    import torch
    c = ctx(name)
    want = c.pack_out(ref_tx(name), c.sym_off, c.tot["sym"], per=2)
    for go in (0, 1, 2):  # (dword-aligned bits: the word loads; otherwise byte loads)
        src, dst = T.Slot(c.g_packed.size, go, c.g_packed), T.Slot(want.size, 4 * go)
        c.plan.modulate(src.ptr, dst.ptr)
        torch.cuda.synchronize()
        same_bytes(dst, want, (name, go))
    if name == "main":  # unit average power, configuration by configuration (the single calls themselves)
        for i, tx in enumerate(ref_tx(name)):
            if tx.size > 2000:
                assert abs(float((tx.astype(np.float64) ** 2).sum()) / (tx.size // 2) - 1.0) < 0.1, i


# ---- 3. the noise stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_symbol", [False, True])
@pytest.mark.parametrize("name", ["main", "tails"])
def test_noise_stage_equals_the_loop_of_single_calls_bit_for_bit(name, per_symbol):
    """Scalar variance from the points and a per-symbol array; out of place and in place."""
    import torch
    c = ctx(name)
    tx = c.pack_in(ref_tx(name), c.sym_off, c.tot["sym"], np.random.default_rng(3), per=2)
    rx = ref_rx(name, per_symbol)
    var = dev(c.var_packed) if per_symbol else None
    vp = var.data_ptr() if per_symbol else None
    # out of place: the gaps of the output keep the fill
    src, dst = T.Slot(tx.nbytes, 0, tx.view(np.uint8)), T.Slot(tx.nbytes, 4)
    c.plan.awgn(src.ptr, c.d_pt.data_ptr(), dst.ptr, d_variance=vp)
    torch.cuda.synchronize()
    same_bytes(dst, c.pack_out(rx, c.sym_off, c.tot["sym"], per=2), (name, per_symbol, "out of place"))
    same_bytes(src, tx.view(np.uint8), (name, per_symbol, "the source"))
    # in place: the gaps keep what the input held there
    want = np.array(tx, copy=True)
    for x, o in zip(rx, c.sym_off):
        want[2 * o: 2 * o + x.size] = x
    c.plan.awgn(src.ptr, c.d_pt.data_ptr(), src.ptr, d_variance=vp)
    torch.cuda.synchronize()
    same_bytes(src, want.view(np.uint8), (name, per_symbol, "in place"))
    if name == "main":  # (the noise is there: the sample variance of rx - tx is the point's N0 within 10 %)
        i = 5
        d = (rx[i].astype(np.float64) - ref_tx(name)[i]).reshape(-1, 2)
        n0 = float((d ** 2).sum(axis=1).mean())
        assert (0.6 if per_symbol else 0.9) * c.n0[i] < n0 < (1.6 if per_symbol else 1.1) * c.n0[i]


# ---- 4. the demapper ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,kind", [("llr", "f32"), ("llr", "f16"), ("approx", "f32"), ("approx", "f16"), ("hard", "hard")])
@pytest.mark.parametrize("name", ["main", "tails"])
def test_demapper_equals_the_loop_of_single_calls_bit_for_bit(name, method, kind):
    """All three methods, f32 and clamped f16 LLRs and hard-bit bytes, scalar and per-symbol variance; f16 and hard-bit outputs also at
    odd multiples of their element size (no dword stores there).  The operating points are not read for the hard decision, nor with
    the per-symbol array: the call gets no address for them."""
    import torch
    c = ctx(name)
    rx = dev(c.pack_in(ref_rx(name, False), c.sym_off, c.tot["sym"], np.random.default_rng(4), per=2))
    var = dev(c.var_packed)
    es = ESIZE[kind]
    for per_symbol in ((False,) if method == "hard" else (False, True)):
        want = c.pack_out(ref_demod(name, method, kind, per_symbol), c.g_off, c.tot["g"])
        for oo in {"f32": (0, 4), "f16": (0, 2, 6), "hard": (0, 1, 3)}[kind]:
            dst = T.Slot(want.size, oo)
            c.plan.demodulate(rx.data_ptr(), None if (method == "hard" or per_symbol) else c.d_pt.data_ptr(), dst.ptr, method=method,
                              d_variance=var.data_ptr() if per_symbol else None, out_dtype=F16 if kind == "f16" else F32)
            torch.cuda.synchronize()
            same_bytes(dst, want, (name, method, kind, per_symbol, oo))
    assert es * c.tot["g"] == want.size
    if kind == "hard":  # every output byte is 0 or 1, and the decisions are mostly the bits sent
        seg = [want[o: o + b] for o, b in zip(c.g_off, c.bits)]
        assert all(s.max(initial=0) <= 1 for s in seg)
        if name == "main":
            assert c.ps[6].Q_m == 2 and float((seg[6] != (c.g[6] & 1)).mean()) < 0.25  # (QPSK at 0 dB: Q(1) = 0.16)


# ---- 5. separate route against fused route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "tails"])
def test_separate_route_agrees_with_the_fused_route(name):
    """MixedChannel.step: mapper -> noise -> exact demapper against the fused kernel, |dLLR| <= 1e-3 * max(1, |LLR|): the bound
    include/nrldpc.h states for the single calls; and each route is the loop of its single calls."""
    import torch
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    c = ctx(name)
    chan = DC.MixedChannel(c.ps, c.n_tb)
    try:
        g = dev(c.g_packed)
        fused = chan.step(g, c.es, c.seeds, c.first).clone()
        sep = chan.step(g, c.es, c.seeds, c.first, separate=True)
        torch.cuda.synchronize()
        assert sep.dtype == fused.dtype == torch.float32 and sep.numel() == fused.numel() == c.tot["g"]
        fv, sv = chan.views(fused, "g"), chan.views(sep, "g")
        for i in range(c.n):
            a, b = fv[i].cpu().numpy().reshape(-1).astype(np.float64), sv[i].cpu().numpy().reshape(-1).astype(np.float64)
            if a.size:
                err = np.abs(a - b) / np.maximum(1.0, np.abs(a))
                print("%s configuration %d (Q_m %d): separate vs fused max |dLLR| / max(1, |LLR|) = %.3g" % (name, i, c.ps[i].Q_m, err.max()))
                assert err.max() <= 1e-3, (name, i, float(err.max()))
            assert (fv[i].cpu().numpy().reshape(-1).view(np.uint32) == ref_fused(name)[i].view(np.uint32)).all(), i
            assert (sv[i].cpu().numpy().reshape(-1).view(np.uint32) == ref_demod(name, "llr", "f32", False)[i].view(np.uint32)).all(), i
        # the other outputs of the separate route
        half = chan.step(g, c.es, c.seeds, c.first, separate=True, method="approx", llr_dtype=torch.float16)
        hard = chan.step(g, c.es, c.seeds, c.first, separate=True, method="hard")
        torch.cuda.synchronize()
        assert half.dtype == torch.float16 and hard.dtype == torch.uint8
        for i in range(c.n):
            assert (chan.views(half, "g")[i].cpu().numpy().reshape(-1).view(np.uint16) == ref_demod(name, "approx", "f16", False)[i].view(np.uint16)).all(), i
            assert (chan.views(hard, "g")[i].cpu().numpy().reshape(-1) == ref_demod(name, "hard", "hard", False)[i]).all(), i
    finally:
        chan.close()


# ---- 6. split invariance -----------------------------------------------------------------------------------------------------------------
def test_the_mix_split_into_two_plans_gives_the_bits_of_the_one_plan():
    """Configurations 0-4 and 5-8 as plans of their own, each with its own packed arrays and its share of the operating points: all
    four stages leave in every segment the bits the nine-configuration plan leaves."""
    import torch
    whole = ctx("main")
    fused, tx, rx, llr = ref_fused("main"), ref_tx("main"), ref_rx("main", False), ref_demod("main", "llr", "f32", False)
    for lo, hi in ((0, 5), (5, 9)):
        c = ctx("main", lo, hi)
        assert c.n == hi - lo and c.seeds == whole.seeds[lo:hi]
        g = [whole.g[i] for i in range(lo, hi)]
        gp = dev(c.pack_in(g, c.g_off, c.tot["g"], np.random.default_rng(5)))
        dst = T.Slot(4 * c.tot["g"], 0)
        c.plan.awgn_llr(gp.data_ptr(), c.d_pt.data_ptr(), dst.ptr)
        torch.cuda.synchronize()
        same_bytes(dst, c.pack_out(fused[lo:hi], c.g_off, c.tot["g"]), ("fused", lo))
        sym = T.Slot(8 * c.tot["sym"], 0)
        c.plan.modulate(gp.data_ptr(), sym.ptr)
        torch.cuda.synchronize()
        same_bytes(sym, c.pack_out(tx[lo:hi], c.sym_off, c.tot["sym"], per=2), ("mapper", lo))
        c.plan.awgn(sym.ptr, c.d_pt.data_ptr(), sym.ptr)
        torch.cuda.synchronize()
        same_bytes(sym, c.pack_out(rx[lo:hi], c.sym_off, c.tot["sym"], per=2), ("noise", lo))
        out = T.Slot(4 * c.tot["g"], 0)
        c.plan.demodulate(sym.ptr, c.d_pt.data_ptr(), out.ptr)
        torch.cuda.synchronize()
        same_bytes(out, c.pack_out(llr[lo:hi], c.g_off, c.tot["g"]), ("demapper", lo))


# ---- 7. the three mixed chains in a row --------------------------------------------------------------------------------------------------
def test_encode_channel_decode_equals_the_decode_of_loop_built_llrs():
    """MixedEncodeChain -> MixedChannel (fused) -> MixedDecodeChain: b_hat, ok and cb_pass equal those of the same decode chain fed
    with LLRs built by the per-configuration loop of nrldpc_awgn_llr_dev, and the packed g of the transmit chain IS the channel's input
    layout, the channel's output the receive chain's."""
    import torch
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    c = ctx("main")
    pkg = c.pkg
    es = [e + 6.0 for e in c.es]  # (a point at which most transport blocks decode: the comparison holds at any)
    txc, chan, rxc = DC.MixedEncodeChain(c.ps, c.n_tb, one_launch_encode=True), DC.MixedChannel(c.ps, c.n_tb), DC.MixedDecodeChain(c.ps, c.n_tb, iterations=10, I_HARQ=1)
    try:
        rng = np.random.default_rng(11)
        a = [dev(rng.integers(0, 2, (k, p.A), dtype=np.uint8)) for p, k in zip(c.ps, c.n_tb)]
        g = txc.step(txc.pack(a, "a"))
        assert g.numel() == chan.plan.totals()["g"] == rxc.plan.totals.g
        llr = chan.step(g, es, c.seeds, c.first)
        b_hat, ok, _ = rxc.step(llr)
        torch.cuda.synchronize()
        got = [x.clone() for x in (b_hat, ok, rxc.cb_pass)]
        loop = []
        for i, gv in enumerate(txc.views(g, "g")):
            o = torch.zeros(gv.shape, dtype=torch.float32, device="cuda")
            if gv.numel():
                pkg.awgn_llr_dev(gv.data_ptr(), gv.numel(), c.ps[i].Q_m, es[i], c.seeds[i], c.first[i], o.data_ptr())
            loop.append(o)
        torch.cuda.synchronize()
        packed = rxc.pack(loop, "g")
        assert bool((packed.view(torch.int32) == llr.view(torch.int32)).all())  # (gaps are zero on both sides)
        rxc.reset()  # (I_HARQ keeps cb_pass, the soft buffer and b_hat: the second step starts from nothing, as the first did)
        b_hat, ok, _ = rxc.step(packed)
        torch.cuda.synchronize()
        for x, y, what in zip(got, (b_hat, ok, rxc.cb_pass), ("b_hat", "ok", "cb_pass")):
            assert bool((x == y).all()), what
        okv = [v.cpu().numpy() for v in rxc.views(ok, "tb")]
        print("ok per configuration:", [v.tolist() for v in okv])
        assert sum(int((v != 0).sum()) for v in okv) >= 8  # the chain decodes: most of the 13 transport blocks pass
    finally:
        for x in (txc, chan, rxc):
            x.close()


def test_stage_calls_refuse_null_pointers_of_a_non_empty_plan():
    """Before any device call: a null base pointer of a non-empty array, a null d_pt where it is read."""
    c = ctx("tails")
    P = 0x1000
    for call in (lambda: c.plan.awgn_llr(None, P, P), lambda: c.plan.awgn_llr(P, None, P), lambda: c.plan.awgn_llr(P, P, None),
                 lambda: c.plan.modulate(None, P), lambda: c.plan.modulate(P, None),
                 lambda: c.plan.awgn(None, P, P), lambda: c.plan.awgn(P, None, P), lambda: c.plan.awgn(P, P, None), lambda: c.plan.awgn(P, None, P, d_variance=P),
                 lambda: c.plan.demodulate(None, P, P), lambda: c.plan.demodulate(P, None, P), lambda: c.plan.demodulate(P, P, None),
                 lambda: c.plan.demodulate(P, None, P, method="approx", out_dtype=F16), lambda: c.plan.demodulate(P, None, None, method="hard")):
        with pytest.raises(c.pkg.NRLDPCError, match="null"):
            call()
    assert ctypes.sizeof(c.pkg.MixChanPoint) * c.n == c.d_pt.numel()

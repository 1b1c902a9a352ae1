"""Mixed transport-block batches on the device, transmit side: nrldpc_mix_tx_crc_attach_dev, nrldpc_mix_tx_encode_dev and
nrldpc_mix_tx_rate_match_dev against the single-configuration calls (every comparison is bit for bit: integer arithmetic), the whole
MixedEncodeChain against the CPU oracle's transmit chain and against one DeviceEncodeChain per configuration, split invariance, one
plan shared by two streams, and the round trip through MixedDecodeChain.

The three plans (tests/test_mix_tx_api.py holds them to "every path of both kernels is reached", on the CPU):
  P9     the nine sets of tests/mix_cases.py with n_tb = (3, 1, 2, 0, 1, 2, 1, 1, 2): C = 1, 2, 3, a code block with E_r = 0, an empty
         configuration, Z = 20 and 384, every Q_m;
  P_rm   tests/tx_cases.py::RM_SETS as one plan, 3 transport blocks each: all 45 run classes and all 10 store forms of the rate-matching
         body at an aligned base;
  P_crc  tests/tx_cases.py::CRC_SETS with their counts (C = 1, 2, 3, 5, 9, both transport-block CRCs, 17 odd-length rows), run at
         the 16 pairs of CRC_OFFSETS on the two base pointers: all 324 attach classes of stage_row / store_row.

Every output array is pre-filled with 0xAA and has guards either side (tx_cases.Slot); gaps and guards must be unchanged after every
call.  Input bytes carry random bits 1..7, gaps included: only bit 0 of a byte may be read."""
import functools
import importlib

import numpy as np
import pytest

import mix_cases as M
import tx_cases as T

pytestmark = pytest.mark.gpu


class Plan:
    """One test plan: parameter objects, counts, the transmit plan, the per-field segment offsets and shapes."""

    def __init__(self, pkg, ps, n_tb):
        self.pkg, self.ps, self.n_tb = pkg, ps, list(n_tb)
        self.plan = pkg.MixTxPlan(ps, self.n_tb)
        self.tot = self.plan.totals()
        self.off = {"a": self.plan.a_off, "c": [o.c_hat for o in self.plan.off], "cw": [o.cw for o in self.plan.off], "g": [o.g for o in self.plan.off]}
        rx = pkg.mix_layout(ps, self.n_tb)
        assert all(getattr(x, f) == getattr(y, f) for x, y in zip(self.plan.off, rx) for f in pkg._capi.MIX_FIELDS)  # .off IS the receive layout
        assert [self.tot["c"], self.tot["cw"], self.tot["g"]] == [rx[-1].c_hat, rx[-1].cw, rx[-1].g]

    def shape(self, i, field):
        p, n = self.ps[i], self.n_tb[i]
        return {"a": (n, p.A), "c": (n * p.C, p.K), "cw": (n * p.C, 2 * p.Z_c + p.N), "g": (n, p.G)}[field]

    def size(self, i, field):
        return int(np.prod(self.shape(i, field), dtype=np.int64))

    def pack(self, field, arrays, rng=None):
        """numpy packed array: gaps random bytes (rng given: an input) or FILL (an expected output)."""
        n = self.tot[field]
        out = rng.integers(0, 256, n, dtype=np.uint8) if rng is not None else np.full(n, T.FILL, np.uint8)
        for i, x in enumerate(arrays):
            o = self.off[field][i]
            out[o:o + x.size] = x.reshape(-1)
        return out

    def segments(self, field, packed):
        return [packed[self.off[field][i]: self.off[field][i] + self.size(i, field)].reshape(self.shape(i, field)) for i in range(len(self.ps))]


@functools.lru_cache(maxsize=None)
def plan_of(name):
    pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
    if name == "P9":
        return Plan(pkg, M.mix(pkg), M.N_TB)
    sets = [(kw, T.RM_N_TB) for kw in T.RM_SETS] if name == "P_rm" else T.CRC_SETS
    ps = [pkg.NRLDPC(**kw) for kw, _ in sets]
    for p in ps:
        p.validate()
    return Plan(pkg, ps, [k for _, k in sets])


def garbage(rng, bits):
    """The same bits with bits 1..7 of every byte random: what a stage must read as `bits`."""
    return bits | (rng.integers(0, 128, bits.shape, dtype=np.uint8) << 1)


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()  # (a copy: `x` may be read-only)


def run_single(P, stage, inputs, codecs=None):
    """The single-configuration call of `stage` per configuration on tensors of their own -> one numpy array per configuration."""
    import torch
    out_field = {"attach": "c", "encode": "cw", "rm": "g"}[stage]
    outs = []
    for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
        o = torch.full((max(P.size(i, out_field), 1),), T.FILL, dtype=torch.uint8, device="cuda")
        if n:
            x = dev(inputs[i])
            if stage == "attach":
                P.pkg.crc_attach_dev(p, x.data_ptr(), n, o.data_ptr())
            elif stage == "encode":
                codecs[i].encode_dev(x.data_ptr(), n * p.C, o.data_ptr())
            else:
                P.pkg.rate_match_dev(p, x.data_ptr(), n, o.data_ptr() if p.G else None)
            torch.cuda.synchronize()
        outs.append(o[:P.size(i, out_field)].cpu().numpy().reshape(P.shape(i, out_field)))
    return outs


@functools.lru_cache(maxsize=None)
def attach_case(name):
    """(inputs per configuration with random upper bits, the packed input with random gaps, the expected packed c): computed once."""
    P = plan_of(name)
    rng = np.random.default_rng(100 + len(name))
    a = [garbage(rng, rng.integers(0, 2, P.shape(i, "a"), dtype=np.uint8)) for i in range(len(P.ps))]
    want = P.pack("c", run_single(P, "attach", a))
    packed = P.pack("a", a, rng)
    for x in (packed, want):
        x.setflags(write=False)
    return a, packed, want


def check_attach(name, ao, co):
    import torch
    P = plan_of(name)
    _, packed, want = attach_case(name)
    src, dst = T.Slot(packed.size, ao, packed), T.Slot(want.size, co)
    P.plan.crc_attach(src.ptr, dst.ptr)
    torch.cuda.synchronize()
    got = dst.data()
    assert (got == want).all(), (name, ao, co, np.argwhere(got != want)[:4].tolist())
    assert dst.guards_intact(), (name, ao, co)
    assert got[want != T.FILL].max() <= 1  # every output byte is 0 or 1


def test_crc_attach_equals_the_single_calls_on_the_nine_set_mix():
    check_attach("P9", 0, 0)
    a, _, want = attach_case("P9")
    P = plan_of("P9")
    # (the single calls themselves: payload bits in place, the filler tail zero)
    for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
        c = P.segments("c", want)[i].reshape(n, p.C, p.K)
        pay = int(p.K_prime) - p.code_block_L
        assert (c[:, :, int(p.K_prime):] == 0).all() and (c[:, 0, :min(pay, p.A)] == (a[i] & 1)[:, :min(pay, p.A)]).all(), i


@pytest.mark.parametrize("ao", T.CRC_OFFSETS)
def test_crc_attach_equals_the_single_calls_at_every_alignment(ao):
    """P_crc with the two base pointers at the 16 pairs of CRC_OFFSETS: every (source phase, destination phase, rotation) of a staged
    and stored row, C = 1, 2, 3, 5, 9 under a plan-wide count of four waves (a workgroup of C = 1 leaves three waves idle at the
    barrier; C = 9 takes three rounds), both transport-block CRCs."""
    P = plan_of("P_crc")
    assert sorted({p.C for p in P.ps}) == [1, 2, 3, 5, 9] and {p.transport_block_L for p in P.ps} == {16, 24}
    for co in T.CRC_OFFSETS:
        check_attach("P_crc", ao, co)


@functools.lru_cache(maxsize=None)
def rm_case(name):
    P = plan_of(name)
    rng = np.random.default_rng(200 + len(name))
    cw = []
    for i, p in enumerate(P.ps):
        x = rng.integers(0, 2, P.shape(i, "cw"), dtype=np.uint8)
        # the punctured 2Z prefix and every filler position of d at 1: the reference reads neither, so a gather that lands on one shows
        x[:, :2 * p.Z_c] = 1
        x[:, 2 * p.Z_c + max(int(p.K_prime) - 2 * p.Z_c, 0):p.K] = 1
        cw.append(garbage(rng, x))
    want = P.pack("g", run_single(P, "rm", cw))
    packed = P.pack("cw", cw, rng)
    for x in (packed, want):
        x.setflags(write=False)
    return cw, packed, want


@pytest.mark.parametrize("name", ["P9", "P_rm"])
def test_rate_match_equals_the_single_calls(orc, name):
    import torch
    P = plan_of(name)
    cw, packed, want = rm_case(name)
    for base in (0, 3):
        src, dst = T.Slot(packed.size, base, packed), T.Slot(want.size, base)
        P.plan.rate_match(src.ptr, dst.ptr)
        torch.cuda.synchronize()
        got = dst.data()
        assert (got == want).all(), (name, base, np.argwhere(got != want)[:4].tolist())
        assert dst.guards_intact(), (name, base)
        assert got[want != T.FILL].max() <= 1
    # (the single calls themselves, against the literal loops of the oracle, on the smallest and the largest set of the plan)
    for i in (0, len(P.ps) - 1):
        p, n = P.ps[i], P.n_tb[i]
        if n:
            ref = orc.rate_match(p.Z_c, p.C, p.K, int(p.K_prime), p.N, p.N_cb, p.k_0, p.Q_m, p.G, list(p.E_r), cw[i] & 1)
            assert (P.segments("g", want)[i] == ref).all(), (name, i)


@functools.lru_cache(maxsize=None)
def codecs_of(name):
    P = plan_of(name)
    made = {}
    out = []
    for p, n in zip(P.ps, P.n_tb):
        if n and (p.BG, p.Z_c) not in made:
            made[(p.BG, p.Z_c)] = P.pkg.Codec(p.BG, p.Z_c, max_iter=1)
        out.append(made[(p.BG, p.Z_c)] if n else None)
    return out


def test_encode_stage_equals_encode_dev_and_refuses_wrong_handles():
    import torch
    P = plan_of("P9")
    pkg = P.pkg
    codecs = codecs_of("P9")
    assert len({id(c) for c in codecs if c is not None}) < sum(1 for c in codecs if c is not None)  # handles repeat for a shared (BG, Z_c)
    rng = np.random.default_rng(300)
    c = [garbage(rng, rng.integers(0, 2, P.shape(i, "c"), dtype=np.uint8)) for i in range(len(P.ps))]
    want = P.pack("cw", run_single(P, "encode", c, codecs))
    packed = P.pack("c", c, rng)
    src, dst = T.Slot(packed.size, 0, packed), T.Slot(want.size, 0)
    P.plan.encode(codecs, src.ptr, dst.ptr)
    torch.cuda.synchronize()
    got = dst.data()
    assert (got == want).all() and dst.guards_intact()
    # refusals, before any launch: the output stays as it was
    dst = T.Slot(want.size, 0)
    wrong = list(codecs)
    i = next(k for k, p in enumerate(P.ps) if (p.BG, p.Z_c) != (P.ps[0].BG, P.ps[0].Z_c) and P.n_tb[k])
    wrong[i] = codecs[0]
    with pytest.raises(pkg.NRLDPCError, match=r"\(BG, Z\).*\(configuration %d\)" % i):
        P.plan.encode(wrong, src.ptr, dst.ptr)
    wrong = list(codecs)
    wrong[4] = None
    with pytest.raises(pkg.NRLDPCError, match=r"null handle \(configuration 4\)"):
        P.plan.encode(wrong, src.ptr, dst.ptr)
    torch.cuda.synchronize()
    assert (dst.whole() == T.FILL).all()
    empty = P.n_tb.index(0)
    ok = list(codecs)
    ok[empty] = None  # the handle of an empty configuration is not read
    P.plan.encode(ok, src.ptr, dst.ptr)
    torch.cuda.synchronize()
    assert (dst.data() == want).all()


def test_null_base_pointers_of_non_empty_arrays_are_refused():
    P = plan_of("P9")
    pkg = P.pkg
    for call, args in ((P.plan.crc_attach, (None, 0x1000)), (P.plan.crc_attach, (0x1000, None)), (P.plan.rate_match, (None, 0x1000)),
                       (P.plan.rate_match, (0x1000, None))):
        with pytest.raises(pkg.NRLDPCError, match="null pointer"):
            call(*args)
    for args in ((None, 0x1000), (0x1000, None)):
        with pytest.raises(pkg.NRLDPCError, match="null pointer"):
            P.plan.encode(codecs_of("P9"), *args)


# ---- the whole chain ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_run():
    """Payloads of P9 and what MixedEncodeChain.step makes of them (numpy, per configuration): computed once."""
    import torch
    P = plan_of("P9")
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    rng = np.random.default_rng(51)
    a = [rng.integers(0, 2, P.shape(i, "a"), dtype=np.uint8) for i in range(len(P.ps))]
    chain = DC.MixedEncodeChain(P.ps, P.n_tb)
    try:
        g = chain.step(chain.pack([dev(x) for x in a], "a"))
        torch.cuda.synchronize()
        packed = g.cpu().numpy().copy()
        views = [v.cpu().numpy().copy() for v in chain.views(g, "g")]
        with pytest.raises(P.pkg.NRLDPCError, match="at least"):
            chain.step(torch.zeros(P.tot["a"] - 1, dtype=torch.uint8, device="cuda"))
        with pytest.raises(P.pkg.NRLDPCError, match="uint8"):
            chain.step(torch.zeros(P.tot["a"], dtype=torch.int32, device="cuda"))
    finally:
        chain.close()
    packed.setflags(write=False)
    return a, packed, views


def test_chain_gives_the_oracles_transmit_chain(orc):
    """MixedEncodeChain.step on P9 against the CPU oracle per transport block -- the bit-serial CRC construction of
    NRLDPCEncoder.m:70-124, the oracle's encoder and the literal rate-matching loops; no code shared with the product."""
    P = plan_of("P9")
    a, packed, views = chain_run()
    assert packed.size == P.tot["g"] and packed.max() <= 1
    for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
        if not n:
            assert views[i].shape == (0, p.G)
            continue
        L = p.transport_block_L
        tb_poly = 0x1864CFB if L == 24 else 0x11021
        pay = int(p.K_prime) - p.code_block_L
        c = np.zeros((n, p.C, p.K), np.uint8)
        for t in range(n):
            crc = orc.crc(tb_poly, L, a[i][t])
            b = np.concatenate([a[i][t], [(crc >> (L - 1 - k)) & 1 for k in range(L)]]).astype(np.uint8)
            for r in range(p.C):
                c[t, r, :pay] = b[r * pay:(r + 1) * pay]
                if p.code_block_L:
                    cb = orc.crc(0x1800063, 24, c[t, r, :pay])
                    c[t, r, pay:int(p.K_prime)] = [(cb >> (23 - k)) & 1 for k in range(24)]
        cw = orc.encode(p.BG, p.Z_c, c.reshape(n * p.C, p.K))
        want = orc.rate_match(p.Z_c, p.C, p.K, int(p.K_prime), p.N, p.N_cb, p.k_0, p.Q_m, p.G, list(p.E_r), cw)
        assert (views[i] == want).all(), (i, np.argwhere(views[i] != want)[:4].tolist())


def test_chain_equals_one_device_encode_chain_per_configuration():
    import torch
    P = plan_of("P9")
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    a, _, views = chain_run()
    for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
        if not n:
            continue
        one = DC.DeviceEncodeChain(p)
        try:
            want = one.step(dev(a[i])).cpu().numpy()
        finally:
            one.close()
        assert (views[i] == want).all(), i


def run_stages(P, plans, a_packed, streams=None):
    """attach, encode, rate matching through `plans` = [(plan, first configuration, codecs)] over ONE set of packed arrays; returns the
    three output slots."""
    import torch
    s_a = T.Slot(a_packed.size, 0, a_packed)
    s_c, s_cw, s_g = T.Slot(P.tot["c"], 0), T.Slot(P.tot["cw"], 0), T.Slot(P.tot["g"], 0)
    stream = streams.cuda_stream if streams is not None else 0
    for plan, first, codecs in plans:
        plan.crc_attach(s_a.ptr + P.off["a"][first], s_c.ptr + P.off["c"][first], stream=stream)
        plan.encode(codecs, s_c.ptr + P.off["c"][first], s_cw.ptr + P.off["cw"][first], stream=stream)
        plan.rate_match(s_cw.ptr + P.off["cw"][first], s_g.ptr + P.off["g"][first], stream=stream)
    return s_a, s_c, s_cw, s_g


def test_results_do_not_depend_on_how_the_mix_is_split_into_plans():
    import torch
    P = plan_of("P9")
    codecs = codecs_of("P9")
    _, a_packed, _ = attach_case("P9")
    whole = run_stages(P, [(P.plan, 0, codecs)], a_packed)
    torch.cuda.synchronize()
    cut = 5
    left, right = P.pkg.MixTxPlan(P.ps[:cut], P.n_tb[:cut]), P.pkg.MixTxPlan(P.ps[cut:], P.n_tb[cut:])
    try:
        split = run_stages(P, [(left, 0, codecs[:cut]), (right, cut, codecs[cut:])], a_packed)
        torch.cuda.synchronize()
    finally:
        left.close()
        right.close()
    for x, y in zip(whole[1:], split[1:]):
        assert (x.whole() == y.whole()).all() and x.guards_intact() and y.guards_intact()
    # (what was compared is the real thing: the code blocks are the attach test's, and the chained stages reached g)
    assert (whole[1].data() == attach_case("P9")[2]).all()
    assert all(v.max() <= 1 and v.any() for v in P.segments("g", whole[3].data()) if v.size)


def test_one_plan_shared_by_two_streams():
    import torch
    P = plan_of("P9")
    codecs = codecs_of("P9")
    rng = np.random.default_rng(77)
    data = [P.pack("a", [garbage(rng, rng.integers(0, 2, P.shape(i, "a"), dtype=np.uint8)) for i in range(len(P.ps))], rng) for _ in range(2)]
    ref = []
    for d in data:
        ref.append(run_stages(P, [(P.plan, 0, codecs)], d))
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = [run_stages(P, [(P.plan, 0, codecs)], d, s) for d, s in zip(data, streams)]  # both in flight, no synchronisation between
    for s in streams:
        s.synchronize()
    for r, x in zip(ref, got):
        for u, v in zip(r[1:], x[1:]):
            assert (u.whole() == v.whole()).all() and v.guards_intact()
    assert not (ref[0][3].data() == ref[1][3].data()).all()  # (the two streams did work on different data)


def test_round_trip_through_the_mixed_decode_chain():
    """g -> noiseless LLRs (1 - 2g) * 8 over the PACKED array -> MixedDecodeChain.step: the transmit plan's g is the receive plan's
    g_tilde layout.  a_hat == a and ok == 1 for every transport block whose configuration transmits all its code blocks; ok, b_hat and
    iters equal one DeviceDecodeChain per configuration everywhere (the E_r = 0 configuration fails its third block on both sides)."""
    import torch
    P = plan_of("P9")
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    a, packed, _ = chain_run()
    llr = (1.0 - 2.0 * dev(packed).to(torch.float32)) * 8.0
    kw = dict(iterations=20)
    rx = DC.MixedDecodeChain(P.ps, P.n_tb, **kw)
    try:
        assert rx.plan.totals.g == P.tot["g"] == llr.numel()
        b_hat, ok, iters = rx.step(llr)
        torch.cuda.synchronize()
        seen_failed = False
        for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
            if not n:
                continue
            okv = rx.views(ok, "tb")[i].cpu().numpy()
            bv = rx.views(b_hat, "b_hat")[i].cpu().numpy()
            if all(e > 0 for e in p.E_r):
                assert (okv == 1).all() and (bv[:, :p.A] == a[i]).all(), i
            else:
                assert list(p.E_r).index(0) == p.C - 1 and (okv == 0).all(), i
                seen_failed = True
            one = DC.DeviceDecodeChain(p, **kw)
            try:
                a_ref, ok_ref, it_ref = one.step(rx.views(llr, "g")[i].contiguous())
                torch.cuda.synchronize()
                assert ((okv != 0) == ok_ref.cpu().numpy()).all() and (bv == one.b_hat.cpu().numpy()).all(), i
                assert bool((rx.views(iters, "cb")[i] == it_ref).all()), i
            finally:
                one.close()
        assert seen_failed
    finally:
        rx.close()

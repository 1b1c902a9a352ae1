"""The one-launch mixed encoder on the device: MixTxPlan.encode_all (nrldpc_mix_tx_encode_all_dev) against one encode_dev per
configuration, against the per-configuration stage call plan.encode and against the CPU oracle's encoder -- every comparison is bit
for bit --, split invariance, one plan shared by two streams, and MixedEncodeChain(one_launch_encode=True) against the default chain
and through MixedDecodeChain.

The two plans (tests/test_mix_tx_encode_api.py holds P_enc to "every class of the encoder body is reached", on the CPU):
  P9     the nine sets of tests/mix_cases.py with n_tb = (3, 1, 2, 0, 1, 2, 1, 1, 2): C up to 3, an empty configuration, two
         configurations that share a (BG, Z) and its table, Z = 20 and 384;
  P_enc  tests/mix_tx_enc_cases.py: one C = 1 configuration per (BG, Z) of tx_cases.ENC_SIZES, ragged last workgroups, the one-wave and
         the workgroup-per-codeword body alternating, run at the seven ENC_OFFSETS pairs of the two base pointers.

Every output array is pre-filled with 0xAA and has guards either side (tx_cases.Slot); gaps and guards must be unchanged after every
call, and so must the input."""
import functools
import importlib

import numpy as np
import pytest

import mix_cases as M
import mix_tx_enc_cases as E
import tx_cases as T

pytestmark = pytest.mark.gpu


class Plan:
    """One test plan: parameter objects, counts, the transmit plan, segment offsets and shapes of the code blocks and the codewords."""

    def __init__(self, pkg, ps, n_tb):
        self.pkg, self.ps, self.n_tb = pkg, ps, list(n_tb)
        self.plan = pkg.MixTxPlan(ps, self.n_tb)
        self.tot = self.plan.totals()
        self.off = {"a": self.plan.a_off, "c": [o.c_hat for o in self.plan.off], "cw": [o.cw for o in self.plan.off], "g": [o.g for o in self.plan.off]}

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
    return Plan(pkg, *E.p_enc(pkg))


@functools.lru_cache(maxsize=None)
def codecs_of(name):
    P = plan_of(name)
    made, out = {}, []
    for p, n in zip(P.ps, P.n_tb):
        if n and (p.BG, p.Z_c) not in made:
            made[(p.BG, p.Z_c)] = P.pkg.Codec(p.BG, p.Z_c, max_iter=1)
        out.append(made[(p.BG, p.Z_c)] if n else None)
    return out


def garbage(rng, bits):
    """The same bits with bits 1..7 of every byte random: what the stage must read as `bits`."""
    return bits | (rng.integers(0, 128, bits.shape, dtype=np.uint8) << 1)


def dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()  # (a copy: `x` may be read-only)


@functools.lru_cache(maxsize=None)
def case(name):
    """(code blocks per configuration, the packed input with random gaps, the same with random bits 1..7, the expected packed cw from
    one encode_dev per configuration on tensors of their own): computed once, read-only."""
    import torch
    P = plan_of(name)
    codecs = codecs_of(name)
    rng = np.random.default_rng(400 + len(name))
    c = [rng.integers(0, 2, P.shape(i, "c"), dtype=np.uint8) for i in range(len(P.ps))]
    outs = []
    for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
        o = torch.full((max(P.size(i, "cw"), 1),), T.FILL, dtype=torch.uint8, device="cuda")
        if n:
            x = dev(c[i])
            codecs[i].encode_dev(x.data_ptr(), n * p.C, o.data_ptr())
            torch.cuda.synchronize()
        outs.append(o[:P.size(i, "cw")].cpu().numpy().reshape(P.shape(i, "cw")))
    want = P.pack("cw", outs)
    packed = P.pack("c", c, rng)
    dirty = P.pack("c", [garbage(rng, x) for x in c], rng)
    for x in (packed, dirty, want):
        x.setflags(write=False)
    return c, packed, dirty, want


def check_encode_all(name, io, oo, packed, loop=True):
    """encode_all at base offsets (io, oo): equal to `want`, guards and gaps untouched, the input unchanged, bytes 0 or 1; with
    `loop`, the per-configuration stage call at the same addresses gives the same."""
    import torch
    P = plan_of(name)
    want = case(name)[3]
    src, dst = T.Slot(packed.size, io, packed), T.Slot(want.size, oo)
    before = src.whole()
    P.plan.encode_all(src.ptr, dst.ptr)
    torch.cuda.synchronize()
    got = dst.data()
    assert (got == want).all(), (name, io, oo, np.argwhere(got != want)[:4].tolist())
    assert dst.guards_intact() and (src.whole() == before).all(), (name, io, oo)
    assert got[want != T.FILL].max() <= 1  # every output byte is 0 or 1 (gap bytes are still FILL: equal to `want` above)
    if loop:
        dst2 = T.Slot(want.size, oo)
        P.plan.encode(codecs_of(name), src.ptr, dst2.ptr)
        torch.cuda.synchronize()
        assert (dst2.whole() == dst.whole()).all(), (name, io, oo)


def test_p9_equals_the_single_calls_and_the_per_configuration_stage():
    P = plan_of("P9")
    shared = [(p.BG, p.Z_c) for p, n in zip(P.ps, P.n_tb) if n]
    assert len(set(shared)) < len(shared) and 0 in P.n_tb and max(p.C for p in P.ps) == 3
    check_encode_all("P9", 0, 0, case("P9")[1])


def test_p9_reads_only_bit_0_of_an_input_byte():
    P = plan_of("P9")
    c, _, dirty, _ = case("P9")
    assert all(((x & 1) == y).all() and (x > 1).any() for x, y in zip(P.segments("c", dirty), c) if y.size)
    check_encode_all("P9", 0, 0, dirty)


@pytest.mark.parametrize("io,oo", T.ENC_OFFSETS)
def test_p_enc_equals_the_single_calls_at_every_alignment(io, oo):
    """All 48 classes of the encoder body between the seven pairs; the one-wave and the workgroup-per-codeword configurations alternate,
    so the launch carries both bodies under a plan-wide LDS size."""
    P = plan_of("P_enc")
    nwc = [T.enc_nwc(p.BG, p.Z_c) for p in P.ps]
    assert {1, 4} == set(nwc) and all(nwc[i - 1] == 1 == nwc[i + 1] for i, w in enumerate(nwc) if w == 4)
    _, _, dirty, want = case("P_enc")
    assert (want == T.FILL).any() and (want != T.FILL).any()  # (the codeword array of this plan has gaps, and they are compared)
    check_encode_all("P_enc", io, oo, dirty)  # (the input with random bits 1..7)


def test_p_enc_equals_the_oracle_and_satisfies_every_check(orc):
    """The single calls the other tests compare with, against the CPU oracle's encoder (no code shared with the product), and H cw = 0
    on the first and last codeword of every configuration -- of what encode_all itself left."""
    import torch
    P = plan_of("P_enc")
    c, packed, _, want = case("P_enc")
    src, dst = T.Slot(packed.size, 0, packed), T.Slot(want.size, 0)
    P.plan.encode_all(src.ptr, dst.ptr)
    torch.cuda.synchronize()
    got = P.segments("cw", dst.data())
    for i, p in enumerate(P.ps):
        assert (got[i] == orc.encode(p.BG, p.Z_c, c[i])).all(), i
        for k in (0, got[i].shape[0] - 1):
            assert orc.syndrome_weight(p.BG, p.Z_c, got[i][k]) == 0, (i, k)
            assert got[i][k].any()


def run_encode_all(P, plans, packed, stream=None):
    src, dst = T.Slot(packed.size, 0, packed), T.Slot(P.tot["cw"], 0)
    for plan, first in plans:
        plan.encode_all(src.ptr + P.off["c"][first], dst.ptr + P.off["cw"][first], stream=stream.cuda_stream if stream is not None else 0)
    return src, dst


def test_results_do_not_depend_on_how_the_mix_is_split_into_plans():
    import torch
    P = plan_of("P9")
    _, packed, _, want = case("P9")
    cut = 5
    left, right = P.pkg.MixTxPlan(P.ps[:cut], P.n_tb[:cut]), P.pkg.MixTxPlan(P.ps[cut:], P.n_tb[cut:])
    try:
        _, dst = run_encode_all(P, [(left, 0), (right, cut)], packed)
        torch.cuda.synchronize()
    finally:
        left.close()
        right.close()
    assert (dst.data() == want).all() and dst.guards_intact()


def test_one_plan_shared_by_two_streams():
    import torch
    P = plan_of("P9")
    _, packed, dirty, want = case("P9")
    rng = np.random.default_rng(78)
    other = packed.copy()
    for i in range(len(P.ps)):  # other code blocks in the same layout
        o, n = P.off["c"][i], P.size(i, "c")
        other[o:o + n] = rng.integers(0, 2, n, dtype=np.uint8)
    _, ref = run_encode_all(P, [(P.plan, 0)], other)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got = [run_encode_all(P, [(P.plan, 0)], d, s) for d, s in zip((dirty, other), streams)]  # both in flight, no synchronisation between
    for s in streams:
        s.synchronize()
    assert (got[0][1].data() == want).all() and (got[1][1].whole() == ref.whole()).all()
    assert all(dst.guards_intact() for _, dst in got) and not (ref.data() == want).all()  # (the two streams did work on different data)


def test_null_base_pointers_of_non_empty_arrays_are_refused():
    P = plan_of("P9")
    for args in ((None, 0x1000), (0x1000, None)):
        with pytest.raises(P.pkg.NRLDPCError, match="null pointer"):
            P.plan.encode_all(*args)


def test_one_launch_chain_equals_the_default_chain_and_round_trips():
    """MixedEncodeChain(one_launch_encode=True).step(a) == the default chain's g (and it built no Codec); g -> noiseless LLRs ->
    MixedDecodeChain returns the payload of every transport block whose configuration transmits all its code blocks."""
    import torch
    P = plan_of("P9")
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    rng = np.random.default_rng(52)
    a = [rng.integers(0, 2, P.shape(i, "a"), dtype=np.uint8) for i in range(len(P.ps))]
    g = []
    for one in (False, True):
        chain = DC.MixedEncodeChain(P.ps, P.n_tb, one_launch_encode=one)
        try:
            assert all(c is None for c in chain.codecs) == one and bool(chain._codecs) != one
            out = chain.step(chain.pack([dev(x) for x in a], "a"))
            torch.cuda.synchronize()
            g.append(out.cpu().numpy().copy())
        finally:
            chain.close()
    assert g[0].size == P.tot["g"] and (g[0] == g[1]).all() and g[1].max() <= 1
    llr = (1.0 - 2.0 * dev(g[1]).to(torch.float32)) * 8.0
    rx = DC.MixedDecodeChain(P.ps, P.n_tb, iterations=20)
    try:
        b_hat, ok, _ = rx.step(llr)
        torch.cuda.synchronize()
        checked = 0
        for i, (p, n) in enumerate(zip(P.ps, P.n_tb)):
            if n and all(e > 0 for e in p.E_r):
                assert (rx.views(ok, "tb")[i].cpu().numpy() == 1).all(), i
                assert (rx.views(b_hat, "b_hat")[i].cpu().numpy()[:, :p.A] == a[i]).all(), i
                checked += 1
        assert checked >= 7
    finally:
        rx.close()

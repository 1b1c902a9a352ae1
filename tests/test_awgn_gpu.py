"""The stand-alone AWGN stage (nrldpc_awgn_dev, csrc/nrldpc_awgn.hip) on the GPU.

References (none of them under test): oracle/channel_oracle.py:noise, the float64 definition of the library's noise; numpy float32
addition; the fused kernel nrldpc_awgn_llr_dev for the three-stage leg.  Sizes: n_sym in 1, 2, 3, 63, 64, 65, 257, 513 -- around one
thread's pair, one wave, one workgroup and two -- at first_symbol 0, 1 (an odd start: the first thread holds one symbol), 2^33 - 1 (the
Philox counter's carry into its high word falls inside a 3-symbol call) and 3 * 2^40 + 12345 (the harness's attempt stride), with
every device pointer at the start of its allocation and one symbol into it (8-byte but not 16-byte aligned), and 20011 symbols (more
than one workgroup, odd) wherever the operating points of tests/test_modem_gpu.py are used.
"""
import importlib

import numpy as np
import pytest

import test_modem_gpu as TM
from test_modem_gpu import FIRST, N_BIG, POINTS, SEED

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 257, 513)
FIRSTS = (0, 1, (1 << 33) - 1, 3 * (1 << 40) + 12345)
VARIANCES = (1.0, 1e-3, 10.0 ** 0.2)
# test_noise_matches_the_definition: largest |d| / sqrt(N0) per component measured on the MI355X over its cases, and the asserted bound,
# 8 times that (the margin is for seeds and counters the test does not visit).  The bound may not exceed 1e-4: the LLR tolerance
# 5e-4 * max(1, |LLR|) allows dy = 1.77e-4 * sqrt(N0) at QPSK 0 dB, and the three-stage leg has to stay inside it.
NOISE_MEASURED = 2.609e-6
NOISE_BOUND = 8 * NOISE_MEASURED
assert NOISE_BOUND <= 1e-4


def H():
    return importlib.import_module("ldpc-3gpp-matlab_amd.harness")


def bits_of(x):
    return np.ascontiguousarray(x).view(np.uint32)


def dev_awgn(pkg, tx, N0, seed, first, var=None, offset=0, in_place=False):
    """nrldpc_awgn_dev on tx (numpy complex64), every device pointer `offset` symbols into its allocation; guard symbols either side."""
    import torch
    n = tx.size
    d_tx = torch.full((2 * (n + offset + 1),), 77.0, dtype=torch.float32, device="cuda")
    d_tx[2 * offset:2 * (offset + n)] = torch.from_numpy(np.array(tx).view(np.float32)).cuda()  # (a copy: shared inputs are read-only)
    d_rx = d_tx if in_place else torch.full((2 * (n + offset + 1),), 77.0, dtype=torch.float32, device="cuda")
    d_var = None
    if var is not None:
        d_var = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
        d_var[offset:] = torch.from_numpy(np.array(var, np.float32)).cuda()
    pkg.awgn_dev(d_tx.data_ptr() + 8 * offset, n, d_rx.data_ptr() + 8 * offset, variance=N0,
                 d_variance=None if d_var is None else d_var.data_ptr() + 4 * offset, seed=seed, first_symbol=first)
    torch.cuda.synchronize()
    out = d_rx.cpu().numpy()
    assert (out[:2 * offset] == 77).all() and (out[2 * (offset + n):] == 77).all(), "wrote outside [offset, offset + n)"
    if not in_place:
        assert (bits_of(d_tx.cpu().numpy()[2 * offset:2 * (offset + n)]) == bits_of(np.array(tx).view(np.float32))).all(), "wrote to tx"
    return out[2 * offset:2 * (offset + n)].view(np.complex64)


@pytest.mark.parametrize("N0", VARIANCES)
def test_noise_matches_the_definition(pkg, N0):
    """tx = 0, so rx is the noise: each component against channel_oracle.noise (float64), every size, first_symbol and pointer offset
    above at each variance, and 20011 symbols at test_modem_gpu's (SEED, FIRST).  Measured on the MI355X: max |d| / sqrt(N0) = 2.609e-6
    over the three variances (NOISE_MEASURED); asserted: 8 times that, 2.087e-5 (NOISE_BOUND, at most 1e-4)."""
    import channel_oracle as CO
    worst = 0.0
    cases = [(n, first, off, 0xC0DE) for n in SIZES for first in FIRSTS for off in (0, 1)] + [(N_BIG, FIRST, 0, SEED)]
    for n, first, off, seed in cases:
        got = dev_awgn(pkg, np.zeros(n, np.complex64), N0, seed, first, offset=off).astype(np.complex128)
        ref = CO.noise(n, seed, first, float(np.float32(N0)))  # (the variance as the kernel receives it: f32)
        err = max(float(np.abs(got.real - ref.real).max()), float(np.abs(got.imag - ref.imag).max())) / np.sqrt(N0)
        worst = max(worst, err)
        assert err <= NOISE_BOUND, (n, first, off, N0, err)
    print("awgn noise vs definition: max |d| / sqrt(N0) = %.4g (bound %.4g)" % (worst, NOISE_BOUND))


@pytest.mark.parametrize("Q_m,esn0", POINTS)
def test_the_add_is_one_f32_add(pkg, Q_m, esn0):
    """awgn(tx) == tx + awgn(0) bit for bit, the right-hand side a numpy float32 add of the kernel's own zero-input output."""
    p = TM.point(Q_m, esn0)
    tx = TM.dev_mod(pkg, p["g"], Q_m)
    for off in (0, 1):
        w = dev_awgn(pkg, np.zeros(N_BIG, np.complex64), p["N0"], SEED, FIRST + off, offset=off)
        rx = dev_awgn(pkg, tx, p["N0"], SEED, FIRST + off, offset=off)
        want = tx.view(np.float32) + w.view(np.float32)
        assert want.dtype == np.float32 and (bits_of(rx.view(np.float32)) == bits_of(want)).all(), off


@pytest.mark.parametrize("off", [0, 1])
def test_bit_exact_identities(pkg, off):
    """Split at 256 and at 257 (even and odd first_symbol) == one call; in place == out of place; a variance array filled with N0 ==
    the scalar; two variances on the two halves == two scalar calls; variance 0 gives rx == tx."""
    p = TM.point(4, 8.0)
    n = 513
    tx = TM.dev_mod(pkg, p["g"][:n * 4], 4)
    N0a, N0b = VARIANCES[2], VARIANCES[1]
    for first in FIRSTS:
        whole = dev_awgn(pkg, tx, N0a, SEED, first, offset=off)
        for cut in (256, 257):
            parts = np.concatenate([dev_awgn(pkg, tx[:cut], N0a, SEED, first, offset=off),
                                    dev_awgn(pkg, tx[cut:], N0a, SEED, first + cut, offset=off)])
            assert (bits_of(parts) == bits_of(whole)).all(), (first, cut)
            two = dev_awgn(pkg, tx, 123.0, SEED, first, var=np.where(np.arange(n) < cut, N0a, N0b), offset=off)
            ref = np.concatenate([whole[:cut], dev_awgn(pkg, tx[cut:], N0b, SEED, first + cut, offset=off)])
            assert (bits_of(two) == bits_of(ref)).all(), (first, cut)
        assert (bits_of(dev_awgn(pkg, tx, N0a, SEED, first, offset=off, in_place=True)) == bits_of(whole)).all(), first
        filled = dev_awgn(pkg, tx, 123.0, SEED, first, var=np.full(n, N0a), offset=off)
        assert (bits_of(filled) == bits_of(whole)).all(), first
        assert (bits_of(dev_awgn(pkg, tx, 123.0, SEED, first, var=np.full(n, N0a), offset=off, in_place=True)) == bits_of(whole)).all(), first
        assert (dev_awgn(pkg, tx, 0.0, SEED, first, offset=off) == tx).all(), first
    for m in (1, 2, 3, 63, 64, 65, 257):  # the small sizes in place, at an odd start
        a = dev_awgn(pkg, tx[:m], N0a, SEED, 1, offset=off)
        assert (bits_of(dev_awgn(pkg, tx[:m], N0a, SEED, 1, offset=off, in_place=True)) == bits_of(a)).all(), m
        assert (bits_of(a) == bits_of(dev_awgn(pkg, tx, N0a, SEED, 1, offset=off)[:m])).all(), m


@pytest.mark.parametrize("Q_m,esn0", POINTS)
def test_three_stages_agree_with_the_fused_kernel(pkg, Q_m, esn0):
    """demodulate_dev(awgn_dev(modulate_dev(g)), exact, variance = N0) against awgn_llr_dev(g) on the same (seed, first_symbol):
    |d| <= 1e-3 * max(1, |LLR|), the pairwise form of the 5e-4 rule.  20011 symbols at (SEED, FIRST), the small sizes at an odd
    first_symbol and both pointer offsets."""
    import torch
    p = TM.point(Q_m, esn0)
    worst = 0.0
    for n, off, first in [(N_BIG, 0, FIRST)] + [(n, off, FIRST + 1) for n in SIZES for off in (1, 0)]:
        g = p["g"][:n * Q_m]
        rx = dev_awgn(pkg, TM.dev_mod(pkg, g, Q_m, off), p["N0"], SEED, first, offset=off)
        got = TM.dev_demod(pkg, rx, Q_m, "llr", p["N0"], offset=off).astype(np.float64)
        d_g = torch.from_numpy(g.copy()).cuda()
        fused = torch.empty(n * Q_m, dtype=torch.float32, device="cuda")
        pkg.awgn_llr_dev(d_g.data_ptr(), g.size, Q_m, esn0, SEED, first, fused.data_ptr())
        torch.cuda.synchronize()
        ref = fused.cpu().numpy().astype(np.float64)
        rel = np.abs(got - ref) / (1e-3 * np.maximum(1.0, np.abs(ref)))
        worst = max(worst, float(rel.max()))
        assert np.isfinite(got).all() and (rel <= 1.0).all(), (n, off, float(rel.max()))
    print("three stages vs fused Q_m=%d %g dB: max error = %.4g of the tolerance" % (Q_m, esn0, worst))


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


@pytest.mark.parametrize("seed,first", [(0xC0DE, 0), (0xC0DE, (1 << 33) - 1), (7, 3 * (1 << 40) + 12345)])
def test_statistics(pkg, seed, first):
    """2^18 symbols at N0 = 1: means, variances (0.5 per rail) and correlations within 4 standard errors -- sqrt(0.5/n) for a mean,
    0.5 sqrt(2/n) for a variance, 1/sqrt(m) for a correlation over m pairs.  (The float64 definition alone stays within 2.9.)"""
    n = 1 << 18
    w = dev_awgn(pkg, np.zeros(n, np.complex64), 1.0, seed, first).astype(np.complex128)
    re, im = w.real, w.imag
    for name, x in (("re", re), ("im", im)):
        assert abs(x.mean()) <= 4 * np.sqrt(0.5 / n), (name, x.mean())
        assert abs(x.var() - 0.5) <= 4 * 0.5 * np.sqrt(2.0 / n), (name, x.var())
    assert abs(corr(re, im)) <= 4 / np.sqrt(n)
    assert abs(corr(re[:-1], re[1:])) <= 4 / np.sqrt(n - 1)               # lag 1
    assert abs(corr(re[0::2], re[1::2])) <= 4 / np.sqrt(n // 2)           # the two symbols of a Philox block


def test_seeds_and_attempts_are_uncorrelated(pkg):
    """Seed 1 against seed 2, and attempt 0 against attempt 1 (first_symbol 0 and 2^40): |correlation| < 4 / sqrt(n)."""
    n = 1 << 18
    z = np.zeros(n, np.complex64)
    a, b = dev_awgn(pkg, z, 1.0, 1, 0).astype(np.complex128), dev_awgn(pkg, z, 1.0, 2, 0).astype(np.complex128)
    c = dev_awgn(pkg, z, 1.0, 1, 1 << 40).astype(np.complex128)
    for x, y in ((a, b), (a, c)):
        assert abs(corr(x.real, y.real)) < 4 / np.sqrt(n) and abs(corr(x.imag, y.imag)) < 4 / np.sqrt(n)
        assert abs(corr(x.real, y.imag)) < 4 / np.sqrt(n)


def test_system_object(pkg):
    """AWGNChannel: numpy in, numpy out; device tensor in, device tensor out; the symbol counter, reset(), first_symbol=; the four
    noise methods and the input port against awgn_dev at that variance, bit for bit."""
    import torch
    p = TM.point(4, 8.0)
    n = 257
    tx = TM.dev_mod(pkg, p["g"][:n * 4], 4)
    seed = 0xABCDEF
    h = pkg.AWGNChannel(NoiseMethod="Signal to noise ratio (SNR)", SNR=8.0, Seed=seed)
    N0 = h.N0
    want = dev_awgn(pkg, tx, N0, seed, 0)
    rx = h.step(tx)
    assert isinstance(rx, np.ndarray) and rx.dtype == np.complex64 and rx.shape == (n,) and (bits_of(rx) == bits_of(want)).all()
    h.reset()
    t = torch.from_numpy(tx.copy()).cuda().reshape(1, n)
    rx_t = h(t)
    assert isinstance(rx_t, torch.Tensor) and rx_t.device == t.device and rx_t.shape == (1, n) and rx_t.dtype == torch.complex64
    assert (bits_of(rx_t.cpu().numpy().reshape(-1)) == bits_of(want)).all()
    assert (t.cpu().numpy().reshape(-1) == tx).all()  # the input is left as it is
    # two steps of 100 and 157 symbols draw what one step of 257 draws; reset() repeats the sequence
    for _ in range(2):
        h.reset()
        two = np.concatenate([h.step(tx[:100]), h.step(tx[100:])])
        assert (bits_of(two) == bits_of(want)).all()
    # first_symbol = k: awgn_dev at k, the counter left alone
    k = (1 << 33) - 1
    h.reset()
    h.step(tx[:100])
    assert (bits_of(h.step(tx, first_symbol=k)) == bits_of(dev_awgn(pkg, tx, N0, seed, k))).all()
    assert (bits_of(h.step(tx[100:])) == bits_of(want[100:])).all()
    # the four noise methods call the kernel with their N0; SNR-type properties are tunable between steps
    for kw in (dict(NoiseMethod="Signal to noise ratio (Eb/No)", EbNo=3.0, BitsPerSymbol=4),
               dict(NoiseMethod="Signal to noise ratio (Es/No)", EsNo=3.0, SamplesPerSymbol=4, SignalPower=2.0),
               dict(NoiseMethod="Signal to noise ratio (SNR)", SNR=-2.0), dict(NoiseMethod="Variance", Variance=0.25)):
        c = pkg.AWGNChannel(Seed=seed, **kw)
        assert (bits_of(c.step(tx)) == bits_of(dev_awgn(pkg, tx, c.N0, seed, 0))).all(), kw
    h.reset()
    h.SNR = 1.5
    assert h.N0 != N0 and (bits_of(h.step(tx)) == bits_of(dev_awgn(pkg, tx, h.N0, seed, 0))).all()
    # the input port: a scalar, and one value per symbol (numpy or device tensor, shaped like tx)
    c = pkg.AWGNChannel(NoiseMethod="Variance", VarianceSource="Input port", Seed=seed)
    assert (bits_of(c.step(tx, 0.125)) == bits_of(dev_awgn(pkg, tx, 0.125, seed, 0))).all()
    var = np.where(np.arange(n) % 2 == 0, 0.125, 0.5).astype(np.float32)
    ref = dev_awgn(pkg, tx, 1.0, seed, n, var=var)
    assert (bits_of(c.step(tx, var)) == bits_of(ref)).all()                  # (the counter stands at n after the first step)
    c.reset()
    c.step(tx, 0.125)
    got = c.step(t, torch.from_numpy(var).cuda().reshape(1, n))
    assert (bits_of(got.cpu().numpy().reshape(-1)) == bits_of(ref)).all()
    with pytest.raises(pkg.NRLDPCError):
        c.step(tx)                                                           # the port's value is missing
    with pytest.raises(pkg.NRLDPCError):
        h.step(tx, 0.5)                                                      # no port on this object
    with pytest.raises(pkg.NRLDPCError):
        c.step(tx, var[:-1])


def test_harness_with_the_stand_alone_channel(pkg):
    """simulate_point_device(channel="awgn") on the committed harness_golden.json curve (BG2, A = 100, R = 1/3, QPSK, 10 iterations,
    rv [0], batch 256, seed 11: BLER 0.32 at 0 dB).  One shard and two give the identical outcome vector; the three-stage and the fused
    leg disagree on at most 5 of 256 blocks at -6, 0 and +6 dB; at 0 dB both BLERs lie in [0.15, 0.50] (0.32 +- 5 binomial standard
    deviations at 256 blocks); f16 LLRs run with channel="awgn" as with a callable."""
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    seed, batch = 11, 256
    chains = []
    for _ in range(2):
        shared = pkg.NRLDPC(BG=2, A=100, G=300, Q_m=2)
        chains.append((DC.DeviceEncodeChain(shared), DC.DeviceDecodeChain(shared, iterations=10, I_HARQ=1)))
    try:
        sim = lambda ch, esn0, **kw: H().simulate_point_device(ch, 2, esn0, [0], batch, seed, 0, **kw)
        one = sim(chains[:1], 0.0, channel="awgn")
        two = sim(chains, 0.0, channel="awgn")
        assert one.shape == (batch,) and (one == two).all()
        assert (sim(chains[:1], 0.0, channel=H().awgn_channel(seed)) == one).all()  # the string is awgn_channel(seed)
        for esn0 in (-6.0, 0.0, 6.0):
            split = one if esn0 == 0.0 else sim(chains[:1], esn0, channel="awgn")
            fused = sim(chains[:1], esn0)
            differ = int((split != fused).sum())
            print("harness %g dB: BLER three-stage %.4f, fused %.4f, blocks that differ: %d" % (esn0, 1 - split.mean(), 1 - fused.mean(), differ))
            assert differ <= 5, (esn0, differ)
            if esn0 == 0.0:
                assert 0.15 <= 1 - split.mean() <= 0.50 and 0.15 <= 1 - fused.mean() <= 0.50
        half = sim(chains[:1], 6.0, channel="awgn", llr_dtype=np.float16)
        assert half.shape == (batch,) and half.all()  # 6 dB: far above the waterfall, every block decodes
    finally:
        for enc, dec in chains:
            enc.close(); dec.close()

"""Pass 2 of the compile-time-Z kernels selects the outgoing magnitude arithmetically (LayerZ64::min_select: clamp01(|t| - m1),
then one fused multiply-add) and clamps the row scaling from below with a clamp modifier (scale_mag_magic): bit-exact against the
C oracle on inputs built to hit the conditions that make the arithmetic form exact -- ties at the minimum, rows with no edge or
exactly one edge below the cap the pipelined search starts from (a non-integer), +-inf / NaN LLRs, zero minima, and minima that
scale to magnitude 0 under a negative row parity (where the new form returns +0 and the compare form returned -0).

Codeword 0 of every batch is laid out by hand for the first layer of the first iteration, where every t is simply the ingested
LLR of its variable (a layer's rows share no variable, so each row z gets a pattern of its own, z mod 8); codewords 1..7 hit the
same conditions statistically in the later layers and iterations.  The CPU test at the end checks the scaling identity alone."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from conftest import BG_DIMS, awgn_llr, rule_kw

SCALE = 8
B = 8
# (bg, Z): split form with dual rows (the headline kernel); one thread per row; split form without dual rows; one thread per
# row with 5-wave codewords; packed / interleaved geometry (fixed iterations) and split form (parity stop); interleaved geometry
SHAPES = [(1, 384), (2, 384), (2, 256), (1, 320), (2, 52), (1, 64)]
RULES = [(None, 0.0), (0.625, 0.5)]  # the library's own rule (cfg.alpha = 0) / explicit alpha with beta = 4 grid units


def _hand_made(orc, rng, bg, Z, llr):
    """Row z of layer 0 (degree d, no extension bit) gets pattern z mod 8; magnitudes in grid units (LLR * SCALE)."""
    r, c, s = orc.graph_edges(bg, Z)
    e = np.flatnonzero(r == 0)
    d = len(e)
    z = np.arange(Z)
    var = c[e][:, None] * Z + (z[None, :] + s[e][:, None]) % Z  # [d, Z]: the variable of edge j of row z
    mag = rng.integers(9, 120, (d, Z)).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], (d, Z))
    pos = np.argsort(rng.random((d, Z)), axis=0)  # a random order of the edges of every row
    for zz in range(Z):
        p, m, sg = pos[:, zz], mag[:, zz], sign[:, zz]
        k = zz % 8
        if k == 0:    # two edges tied at the minimum
            m[p[:2]] = 5
        elif k == 1:  # three edges tied at the minimum, which scales to magnitude 0 under both rules
            m[p[:3]] = 2
        elif k == 2:  # every magnitude above the cap: m1 = m2 = cap, d fractional, D = 0
            m[:] = np.inf
        elif k == 3:  # exactly one edge below the cap: m1 an integer, m2 = cap
            m[:] = np.inf
            m[p[0]] = 7
        elif k == 4:  # zero minima (t = 0, m1 = m2 = 0), one of them from a NaN
            m[p[:2]] = 0
            m[p[2]] = np.nan
        elif k == 5:  # minimum below beta/alpha with a negative row parity: magnitude 0 carrying a sign
            m[p[0]] = 1
            sg[:] = 1.0
            sg[p[: 1 + 2 * int(rng.integers(0, d // 2))]] = -1.0  # an odd number of negative edges
        elif k == 6:  # every edge saturated and tied
            m[:] = 127
        # k == 7: no ties, nothing special
    flat = llr[0]
    flat[var] = sign * mag / SCALE
    # what was built, counted: ties of exactly two and exactly three, capped rows, zero minima
    mn = np.nanmin(np.where(np.isnan(mag), 0.0, mag), axis=0)
    ties = (np.where(np.isnan(mag), 0.0, mag) == mn[None, :]).sum(axis=0)
    assert (ties[0::8] == 2).all() and (ties[1::8] == 3).all() and np.isinf(mn[2::8]).all() and (mn[4::8] == 0).all()
    assert ((mag[:, 3::8] < 146).sum(axis=0) == 1).all() and (((sign * mag)[:, 5::8] < 0).sum(axis=0) % 2 == 1).all()


@functools.lru_cache(maxsize=None)
def _inputs(bg, Z):
    import oracle as orc
    orc.lib()
    rows, cols, kb = BG_DIMS[bg]
    rng = np.random.default_rng(9100 + 1000 * bg + Z)
    info = rng.integers(0, 2, (B, kb * Z), dtype=np.uint8)
    cw = orc.encode(bg, Z, info)
    bip = 1 - 2.0 * cw
    llr = awgn_llr(rng, cw, -1.5 if bg == 1 else -2.5, np.float64, Z)  # below the waterfall: nothing converges early
    _hand_made(orc, rng, bg, Z, llr)
    # 1: magnitudes 1 .. 8 grid units, random signs: ties of two, three and more at the minimum in rows of every degree, and
    #    minima of 1 .. 3 (1 .. 7) units, which scale to 0, under row parities of either sign
    llr[1] = rng.choice([-1.0, 1.0], cols * Z) * rng.integers(1, 9, cols * Z) / SCALE
    # 2: one magnitude everywhere: every edge of every row tied
    llr[2] = bip[2] * 0.75
    # 3: saturated (127 units): the a-posteriori values pass the cap (~146 units) after one update, so later rows have no
    #    core edge below it -- and exactly one, the extension bit (an int8: never above 127), in the rows that have one
    llr[3] = bip[3] * 40.0
    # 4: +-inf on the core columns (grid value +-2^20), NaN sprinkled over them
    llr[4, : (kb + 4) * Z] = bip[4, : (kb + 4) * Z] * np.inf
    llr[4, rng.integers(0, (kb + 4) * Z, 40)] = np.nan
    # 5: nine in ten certain, one in ten small: rows with exactly one or two edges below the cap
    small = rng.random(cols * Z) < 0.1
    llr[5] = np.where(small, rng.choice([-1.0, 1.0], cols * Z) * rng.integers(0, 6, cols * Z) / SCALE, bip[5] * np.inf)
    # 6: whole columns of zeros beyond the punctured prefix, core and extension
    for col in (2, 3, 5, kb - 1, kb + 1, kb + 4, kb + 7, cols - 1):
        llr[6, col * Z: (col + 1) * Z] = 0.0
    # 7: certain but inconsistent (random signs), with NaNs and zeros among them
    llr[7] = rng.choice([-1.0, 1.0], cols * Z) * np.inf
    llr[7, rng.integers(0, cols * Z, 200)] = np.nan
    llr[7, rng.integers(0, cols * Z, 200)] = 0.0
    llr = llr.astype(np.float32)
    llr.setflags(write=False)
    return llr


def _check(pkg, orc, bg, Z, llr, alpha, beta, iters, et, app):
    c = pkg.Codec(bg, Z, max_iter=iters, early_term=et, alpha=alpha or 0.0, beta=beta, llr_scale=SCALE, llr_dtype=np.float32)
    try:
        out = c.decode(llr, want_iters=True, want_app=app)
    finally:
        c.close()
    ref = orc.decode_nmsq(bg, Z, llr.astype(np.float64), iters, early_term=et, scale=SCALE, want_app=app, **rule_kw(c, SCALE))
    what = "bg %d Z %d alpha %s iters %d stop %d app %d" % (bg, Z, alpha, iters, et, app)
    assert (out[0] == ref[0]).all(), "hard decisions differ: " + what
    assert (out[1] == ref[1]).all(), "iteration counts differ: " + what
    if app:
        assert (out[2] == ref[2]).all(), "soft outputs differ: " + what


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,beta", RULES)
@pytest.mark.parametrize("bg,Z", SHAPES)
def test_arithmetic_select_is_bit_exact(pkg, orc, bg, Z, alpha, beta):
    llr = _inputs(bg, Z)
    for iters in (1, 2, 3, 25):
        _check(pkg, orc, bg, Z, llr, alpha, beta, iters, False, False)  # the pipelined kernels (hard output)
    _check(pkg, orc, bg, Z, llr, alpha, beta, 25, True, False)           # ... and their parity-stop builds (extension bits: ext())
    for iters, et in ((1, False), (3, False), (25, True)):               # soft output: the unpipelined kernel (update())
        _check(pkg, orc, bg, Z, llr, alpha, beta, iters, et, True)


def _rules():
    """Every (alpha, beta in grid units) nrldpc_default_rule can resolve to at an llr_scale the library accepts, on the grid of
    half units nrldpc_create keeps beta on, and the explicit pair of the GPU test."""
    out = {(0.625, 4.0)}
    for scale in (1, 2, 4, 8, 16, 32):
        for b in (0.375, 0.25, 0.3125):
            out.add((0.875, float(np.rint(2 * np.float32(b) * scale) / (2 * scale) * scale)))
    return sorted(out)


def _fma_f32(a, b, c):
    """float32 fused multiply-add: the exact value, rounded once (the float64 step is checked to be exact)."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    d = float(exact)
    assert Fraction(d) == exact, "not exact in float64: the rounding to float32 below would be a second one"
    return np.float32(d)


@pytest.mark.parametrize("alpha,beta", _rules())
def test_scaling_by_clamp_equals_the_oracle_rule(alpha, beta):
    """scale_mag_magic as built (everything times 2^-23, subtrahend 1.0) and in the form with 2^-7 and 65536: for every integer
    minimum up to the cap the search starts from, and the cap itself, both equal clamp(rint(alpha*m - beta), 0, 127)."""
    a32, b32 = np.float32(alpha), np.float32(beta)
    cap = (np.float32(127.49) + b32) / a32
    ms = [np.float32(m) for m in range(4096) if m <= cap] + [cap]
    assert len(ms) > 128
    for k, off in ((23, np.float32(1.0)), (7, np.float32(65536.0))):
        s = np.float32(2.0 ** -k)
        a_s, nb_s = a32 * s, (np.float32(8388608.0) - b32) * s
        assert Fraction(float(a_s)) == Fraction(float(a32)) / 2 ** k and Fraction(float(nb_s)) == (2 ** 23 - Fraction(float(b32))) / 2 ** k
        for m in ms:
            y = _fma_f32(a_s, m, nb_s)
            z = np.float32(y - off)  # exact: y is within a factor of two of off
            assert Fraction(float(z)) == Fraction(float(y)) - Fraction(float(off))
            got = np.float32(min(max(z, np.float32(0.0)), np.float32(1.0))) * np.float32(2.0 ** k)
            want = min(max(np.rint(float(a32) * float(m) - float(b32)), 0.0), 127.0)  # the oracle's scale_mag(), in double
            assert float(got) == want, (alpha, beta, float(m), float(got), want)

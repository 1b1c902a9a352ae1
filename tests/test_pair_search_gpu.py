"""The split decoder of BG1 Z = 384 finds a row's two smallest magnitudes over pairs of edges (csrc/nrldpc_decode_z64_pair.h):
bit-exact against the C oracle on inputs built for what a paired search can get wrong -- the two minima in the same pair, in
different pairs, in a part's leftover edge, on either side of the barrier between the early and the late part, ties of two and
three, rows with no edge or exactly one edge below the cap the search starts from, and the extension edge as the minimum.

Codeword 0 is laid out by hand for layer 0 of iteration 1, where every t is the ingested LLR of its variable (a layer's rows
share no variable; row 0 has 19 edges and no extension edge): rows z < 342 put the row's smallest and second smallest values at
the positions of pair number z mod 171 of the C(19, 2) = 171 pairs of positions, distinct in the first 171 rows and tied in the
next 171, so whichever way the kernel splits the row into parts and pairs, every relative placement of the two minima occurs;
rows z >= 342 take three-way ties, every edge above the cap, and exactly one edge below it at an even, an odd and the last
position.  Codewords 1..3 work on the extension edge (rows >= 4), codewords 4..7 are AWGN below the waterfall and meet the same
conditions statistically in the later layers and iterations."""
import functools
import itertools

import numpy as np
import pytest

from conftest import BG_DIMS, awgn_llr, rule_kw

SCALE = 8
B = 8
BG, Z = 1, 384  # the unit is compile-time Z: this is its smallest shape
RULES = [(None, 0.0), (0.625, 0.5)]  # the library's own rule (cfg.alpha = 0) / explicit alpha with beta = 4 grid units
DTYPES = [np.float16, np.float32]
CAP_UNITS = 146  # below (127.49 + beta) / alpha of every rule in use: 145.7 at alpha 0.875 is the smallest cap; inf is above all
PAIRS = list(itertools.combinations(range(19), 2))
NPAIR = len(PAIRS)


def _hand_made(orc, rng, llr):
    """Row z of layer 0: magnitudes in grid units (LLR * SCALE), all exact in float16."""
    r, c, s = orc.graph_edges(BG, Z)
    e = np.flatnonzero(r == 0)
    d = len(e)
    assert d == 19 and NPAIR == 171 and 2 * NPAIR == 342
    z = np.arange(Z)
    var = c[e][:, None] * Z + (z[None, :] + s[e][:, None]) % Z  # [d, Z]: the variable of edge j of row z
    assert len(np.unique(var)) == d * Z  # the rows of a layer share no variable: every pattern lands where it is put
    mag = rng.integers(9, 120, (d, Z)).astype(np.float64)
    sign = rng.choice([-1.0, 1.0], (d, Z))
    for zz in range(Z):
        m = mag[:, zz]
        if zz < 2 * NPAIR:
            i, j = PAIRS[zz % NPAIR]
            if zz < NPAIR:  # distinct: the smaller one at either position of the pair
                lo, hi = (i, j) if (zz // 3) % 2 == 0 else (j, i)
                m[lo], m[hi] = 3, 6
            else:           # tied
                m[i] = m[j] = 4
        else:
            k = (zz - 2 * NPAIR) % 6
            if k == 0:    # three edges tied at the minimum
                m[rng.choice(d, 3, replace=False)] = 5
            elif k == 1:  # every magnitude above the cap: m1 = m2 = cap
                m[:] = np.inf
            elif k == 2:  # exactly one edge below the cap, at an even position
                m[:] = np.inf
                m[2 * int(rng.integers(0, 9))] = 7
            elif k == 3:  # ... at an odd position
                m[:] = np.inf
                m[1 + 2 * int(rng.integers(0, 9))] = 7
            elif k == 4:  # ... at the last position (the leftover of the row, whichever part it is in)
                m[:] = np.inf
                m[d - 1] = 7
            else:         # three tied at the minimum, the last position among them
                m[[0, 9, d - 1]] = 2
    llr[0][var] = sign * mag / SCALE
    # what was built, counted
    srt = np.sort(mag, axis=0)
    pos = np.argsort(mag, axis=0, kind="stable")
    first = slice(0, NPAIR), slice(NPAIR, 2 * NPAIR)
    assert (srt[0, first[0]] == 3).all() and (srt[1, first[0]] == 6).all() and (srt[2, first[0]] >= 9).all()
    assert (srt[0, first[1]] == 4).all() and (srt[1, first[1]] == 4).all() and (srt[2, first[1]] >= 9).all()
    for sl in first:  # every pair of positions, once each
        got = sorted(tuple(sorted(p)) for p in pos[:2, sl].T.tolist())
        assert got == PAIRS
    assert len({tuple(p) for p in pos[:2, first[0]].T.tolist()} - set(PAIRS)) > 50  # the smaller one is the later one as well
    tail = mag[:, 2 * NPAIR:]
    below = (tail < CAP_UNITS).sum(axis=0)
    k = np.arange(Z - 2 * NPAIR) % 6
    assert ((tail == tail.min(axis=0)).sum(axis=0)[(k == 0) | (k == 5)] == 3).all()
    assert (below[k == 1] == 0).all() and (below[(k == 2) | (k == 3) | (k == 4)] == 1).all()
    assert (np.argmin(tail, axis=0)[k == 2] % 2 == 0).all() and (np.argmin(tail, axis=0)[k == 3] % 2 == 1).all()
    assert (np.argmin(tail, axis=0)[k == 4] == d - 1).all() and (k == 4).sum() >= 7
    return var


@functools.lru_cache(maxsize=None)
def _inputs():
    import oracle as orc
    orc.lib()
    rows, cols, kb = BG_DIMS[BG]
    rng = np.random.default_rng(7100)
    info = rng.integers(0, 2, (B, kb * Z), dtype=np.uint8)
    cw = orc.encode(BG, Z, info)
    bip = 1 - 2.0 * cw
    llr = awgn_llr(rng, cw, -1.5, np.float64, Z)  # below the waterfall: nothing converges early
    var = _hand_made(orc, rng, llr)
    ext = slice((kb + 4) * Z, cols * Z)
    core = slice(0, (kb + 4) * Z)
    # 1: magnitudes 1 .. 8 grid units everywhere, random signs: the extension edge ties with core edges at every rank
    llr[1] = rng.choice([-1.0, 1.0], cols * Z) * rng.integers(1, 9, cols * Z) / SCALE
    # 2: extension columns at +-1 unit, every core value at least 1 unit: the extension edge of a row >= 4 enters the search at
    #    or tied for the minimum of what was ingested
    llr[2] = rng.choice([-1.0, 1.0], cols * Z) * rng.integers(1, 9, cols * Z) / SCALE
    llr[2, ext] = rng.choice([-1.0, 1.0], (cols - kb - 4) * Z) / SCALE
    # 3: extension columns saturated (127 units, the largest value an extension edge can have): never the minimum unless every
    #    core edge is at the cap
    llr[3, ext] = bip[3, ext] * 40.0
    assert (np.abs(llr[1]) * SCALE >= 1).all() and (np.abs(llr[1]) * SCALE <= 8).all()
    assert (np.abs(llr[2, ext]) * SCALE == 1).all() and (np.abs(llr[2, core]) * SCALE >= 1).all()
    assert (np.abs(llr[3, ext]) * SCALE >= 127).all()
    # 4 .. 7: AWGN as drawn
    llr = llr.astype(np.float32)
    for built in (llr[0][var], llr[1], llr[2], llr[3, ext]):  # the built patterns survive float16
        assert (built.astype(np.float16).astype(np.float32) == built).all()
    llr.setflags(write=False)
    return llr


# (iterations, parity stop, active rows): fixed counts, the parity stop, the pruned units of the same size
CONFIGS = [(1, False, 0), (2, False, 0), (3, False, 0), (25, False, 0), (25, True, 0), (3, False, 5), (3, False, 13), (3, False, 24)]


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,beta", RULES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_paired_search_is_bit_exact(pkg, orc, dtype, alpha, beta):
    bld = pkg._capi._build
    assert (BG, Z) in bld.Z64_PAIR  # what this test is about is what the library runs
    llr = _inputs().astype(dtype)
    ref_in = llr.astype(np.float64)
    for iters, et, nl in CONFIGS:
        c = pkg.Codec(BG, Z, max_iter=iters, n_layers=nl, early_term=et, alpha=alpha or 0.0, beta=beta, llr_scale=SCALE, llr_dtype=dtype)
        try:
            hard, it = c.decode(llr, want_iters=True)
        finally:
            c.close()
        ref = orc.decode_nmsq(BG, Z, ref_in, iters, n_layers=nl, early_term=et, scale=SCALE, **rule_kw(c, SCALE))
        what = "%s alpha %s iters %d stop %d rows %d" % (np.dtype(dtype).name, alpha, iters, et, nl)
        assert (hard == ref[0]).all(), "hard decisions differ: " + what
        assert (it == ref[1]).all(), "iteration counts differ: " + what

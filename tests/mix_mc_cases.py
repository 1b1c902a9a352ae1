"""What the tests of the mixed batches' Monte-Carlo stages share (tests/test_mix_mc_api.py, tests/test_mix_mc_gpu.py): the two plans
and the per-configuration draws.

  P_small  A = 1, 3, 4, 63, 64, 65, 130 with 3, 0, 1, 2, 5, 1, 2 transport blocks: a row end inside a four-bit chunk (A = 1, 3, 63, 65,
           130), a hash-word boundary inside a row (A = 65, 130) and at its end (A = 64), an empty configuration, rows at odd addresses
           (A odd and more than one block), a configuration of one chunk (A = 4);
  P_two    one BG1 and one BG2 configuration with two code blocks each: B = A + 24, so b_hat rows are not A + 16 apart.

Draws: distinct seeds; first blocks 0, small, 2^32 + 5 (the block index no longer fits 32 bits) and one whose range crosses 2^32."""
SMALL_A = (1, 3, 4, 63, 64, 65, 130)
SMALL_N_TB = (3, 0, 1, 2, 5, 1, 2)
SMALL_FIRST = (0, 9, (1 << 32) + 5, 7, (1 << 32) - 2, 1, (1 << 32) + 5)
SMALL_SEEDS = tuple((0xABCDEF0123 + 0x9E3779B97F4A7C15 * i) & ((1 << 64) - 1) for i in range(7))

TWO_KW = (dict(BG=1, A=9000, G=27000, Q_m=2), dict(BG=2, A=4000, G=12000, Q_m=4))
TWO_N_TB = (2, 3)
TWO_FIRST = ((1 << 32) + 5, 3)
TWO_SEEDS = (0x5EED, (1 << 64) - 1)


def small(pkg):
    ps = [pkg.NRLDPC(BG=2, A=a, G=2 * max(30, 2 * a), Q_m=2) for a in SMALL_A]
    for p in ps:
        p.validate()
    assert all(p.C == 1 and p.B == p.A + 16 for p in ps)
    return ps, list(SMALL_N_TB)


def two(pkg):
    ps = [pkg.NRLDPC(**kw) for kw in TWO_KW]
    for p in ps:
        p.validate()
    assert [p.C for p in ps] == [2, 2] and all(p.B == p.A + 24 for p in ps)
    return ps, list(TWO_N_TB)


PLANS = {"P_small": (small, SMALL_SEEDS, SMALL_FIRST), "P_two": (two, TWO_SEEDS, TWO_FIRST)}


def plan(pkg, name):
    """(parameter objects, counts, seeds, first blocks) of a named plan."""
    make, seeds, first = PLANS[name]
    ps, n_tb = make(pkg)
    return ps, n_tb, list(seeds), list(first)

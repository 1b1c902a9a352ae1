"""What the channel-leg tests of the mixed batches share (tests/test_mix_chan_api.py, tests/test_mix_chan_gpu.py): the two plans, the
properties the new kernels need from them, and the per-configuration operating points.

  main   the nine sets of tests/mix_cases.py with their counts: all five Q_m, an empty configuration, 237 341 bits in all; odd symbol
         counts (301 and 5763: the last pair thread of an even first_symbol, the first AND last of an odd one, hold one symbol), a BPSK
         count that is no multiple of its four symbols per thread (80006 mod 4 = 2: the ragged last mapper / demapper thread), a
         configuration smaller than one workgroup (301 symbols), several that take more than one;
  tails  per Q_m one configuration with one transport block and the smallest G the parameter object accepts that gives an odd symbol
         count -- G = Q_m, ONE symbol: every thread that has work is a ragged one, in both grids, at either parity -- and a
         configuration with a transport block but G = 0: a non-empty configuration without symbols, which shares its prefix entry with
         its neighbour like an empty one.

Operating points: Es/N0 by Q_m from the operating points of tests/test_chain_gpu.py::test_channel_kernel_matches_numpy_restatement
(the low one of each Q_m for `main`, the high one for `tails`), distinct seeds, and first_symbol values that are even, odd, that cross
2^32 inside the segment, and that cross 2^33 inside the segment (there the pair counter's high word changes)."""
import mix_cases as M

ESN0_MAIN = {1: -2.0, 2: 0.0, 4: 8.0, 6: 14.0, 8: 20.0}
ESN0_TAILS = {1: -2.0, 2: 30.0, 4: 8.0, 6: 14.0, 8: 45.0}
TOTAL_BITS = 237341
MAIN_SYMBOLS = (450, 301, 1000, 0, 5763, 80006, 12636, 7500, 26668)
# even, odd, even, (empty), odd, odd and across 2^32, even, even and far up, odd and across 2^33 (the Philox counter's high word)
MAIN_FIRST = (0, 7, 1000, 4, 12345, (1 << 32) - 40001, (1 << 33) + 2, 1 << 40, (1 << 33) - 3)
MAIN_SEEDS = tuple(0xC0DE1234ABCD + 0x9E3779B97F4A7C15 * i & (1 << 64) - 1 for i in range(9))

TAILS_KW = [dict(BG=2, A=40, G=q, Q_m=q) for q in (1, 2, 4, 6, 8)] + [dict(BG=2, A=40, G=0, Q_m=4)]
TAILS_N_TB = (1, 1, 1, 1, 1, 1)
TAILS_FIRST = (1, 0, (1 << 32) - 1, 5, (1 << 33) - 1, 3)
TAILS_SEEDS = tuple(0xFEEDFACE + 77 * i for i in range(6))


def n_sym(ps, n_tb):
    return [k * p.G // p.Q_m for p, k in zip(ps, n_tb)]


def main(pkg):
    """(parameter objects, counts) of the nine-set mix, with the properties the channel kernels need from it."""
    ps, n_tb = M.mix(pkg), list(M.N_TB)
    ns = n_sym(ps, n_tb)
    assert sum(k * p.G for p, k in zip(ps, n_tb)) == TOTAL_BITS and tuple(ns) == MAIN_SYMBOLS
    assert all((k * p.G) % p.Q_m == 0 for p, k in zip(ps, n_tb))
    assert {ns[1], ns[4]} == {301, 5763} and ns[1] % 2 == ns[4] % 2 == 1                 # odd symbol counts
    assert ps[5].Q_m == 1 and ns[5] == 80006 and ns[5] % 4 == 2                          # BPSK: no multiple of S = 4
    assert ps[1].Q_m == 1 and (ns[1] + 3) // 4 < 256 and ns[1] // 2 + 1 < 256            # fewer threads than one workgroup, either grid
    assert min(x for x in ns if x) == ns[1]
    assert ns[3] == 0 and n_tb[3] == 0                                                   # the empty configuration
    assert sum(1 for x in ns if x > 4 * 256) >= 4                                        # more than one workgroup, several times
    for first, cnt in zip(MAIN_FIRST, ns):
        assert first + cnt < 1 << 64
    assert {f % 2 for f, c in zip(MAIN_FIRST, ns) if c} == {0, 1}
    assert MAIN_FIRST[5] % 2 == 1 and MAIN_FIRST[5] < 1 << 32 < MAIN_FIRST[5] + ns[5]    # crosses 2^32 inside the segment
    assert MAIN_FIRST[8] % 2 == 1 and MAIN_FIRST[8] < 1 << 33 < MAIN_FIRST[8] + ns[8]    # the pair counter crosses 2^32 there
    assert len(set(MAIN_SEEDS)) == 9
    return ps, n_tb


def tails(pkg):
    ps = [pkg.NRLDPC(**kw) for kw in TAILS_KW]
    for p in ps:
        p.validate()
    n_tb = list(TAILS_N_TB)
    assert n_sym(ps, n_tb) == [1, 1, 1, 1, 1, 0] and [p.Q_m for p in ps[:5]] == [1, 2, 4, 6, 8]
    for kw in TAILS_KW[:5]:  # the smallest: the next smaller multiple of Q_m is G = 0, an even (zero) symbol count
        assert kw["G"] == kw["Q_m"]
    assert {f % 2 for f in TAILS_FIRST} == {0, 1} and len(set(TAILS_SEEDS)) == 6
    return ps, n_tb


def esn0(ps, table):
    return [table[p.Q_m] for p in ps]


PLANS = {"main": (main, ESN0_MAIN, MAIN_SEEDS, MAIN_FIRST), "tails": (tails, ESN0_TAILS, TAILS_SEEDS, TAILS_FIRST)}


def plan(pkg, name):
    """(parameter objects, counts, EsN0_dB per configuration, seeds, first symbols) of a named plan."""
    make, table, seeds, first = PLANS[name]
    ps, n_tb = make(pkg)
    return ps, n_tb, esn0(ps, table), list(seeds), list(first)


def sym_rule(ps, n_tb):
    """sym_off[0] = 0, sym_off[i+1] = round_up(sym_off[i] + n_tb[i] * G_i / Q_m_i, 16), restated."""
    off = [0]
    for c in n_sym(ps, n_tb):
        off.append((off[-1] + c + 15) // 16 * 16)
    return off

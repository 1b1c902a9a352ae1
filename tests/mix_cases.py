"""The mix the mixed-batch tests share (tests/test_mix_chain_api.py, tests/test_mix_chain_gpu.py): the nine parameter sets of
tests/test_half_soft_path_gpu.py::CASES, restated with the same property assertions, and the transport-block counts.

What the nine sets reach: C = 1, 2 and 3; an odd G; repetition; wrap-around; an odd N_cb under LBRM; unequal E_r; a code block with
E_r = 0; Z = 20 and 384; Q_m = 1, 2, 4, 6, 8; every form of the single-configuration launch rule (general, plain gather, and the
input-driven form the rule picks once a soft buffer is given).  N_TB leaves one configuration empty.  These are the smallest shapes
that reach every form and every alignment case."""
import numpy as np

# kw, then what the case is there to reach: C, parity of N_cb (None: any), repetition, the form the single-configuration launch rule
# picks without / with the buffer, and further properties checked in params()
CASES = [
    (dict(BG=2, A=100, G=300, Q_m=2), dict(C=1, rep=False, forms=("fast", "fast"), Z=20)),
    (dict(BG=2, A=101, G=301, Q_m=1), dict(C=1, rep=False, forms=("fast", "fast"), G_odd=True)),
    (dict(BG=2, A=100, G=3000, Q_m=6, rv_id=2), dict(C=1, rep=True, forms=("general", "general"))),
    (dict(BG=1, A=5000, G=6000, Q_m=4, rv_id=3), dict(C=1, rep=False, forms=("fast", "fast"), wraps=True)),
    (dict(BG=2, A=3842, G=11526, Q_m=2, I_LBRM=1, TBS_LBRM=6002, rv_id=2),
     dict(C=2, N_cb=4501, rep=True, forms=("general", "general"))),
    (dict(BG=1, A=20019, G=40003, Q_m=1, rv_id=1, I_LBRM=1, TBS_LBRM=30003),
     dict(C=3, N_cb=15001, rep=False, forms=("fast", "scatter"), E_r=(13334, 13334, 13335), N=21120)),
    (dict(BG=1, A=8424, G=25272, Q_m=2), dict(C=1, rep=False, forms=("fast", "scatter"), Z=384)),
    (dict(BG=1, A=20016, G=60000, Q_m=8, N_L=2, rv_id=1), dict(C=3, rep=False, forms=("fast", "fast"))),
    (dict(BG=1, A=20019, G=26668, Q_m=2, CBGTI=[2]), dict(C=3, rep=False, forms=("fast", "scatter"), E_r=(13334, 13334, 0))),
]
N_TB = (3, 1, 2, 0, 1, 2, 1, 1, 2)
assert len(N_TB) == len(CASES) and 0 in N_TB


def geometry(p):
    """(filler positions of d, non-filler positions inside the circular buffer) as index arrays; d = the code block without
    its 2Z punctured columns (NRLDPCDecoder.m:224)."""
    Z2 = 2 * p.Z_c
    pos = np.arange(p.N)
    filler = (pos >= max(int(p.K_prime) - Z2, 0)) & (pos < p.K - Z2)
    return np.nonzero(filler)[0], np.nonzero(~filler[:p.N_cb])[0]


def launch_forms(p):
    """The form the single-configuration launch rule picks (without, with) the buffer, restated from the parameter object."""
    _, body = geometry(p)
    if any(e > body.size for e in p.E_r):
        return ("general", "general")
    return ("fast", "scatter" if p.Q_m <= 2 and p.N >= 4096 else "fast")


def params(pkg, i):
    kw, want = CASES[i]
    p = pkg.NRLDPC(**kw)
    p.validate()
    # the properties the case is listed for, from the parameter object itself
    _, body = geometry(p)
    assert p.C == want["C"], (kw, p.C)
    assert any(e > body.size for e in p.E_r) == want["rep"], kw
    assert launch_forms(p) == want["forms"], (kw, launch_forms(p))
    if "N_cb" in want:
        assert p.N_cb == want["N_cb"] and p.N_cb % 2 == 1, (kw, p.N_cb)
    if "E_r" in want:
        assert tuple(p.E_r) == want["E_r"], (kw, p.E_r)
    if "Z" in want:
        assert p.Z_c == want["Z"], (kw, p.Z_c)
    if "N" in want:
        assert p.N == want["N"], (kw, p.N)
    if "G_odd" in want:
        assert p.G % 2 == 1
    if "wraps" in want:
        assert p.k_0 > 0 and p.k_0 + max(p.E_r) > p.N_cb, (kw, p.k_0)
    return p


def mix(pkg):
    """The nine parameter objects, and the properties of the mix as a whole."""
    ps = [params(pkg, i) for i in range(len(CASES))]
    assert {p.C for p in ps} == {1, 2, 3} and {p.Q_m for p in ps} == {1, 2, 4, 6, 8} and {20, 384} <= {p.Z_c for p in ps}
    assert any(0 in p.E_r for p in ps) and any(len(set(p.E_r)) > 1 for p in ps)
    return ps


def sizes(p, n_tb):
    """Elements configuration (p, n_tb) takes in the seven packed arrays, in the order of nrldpc_mix_offsets."""
    ncw = 2 * p.Z_c + p.N
    return (n_tb * p.G, n_tb * p.C * p.N_cb, n_tb * p.C * ncw, n_tb * p.C * p.K, n_tb * p.C, n_tb * p.B, n_tb)


def layout(ps, n_tb):
    """The layout rule of include/nrldpc.h restated: an int64 array [n + 1][7]."""
    off = np.zeros((len(ps) + 1, 7), np.int64)
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        off[i + 1] = (off[i] + np.array(sizes(p, k), np.int64) + 15) // 16 * 16
    return off

"""The paired two-smallest search of the split decoder (csrc/nrldpc_decode_z64_pair.h, LayerZ64Pair::track3) against the
one-edge-at-a-time search it replaces (LayerZ64::track3), as a numpy model of both: random rows of degree 1 .. 19, magnitudes
from small ranges so that ties are common, three caps the search starts from (non-integers, one of them below most
magnitudes), a random split of the row's edges into the part tracked before the barrier and the part tracked after it, and
the extension edge behind the first part -- the partner of that part's leftover where its edge count is odd, a single step
otherwise.  The two smallest values of a multiset and the xor of the sign bits do not depend on the order of the search, so
m1, m2 and the parity must be identical, bit for bit."""
import numpy as np

F = np.float32
CAPS = (F((127.49 + 0.0) / 0.875), F((127.49 + 4.0) / 0.625), F(3.49))
ROWS_PER_STRUCTURE = 100


def med3(a, b, c):
    return np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))


def sign_bits(x):
    return x.view(np.uint32) & np.uint32(0x80000000)


class Search:
    """pm1 <= pm2 and the parity word of a batch of rows; t: [edges, rows] float32."""

    def __init__(self, cap, n):
        self.pm1 = np.full(n, cap, F)
        self.pm2 = np.full(n, cap, F)
        self.pS = np.zeros(n, np.uint32)

    def fold1(self, x):
        ax = np.abs(x)
        self.pm2 = med3(ax, self.pm1, self.pm2)
        self.pm1 = np.minimum(self.pm1, ax)

    def fold2(self, x, y):
        ax, ay = np.abs(x), np.abs(y)
        s2 = med3(self.pm1, ax, ay)
        self.pm1 = np.minimum(np.minimum(self.pm1, ax), ay)
        self.pm2 = np.minimum(s2, self.pm2)

    def result(self):
        return self.pm1, self.pm2, self.pS


def one_at_a_time(t, lam, cap):
    """LayerZ64::track3 over all parts: every edge, then the extension edge, one step each."""
    s = Search(cap, t.shape[1])
    for x in list(t) + ([lam] if lam is not None else []):
        s.fold1(x)
        s.pS = s.pS ^ sign_bits(x)
    return s.result()


def paired(t, late, lam, cap):
    """LayerZ64Pair::track3: part 0 (the early edges, then the extension edge), then part 2 (the late edges)."""
    s = Search(cap, t.shape[1])
    for part in (0, 2):
        edges = [t[j] for j in range(t.shape[0]) if late[j] == (part == 2)]
        ext_here = part == 0 and lam is not None
        pend = None
        for k, x in enumerate(edges):
            if k % 2 == 0:
                pend = x
                if k + 1 == len(edges) and not ext_here:
                    s.fold1(x)
            else:
                s.fold2(pend, x)
                s.pS = s.pS ^ sign_bits(pend) ^ sign_bits(x)
        if ext_here:
            if len(edges) % 2 == 1:
                s.fold2(pend, lam)
                s.pS = s.pS ^ sign_bits(pend) ^ sign_bits(lam)
            else:
                s.fold1(lam)
                s.pS = s.pS ^ sign_bits(lam)
        elif len(edges) % 2 == 1:
            s.pS = s.pS ^ sign_bits(pend)
    return s.result()


def _rows(rng, d, n, hi):
    return (rng.choice([-1.0, 1.0], (d, n)) * rng.integers(0, hi, (d, n))).astype(F)


def test_paired_search_equals_the_one_at_a_time_search():
    rng = np.random.default_rng(715)
    n = ROWS_PER_STRUCTURE
    rows = leftover_with_ext = leftover_late = 0
    for d in range(1, 20):
        for rep in range(20):
            late = rng.random(d) < rng.choice([0.0, 0.3, 0.5, 1.0])  # all early and all late included
            hi = int(rng.choice([2, 4, 9, 128, 400]))                # 400: magnitudes above every cap
            t = _rows(rng, d, n, hi)
            for has_ext in (False, True):
                lam = _rows(rng, 1, n, min(hi, 128))[0] if has_ext else None
                n_early = int((~late).sum())
                leftover_with_ext += has_ext and n_early % 2 == 1
                leftover_late += (d - n_early) % 2 == 1
                for cap in CAPS:
                    want = one_at_a_time(t, lam, cap)
                    got = paired(t, late, lam, cap)
                    for w, g, name in zip(want, got, ("m1", "m2", "parity")):
                        assert w.tobytes() == g.tobytes(), (name, d, late.tolist(), has_ext, float(cap))
                    assert (got[0] <= got[1]).all()
                    rows += n
    assert rows >= 200000 and leftover_with_ext > 100 and leftover_late > 100


def test_ties_and_caps_by_hand():
    """The cases the identity rests on, spelled out: a tie inside a pair, a tie across pairs, every edge above the cap, one edge
    below it, and the extension edge as the minimum's partner."""
    cap = CAPS[0]
    def run(vals, late, lam=None):
        t = np.array(vals, F)[:, None]
        l = None if lam is None else np.array([lam], F)
        a, b = one_at_a_time(t, l, cap), paired(t, np.array(late, bool), l, cap)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        return float(b[0][0]), float(b[1][0])
    assert run([5, -5, 9, 7], [0, 0, 0, 0]) == (5.0, 5.0)               # tied inside a pair
    assert run([5, 9, -5, 7], [0, 0, 0, 0]) == (5.0, 5.0)               # tied across pairs
    assert run([5, 9, 7, 5], [0, 0, 1, 1]) == (5.0, 5.0)                # tied across the barrier
    assert run([400, 500, 300], [0, 1, 0]) == (float(cap), float(cap))  # nothing below the cap
    assert run([400, 500, -3], [0, 1, 0]) == (3.0, float(cap))          # exactly one edge below it, a leftover
    assert run([8, 9, 7], [0, 0, 0], lam=-1) == (1.0, 7.0)              # the extension edge pairs with the leftover
    assert run([8, 9], [0, 0], lam=-1) == (1.0, 8.0)                    # ... and takes the single step
    assert run([8], [1], lam=2) == (2.0, 8.0)                           # no early edge at all

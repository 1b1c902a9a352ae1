"""The cases the transmit-side stage tests share (tests/test_encode_paths_gpu.py, tests/test_tx_stages_gpu.py) and a census of
what they reach (tests/test_tx_cases.py, CPU).

Each of the three transmit kernels picks its code path from sizes and from the ALIGNMENT of the pointers it is given:
nrldpc_encode_kernel (csrc/nrldpc_encode.hip), nrldpc_rate_match_kernel (csrc/nrldpc_ratematch.hip) and the CRC attach / check
kernels (csrc/nrldpc_crc.hip through stage_row / store_row of csrc/nrldpc_wave.h).  The functions below restate those conditions
from the parameters alone -- nothing here runs a kernel -- so that the lists can be held to "every path is reached" on the CPU,
and a later change of a kernel's conditions that strands a path shows up there.  Every derived parameter comes from
testbench_ref.derive (the transcription of NRLDPC.m that shares no code with the product's mirror).

The rate-matching and CRC lists are the smallest shapes that reach everything, and every set of either is needed; the encoder
list also holds three sizes kept for their size alone (ENC_SIZES_FOR_SIZE).  Nothing here is workload-sized (the largest is C = 9
at n_tb = 2)."""
import testbench_ref as TB
from conftest import ALL_Z, BG_DIMS


GUARD = 32    # bytes checked either side of an output range
FILL = 0xAA   # what output buffers hold before a call


class Slot:
    """n bytes at byte offset `off` above a 256-byte boundary inside a larger device buffer that is pre-filled with FILL (GPU tests
    only).  ptr is the raw address; data() / guards_intact() / whole() read it back."""

    def __init__(self, n, off, data=None):
        import torch
        self.n, self.lo = n, 256 + off
        self.buf = torch.full((self.lo + n + 256,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        if data is not None:
            self.buf[self.lo:self.lo + n] = torch.from_numpy(data.reshape(-1).copy()).cuda()  # (a copy: `data` may be read-only)
        self.ptr = self.buf.data_ptr() + self.lo

    def data(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def whole(self):
        return self.buf.cpu().numpy()

    def guards_intact(self):
        w = self.whole()
        assert self.lo >= GUARD and w.size - self.lo - self.n >= GUARD
        return bool((w[:self.lo] == FILL).all() and (w[self.lo + self.n:] == FILL).all())  # at least GUARD bytes either side


def derive(kw):
    """testbench_ref.derive with the defaults of NRLDPC.m:28-84 filled in; returns the derived dict plus the set's own fields."""
    full = dict(I_LBRM=0, TBS_LBRM=10 ** 9, rv_id=0, N_L=1, CBGTI=())  # TBS_LBRM is not read at I_LBRM = 0
    full.update(kw)
    ref = TB.derive(**full)
    ref.update(BG=full["BG"], A=full["A"], G=full["G"], Q_m=full["Q_m"])
    return ref


# ---- encoder -------------------------------------------------------------------------------------------------------------------
# Sizes: for each combination of waves per codeword x ring build x ballot batch x extension store that exists, a lifting size that
# has it (Z % 4 != 0: 2, 3, 6; ballot batch 2, 4 | Z: 20; Z % 32 == 0 with batch 2: 32; batch 7: 52; Z % 32 == 0 with batch 7: 96,
# 352; a workgroup per codeword with and without Z % 32 == 0: 128, 144) and the largest size of either base graph.
# From Z = 52 on every valid lifting size is a multiple of 4, and from 128 on of 16: a workgroup per codeword (NWC = 4) with
# Z % 4 != 0 does not exist, nor does the batch of 7 ballots with Z % 4 != 0.
ENC_SIZES = {1: (2, 3, 20, 32, 52, 96, 128, 144, 384), 2: (6, 20, 32, 52, 352, 384)}
# Of these, the ones kept for their size and not for a class of their own: an odd size (the alignment differs from codeword to
# codeword) and the largest of either base graph.  Without them every remaining size is the only one that reaches some class
# (tests/test_tx_cases.py).
ENC_SIZES_FOR_SIZE = {1: (3, 384), 2: (384,)}
# (info, out) byte offsets from a 256-byte-aligned allocation
ENC_OFFSETS = ((0, 0), (4, 0), (0, 4), (8, 8), (1, 0), (0, 1), (3, 5))
ENC_WAVES = 4  # waves per workgroup (launch_encode)


def enc_nwc(bg, Z):
    """Waves per codeword: the whole workgroup for BG1 from Z = 128 on, one wave otherwise (launch_encode)."""
    return 4 if bg == 1 and Z >= 128 else 1


def enc_batches(bg, Z):
    """One wave per codeword: four codewords per workgroup, so 1, 5 and 7 leave the last workgroup ragged."""
    return (1, 4, 5, 7) if enc_nwc(bg, Z) == 1 else (1, 3)


def enc_class(bg, Z, info_off, out_off, cw=0):
    """(BG, NWC, Z % 32 == 0, ring build, systematic copy width, extension store) of codeword `cw` of a call whose info / out
    pointers lie info_off / out_off bytes above a 16-byte boundary: the conditions of nrldpc_encode_kernel, in its order."""
    _, ncols, kb = BG_DIMS[bg]
    info = info_off + cw * kb * Z
    out = out_off + cw * ncols * Z
    DW = 2 * ((2 * Z + 32 + 63) >> 6)
    z32 = Z % 32 == 0
    ring = "words" if z32 and info % 16 == 0 else ("ballot2" if DW <= 4 else "ballot7")
    al = info | out
    copy = 16 if al % 16 == 0 else (4 if al % 4 == 0 else 1)
    ext = "dword" if Z % 4 == 0 and (out + (kb + 4) * Z) % 4 == 0 else "byte"
    return (bg, enc_nwc(bg, Z), z32, ring, copy, ext)


def enc_universe():
    """Every encoder class that exists: all lifting sizes, all pointer alignments."""
    return {enc_class(bg, Z, i, o) for bg in (1, 2) for Z in ALL_Z for i in range(16) for o in range(16)}


def enc_reached(sizes=None, offsets=ENC_OFFSETS):
    """class -> the first (Z, offsets, codeword) of the lists that reaches it."""
    sizes = ENC_SIZES if sizes is None else sizes
    seen = {}
    for bg in sizes:
        for Z in sizes[bg]:
            for io, oo in offsets:
                for cw in range(max(enc_batches(bg, Z))):
                    seen.setdefault(enc_class(bg, Z, io, oo, cw), (Z, (io, oo), cw))
    return seen


def enc_reached_from_aligned_bases():
    """What callers whose buffers start on an allocation boundary reach, at every lifting size and any batch: the state of the suite
    before the offset-pointer tests (Codec.encode and DeviceEncodeChain on hipMalloc / torch.empty buffers)."""
    return {enc_class(bg, Z, 0, 0, cw) for bg in (1, 2) for Z in ALL_Z for cw in range(16)}


# one size per ring-build class for the bit-0 and host-entry tests: (BG, Z)
ENC_RING_SIZES = ((2, 6), (1, 20), (2, 32), (1, 52), (1, 96), (1, 128), (1, 144), (1, 384))


# ---- rate matching -------------------------------------------------------------------------------------------------------------
RM_QM = (1, 2, 4, 6, 8)
RM_RUNS = ("contiguous", "tail", "kend", "wrapP", "gap")
# (cw, g) byte offsets of the two base pointers, and the transport blocks per call
RM_OFFSETS = ((0, 0), (1, 0), (0, 1), (0, 2), (3, 3))
RM_N_TB = 3

# The first three are there for a property of their own (RM_PROPERTIES); the rest is what a greedy search over BG2 with
# A in {20, 100, 101} (Z_c = 6, 20, 20), G <= 310, every rv_id and Q_m, with and without LBRM (TBS_LBRM = 1.5 A) needs for the
# run classes the first three leave, pruned until every set is the only one that reaches some class.
RM_SETS = [
    dict(BG=2, A=7701, G=3335, Q_m=1),                    # C = 3, E_r = (1111, 1112, 1112): odd G, off[1] and off[2] odd
    dict(BG=2, A=7701, G=2224, Q_m=2, CBGTI=[1]),         # the middle code block is not transmitted: E_r = (1112, 0, 1112)
    dict(BG=1, A=8424, G=26000, Q_m=4, rv_id=3),          # BG1, Z = 384; wraps around the buffer end
    dict(BG=2, A=100, G=144, Q_m=8, rv_id=3, I_LBRM=1, TBS_LBRM=150),
    dict(BG=2, A=100, G=145, Q_m=1, rv_id=3, I_LBRM=1, TBS_LBRM=150),
    dict(BG=2, A=100, G=148, Q_m=2, rv_id=3, I_LBRM=1, TBS_LBRM=150),
    dict(BG=2, A=100, G=156, Q_m=6, rv_id=1, I_LBRM=1, TBS_LBRM=150),
    dict(BG=2, A=20, G=72, Q_m=8, rv_id=3),
    dict(BG=2, A=20, G=78, Q_m=6, rv_id=3),
    dict(BG=2, A=100, G=104, Q_m=4, rv_id=1, I_LBRM=1, TBS_LBRM=150),
    dict(BG=2, A=101, G=148, Q_m=4, rv_id=3, I_LBRM=1, TBS_LBRM=152),
    dict(BG=2, A=20, G=70, Q_m=2, rv_id=3),
    dict(BG=2, A=20, G=68, Q_m=1, rv_id=3),
]
RM_PROPERTIES = ("C=3 unequal E_r, odd G, odd off[r] at Q_m=1", "a code block with E_r=0", "BG1 Z=384")


def rm_geometry(ref):
    """(lo_f, F, P, nfk0) as every rate-matching kernel computes them: first filler position of d, fillers inside the circular
    buffer, non-filler positions inside it, and k_0 counted in non-filler positions."""
    Z, K, Kp, N_cb, k0 = ref["Z_c"], ref["K"], ref["K_prime"], ref["N_cb"], ref["k_0"]
    lo_f = max(Kp - 2 * Z, 0)
    hi_f = K - 2 * Z
    F = max(min(hi_f, N_cb) - lo_f, 0)

    def nf(p):
        return p - min(max(p - lo_f, 0), F)
    return lo_f, F, N_cb - F, nf(k0)


def rm_offsets(ref):
    off, o = [], 0
    for e in ref["E_r"]:
        off.append(o)
        o += e
    assert o == ref["G"]
    return off


def rm_census(ref, offsets=RM_OFFSETS, n_tb=RM_N_TB):
    """The classes one set reaches: {(Q_m, rep, run class)} over every (code block, interleaver row i, j0) -- the branch of
    nrldpc_rate_match_kernel with its precedence: nj == 4, k + 3 < kend, q + 3 < P, q >= lo_f || q + 3 < lo_f -- and
    {(Q_m, store form of g)} over the transport blocks and the g base offsets: dword iff nj == 4 && (g address & 3) == 0."""
    Qm, G = ref["Q_m"], ref["G"]
    lo_f, F, P, nfk0 = rm_geometry(ref)
    off = rm_offsets(ref)
    runs, stores = set(), set()
    for r, E in enumerate(ref["E_r"]):
        rows = E // Qm
        rep = E > P
        for j0 in range(0, rows, 4):
            nj = min(rows - j0, 4)
            for i in range(Qm):
                k = i * rows + j0
                if rep:
                    d = k // P
                    q, kend = k - d * P + nfk0, P * (d + 1)
                else:
                    q, kend = k + nfk0, P
                if q >= P:
                    q -= P
                if nj < 4:
                    c = "tail"
                elif not k + 3 < kend:
                    c = "kend"
                elif not q + 3 < P:
                    c = "wrapP"
                elif not (q >= lo_f or q + 3 < lo_f):
                    c = "gap"
                else:
                    c = "contiguous"
                runs.add((Qm, rep, c))
            for _, g_off in offsets:
                for tb in range(n_tb):
                    addr = g_off + tb * G + off[r] + j0 * Qm
                    stores.add((Qm, "dword" if nj == 4 and addr % 4 == 0 else "byte"))
    return runs, stores


def rm_universe():
    """The 45 run classes (kend exists only with repetition) and the 10 store forms."""
    runs = {(q, rep, c) for q in RM_QM for rep in (False, True) for c in RM_RUNS if rep or c != "kend"}
    return runs, {(q, s) for q in RM_QM for s in ("dword", "byte")}


def rm_properties(refs):
    """Which of RM_PROPERTIES the derived sets `refs` have between them."""
    have = set()
    for ref in refs:
        off = rm_offsets(ref)
        if ref["C"] == 3 and len(set(ref["E_r"])) > 1 and ref["G"] % 2 and ref["Q_m"] == 1 and any(o % 2 for o in off):
            have.add(RM_PROPERTIES[0])
        if ref["C"] > 1 and 0 in ref["E_r"] and any(ref["E_r"]):
            have.add(RM_PROPERTIES[1])
        if ref["BG"] == 1 and ref["Z_c"] == 384:
            have.add(RM_PROPERTIES[2])
    return have


def rm_missing(sets):
    """What the list `sets` leaves unreached: run classes, store forms and properties, sorted; empty when it reaches everything."""
    refs = [derive(kw) for kw in sets]
    runs, stores = set(), set()
    for ref in refs:
        r, s = rm_census(ref)
        runs |= r
        stores |= s
    want_runs, want_stores = rm_universe()
    return sorted(want_runs - runs) + sorted(want_stores - stores) + sorted(set(RM_PROPERTIES) - rm_properties(refs))


# ---- CRC attach / check --------------------------------------------------------------------------------------------------------
# (set, transport blocks).  One wave per code block, at most four waves: C = 1, 2, 3 are workgroups of 1, 2, 3 waves, C = 5 a second
# round of one wave, C = 9 three rounds with a remainder; the first has one code block under the 24-bit transport-block CRC, the
# last three under the 16-bit one.  The last three have an odd A, an odd B and K = 150 = 6 (mod 16), so that the 17 rows of a, c,
# c_hat and b_hat of each start at every alignment.  The rows of one call advance both pointers together: one such set and the four
# base offsets reach only some of the 256 pairs (src & 15, dst & 15) of a call (220 with A = 73); A = 5, 7 and 9 (mod 16) between
# them reach every pair, in either call.
CRC_SETS = [
    (dict(BG=1, A=5000, G=6000, Q_m=4), 3),
    (dict(BG=2, A=3842, G=11526, Q_m=2), 3),
    (dict(BG=2, A=7701, G=3335, Q_m=1), 2),
    (dict(BG=2, A=15301, G=40000, Q_m=2), 2),
    (dict(BG=1, A=70005, G=200000, Q_m=2), 2),
    (dict(BG=2, A=69, G=300, Q_m=2), 17),
    (dict(BG=2, A=71, G=300, Q_m=2), 17),
    (dict(BG=2, A=73, G=300, Q_m=2), 17),
]
CRC_C = (1, 2, 3, 5, 9)
# base offsets of both pointers of a call (a and c; c_hat and b_hat), every pair of them
CRC_OFFSETS = (0, 1, 7, 12)


def _store_visit(src15, dst, n):
    """(src & 15, dst & 15, rotation) of one store_row(dst, LDS row, n): the LDS row sits at the 16-byte phase of the global
    pointer it was staged from (stage_row), and the 16-byte body starts `head` bytes in."""
    head = min((16 - dst % 16) % 16, n)
    return (src15, dst % 16, (src15 + head) % 4)


def crc_visits(ref, n_tb, src_off, dst_off):
    """{(call, src & 15, dst & 15, rotation)} of the stage_row -> store_row pairs of one attach and one check call."""
    C_, K, Kp, A, B = ref["C"], ref["K"], ref["K_prime"], ref["A"], ref["B"]
    pay = Kp - ref["code_block_L"]
    out = set()
    for tb in range(n_tb):
        for r in range(C_):
            src = src_off + tb * A + r * pay                      # attach: the block's share of a -> its row of c
            out.add(("attach",) + _store_visit(src % 16, dst_off + (tb * C_ + r) * K, K))
            src = src_off + (tb * C_ + r) * K                     # check: the row of c_hat -> its payload in b_hat
            out.add(("check",) + _store_visit(src % 16, dst_off + tb * B + r * pay, pay))
    return out


def crc_universe():
    """Per call: all 16 x 16 pairs (src & 15, dst & 15) of a staged and stored row, all 16 x 4 joints (dst & 15, rotation) -- what
    the head, body and alignbyte path of store_row depend on -- and each rotation; every wave-count form of CRC_C with the 24-bit
    transport-block CRC, and one code block with either transport-block CRC."""
    want = set()
    for call in ("attach", "check"):
        want |= {(call, "src,dst", s, d) for s in range(16) for d in range(16)}
        want |= {(call, "dst,rot", d, v) for d in range(16) for v in range(4)} | {(call, "rot", v) for v in range(4)}
    return want | {("C", c, "L_tb", 24) for c in CRC_C} | {("C", 1, "L_tb", 16)}


def crc_missing(sets):
    """What the list `sets` leaves unreached, sorted; empty when it reaches everything."""
    refs = [(derive(kw), n_tb) for kw, n_tb in sets]
    have = {("C", ref["C"], "L_tb", ref["transport_block_L"]) for ref, _ in refs}
    for ref, n_tb in refs:
        for so in CRC_OFFSETS:
            for do in CRC_OFFSETS:
                for call, s, d, rot in crc_visits(ref, n_tb, so, do):
                    have |= {(call, "src,dst", s, d), (call, "dst,rot", d, rot), (call, "rot", rot)}
    return sorted(crc_universe() - have, key=repr)

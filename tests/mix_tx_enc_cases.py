"""What the tests of the one-launch mixed encoder share (tests/test_mix_tx_encode_api.py on the CPU, tests/test_mix_tx_encode_gpu.py on
the device): the plan P_enc, its census on the plan's real offsets, and the input of the host walk.

P_enc holds one C = 1 configuration per (BG, Z) of tx_cases.ENC_SIZES -- 15 in all -- with the smallest payload length whose code
block takes that lifting size, and as many transport blocks as the largest count of tx_cases.enc_batches: 7 codewords where a wave
serves a codeword (two workgroups, the second with one idle wave), 3 where the whole workgroup does.  The three workgroup-per-codeword
sizes sit between one-wave sizes in configuration order, so one launch carries both bodies and a plan-wide LDS size that is not the
configuration's own."""
import tx_cases as T

# smallest A whose single code block has lifting size Z (checked against tx_cases.derive in p_enc_sets)
ENC_A = {1: {2: 1, 3: 29, 20: 381, 32: 645, 52: 1041, 96: 1921, 128: 2625, 144: 2801, 384: 7721},
         2: {6: 15, 20: 93, 32: 165, 52: 369, 352: 3185, 384: 3505}}


def p_enc_sets(sizes=None):
    """[(kw, n_tb)] in configuration order: the sizes of `sizes` (default tx_cases.ENC_SIZES), the workgroup-per-codeword ones spread
    between the others."""
    sizes = T.ENC_SIZES if sizes is None else sizes
    one, four = [], []
    for bg in sorted(sizes):
        for Z in sizes[bg]:
            A = ENC_A[bg][Z]
            kw = dict(BG=bg, A=A, G=6 * (A + 24), Q_m=2)
            ref = T.derive(kw)
            assert ref["Z_c"] == Z and ref["C"] == 1, (bg, Z, A, ref["Z_c"], ref["C"])
            if A > 1:  # ... and it is the smallest such length
                below = T.derive(dict(kw, A=A - 1, G=6 * (A + 23)))
                assert below["Z_c"] < Z, (bg, Z, A)
            (four if T.enc_nwc(bg, Z) == 4 else one).append((kw, max(T.enc_batches(bg, Z))))
    out = []
    while one or four:
        if one:
            out.append(one.pop(0))
        if four:
            out.append(four.pop(0))
    return out


def p_enc(pkg, sizes=None):
    sets = p_enc_sets(sizes)
    ps = [pkg.NRLDPC(**kw) for kw, _ in sets]
    for p in ps:
        p.validate()
    return ps, [k for _, k in sets]


def plan_census(pkg, ps, n_tb, offsets=T.ENC_OFFSETS):
    """class -> the first (configuration, base offsets, codeword) that reaches it: tx_cases.enc_class evaluated at the REAL addresses
    of the plan -- the segment offsets the library reports plus the byte offsets of the two base pointers."""
    off = pkg.mix_layout(ps, n_tb)
    seen = {}
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        for io, oo in offsets:
            for cw in range(k * p.C):
                seen.setdefault(T.enc_class(p.BG, p.Z_c, io + off[i].c_hat, oo + off[i].cw, cw), (i, (io, oo), cw))
    return seen


def walk_input(pkg, ps, n_tb, offsets=T.ENC_OFFSETS):
    """The text tests/mix_host/mix_tx_enc_check.cpp reads."""
    off = pkg.mix_layout(ps, n_tb)
    lines = [str(len(ps))]
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        lines.append(" ".join(str(int(x)) for x in (k, p.C, p.BG, p.Z_c, p.K, p.N, off[i].c_hat, off[i].cw)))
    lines.append("%d %d" % (off[len(ps)].c_hat, off[len(ps)].cw))
    lines.append(" ".join([str(len(offsets))] + ["%d %d" % pair for pair in offsets]))
    return "\n".join(lines) + "\n"

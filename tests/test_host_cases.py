"""The census of tests/host_cases.py: the calls of tests/test_host_paths_gpu.py reach every class of decode_host -- the three routes
and why a call took one copy, where doubles are narrowed, the wire format of a chunk, every branch of the two expand kernels and of
the pack kernel, the row geometry of compact chunks, the chunk plan, the source of the layer count -- a condition on the shapes,
checked without a GPU.  Each test fails with the list of classes it misses.

The universe holds 71 classes; the host-pointer calls of the older files (test_full_size_gpu.py, test_layers_gpu.py,
test_decode_gpu.py::test_bit_packed_hard_output, test_sum_product_gpu.py) reached 46 of them.  Dropping any one planned call strands
a class, for instance: without z20_rows_scalar nothing reaches (wire, int8, neg-above-act); without z384_neg_piece2 nothing reaches
(wire, native-neg-after-sent)."""
import numpy as np
import pytest

import host_cases as H

N_CLASSES = 71
N_BEFORE = 46


def test_plan_reaches_every_class():
    U = H.universe()
    assert len(U) == N_CLASSES, len(U)
    missing = H.missing(H.HOST_PLAN)
    assert missing == [], "classes no planned call reaches: %r" % missing
    assert not H.reached(H.HOST_PLAN) - U and not H.reached(H.OLDER_CALLS) - U
    # every exclusion carries its reason; what the arithmetic forbids is kept apart from what exists outside the C ABI's calls
    assert all(len(reason) > 40 for reason, _ in H.IMPOSSIBLE + H.OUTSIDE_THE_CALLS)
    prod = H.product()
    impossible = {c for c in prod if any(t(c) for _, t in H.IMPOSSIBLE)}
    outside = {c for c in prod if any(t(c) for _, t in H.OUTSIDE_THE_CALLS)}
    assert outside == {("expand", "flat-scalar"), ("expand", "flat-scalar", "trip2"), ("expand", "flat-vec", "trip2"),
                       ("expand", "rows-vec", "trip2")} and not outside & impossible
    assert len(impossible) + len(outside) + len(U) == len(prod) == len(set(prod))
    assert {c[2] for c in U if c[:2] == ("expand", "flat-tail")} == {4, 8, 12}


def test_no_chunk_starts_off_a_multiple_of_sixteen_bytes():
    """The flat kernel's vec == 0 launch lies outside the calls: proved by enumeration over every lifting size, element type, wire
    format and both values of NRLDPC_HOST_CHUNK_MB the suite uses, and by the bound behind it: only fp16 at an odd Z <= 15 has a
    codeword that is no multiple of 16 bytes, and both limits of its chunk are 512 codewords or more, so the chunk is rounded."""
    assert H.misaligned_chunk_shapes() == []
    for bg in (1, 2):
        for Z in H.ALL_Z:
            for dt in ("f16", "f32", "f64"):
                ncw = H.BG_DIMS[bg][1] * Z
                if ncw * H.DEV_EB[dt] % 16:
                    assert dt == "f16" and Z % 2 == 1 and Z <= 15
                    # the smallest chunk any pipelined call of this shape can have is still 512 codewords or more
                    assert (H.MiB // 2) // ncw >= 512 and H.PIPE_MIN // (ncw * 2) // 4 >= 512
    # K % 8 == 0 with an unaligned d_hard: s_hard + c0 * K is a multiple of 8 whenever K is
    assert all((c0 * H.BG_DIMS[bg][2] * Z) % 8 == 0 for bg in (1, 2) for Z in H.ALL_Z if (H.BG_DIMS[bg][2] * Z) % 8 == 0 for c0 in (1, 3, 41, 87))


@pytest.mark.parametrize("i", range(len(H.HOST_PLAN)), ids=[c.name for c in H.HOST_PLAN])
def test_every_planned_call_is_needed(i):
    stranded = H.missing(H.HOST_PLAN[:i] + H.HOST_PLAN[i + 1:])
    assert stranded, "call %s reaches nothing of its own" % H.HOST_PLAN[i].name


def test_planned_calls_are_the_smallest_that_reach_their_class():
    """one codeword fewer, and the call misses what it is there for"""
    largest = 1237 * 68 * 384 * 8  # the largest array test_pipelined_host_path_equals_one_device_launch builds
    for c in H.HOST_PLAN:
        rows, cols, kb, ncw, K = H.dims(c)
        assert c.batch * ncw * H.HOST_EB[c.dtype] <= largest, c.name
        p = H.plan(c)
        if p["route"] == "pipeline" and c.mode == "default" and c.name not in ("z7_tail12", "z7_tail4_packed", "z8_rows_vec_64"):
            # (the three named ones wait for a tail length / share a threshold with a sibling: checked below)
            smaller = c._replace(batch=c.batch - 1, neg=tuple((min(b, c.batch - 2), e) for b, e in c.neg),
                                 auto=c.auto and (c.auto[0], c.auto[1] and (c.batch - 2, c.auto[1][1])))
            own = [x for x in H.missing([x for x in H.HOST_PLAN if x is not c])  # what it alone reaches, of the pipeline's classes
                   if x[0] in ("expand", "rows", "wire", "first", "last", "split") or x[:2] == ("out", "pipeline")]
            assert not own or not set(own) <= H.census(smaller), (c.name, own)
        if p["route"] == "one-copy" and p["why"] == "size":  # one codeword fewer goes zero-copy
            assert H.plan(c._replace(batch=c.batch - 1, app=False))["route"] == "zero-copy", c.name
    by = H.BY_NAME
    assert H.plan(by["z7_tail8"]._replace(batch=5761))["route"] == "one-copy"  # 5762 is the first pipelined batch: tails 8, 4, (0, ) 12
    assert [H.plan(by["z7_tail8"]._replace(batch=b))["chunks"][-1]["tail"] for b in (5762, 5763, 5764, 5765)] == [8, 4, 0, 12]
    assert H.plan(by["z8_rows_vec_64"]._replace(batch=10082))["route"] == "one-copy"
    # the worked values of the plan
    p = H.plan(by["z20_rows_scalar"])
    assert (p["chunk"], [ch["n"] for ch in p["chunks"]], p["act"]) == (504, [504] * 4 + [1], 440)
    assert [ch["wire"] for ch in p["chunks"]] == ["int8"] * 4 + ["native-later-chunk"] and p["chunks"][1]["neg_above_act"]
    p = H.plan(by["z7_tail8"])
    assert (p["chunk"], len(p["chunks"]), p["K"]) == (1024, 6, 70)
    p = H.plan(by["z8_rows_vec"])
    assert (p["act"], p["chunks"][0]["expand"]) == (112, "rows-vec")
    for name, piece in (("z384_neg_piece0", 0), ("z384_neg_piece2", 2)):
        p = H.plan(by[name])
        ch = p["chunks"][0]
        (b, e), = by[name].neg
        assert (p["chunk"], len(p["chunks"]), ch["parts"]) == (41, 4, 4) and ch["n"] * p["act"] >= H.MiB
        assert ch["pieces"][piece][0] <= b * p["act"] + e < ch["pieces"][piece][1]
    p = H.plan(by["z88_trip2"])
    assert p["chunk"] * p["act"] == 508 * 4136 > H.GRID_THREADS >= 507 * 4136 and all(ch["trip2"] for ch in p["chunks"])
    assert H.plan(by["z20_auto_first"])["nl"] == 12 and H.plan(by["z20_auto_restart"])["nl"] == 20 and H.plan(by["z20_auto_restart"])["restarted"]


def test_the_older_tests_reach_46_of_the_classes():
    """The gap this census closes, kept on record.  Of the classes first listed as never executed, two turn out to have run before,
    at Z = 384 only: a last chunk of one codeword (f64, batch 1237 = 4 * 309 + 1) and more chunks than slots (the same call)."""
    U = H.universe()
    before = H.reached(H.OLDER_CALLS) & U
    assert len(before) == N_BEFORE, len(before)
    gone = U - before
    for c in (("expand", "rows-scalar"), ("rows", "compact", "rows-scalar", "act%64!=0"), ("expand", "flat-tail", 4), ("expand", "flat-tail", 8),
              ("expand", "flat-tail", 12), ("out", "one-copy", "pack-kernel-wide"), ("out", "one-copy", "pack-kernel-narrow"),
              ("out", "pipeline", "pack-kernel-narrow"), ("wire", "native-neg-after-sent"), ("wire", "native-neg-nothing-sent"),
              ("rows", "compact", "rows-vec", "act%64!=0"), ("route", "one-copy", "timing"), ("expand", "rows-scalar", "trip2"),
              ("wire", "int8", "neg-above-act"), ("route", "one-copy", "pipeline-off"), ("route", "one-copy", "zerocopy-off")):
        assert c in gone, c
    assert ("last", "single") in before and ("nchunks", ">4") in before
    # the lazy AUTO scan and its restart ran at Z = 384 only
    assert {c.Z for c in H.OLDER_CALLS if H.census(c) & {("layers", "auto-first-chunk"), ("layers", "auto-restart")}} == {384}
    assert len(H.missing(H.OLDER_CALLS)) == N_CLASSES - N_BEFORE


def test_the_piece_walk_writes_every_compact_byte_once():
    """quantise_rows_start as the model states it, for every worker count and every int8 chunk of the plan: the pieces tile the
    compact range exactly, and no source element at or beyond act of a row is read"""
    for c in H.HOST_PLAN:
        p = H.plan(c)
        if p["route"] != "pipeline" or not p["i8"]:
            continue
        act, ncw = p["act"], p["ncw"]
        for ch in (p["chunks"][0], p["chunks"][-1]):
            for nw in range(1, 17):
                hits = np.zeros(ch["n"] * act, np.uint8)
                for lo, hi in ch["pieces"]:
                    assert lo % 64 == 0 and (hi % 64 == 0 or hi == ch["n"] * act)
                    for a, b in H.worker_ranges(lo, hi, nw):
                        for pos, src, ln in H.row_walk(a, b, act, ncw):
                            hits[pos:pos + ln] += 1
                            assert src % ncw + ln <= act and src // ncw < ch["n"], (c.name, nw, pos, src, ln)
                assert (hits == 1).all(), (c.name, ch["k"], nw)


@pytest.fixture(scope="module")
def orc_cpu(orc):
    return orc


WITNESS_CALLS = [c.name for c in H.HOST_PLAN if c.mode == "default" and not c.app and not c.timing and H.critical(c)]


@pytest.mark.parametrize("name", WITNESS_CALLS)
def test_helper_classes_have_witnesses(orc_cpu, name):
    """For each helper class of a planned call, at least three of its critical positions are witnesses: negating that one LLR changes
    the oracle's hard decisions or iteration count of its codeword (one codeword per candidate, the oracle alone).  The first
    inactive element of a compact row is the opposite case: under an explicit count it changes nothing."""
    c = H.BY_NAME[name]
    llr, info, crit = H.build_input(orc_cpu, c)
    nl = H.plan(c)["nl"]
    assert crit
    for cls, pos in crit.items():
        step = max(1, len(pos) // 40)
        w = H.witnesses(orc_cpu, c, llr, pos[::step], nl)
        if cls == "inactive":
            assert w == [], (name, "junk above the active columns changes a decision", w)
        else:
            assert len(w) >= 3, (name, cls, "witnesses", w)
            if cls[:2] == ("expand", "flat-tail"):  # the tail's last element: what a loop bound of n - 1 leaves unwritten
                assert pos[-1] in w and pos[0] in w, (name, cls, w)


def test_the_restart_input_restarts_on_the_data(orc_cpu):
    """The AUTO inputs are what the model was told, by a plain scan of the arrays themselves: in z20_auto_first every chunk shows 12
    rows; in z20_auto_restart the first chunk -- every codeword but the last, in fact -- shows 12 and the batch 20, so the lazy scan
    settles on 12 and the last chunk's check lifts it; the poison array of that call shows 12 throughout and does not restart."""
    for name, first, whole in (("z20_auto_first", 12, 12), ("z20_auto_restart", 12, 20)):
        c = H.BY_NAME[name]
        p = H.plan(c)
        llr, _, crit = H.build_input(orc_cpu, c)
        assert H.np_count_layers(c, llr[:p["chunk"]]) == first and H.np_count_layers(c, llr[:c.batch - 1]) == first
        assert H.np_count_layers(c, llr) == whole == p["nl"] and p["restarted"] == (whole > first)
        assert H.np_count_layers(c, H.poison_of(c, llr)) == first
        # the row ends the scalar rows form is watched at: the first count's last element everywhere, the final one in the lifter
        ends = {e for b, e in crit[("expand", "rows-scalar")] if e}
        assert ends == ({439, 599} if whole > first else {439}) and (c.batch - 1, p["act"] - 1) in crit[("expand", "rows-scalar")]


def test_each_helper_class_is_witnessed_somewhere():
    have = set()
    for name in WITNESS_CALLS:
        have |= set(H.critical(H.BY_NAME[name]))
    assert have == {"inactive", ("expand", "rows-scalar"), ("expand", "rows-scalar", "trip2"), ("expand", "rows-vec"),
                    ("expand", "flat-tail", 4), ("expand", "flat-tail", 8), ("expand", "flat-tail", 12)}
    # the packed calls with a last partial byte: run_call checks that each of its bits takes both values over the batch
    assert {c.name for c in H.HOST_PLAN if c.packed and H.dims(c)[4] % 8 and c.mode == "default"} == {
        "z7_tail4_packed", "one_copy_narrow", "zero_copy_partial"}

"""CPU tests of tests/decode_cases.py: the model of the decoder's dispatch against build.py's lists and the existing parametrisations,
the plan against the universe, and the conditions on the plan's inputs, asked of the oracle for every planned call."""
import importlib
import os

import numpy as np
import pytest

import decode_cases as D
from conftest import ALL_Z, awgn_llr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bld():
    return importlib.import_module("ldpc-3gpp-matlab_amd.build")


def test_the_models_lists_are_build_pys():
    b = _bld()
    for name in ("Z64_PAIRS", "Z64P_PAIRS", "Z64I", "Z64_NL", "Z64P_NL", "Z64PR", "Z64_PAIR"):
        assert list(getattr(D, name)) == list(getattr(b, name)), name
    assert D.ALL_Z == ALL_Z


def test_restated_constants_stand_in_the_source():
    """the lines the model restates, looked up in the source: a change there must be carried into the model"""
    src = lambda f: open(os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc", f)).read()
    k, z, zs, zp, dev, sch = (src(f) for f in ("nrldpc_kernels.h", "nrldpc_decode_z64.h", "nrldpc_decode_z64s.h", "nrldpc_decode_z64p.h",
                                               "nrldpc_device.h", "nrldpc_sched.h"))
    assert "#define NRLDPC_Z64P_NOT_ET(X) " + " ".join("X(%d, %d)" % p for p in D.Z64P_NOT_ET) + "\n" in k
    assert "constexpr int NL_RT = %d;" % D.NL_RT in dev
    assert "template <int BG> constexpr bool z64pg_serves() { return BG == 2; }" in zp
    assert "static constexpr bool usable() { return THREADS <= 1024 && NG >= 2; }" in zs
    assert "if (NL != BGT<BG>::ROWS) return (BG == 1 && ZC == 384) || (BG == 2 && ZC == 208);" in z
    for bg, lead in ((1, "        return "), (2, "    return ")):
        want = [Z for Z in ALL_Z if D.split_default(bg, Z, D.BG_DIMS[bg][0])]
        line = next(ln for ln in z.split("\n") if ln.startswith(lead + "ZC == %d ||" % want[0]))
        i = z.index(line)
        text = z[i: z.index(";", i)]
        assert sorted(int(t) for t in __import__("re").findall(r"ZC == (\d+)", text)) == want, bg
    assert "#define NRLDPC_GEN_THREADS_BG1 512" in k and "#define NRLDPC_GEN_THREADS_BG2 512" in k
    assert "#define NRLDPC_GEN_WPE_BG2 6" in k and "#define NRLDPC_GEN_WPE_BG1 4" in k
    assert "if (waves % 4) score *= (waves > 4 ? 0.85 : 0.97);" in sch and "if (n > 4 && (n & 1) == 0) continue;" in sch
    assert "if (BG == 1 && (Z == 88 || Z == 96 || Z == 176 || Z == 352)) return 6;" in z


def test_every_list_entry_maps_to_an_instantiation():
    uni = D.universe()
    units = {u for u, k in uni}
    for bg, Z in D.Z64_PAIRS:
        assert "u_z64_%d_%d" % (bg, Z) in units
    # a finding of the census: eight packed units are compiled and linked, and no call of the default process reaches them -- an
    # interleaved entry serves every mode the packed build would (BG1: mode 7; BG2 Z = 52: NRLDPC_Z64P_NOT_ET leaves it fixed
    # iterations only, which the interleaved entry takes) and BG1 has no general kernel of the packed geometry.  They run under
    # NRLDPC_NO_ILV only, an excluded knob.
    shadowed = [p for p in D.Z64P_PAIRS if "u_z64p_%d_%d" % p not in units]
    assert shadowed == D.SHADOWED_PACKED == [(1, 3), (1, 5), (1, 6), (1, 36), (1, 44), (1, 80), (1, 96), (2, 52)]
    for bg, Z in shadowed:
        mode = next(m for b, z, n, m in D.Z64I if (b, z) == (bg, Z))
        assert mode == 7 or ((bg, Z) in D.Z64P_NOT_ET and mode & 1 and (bg, Z) in D.Z64_PAIRS)
    for bg, Z, ncw, mode in D.Z64I:
        mine = [uni[i][0] for i in uni if i[0] == "u_z64i_%d_%d" % (bg, Z)]
        assert mine and all(r.ncw == ncw for r in mine)
        assert {r.admitted for r in mine} == {b for b in (1, 2, 4) if mode & b}, (bg, Z)  # every mode bit admits a build, no other does
    for bg, Z, nl in D.Z64_NL:
        assert "u_z64_%d_%d_nl%d" % (bg, Z, nl) in units
    # ... and so is the one packed unit with a layer count of its own: (2, 20, 12, mode 5) takes its fixed-iteration calls (bit 1) and
    # its parity-stop calls (bit 4, pruned rows) before NRLDPC_Z64P_NL_LIST is looked at (nrldpc_decode.hip:386-399)
    assert [e for e in D.Z64P_NL if "u_z64p_%d_%d_nl%d" % e not in units] == D.SHADOWED_PACKED_NL == [(2, 20, 12)]
    assert not D.Z64PR
    assert len({(bg, Z) for bg, Z, ncw, mode in D.Z64I}) == len(D.Z64I)  # one entry per size: no two entries claim one call


def test_geometry_is_launchable():
    for r, shape in D.universe().values():
        assert r.ncw >= 1 and r.threads % 64 == 0 and 64 <= r.threads <= 1024, (r, shape)
        if r.kind == "split":
            assert r.ncw == 1 and D.split_usable(shape[0], shape[1])


def _existing_parametrisations():
    """(bg, Z, resolved layer count, early_term, soft) of the calls test_decode_gpu.py makes through its parametrisations, read
    from that file's own tables"""
    import test_decode_gpu as T
    out = []
    for bg in (1, 2):
        rows = D.BG_DIMS[bg][0]
        for Z in ALL_Z:
            out.append((bg, Z, rows, int(bool(Z & 2)), True))                       # test_every_lifting_size
            out += [(bg, Z, rows, 0, False), (bg, Z, rows, 1, False)]               # test_hard_output_kernels_iteration_by_iteration
        for Z in T.RT_GRID_Z:                                                       # test_run_time_layer_count_grid
            for nl in T.RT_GRID_NL + (rows - 1,):
                out += [(bg, Z, nl, 0, False), (bg, Z, nl, 1, False)]
        for b, Z, ncw, mode in D.Z64I:                                              # test_interleaved_block_geometry
            if b == bg:
                for nl in (rows, 7 if bg == 2 else 13, rows - 3):
                    out += [(bg, Z, nl, 0, False), (bg, Z, nl, 1, False)]
        for nl in (rows, rows - 1, 17):                                             # test_z384_kernel_variants
            out += [(bg, 384, nl, et, soft) for et in (0, 1) for soft in (False, True)]
    for m in T.test_rate_pruned_layers.pytestmark:
        if m.name == "parametrize":
            for bg, Z, nl, esn0 in m.args[1]:
                out += [(bg, Z, nl, et, soft) for et in (0, 1) for soft in (False, True)]
    for m in T.test_crc_aided_stop.pytestmark:
        if m.name == "parametrize":
            for bg, Z, nl, Kp, crc, esn0 in m.args[1]:
                out += [(bg, Z, nl or D.BG_DIMS[bg][0], 2, False), (bg, Z, nl or D.BG_DIMS[bg][0], 1, False)]
    return out


def test_every_call_of_the_existing_parametrisations_has_a_route():
    """every call of test_decode_gpu.py's parametrisations lands on an instantiation of the universe -- which is enumerated from
    other layer counts than these, so a count that routed to a kernel nobody enumerated would show -- then what that file's comments say about families.  That one call has one route is the shape of route() as of
    launch_decode (the first family that admits it returns); the kernel trace holds it from outside: one decoder launch per call."""
    uni = D.universe()
    calls = _existing_parametrisations()
    assert len(calls) == 1400
    seen = set()
    for bg, Z, nl, et, soft in calls:
        r = D.route(bg, Z, nl, et, soft)
        assert D.instantiation(r) in uni or D.instantiation(D.route(bg, Z, nl, et, soft, "f32")) in uni, (bg, Z, nl, et, soft)
        seen.add(r.kind)
    assert len(seen) == 7
    assert D.route(1, 384, 46, 0, False).kind == "split" and D.route(2, 384, 42, 0, False).kind == "row"
    for Z in (144, 192, 320):
        assert D.route(1, Z, 17, 1, False).kind == "row", Z
    assert D.route(2, 352, 17, 1, False).kind == "row" and D.route(1, 352, 17, 1, False).kind == "packed"
    assert D.route(1, 288, 17, 0, False).kind == "split"
    assert D.route(2, 208, 21, 1, False).build == ("ETP", "NL21") and D.route(2, 20, 12, 0, False).kind == "ilv"


def test_the_waterfall_table_is_test_decode_gpus():
    import test_decode_gpu as T
    for bg in (1, 2):
        for nl in range(4, D.BG_DIMS[bg][0] + 1):
            assert D.waterfall(bg, nl) == T._waterfall_esn0(bg, nl)


def test_the_plan_reaches_the_whole_universe():
    uni, plan = D.universe(), D.plan()
    reached = {D.instantiation(D.call_route(c)) for c in plan}
    assert reached == set(uni)
    cls = set().union(*(D.classes(c) for c in plan))
    assert cls == D.universe_classes()
    for c in plan:  # every planned call states what it is there for, and is there for it
        why = D.reason(c)
        assert why[0] in ("instantiation", "classes", "soft")
        if why[0] == "instantiation":
            assert D.instantiation(D.call_route(c)) == why[1:], c.name
        else:
            assert D.call_route(c).kind == why[1], c.name
    refill = [c for c in plan if c.refill_grid]
    assert refill and all(D.call_route(c).refills and D.grid(D.call_route(c), c.batch, c.refill_grid) == 1 for c in refill)
    assert {D.instantiation(D.call_route(c)) for c in refill} == {i for i, (r, s) in uni.items() if r.refills}


def test_what_the_older_device_pointer_tests_reached():
    """every earlier call that hands the device entries buffers of the test's own (decode_cases.older_calls / older_multi), through
    the same model"""
    inst, cls, multi, tcls = D.older_reached()
    uni, uc = D.universe(), D.universe_classes()
    assert inst <= set(uni) and cls <= uc
    assert (len(inst), len(uni), len(cls), len(uc)) == (138, 560, 33, 59)
    kinds = {uni[i][0].kind for i in inst}
    assert kinds == {"ilv", "packed", "packed_general", "split", "row", "rtz"}   # the block geometry's general kernel never
    assert multi == {(1, "f16"), (1, "f32"), (2, "f16"), (2, "f32")} and tcls == {256, 512}
    never = uc - cls
    assert {c for c in never if c[0] != "general"} == {
        ("ilv", "iters", "null"), ("packed", "iters", "null"), ("packed_general", "iters", "null"), ("row", "iters", "null"),
        ("rtz", "iters", "null"),   # (a null iters reached launch_decode only in cfg4's two split launches)
        ("ilv", "refill", "active"), ("packed", "refill", "active"),   # (as the model counts it: under the test hook's cap)
        ("packed_general", "tail", "full"), ("packed_general", "tail", "small"), ("rtz", "tail", "full"), ("rtz", "tail", "small"),
        ("rtz", "soft", "yes"), ("row", "llr", "narrow4"), ("row", "llr", "narrow8"), ("split", "llr", "narrow8")}
    # the only misaligned calls moved both pointers together, by one element and one byte
    old = D.older_calls()
    assert not [c for c in old if D.llr_class(c.llr_off) == "wide" and c.hard_off]
    assert not [c for c in old if D.llr_class(c.llr_off) != "wide" and not c.hard_off]
    assert {(c.llr_off, c.hard_off) for c in old} == {(0, 0), (2, 1), (4, 1)}


def test_multi_call_model():
    cfg = [(1, 384, 1, "f16", 3, False), (1, 24, 1, "f16", 5, False), (2, 36, 2, "f16", 4, False), (2, 8, 1, "f32", 0, False),
           (1, 384, 1, "f16", 512, False), (2, 7, 1, "f16", 2, True)]
    shared, own, bp = D.multi_groups(cfg)
    assert own == [2, 4] and bp == [5] and sorted(i for v in shared.values() for i in v[0]) == [0, 1]


_PLAN = D.plan()
_CHUNK = 120


@pytest.mark.parametrize("k", range(-(-len(_PLAN) // _CHUNK)))
def test_conditions_on_the_plans_inputs(orc, k):
    """every planned parity-stop call has an early leaver and a straggler; every planned fixed-iteration call leaves every codeword
    unconverged with both bit values among its decisions -- asked of the oracle, no call left out"""
    for c in _PLAN[k * _CHUNK: (k + 1) * _CHUNK]:
        assert not D.conditions(c, orc, awgn_llr), c.name


def test_recorded_routes_equal_the_model():
    """profiles/decode_routes.json (tools/trace_decode_routes.py: a kernel trace of every planned call) against the model: the kernel
    name is the instantiation the model names, the grid is ceil(batch / ncw) -- capped for the NRLDPC_REFILL_GRID=1 calls -- and the
    workgroup has the model's thread count.  A record of other kernel sources is not compared and not skipped."""
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "decode_routes.json")))
    b = _bld()
    assert (rec["nrldpc_kernel_id"], rec["pair_search_id"]) == (b.kernel_id(), b.pair_search_id()), \
        "re-record: profiles/decode_routes.json was traced from other decoder sources (python tools/trace_decode_routes.py)"
    assert sorted(rec["calls"]) == sorted(c.name for c in _PLAN), "re-record: the plan has changed"
    wrong = []
    for c in _PLAN:
        k, grid, wg = rec["calls"][c.name]
        r = D.call_route(c)
        want = "void nrldpc::%s%s(" % (r.unit + "::" if r.unit else "", r.kernel)
        if not rec["kernels"][k].startswith(want) or (grid, wg) != (D.grid(r, c.batch, c.refill_grid), r.threads):
            wrong.append((c.name, rec["kernels"][k], grid, wg, want, D.grid(r, c.batch, c.refill_grid), r.threads))
    assert not wrong, "%d calls, the first: %r" % (len(wrong), wrong[:3])
    assert len(set(rec["kernels"])) == len(D.universe())

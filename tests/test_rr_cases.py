"""The census of tests/rr_cases.py: the sets of the rate-recovery path tests reach every class of every rate-recovery kernel -- the
three units, their general / plain-gather / scatter forms, every Q_m, every boundary a group of positions can straddle, every
width an access can take -- a condition on the inputs, checked without a GPU.  Each test fails with the list of classes it misses.

The universe holds 1207 classes; the two older lists (tests/test_half_soft_path_gpu.py::CASES, tests/test_chain_gpu.py::CASES)
reached 351 of them.  Dropping any one of the 45 searched sets strands a class, for instance: without
dict(BG=2, A=38, G=10, Q_m=1, rv_id=2, I_LBRM=1, TBS_LBRM=38) nothing reaches (ex, fast, Q_m=1, fill>beyond) or
(ex, fast, Q_m=1, wrapk0); without dict(BG=2, A=3842, G=4184, Q_m=1, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]) nothing reaches
(f32, general, Q_m=1, depth3+) or (mix, general, Q_m=1, all:dead)."""
import importlib

import pytest

import mix_cases as M
import rr_cases as R
import test_chain_gpu as CH
import testbench_ref as TB

N_CLASSES = 1207
N_BEFORE = 351


def test_sets_reach_every_class():
    U = R.universe()
    assert len(U) == N_CLASSES
    missing = R.rr_missing(R.RR_SETS, R.MIX_CONFIGS)
    assert missing == [], "classes (unit, form, Q_m, feature) / properties no set reaches: %r" % missing
    assert not set(R.rr_reached(R.RR_SETS, R.MIX_CONFIGS)) - U
    # every exclusion carries its reason, and the classes that exist but lie outside the calls are kept apart from the impossible ones
    assert all(len(reason) > 20 for reason, _ in R.IMPOSSIBLE + R.OUTSIDE_THE_CALLS)
    outside = {c for c in R.product() if any(t(*c) for _, t in R.OUTSIDE_THE_CALLS) and not any(t(*c) for _, t in R.IMPOSSIBLE)}
    assert outside and all(c[1] == "scatter" and c[2] > 2 and c[3].startswith("acc:") for c in outside) and not outside & U


def test_sets_are_small_and_listed_for_what_they_have():
    refs = [R.derive(kw) for kw in R.RR_SETS]
    assert R.rr_properties(refs[:R.N_PROPERTY_SETS]) == set(R.RR_PROPERTIES) and not R.rr_properties(refs[R.N_PROPERTY_SETS:])
    assert refs[0]["E_r"] == [1111, 1112, 1112] and refs[1]["E_r"] == [1112, 0, 0] and refs[2]["Z_c"] == 384
    assert all(r["G"] <= 5000 and r["C"] <= 2 and r["Z_c"] in (9, 20, 208) for r in refs[R.N_PROPERTY_SETS:])
    ns = [n for _, n in R.MIX_CONFIGS]
    assert set(ns) == {0, 1, 2, 3} and {k for k, n in R.MIX_CONFIGS if n} == set(range(len(R.RR_SETS)))
    # under NRLDPC_RR_SCATTER=1 the scatter instantiations at Q_m = 4, 6, 8 are reached, which no default call reaches
    reached = set(R.rr_reached(R.RR_SETS, R.MIX_CONFIGS))
    for unit in ("f32", "ex"):
        for Qm in (4, 6, 8):
            assert (unit, "scatter", Qm, "in:J%d:run" % R.scatter_J(unit, Qm)) in reached
            calls = [c for c in R.plan_single()[0] if c[4] == "default"]
            assert not any(R.launch_form(ref, c[3], c[4]) == "scatter" for ref in refs if ref["Q_m"] == Qm for c in calls)


@pytest.mark.parametrize("i", range(R.N_PROPERTY_SETS, len(R.RR_SETS)))
def test_every_searched_set_is_needed(i):
    sets = R.RR_SETS[:i] + R.RR_SETS[i + 1:]
    cfg = [(k - (k > i), n) for k, n in R.MIX_CONFIGS if k != i]
    stranded = R.rr_missing(sets, cfg)
    assert stranded, "set %d (%r) reaches nothing of its own" % (i, R.RR_SETS[i])


def test_the_older_lists_reach_351_of_the_classes():
    """The gap these lists close, kept on record: the general kernel had run at Q_m = 2 and 6 only, the plain gather never at
    Q_m = 6, no group had straddled the end of an LBRM buffer."""
    half_soft = [kw for kw, _ in M.CASES]
    before = R.reached_before(half_soft, M.N_TB, CH.CASES)
    assert len(before) == N_BEFORE, len(before)
    missing = R.universe() - before
    for c in (("f32", "general", 1, "depth2"), ("ex", "fast", 6, "all:live"), ("mix", "fast", 6, "all:live"), ("f32", "general", 2, "carry"),
              ("f32", "general", 2, "depth3+"), ("ex", "fast", 2, "live>beyond"), ("ex", "scatter", 4, "in:J4:run"),
              ("mix", "general", 4, "live>dead")):
        assert c in missing, c
    # replacing RR_SETS by the 19 older sets fails, and the message names what is unreached
    assert len(R.rr_missing(half_soft + CH.CASES)) > 300


def test_launch_rule_agrees_with_mix_cases():
    pkg = importlib.import_module("ldpc-3gpp-matlab_amd")  # (the parameter object needs no GPU)
    for kw, want in M.CASES:
        ref = R.derive(kw)
        forms = (R.launch_form(ref, False), R.launch_form(ref, True))
        p = pkg.NRLDPC(**kw)
        p.validate()
        assert forms == M.launch_forms(p) == want["forms"], (kw, forms, M.launch_forms(p))
        assert R.mix_form(ref) == ("general" if forms[0] == "general" else "fast", forms[1] == "scatter")
        assert {R.launch_form(ref, b, "general") for b in (False, True)} == {"general"}
        assert R.launch_form(ref, True, "scatter0") == R.launch_form(ref, False, "scatter0") == forms[0]
        assert R.launch_form(ref, False, "scatter1") == ("general" if want["rep"] else "scatter")


def test_a_broad_sweep_reaches_nothing_outside_the_universe():
    """every 20th set of the search space (some 1400), under the calls of the new tests"""
    U = R.universe()
    calls, n_tb = R.plan_single()
    seen = set()
    for kw in R.space(20):
        try:
            ref = R.derive(kw)
        except TB.Unsupported:
            continue
        seen |= R.census(ref, calls, n_tb, mix=(R.MIX_CALLS, 3, [1, 0, 1]))
    outside = sorted(seen - U)
    assert not outside, "classes outside the universe: %r" % outside[:20]
    assert len(seen) > 1000

"""Mixed transport-block batches, transmit side (nrldpc_mix_tx_*) at the C ABI and in the binding, without a device: the six functions
are declared, exported and bound; nrldpc_mix_tx_layout equals the layout rule; every refusal comes back before any HIP call (this
file runs where there is no GPU) with the texts of the single-configuration calls; a census, restated from tests/tx_cases.py on the
plans' real offsets, shows that the three test plans of tests/test_mix_tx_gpu.py reach every path of the two kernels; and the layout
arithmetic and the workgroup mapping of both kernels (csrc/nrldpc_mix_tx.h) are walked on the CPU by a stand-alone program built with
the address and undefined-behaviour sanitizers."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mix_cases as M
import tx_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
NULL = None
NAMES = ("nrldpc_mix_tx_layout", "nrldpc_mix_tx_create", "nrldpc_mix_tx_destroy", "nrldpc_mix_tx_crc_attach_dev",
         "nrldpc_mix_tx_encode_dev", "nrldpc_mix_tx_rate_match_dev")
FIELDS = ("g", "harq", "cw", "c_hat", "cb", "b_hat", "tb")


def as_array(off):
    return np.array([[getattr(o, k) for k in FIELDS] for o in off], np.int64)


def a_rule(ps, n_tb):
    """a_off[0] = 0, a_off[i+1] = round_up(a_off[i] + n_tb[i] * A_i, 16), restated."""
    off = [0]
    for p, k in zip(ps, n_tb):
        off.append((off[-1] + k * p.A + 15) // 16 * 16)
    return off


def p9(pkg):
    return M.mix(pkg), list(M.N_TB)


def p_rm(pkg):
    ps = [pkg.NRLDPC(**kw) for kw in T.RM_SETS]
    for p in ps:
        p.validate()
    return ps, [T.RM_N_TB] * len(ps)


def p_crc(pkg):
    ps = [pkg.NRLDPC(**kw) for kw, _ in T.CRC_SETS]
    for p in ps:
        p.validate()
    return ps, [k for _, k in T.CRC_SETS]


PLANS = {"P9": p9, "P_rm": p_rm, "P_crc": p_crc}


def test_symbols_are_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    for name in NAMES:
        assert name in C.EXPORTS and hasattr(lib, name) and re.search(r"\b(int|void) %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.nrldpc_mix_tx_crc_attach_dev.argtypes) == 4 and len(lib.nrldpc_mix_tx_encode_dev.argtypes) == 5
    assert len(lib.nrldpc_mix_tx_rate_match_dev.argtypes) == 4
    assert "typedef struct nrldpc_mix_tx* nrldpc_mix_tx_handle;" in hdr
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    assert ctypes.sizeof(C.MixOffsets) == 56 and C.MIX_FIELDS == FIELDS  # the receive layout's record did not change
    block = hdr[hdr.index("mixed transport-block batches, transmit side"):hdr.index("typedef struct nrldpc_mix_tx*")]
    for out_of_scope in ("a one-launch mixed encoder", "pool variants", "the MEX gateway"):
        assert out_of_scope in block
    assert pkg.MixTxPlan is C.MixTxPlan and pkg.mix_tx_layout is C.mix_tx_layout
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    assert hasattr(DC, "MixedEncodeChain") and hasattr(DC, "MixedDecodeChain") and hasattr(DC, "DeviceEncodeChain")


def test_new_unit_is_built_and_is_not_part_of_the_decoder_kernels_identity(pkg):
    bld = pkg._capi._build
    assert "nrldpc_mix_tx.hip" in bld.SOURCES and "nrldpc_mix_tx.h" in bld.HEADERS
    assert not {"nrldpc_mix_tx.hip", "nrldpc_mix_tx.h"} & set(bld.KERNEL_SOURCES)
    kernels_h = open(os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc", "nrldpc_kernels.h")).read()
    assert "Mix" not in kernels_h  # the argument structures stay out of the decoder's identity
    assert bld.kernel_id() == pkg.load().nrldpc_kernel_id().decode() == "a54d4abae9865fdf"  # the parent commit's value


def test_payload_layout_equals_the_rule(pkg):
    ps, n_tb = p9(pkg)
    got = pkg.mix_tx_layout(ps, n_tb)
    assert got == a_rule(ps, n_tb) and got[0] == 0 and all(x % 16 == 0 for x in got) and len(got) == 10
    empty = n_tb.index(0)
    assert got[empty + 1] == got[empty]  # a zero count takes no room
    assert pkg.mix_tx_layout([pkg.tb_params(p) for p in ps], n_tb) == got  # TbParams are accepted as well
    # zero counts first, last and adjacent
    for cnt in ([0, 2, 1, 0], [0, 0, 3, 1], [2, 0, 0, 1], [0, 0, 0, 0], [1, 0, 0, 0]):
        assert pkg.mix_tx_layout(ps[:4], cnt) == a_rule(ps[:4], cnt), cnt
    assert pkg.mix_tx_layout([], []) == [0]
    # the segment of configuration i holds exactly its [n_tb][A] bytes; odd A leaves the rows at every alignment
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        assert got[i + 1] - got[i] >= k * p.A and got[i + 1] - got[i] < k * p.A + 16
    for name, make in PLANS.items():
        qs, cnt = make(pkg)
        assert pkg.mix_tx_layout(qs, cnt) == a_rule(qs, cnt), name


def test_the_other_arrays_are_the_receive_layouts_fields(pkg):
    """.off of a transmit plan is nrldpc_mix_layout's answer, field for field (here on plans that need no device; on the non-empty
    plans in tests/test_mix_tx_gpu.py), and totals() names the four arrays."""
    ps, _ = p9(pkg)
    for qs, cnt in ((ps, [0] * 9), ([], [])):
        plan = pkg.MixTxPlan(qs, cnt)
        assert (as_array(plan.off) == as_array(pkg.mix_layout(qs, cnt))).all() and plan.a_off == a_rule(qs, cnt)
        assert plan.totals() == {"a": 0, "c": 0, "cw": 0, "g": 0}
        plan.close()


def _arrays(pkg, ts, n_tb):
    C = pkg._capi
    n = len(ts)
    arr = (C.TbParams * max(n, 1))()
    for i, t in enumerate(ts):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(t), ctypes.sizeof(C.TbParams))
    return arr, (ctypes.c_int32 * max(n, 1))(*n_tb)


def _both(pkg, ts, n_tb, n=None, null_p=False, null_n=False):
    """(code, text) of nrldpc_mix_tx_layout and of nrldpc_mix_tx_create for the same arguments: they must agree, and create must
    leave no handle behind."""
    lib = pkg.load()
    arr, cnt = _arrays(pkg, ts, n_tb)
    n = len(ts) if n is None else n
    a_off = (ctypes.c_int64 * (max(n, 0) + 1))()
    rc1 = lib.nrldpc_mix_tx_layout(n, None if null_p else arr, None if null_n else cnt, a_off)
    msg1 = lib.nrldpc_last_error()
    h = ctypes.c_void_p()
    rc2 = lib.nrldpc_mix_tx_create(n, None if null_p else arr, None if null_n else cnt, 0, ctypes.byref(h))
    msg2 = lib.nrldpc_last_error()
    assert rc1 == rc2 and msg1 == msg2 and h.value is None, (rc1, msg1, rc2, msg2)
    return rc1, msg1


def test_parameter_refusals_carry_the_single_call_texts_and_the_configuration(pkg):
    """A broken parameter block anywhere in the mix: the code and the text nrldpc_rate_match_dev / nrldpc_crc_attach_dev give for that
    block, with " (configuration i)" appended -- from nrldpc_mix_tx_layout and from nrldpc_mix_tx_create, before any device call --
    and, for the blocks nrldpc_mix_create refuses, the same answer as that call's."""
    C = pkg._capi
    lib = pkg.load()
    ps, n_tb = p9(pkg)
    good = [C.tb_params(p) for p in ps]

    def broken(i, **kw):
        t = C.tb_params(ps[i])
        for k, v in kw.items():
            if k == "E0":
                t.E_r[0] = v
            else:
                setattr(t, k, v)
        return t

    def single(t, stage):
        """what the single-configuration call of `stage` says about t.  Every block here is one that call refuses on the host, so
        the placeholder addresses are never used."""
        if stage == "rm":
            rc = lib.nrldpc_rate_match_dev(ctypes.byref(t), P, 3, P, NULL)
        else:
            rc = lib.nrldpc_crc_attach_dev(ctypes.byref(t), P, 3, P, NULL)
        return rc, lib.nrldpc_last_error()

    def receive(ts):
        arr, cnt = _arrays(pkg, ts, n_tb)
        off = (C.MixOffsets * (len(ts) + 1))()
        return lib.nrldpc_mix_layout(len(ts), arr, cnt, off), lib.nrldpc_last_error()

    short = dict(A=16, B=40, K_prime=44)  # C = 2, L_cb = 24: 20 payload bits per code block, fewer than the 24 of the TB CRC
    seen = set()
    for i, stage, kw in ((0, "rm", dict(C=0)), (1, "rm", dict(C=161)), (2, "att", dict(Z=17)), (3, "rm", dict(bg=3)), (4, "att", dict(Q_m=0)),
                         (5, "rm", dict(N_cb=0)), (6, "att", dict(N_cb=10 ** 6)), (7, "rm", dict(K_prime=10 ** 6)), (8, "rm", dict(E0=13333)),
                         (0, "rm", dict(E0=-2)), (0, "rm", dict(E0=298)), (3, "rm", dict(G=5999)),
                         (2, "att", dict(tb_crc_len=12)), (4, "att", dict(cb_crc_len=16)), (6, "att", dict(B=1)), (5, "att", dict(A=5)),
                         (4, "att", short)):
        t = broken(i, **kw)
        rc, msg = single(t, stage)
        assert rc in (C.ERR_ARG, C.ERR_UNSUPPORTED), (i, kw)
        ts = list(good)
        ts[i] = t
        got = _both(pkg, ts, n_tb)
        assert got == (rc, msg + b" (configuration %d)" % i), (i, kw, got, msg)
        if kw is not short:
            assert receive(ts) == got, (i, kw)  # the same refusals as nrldpc_mix_create
        seen.add(msg)
    assert len(seen) >= 7 and b"code block shorter than the transport-block CRC" in seen
    assert ps[4].C == 2 and receive([good[k] if k != 4 else broken(4, **short) for k in range(9)])[0] == C.OK  # the attach stage's own check
    # a Q_m the rate-matching kernel has no body for (the single call fails at its launch: no host text to carry)
    rc, msg = _both(pkg, [broken(0, Q_m=3)] + good[1:], n_tb)
    assert ps[0].G % 3 == 0 and rc == C.ERR_UNSUPPORTED and msg == b"Unsupported modulation (configuration 0)"
    # the block of an EMPTY configuration is checked too, and the first broken block is the one reported -- whichever check finds it
    ts = list(good)
    ts[3], ts[7] = broken(3, Z=17), broken(7, C=0)
    assert n_tb[3] == 0 and _both(pkg, ts, n_tb)[1].endswith(b"(configuration 3)")
    ts = list(good)
    ts[4], ts[7] = broken(4, **short), broken(7, C=0)
    assert _both(pkg, ts, n_tb)[1].endswith(b"CRC (configuration 4)")


def test_count_and_pointer_refusals(pkg):
    C = pkg._capi
    lib = pkg.load()
    ps, n_tb = p9(pkg)
    good = [C.tb_params(p) for p in ps]
    assert _both(pkg, good, n_tb, n=-1)[0] == C.ERR_ARG
    cnt = list(n_tb)
    cnt[5] = -1
    rc, msg = _both(pkg, good, cnt)
    assert rc == C.ERR_ARG and b"negative" in msg and msg.endswith(b"(configuration 5)")
    assert _both(pkg, good, n_tb, null_p=True)[0] == C.ERR_ARG
    assert _both(pkg, good, n_tb, null_n=True)[0] == C.ERR_ARG
    arr, cnt = _arrays(pkg, good, n_tb)
    assert lib.nrldpc_mix_tx_layout(9, arr, cnt, None) == C.ERR_ARG
    assert lib.nrldpc_mix_tx_create(9, arr, cnt, 0, None) == C.ERR_ARG
    for bad in (dict(n_tb=[1, 2]), dict(n_tb=n_tb + [1])):
        with pytest.raises(pkg.NRLDPCError):
            pkg.mix_tx_layout(ps, **bad)
    # too large for one launch: 2^31 transport blocks
    rc, msg = _both(pkg, good[:2], [2 ** 31 - 1, 1])
    assert rc == C.ERR_UNSUPPORTED and b"too large for one launch" in msg
    # stage calls on a null plan
    assert lib.nrldpc_mix_tx_crc_attach_dev(None, P, P, NULL) == C.ERR_ARG
    assert lib.nrldpc_mix_tx_encode_dev(None, None, P, P, NULL) == C.ERR_ARG
    assert lib.nrldpc_mix_tx_rate_match_dev(None, P, P, NULL) == C.ERR_ARG
    lib.nrldpc_mix_tx_destroy(None)  # as free(NULL)


def test_the_empty_plan_needs_no_device_and_does_nothing(pkg):
    """n == 0, and a mix whose counts are all zero, are valid plans: created without any device call, all three stage calls return OK
    without a launch, null base pointers and handles included."""
    ps, _ = p9(pkg)
    for plan in (pkg.MixTxPlan([], []), pkg.MixTxPlan(ps, [0] * 9)):
        assert plan.a_off == [0] * (plan.n + 1) and (as_array(plan.off) == 0).all()
        for d in (None, 0x1000):
            plan.crc_attach(d, d)
            plan.encode([None] * plan.n, d, d)
            plan.rate_match(d, d)
        with pytest.raises(pkg.NRLDPCError):
            plan.encode([None] * (plan.n + 1), None, None)
        plan.close()
        plan.close()


def test_chain_refuses_bad_tensors_before_device_work(pkg):
    import torch
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    ps, n_tb = p9(pkg)
    with pytest.raises(pkg.NRLDPCError):
        DC.MixedEncodeChain(ps, n_tb[:3])
    chain = DC.MixedEncodeChain(ps, [0] * 9)  # an empty plan: no device, no codec
    assert chain.plan.totals()["a"] == 0 and chain.codecs == [None] * 9
    for bad in (torch.zeros(16, dtype=torch.float32), torch.zeros(16, dtype=torch.int8), torch.zeros((4, 4), dtype=torch.uint8),
                torch.zeros(32, dtype=torch.uint8)[::2], np.zeros(16, np.uint8)):
        with pytest.raises(pkg.NRLDPCError, match="contiguous 1-D uint8"):
            chain.step(bad)
    with pytest.raises(pkg.NRLDPCError, match="lives on cpu"):
        chain.step(torch.zeros(16, dtype=torch.uint8))  # the right type, the wrong device
    for field in ("harq", "b_hat", "x"):
        with pytest.raises(pkg.NRLDPCError, match="unknown field"):
            chain.views(torch.zeros(16, dtype=torch.uint8), field)
    chain.close()
    chain.close()


# ---- census: what the test plans of tests/test_mix_tx_gpu.py reach ---------------------------------------------------------------------
def rm_plan_census(pkg, sets):
    """Run classes and store forms nrldpc_mix_tx_rate_match_kernel reaches on the plan made of `sets` (T.RM_N_TB blocks each) at an
    aligned base: the conditions are nrldpc_rate_match_kernel's (T.rm_census), the address of a row's first byte is the segment's
    offset in the packed g array plus what the single call adds."""
    ps = [pkg.NRLDPC(**kw) for kw in sets]
    for p in ps:
        p.validate()
    off = pkg.mix_layout(ps, [T.RM_N_TB] * len(ps))
    runs, stores = set(), set()
    for i, kw in enumerate(sets):
        r, s = T.rm_census(T.derive(kw), offsets=((0, off[i].g),), n_tb=T.RM_N_TB)
        runs |= r
        stores |= s
    return runs, stores


def crc_plan_census(pkg, sets, base_offsets):
    """Attach classes nrldpc_mix_tx_crc_attach_kernel reaches on the plan made of `sets` with (a, c) base pointers at the byte offsets
    `base_offsets` above a 16-byte boundary: the (source phase, destination phase, rotation) of every stage_row -> store_row pair
    (T._store_visit) at the plan's real addresses, and the (C, L_tb) forms."""
    ps = [pkg.NRLDPC(**kw) for kw, _ in sets]
    for p in ps:
        p.validate()
    cnt = [k for _, k in sets]
    a_off, off = pkg.mix_tx_layout(ps, cnt), pkg.mix_layout(ps, cnt)
    have = set()
    for i, (kw, n_tb) in enumerate(sets):
        ref = T.derive(kw)
        C_, K, A = ref["C"], ref["K"], ref["A"]
        pay = ref["K_prime"] - ref["code_block_L"]
        have.add(("C", C_, "L_tb", ref["transport_block_L"]))
        for so, do in base_offsets:
            for tb in range(n_tb):
                for r in range(C_):
                    src = so + a_off[i] + tb * A + r * pay
                    s, d, rot = T._store_visit(src % 16, do + off[i].c_hat + (tb * C_ + r) * K, K)
                    have |= {("attach", "src,dst", s, d), ("attach", "dst,rot", d, rot), ("attach", "rot", rot)}
    return have


CRC_PAIRS = [(a, c) for a in T.CRC_OFFSETS for c in T.CRC_OFFSETS]


def test_census_the_test_plans_reach_every_path_of_both_kernels(pkg):
    want_runs, want_stores = T.rm_universe()
    assert len(want_runs) == 45 and len(want_stores) == 10
    runs, stores = rm_plan_census(pkg, T.RM_SETS)
    missing = sorted(want_runs - runs) + sorted(want_stores - stores)
    assert not missing, "P_rm at an aligned base leaves unreached: %r" % missing
    # ... and needs its last set for it
    runs, stores = rm_plan_census(pkg, T.RM_SETS[:12])
    assert len(T.RM_SETS) == 13 and (want_runs - runs or want_stores - stores)

    want = {c for c in T.crc_universe() if c[0] == "attach"}
    forms = {c for c in T.crc_universe() if c[0] == "C"}
    assert len(want) == 324 and len(CRC_PAIRS) == 16
    aligned = crc_plan_census(pkg, T.CRC_SETS, [(0, 0)])
    assert len(want - aligned) == 257  # 16-aligned segment starts: an aligned base reaches little
    have = crc_plan_census(pkg, T.CRC_SETS, CRC_PAIRS)
    missing = sorted((want | forms) - have, key=repr)
    assert not missing, "P_crc at the 16 base-offset pairs leaves unreached: %r" % missing
    # ... and needs its last set for it
    assert (want | forms) - crc_plan_census(pkg, T.CRC_SETS[:-1], CRC_PAIRS)


# ---- the host walk under sanitizers -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/mix_host/mix_tx_check.cpp built once with the sanitizers (their runtimes linked statically: the program needs nothing
    preloaded)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path_factory.mktemp("mix_host") / "mix_tx_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mix_host", "mix_tx_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", sorted(PLANS) + ["zero-first-and-last"])
def test_mapping_and_layout_walked_on_the_cpu_under_sanitizers(pkg, checker, tmp_path, name):
    """csrc/nrldpc_mix_tx.h's layout arithmetic, records and workgroup -> work mapping of both grids, exercised by
    tests/mix_host/mix_tx_check.cpp (its own main, -fsanitize=address,undefined) over the three test plans: every byte of g and of c
    has exactly one writer, no gap byte is touched, every read of the codeword bytes lies inside its code block's circular buffer,
    every read of `a` inside its row, every LDS and part[] index inside the plan-wide carve-up, and the offsets the library reports
    are the header's."""
    if name in PLANS:
        ps, n_tb = PLANS[name](pkg)
    else:
        ps, n_tb = M.mix(pkg)[:4], [0, 2, 1, 0]
    off, a_off = pkg.mix_layout(ps, n_tb), pkg.mix_tx_layout(ps, n_tb)
    lines = [str(len(ps))]
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        lines.append(" ".join(str(int(x)) for x in [k, p.C, p.G, p.Z_c, p.K, int(p.K_prime), p.N, p.N_cb, p.A, p.B, p.code_block_L, p.k_0, p.Q_m,
                                                    *p.E_r, a_off[i], off[i].c_hat, off[i].cw, off[i].g]))
    n = len(ps)
    lines.append(" ".join(str(int(x)) for x in [a_off[n], off[n].c_hat, off[n].cw, off[n].g]))
    src = tmp_path / "mix_tx.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([checker, str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and "mix_tx_check ok" in out.stdout, out.stdout + out.stderr

"""Mixed transport-block batches (nrldpc_mix_*) at the C ABI and in the binding, without a device: the five functions and the offset
structure are declared, exported and bound; nrldpc_mix_layout equals a numpy restatement of the layout rule; every refusal comes
back before any HIP call (this file runs where there is no GPU) with the texts of the single-configuration calls; and the layout
arithmetic and the workgroup mapping of the two kernels (csrc/nrldpc_mix.h) are walked on the CPU by a stand-alone program built
with the address and undefined-behaviour sanitizers."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mix_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
NULL = None
NAMES = ("nrldpc_mix_layout", "nrldpc_mix_create", "nrldpc_mix_destroy", "nrldpc_mix_rate_recover_dev", "nrldpc_mix_crc_check_dev")
FIELDS = ("g", "harq", "cw", "c_hat", "cb", "b_hat", "tb")


def as_array(off):
    return np.array([[getattr(o, k) for k in FIELDS] for o in off], np.int64)


def test_symbols_are_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    for name in NAMES:
        assert name in C.EXPORTS and hasattr(lib, name) and re.search(r"\b(int|void) %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.nrldpc_mix_rate_recover_dev.argtypes) == 8 and len(lib.nrldpc_mix_crc_check_dev.argtypes) == 6
    assert "typedef struct nrldpc_mix* nrldpc_mix_handle;" in hdr and "} nrldpc_mix_offsets;" in hdr
    assert ctypes.sizeof(C.MixOffsets) == 56 and C.MIX_FIELDS == FIELDS
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    for out_of_scope in ("nrldpc_crc_check_harq_dev", "pool variants", "the transmit side", "the MEX gateway"):
        assert out_of_scope in hdr[hdr.index("mixed transport-block batches"):hdr.index("typedef struct nrldpc_mix*")]
    assert pkg.MixPlan is C.MixPlan and pkg.mix_layout is C.mix_layout
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    assert hasattr(DC, "MixedDecodeChain")


def test_new_unit_is_built_and_is_not_part_of_the_decoder_kernels_identity(pkg):
    bld = pkg._capi._build
    assert "nrldpc_mix.hip" in bld.SOURCES and "nrldpc_mix.h" in bld.HEADERS
    assert not {"nrldpc_mix.hip", "nrldpc_mix.h"} & set(bld.KERNEL_SOURCES)
    kernels_h = open(os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc", "nrldpc_kernels.h")).read()
    assert "Mix" not in kernels_h  # the argument structures stay out of the decoder's identity
    assert bld.kernel_id() == pkg.load().nrldpc_kernel_id().decode() == "a54d4abae9865fdf"  # the parent commit's value


def test_layout_equals_the_rule_on_the_nine_set_mix(pkg):
    ps = M.mix(pkg)
    off = pkg.mix_layout(ps, M.N_TB)
    got, want = as_array(off), M.layout(ps, M.N_TB)
    assert got.shape == (10, 7) and (got == want).all()
    assert (got[0] == 0).all() and (got % 16 == 0).all()
    empty = M.N_TB.index(0)
    assert (got[empty + 1] == got[empty]).all()  # a zero count takes no room
    # TbParams are accepted as well as parameter objects
    assert (as_array(pkg.mix_layout([pkg.tb_params(p) for p in ps], M.N_TB)) == want).all()
    # the segments of the decoder's arrays are those nrldpc_decode_multi_dev is given: whole codewords, K hard bits each
    for i, p in enumerate(ps):
        assert got[i + 1, 2] - got[i, 2] >= M.N_TB[i] * p.C * (2 * p.Z_c + p.N)


def test_layout_of_other_mixes(pkg):
    ps = M.mix(pkg)
    # every count zero; a single configuration; a permutation: segments follow in the caller's order
    assert (as_array(pkg.mix_layout(ps, [0] * 9)) == 0).all()
    assert (as_array(pkg.mix_layout(ps[4:5], [5])) == M.layout(ps[4:5], [5])).all()
    order = [8, 0, 5, 2, 7, 1, 3, 6, 4]
    assert (as_array(pkg.mix_layout([ps[i] for i in order], [M.N_TB[i] + 1 for i in order])) ==
            M.layout([ps[i] for i in order], [M.N_TB[i] + 1 for i in order])).all()
    # G == 0 is a legal draw of the reference's sweep (testbench.m:35): nothing transmitted, an empty g_tilde segment
    p0 = pkg.NRLDPC(BG=2, A=100, G=0, Q_m=2)
    p0.validate()
    assert p0.G == 0 and sum(p0.E_r) == 0
    got = as_array(pkg.mix_layout([ps[0], p0, ps[1]], [2, 3, 1]))
    assert (got == M.layout([ps[0], p0, ps[1]], [2, 3, 1])).all()
    assert got[2, 0] == got[1, 0] and got[2, 2] > got[1, 2]  # no g_tilde, but codeword LLRs (zeros and fillers) all the same
    # n == 0: one record, all zero
    off = pkg.mix_layout([], [])
    assert len(off) == 1 and (as_array(off) == 0).all()


def _arrays(pkg, ts, n_tb):
    C = pkg._capi
    n = len(ts)
    arr = (C.TbParams * max(n, 1))()
    for i, t in enumerate(ts):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(t), ctypes.sizeof(C.TbParams))
    return arr, (ctypes.c_int32 * max(n, 1))(*n_tb)


def _both(pkg, ts, n_tb, n=None, null_p=False, null_n=False):
    """(code, text) of nrldpc_mix_layout and of nrldpc_mix_create for the same arguments: they must agree, and create must leave
    no handle behind."""
    C = pkg._capi
    lib = pkg.load()
    arr, cnt = _arrays(pkg, ts, n_tb)
    n = len(ts) if n is None else n
    off = (C.MixOffsets * (max(n, 0) + 1))()
    rc1 = lib.nrldpc_mix_layout(n, None if null_p else arr, None if null_n else cnt, off)
    msg1 = lib.nrldpc_last_error()
    h = ctypes.c_void_p()
    rc2 = lib.nrldpc_mix_create(n, None if null_p else arr, None if null_n else cnt, 0, ctypes.byref(h))
    msg2 = lib.nrldpc_last_error()
    assert rc1 == rc2 and msg1 == msg2 and h.value is None, (rc1, msg1, rc2, msg2)
    return rc1, msg1


def test_parameter_refusals_carry_the_single_call_texts_and_the_configuration(pkg):
    """A broken parameter block anywhere in the mix: the code and the text nrldpc_rate_recover_ex_dev / nrldpc_crc_check_dev give
    for that block, with " (configuration i)" appended -- from nrldpc_mix_layout and from nrldpc_mix_create, before any device
    call."""
    C = pkg._capi
    lib = pkg.load()
    ps = M.mix(pkg)
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
        if stage == "rr":
            rc = lib.nrldpc_rate_recover_ex_dev(ctypes.byref(t), P, C.LLR_F32, 3, NULL, 0, P, C.LLR_F32, NULL)
        else:
            rc = lib.nrldpc_crc_check_dev(ctypes.byref(t), P, 3, P, P, NULL, NULL)
        return rc, lib.nrldpc_last_error()

    seen = set()
    for i, stage, kw in ((0, "rr", dict(C=0)), (1, "rr", dict(C=161)), (2, "rr", dict(Z=17)), (3, "rr", dict(bg=3)), (4, "rr", dict(Q_m=0)),
                         (5, "rr", dict(N_cb=0)), (6, "rr", dict(N_cb=10 ** 6)), (7, "rr", dict(K_prime=10 ** 6)), (8, "rr", dict(E0=13333)),
                         (0, "rr", dict(E0=-2)), (0, "rr", dict(E0=298)), (3, "rr", dict(G=5999)),
                         (2, "crc", dict(tb_crc_len=12)), (4, "crc", dict(cb_crc_len=16)), (6, "crc", dict(B=1)), (5, "crc", dict(A=5))):
        t = broken(i, **kw)
        rc, msg = single(t, stage)
        assert rc in (C.ERR_ARG, C.ERR_UNSUPPORTED), (i, kw)
        ts = list(good)
        ts[i] = t
        got = _both(pkg, ts, M.N_TB)
        assert got == (rc, msg + b" (configuration %d)" % i), (i, kw, got, msg)
        seen.add(msg)
    assert len(seen) >= 6  # check_tb_params, fill_rm_blocks and the CRC stage's own checks were all reached
    # the block of an EMPTY configuration is checked too, and the first broken block is the one reported
    ts = list(good)
    ts[3], ts[7] = broken(3, Z=17), broken(7, C=0)
    assert M.N_TB[3] == 0 and _both(pkg, ts, M.N_TB)[1].endswith(b"(configuration 3)")


def test_count_and_pointer_refusals(pkg):
    C = pkg._capi
    lib = pkg.load()
    good = [C.tb_params(p) for p in M.mix(pkg)]
    assert _both(pkg, good, M.N_TB, n=-1)[0] == C.ERR_ARG
    cnt = list(M.N_TB)
    cnt[5] = -1
    rc, msg = _both(pkg, good, cnt)
    assert rc == C.ERR_ARG and b"negative" in msg and msg.endswith(b"(configuration 5)")
    assert _both(pkg, good, M.N_TB, null_p=True)[0] == C.ERR_ARG
    assert _both(pkg, good, M.N_TB, null_n=True)[0] == C.ERR_ARG
    arr, cnt = _arrays(pkg, good, M.N_TB)
    assert lib.nrldpc_mix_layout(9, arr, cnt, None) == C.ERR_ARG
    assert lib.nrldpc_mix_create(9, arr, cnt, 0, None) == C.ERR_ARG
    for bad in (dict(n_tb=[1, 2]), dict(n_tb=list(M.N_TB) + [1])):
        with pytest.raises(pkg.NRLDPCError):
            pkg.mix_layout(M.mix(pkg), **bad)
    # stage calls on a null plan
    assert lib.nrldpc_mix_rate_recover_dev(None, P, 0, NULL, 0, P, 0, NULL) == C.ERR_ARG
    assert lib.nrldpc_mix_crc_check_dev(None, P, P, P, NULL, NULL) == C.ERR_ARG
    lib.nrldpc_mix_destroy(None)  # as free(NULL)


def test_the_empty_plan_needs_no_device_and_does_nothing(pkg):
    """n == 0, and a mix whose counts are all zero, are valid plans: created without any device call, both stage calls return OK
    without a launch (null base pointers included) -- yet a wrong element type is refused on them too."""
    C = pkg._capi
    for plan in (pkg.MixPlan([], []), pkg.MixPlan(M.mix(pkg), [0] * 9)):
        assert (as_array(plan.offsets) == 0).all() and plan.totals.g == 0
        for i in (C.LLR_F32, C.LLR_F16):
            for hd in (C.LLR_F32, C.LLR_F16):
                for od in (C.LLR_F32, C.LLR_F16):
                    plan.rate_recover(None, None, None, in_dtype=i, harq_dtype=hd, out_dtype=od)
                    plan.rate_recover(0x1000, 0x1000, 0x1000, in_dtype=i, harq_dtype=hd, out_dtype=od)
        plan.crc_check(None, None, None)
        plan.crc_check(0x1000, 0x1000, 0x1000, 0x1000)
        for bad in (C.LLR_F64, 3, -1):
            with pytest.raises(pkg.UnsupportedParameters, match="in_dtype"):
                plan.rate_recover(None, None, None, in_dtype=bad)
            with pytest.raises(pkg.UnsupportedParameters, match="harq_dtype"):
                plan.rate_recover(None, 0x1000, None, harq_dtype=bad)
            with pytest.raises(pkg.UnsupportedParameters, match="out_dtype"):
                plan.rate_recover(None, None, None, out_dtype=bad)
            plan.rate_recover(None, None, None, harq_dtype=bad)  # harq_dtype is not read without a buffer
        plan.close()
        plan.close()


def test_chain_refuses_unknown_settings_before_device_work(pkg):
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    ps = M.mix(pkg)
    with pytest.raises(pkg.UnsupportedParameters):
        DC.MixedDecodeChain(ps, M.N_TB, algorithm="belief")
    with pytest.raises(pkg.UnsupportedParameters):
        DC.MixedDecodeChain(ps, M.N_TB, llr_dtype="int8")
    with pytest.raises(pkg.NRLDPCError):
        DC.MixedDecodeChain(ps, M.N_TB[:3])


MIXES = {
    "nine-set": lambda ps: (ps, M.N_TB),
    "all-present": lambda ps: (ps, [k + 1 for k in M.N_TB]),
    "zero-first-and-last": lambda ps: (ps[:4], [0, 2, 1, 0]),
    "split-tail": lambda ps: (ps[1:3], [M.N_TB[1], M.N_TB[2]]),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/mix_host/mix_map_check.cpp built once with the sanitizers (their runtimes linked statically: the program needs nothing
    preloaded)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path_factory.mktemp("mix_host") / "mix_map_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mix_host", "mix_map_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", sorted(MIXES))
def test_mapping_and_layout_walked_on_the_cpu_under_sanitizers(pkg, checker, tmp_path, name):
    """csrc/nrldpc_mix.h's layout arithmetic and workgroup -> (configuration, code block, tile) mapping, exercised by
    tests/mix_host/mix_map_check.cpp (its own main, -fsanitize=address,undefined) over the test mixes: every workgroup of both grids
    lands inside its segment, every element of every segment has exactly one owner, no gap element is touched, and the offsets the
    library reports are the header's."""
    ps, n_tb = MIXES[name](M.mix(pkg))
    off = as_array(pkg.mix_layout(ps, n_tb))
    lines = [str(len(ps))]
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        lines.append(" ".join(str(int(x)) for x in [k, p.C, p.G, p.Z_c, p.K, int(p.K_prime), p.N, p.N_cb, p.B, *p.E_r, *off[i]]))
    lines.append(" ".join(str(int(x)) for x in off[len(ps)]))
    src = tmp_path / "mix.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([checker, str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and "mix_map_check ok" in out.stdout, out.stdout + out.stderr

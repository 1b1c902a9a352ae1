"""HARQ / CBGTI state on mixed transport-block batches (nrldpc_mix_rate_recover_harq_dev, nrldpc_mix_crc_check_harq_dev) at the C ABI
and in the binding, without a device: the two functions are declared, exported and bound; the decoder kernels' identities did not
move; the layout of the nine-set mix does not depend on rv_id (one plan per redundancy version shares the packed arrays); both calls
return OK on the empty plan without a device, and refuse what they must before any HIP call; MixedDecodeChain refuses a bad
harq_dtype before device work; and the flag addressing of the two HARQ kernels (csrc/nrldpc_mix.h) is walked on the CPU by a
stand-alone program built with the address and undefined-behaviour sanitizers."""
import copy
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
NAMES = ("nrldpc_mix_rate_recover_harq_dev", "nrldpc_mix_crc_check_harq_dev")
FIELDS = ("g", "harq", "cw", "c_hat", "cb", "b_hat", "tb")
P = 0x1000  # a non-null address nothing may dereference: every call below is refused, or has nothing to do


def as_array(off):
    return np.array([[getattr(o, k) for k in FIELDS] for o in off], np.int64)


def test_symbols_are_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    for name in NAMES:
        assert name in C.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.nrldpc_mix_rate_recover_harq_dev.argtypes) == 9 and len(lib.nrldpc_mix_crc_check_harq_dev.argtypes) == 8
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    section = hdr[hdr.index("mixed transport-block batches"):hdr.index("typedef struct nrldpc_mix*")]
    assert "Out of scope: the HARQ / CBGTI state machine" not in section
    assert "one plan per redundancy version" in re.sub(r"[\s*]+", " ", section)  # (a plan is immutable; rv_id only moves k_0)
    assert callable(C.MixPlan.rate_recover_harq) and callable(C.MixPlan.crc_check_harq)
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    assert "Out of scope" not in DC.MixedDecodeChain.__doc__ and "keeps no HARQ state" not in DC.MixedDecodeChain.__doc__
    assert hasattr(DC.MixedDecodeChain, "reset")


def test_decoder_kernel_identities_did_not_move(pkg):
    bld = pkg._capi._build
    assert bld.kernel_id() == pkg.load().nrldpc_kernel_id().decode() == "a54d4abae9865fdf"  # the parent commit's values
    assert bld.pair_search_id() == "adf9a346d16d6f78"
    assert bld.SOURCES.count("nrldpc_mix.hip") == 1 and not [s for s in bld.SOURCES if "harq" in s]  # the existing translation unit


def test_layout_does_not_depend_on_rv_id(pkg):
    ps = M.mix(pkg)
    base = as_array(pkg.mix_layout(ps, M.N_TB))
    k0 = set()
    for rv in range(4):
        qs = []
        for p in ps:
            q = copy.copy(p)
            q.rv_id = rv
            qs.append(q)
        assert (as_array(pkg.mix_layout(qs, M.N_TB)) == base).all(), rv
        k0.add(tuple(q.k_0 for q in qs))
    assert len(k0) == 4  # (the four versions are four different plans all the same)


def test_the_empty_plan_needs_no_device_and_does_nothing(pkg):
    C = pkg._capi
    for plan in (pkg.MixPlan([], []), pkg.MixPlan(M.mix(pkg), [0] * 9)):
        for i in (C.LLR_F32, C.LLR_F16):
            for hd in (C.LLR_F32, C.LLR_F16):
                for od in (C.LLR_F32, C.LLR_F16):
                    plan.rate_recover_harq(None, None, None, None, in_dtype=i, harq_dtype=hd, out_dtype=od)
                    plan.rate_recover_harq(P, P, P, P, in_dtype=i, harq_dtype=hd, out_dtype=od)
        plan.crc_check_harq(None, None, None, None)
        plan.crc_check_harq(P, P, P, P, P, P)
        for bad in (C.LLR_F64, 3, -1):
            with pytest.raises(pkg.UnsupportedParameters, match="in_dtype"):
                plan.rate_recover_harq(None, None, None, in_dtype=bad)
            with pytest.raises(pkg.UnsupportedParameters, match="harq_dtype"):
                plan.rate_recover_harq(None, None, None, harq_dtype=bad)
            with pytest.raises(pkg.UnsupportedParameters, match="out_dtype"):
                plan.rate_recover_harq(None, None, None, out_dtype=bad)
        plan.close()
    lib = pkg.load()
    assert lib.nrldpc_mix_rate_recover_harq_dev(None, P, 0, P, 0, P, 0, None, None) == C.ERR_ARG  # a null plan
    assert lib.nrldpc_mix_crc_check_harq_dev(None, P, P, P, P, None, None, None) == C.ERR_ARG


def test_chain_refuses_a_bad_harq_dtype_before_device_work(pkg):
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    ps = M.mix(pkg)
    for bad in (int, "int8", np.float64):
        with pytest.raises(pkg.UnsupportedParameters, match="harq_dtype"):
            DC.MixedDecodeChain(ps, M.N_TB, I_HARQ=1, harq_dtype=bad)


MIXES = {
    "nine-set": lambda ps: (ps, M.N_TB),
    "all-present": lambda ps: (ps, [k + 1 for k in M.N_TB]),
    "zero-first-and-last": lambda ps: (ps[:4], [0, 2, 1, 0]),
    "split-tail": lambda ps: (ps[1:3], [M.N_TB[1], M.N_TB[2]]),
}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/mix_host/mix_harq_check.cpp built once with the sanitizers (their runtimes linked statically: the program needs nothing
    preloaded)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path_factory.mktemp("mix_host") / "mix_harq_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mix_host", "mix_harq_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", sorted(MIXES))
def test_flag_addressing_walked_on_the_cpu_under_sanitizers(pkg, checker, tmp_path, name):
    """Every d_new / d_cbgti index the two HARQ kernels form, over every workgroup of both grids of the test mixes, on flag arrays of
    exactly the packed sizes: inside its segment, one reader per transport block / code block, no gap element touched."""
    ps, n_tb = MIXES[name](M.mix(pkg))
    off = as_array(pkg.mix_layout(ps, n_tb))
    lines = [str(len(ps))]
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        lines.append(" ".join(str(int(x)) for x in [k, p.C, p.G, p.Z_c, p.K, int(p.K_prime), p.N, p.N_cb, p.B, *p.E_r, *off[i]]))
    lines.append(" ".join(str(int(x)) for x in off[len(ps)]))
    src = tmp_path / "mix.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([checker, str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and "mix_harq_check ok" in out.stdout, out.stdout + out.stderr

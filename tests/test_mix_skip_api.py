"""Mixed HARQ steps that decode only the pending code blocks (nrldpc_mix_pending_dev, nrldpc_mix_gather_cw_dev,
nrldpc_mix_scatter_hard_dev; MixedDecodeChain(skip=...)) at the C ABI and in the binding, without a device: the three functions are
declared, exported and bound; the decoder kernels' identities did not move and the new translation unit is outside them; all three
return OK on the empty plan and refuse what they must before any HIP call; MixedDecodeChain refuses a bad skip before device work; and
the rule, the compaction, the workgroup mapping and the row copy (csrc/nrldpc_mix_skip.h) are walked on the CPU by a stand-alone program
built with the address and undefined-behaviour sanitizers."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mix_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrldpc_mix_pending_dev", "nrldpc_mix_gather_cw_dev", "nrldpc_mix_scatter_hard_dev")
P = 0x1000  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
Z9 = dict(BG=2, A=36, G=120, Q_m=2)  # the configuration with a 2-byte aligned hard-bit row: Z_c = 9, K = 90
Z9_N_TB = 5


def test_symbols_are_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    for name in NAMES:
        assert name in C.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, hdr), name
        assert getattr(lib, name).argtypes is not None, name
    assert [len(getattr(lib, name).argtypes) for name in NAMES] == [9, 7, 8]
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    assert hdr.index("int nrldpc_mix_crc_check_harq_dev(") < hdr.index("int nrldpc_mix_pending_dev(") < hdr.index("int nrldpc_crc_attach_dev(")
    assert "#define NRLDPC_MIX_SKIP_UNSCHEDULED 1" in hdr and "#define NRLDPC_MIX_SKIP_SETTLED 2" in hdr
    assert (C.MIX_SKIP_UNSCHEDULED, C.MIX_SKIP_SETTLED) == (1, 2)
    assert "DEVIATION from the reference" in hdr and "d_c_hat is in/out" in hdr
    assert callable(C.MixPlan.pending) and callable(C.MixPlan.gather_cw) and callable(C.MixPlan.scatter_hard)
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    assert '"unscheduled"' in DC.MixedDecodeChain.__doc__ and '"settled"' in DC.MixedDecodeChain.__doc__


def test_decoder_kernel_identities_did_not_move(pkg):
    bld = pkg._capi._build
    assert bld.kernel_id() == pkg.load().nrldpc_kernel_id().decode() == "a54d4abae9865fdf"  # the values tests/test_mix_harq_api.py pins
    assert bld.pair_search_id() == "adf9a346d16d6f78"
    assert bld.SOURCES.count("nrldpc_mix_skip.hip") == 1 and bld.HEADERS.count("nrldpc_mix_skip.h") == 1
    assert not {"nrldpc_mix_skip.hip", "nrldpc_mix_skip.h"} & set(bld.KERNEL_SOURCES)
    csrc = os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc")
    assert "Mix" not in open(os.path.join(csrc, "nrldpc_kernels.h")).read()
    skip_h = open(os.path.join(csrc, "nrldpc_mix_skip.h")).read()
    assert "nrldpc_kernels.h\"" not in skip_h and "nrldpc_mix.h\"" not in skip_h  # nothing that would drag it into the decoder's identity


def test_the_empty_plan_needs_no_device_and_does_nothing(pkg):
    C = pkg._capi
    for plan in (pkg.MixPlan([], []), pkg.MixPlan(M.mix(pkg), [0] * 9)):
        for rule in (C.MIX_SKIP_UNSCHEDULED, C.MIX_SKIP_SETTLED):
            plan.pending(rule, None, None, None, None, None, None)
            plan.pending(rule, P, P, P, P, P, P)
        for dt in (C.LLR_F32, C.LLR_F16):
            plan.gather_cw(None, None, None, None, dtype=dt)
            plan.gather_cw(P, P, P, P, dtype=dt)
        plan.scatter_hard(None, None, None, None, None, None)
        plan.scatter_hard(P, P, P, P, P, P)
        for bad in (0, 3, -1):
            with pytest.raises(pkg.UnsupportedParameters, match="rule"):
                plan.pending(bad, P, P, P, P, P, P)
        for bad in (C.LLR_F64, 3, -1):
            with pytest.raises(pkg.UnsupportedParameters, match="dtype"):
                plan.gather_cw(P, P, P, P, dtype=bad)
        plan.close()
    lib = pkg.load()
    assert lib.nrldpc_mix_pending_dev(None, 1, P, P, None, None, P, P, None) == C.ERR_ARG  # a null plan
    assert lib.nrldpc_mix_gather_cw_dev(None, P, 0, P, P, P, None) == C.ERR_ARG
    assert lib.nrldpc_mix_scatter_hard_dev(None, P, P, P, P, P, P, None) == C.ERR_ARG


def test_chain_refuses_a_bad_skip_before_device_work(pkg):
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    ps = M.mix(pkg)
    for bad in ("nonsense", "", 1, True, ["settled"]):
        with pytest.raises(pkg.UnsupportedParameters, match="skip"):
            DC.MixedDecodeChain(ps, M.N_TB, I_HARQ=1, skip=bad)
    for rule in ("settled", "unscheduled"):
        with pytest.raises(pkg.UnsupportedParameters, match="I_HARQ"):
            DC.MixedDecodeChain(ps, M.N_TB, I_HARQ=0, skip=rule)
        with pytest.raises(pkg.UnsupportedParameters, match="I_HARQ"):
            DC.MixedDecodeChain(ps, M.N_TB, skip=rule)


def test_rule_compaction_mapping_and_copy_walked_on_the_cpu_under_sanitizers(pkg, tmp_path):
    """tests/mix_host/mix_skip_check.cpp, built with the sanitizers (their runtimes linked statically: the program needs nothing
    preloaded) and run as a child process on the nine-set mix plus the Z_c = 9 configuration."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path / "mix_skip_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mix_host", "mix_skip_check.cpp"), "-o", exe])
    z9 = pkg.NRLDPC(**Z9)
    z9.validate()
    assert z9.Z_c == 9 and z9.K == 90 and z9.C == 1
    ps, n_tb = M.mix(pkg) + [z9], list(M.N_TB) + [Z9_N_TB]
    off = pkg.mix_layout(ps, n_tb)
    lines = [str(len(ps))]
    for p, k, o in zip(ps, n_tb, off):
        lines.append(" ".join(str(int(x)) for x in [k, p.C, p.Z_c, 2 * p.Z_c + p.N, p.K, o.cw, o.c_hat, o.cb, o.tb]))
    lines.append(" ".join(str(int(x)) for x in [off[-1].cw, off[-1].c_hat, off[-1].cb, off[-1].tb]))
    src = tmp_path / "mix.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and "mix_skip_check ok" in out.stdout, out.stdout + out.stderr
    for part in ("rule ok", "compaction ok", "copy ok", "mix ok: 10 configurations"):
        assert part in out.stdout, out.stdout

"""nrldpc_rate_recover_ex_dev (f16 demodulator LLRs, f16 HARQ buffer) at the C ABI and in the binding, without a device: the
symbol is declared, exported and bound, every refusal comes back before any HIP call (this file runs where there is no GPU), and
the new unit is outside the decoder kernels' identity."""
import ctypes
import importlib
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
NULL = None
NAME = "nrldpc_rate_recover_ex_dev"


def test_symbol_is_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    assert NAME in C.EXPORTS and hasattr(lib, NAME) and re.search(r"\bint %s\(" % NAME, hdr)
    assert lib.nrldpc_rate_recover_ex_dev.argtypes is not None and len(lib.nrldpc_rate_recover_ex_dev.argtypes) == 9
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    assert NAME in hdr[hdr.index("Rate recovery: replaces"):hdr.index("int nrldpc_rate_recover_dev(")]  # the old call points to the new one


def test_new_unit_is_built_and_is_not_part_of_the_decoder_kernels_identity(pkg):
    bld = pkg._capi._build
    assert "nrldpc_ratematch_ex.hip" in bld.SOURCES and "nrldpc_ratematch_ex.h" in bld.HEADERS
    assert not {"nrldpc_ratematch_ex.hip", "nrldpc_ratematch_ex.h", "nrldpc_ratematch.hip"} & set(bld.KERNEL_SOURCES)
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_pmc_summary.json")))
    assert bld.kernel_id() == d["_nrldpc_kernel_id"] == "a54d4abae9865fdf"


def _call(pkg, t, **kw):
    C = pkg._capi
    a = dict(p=ctypes.byref(t) if t is not None else None, g=P, i=C.LLR_F16, n=3, h=P, hd=C.LLR_F16, o=P, od=C.LLR_F16)
    a.update(kw)
    return pkg.load().nrldpc_rate_recover_ex_dev(a["p"], a["g"], a["i"], a["n"], a["h"], a["hd"], a["o"], a["od"], NULL)


def test_refusals_come_before_any_device_call(pkg):
    C = pkg._capi
    err = pkg.load().nrldpc_last_error
    p = pkg.NRLDPC(BG=2, A=100, G=300, Q_m=2)
    p.validate()
    t = C.tb_params(p)
    for bad in (C.LLR_F64, 3, -1):
        assert _call(pkg, t, i=bad) == C.ERR_UNSUPPORTED and b"in_dtype" in err()
        assert _call(pkg, t, hd=bad) == C.ERR_UNSUPPORTED and b"harq_dtype" in err()
        assert _call(pkg, t, od=bad) == C.ERR_UNSUPPORTED and b"out_dtype" in err()
        assert _call(pkg, t, i=bad, n=0) == C.ERR_UNSUPPORTED   # a type is wrong whatever the size
    assert _call(pkg, t, n=0, h=NULL, hd=77) == C.OK          # harq_dtype is not read without a buffer
    assert _call(pkg, None) == C.ERR_ARG and err() == b"null parameters"
    assert _call(pkg, t, n=-1) == C.ERR_ARG and err() == b"negative batch"
    assert _call(pkg, t, g=NULL) == C.ERR_ARG and err() == b"null pointer"
    assert _call(pkg, t, o=NULL) == C.ERR_ARG and err() == b"null pointer"
    # nothing to do: OK without a launch, null pointers included, for every combination of types
    for i in (C.LLR_F32, C.LLR_F16):
        for hd in (C.LLR_F32, C.LLR_F16):
            for od in (C.LLR_F32, C.LLR_F16):
                assert _call(pkg, t, n=0, i=i, hd=hd, od=od) == C.OK
                assert _call(pkg, t, n=0, i=i, hd=hd, od=od, g=NULL, h=NULL, o=NULL) == C.OK


def test_parameter_checks_are_those_of_the_existing_call(pkg):
    """The same parameter blocks refused by nrldpc_rate_recover_dev and by the new call: same code, same text."""
    C = pkg._capi
    lib = pkg.load()
    p = pkg.NRLDPC(BG=2, A=100, G=300, Q_m=2)
    p.validate()

    def broken(**kw):
        t = C.tb_params(p)
        for k, v in kw.items():
            if k == "E0":
                t.E_r[0] = v
            else:
                setattr(t, k, v)
        return t

    for kw in (dict(C=0), dict(C=161), dict(Z=17), dict(bg=3), dict(Q_m=0), dict(N_cb=0), dict(N_cb=10 ** 6), dict(K_prime=10 ** 6),
               dict(E0=299), dict(E0=-2), dict(E0=298)):
        t = broken(**kw)
        old = lib.nrldpc_rate_recover_dev(ctypes.byref(t), P, 3, P, P, C.LLR_F32, NULL)
        old_msg = lib.nrldpc_last_error()
        assert old in (C.ERR_ARG, C.ERR_UNSUPPORTED), kw
        assert _call(pkg, t) == old and lib.nrldpc_last_error() == old_msg, kw


def test_binding_and_chain_refuse_unknown_types_before_device_work(pkg):
    C = pkg._capi
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    H = importlib.import_module("ldpc-3gpp-matlab_amd.harness")
    p = pkg.NRLDPC(BG=2, A=100, G=300, Q_m=2)
    for bad in ("int8", "float64", "half-precision"):
        with pytest.raises(pkg.UnsupportedParameters):
            DC.DeviceDecodeChain(p, I_HARQ=1, harq_dtype=bad)
    with pytest.raises(pkg.UnsupportedParameters):
        H.simulate_point_device([], 2, 0.0, [0], 0, 1, 0, channel=lambda tx, N0, first: tx, llr_dtype="int8")
    with pytest.raises(pkg.UnsupportedParameters, match="in_dtype"):
        pkg.rate_recover_dev(p, 0x1000, 3, 0x1000, 0x1000, in_dtype=C.LLR_F64)
    with pytest.raises(pkg.UnsupportedParameters, match="harq_dtype"):
        pkg.rate_recover_dev(p, 0x1000, 3, 0x1000, 0x1000, harq_dtype=C.LLR_F64)
    pkg.rate_recover_dev(p, None, 0, None, None, in_dtype=C.LLR_F16, harq_dtype=C.LLR_F16)  # nothing to do

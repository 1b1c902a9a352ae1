"""The stand-alone mapper / demapper at the C ABI and in the binding, without a device: every refusal of nrldpc_modulate_dev /
nrldpc_demodulate_dev comes back before any HIP call (this file runs where there is no GPU), the symbols are exported, and the
method names map to the three NRLDPC_DEMOD_* codes."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
NULL = None


def test_symbols_are_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    for name in ("nrldpc_modulate_dev", "nrldpc_demodulate_dev"):
        assert name in C.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, hdr), name
    for name, code in (("NRLDPC_DEMOD_LLR", 0), ("NRLDPC_DEMOD_APPROX_LLR", 1), ("NRLDPC_DEMOD_HARD", 2)):
        assert re.search(r"#define %s %d\b" % (name, code), hdr), name
    assert (C.DEMOD_LLR, C.DEMOD_APPROX_LLR, C.DEMOD_HARD) == (0, 1, 2)
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == 6  # added without a revision bump
    for name in ("modulate_dev", "demodulate_dev", "NRModulator", "NRDemodulator"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    bld = C._build
    assert "nrldpc_modem.hip" in bld.SOURCES and "nrldpc_modem.h" in bld.HEADERS
    assert not {"nrldpc_modem.hip", "nrldpc_modem.h", "nrldpc_channel.hip"} & set(bld.KERNEL_SOURCES)  # not part of the decoder kernels' identity


def test_method_names(pkg):
    C = pkg._capi
    for name, code in (("llr", 0), ("approx", 1), ("hard", 2), ("Log-likelihood ratio", 0), ("Approximate log-likelihood ratio", 1),
                       ("Hard decision", 2)):
        assert C.demod_method_code(name) == code, name
    for bad in ("LLR", "soft", None, 3):
        with pytest.raises(pkg.UnsupportedParameters):
            C.demod_method_code(bad)
    with pytest.raises(pkg.UnsupportedParameters):  # refused in the binding: the library is not called
        pkg.demodulate_dev(0x1000, 4, 2, 0x1000, method="soft")


def test_modulate_refusals_come_before_any_device_call(pkg):
    C = pkg._capi
    f = pkg.load().nrldpc_modulate_dev
    for Q_m in (0, 3, 5, 7, 10, -2):  # 3 = 8PSK (NRModulator.m:83)
        assert f(P, 840, Q_m, P, NULL) == C.ERR_UNSUPPORTED, Q_m
        assert pkg.load().nrldpc_last_error() == b"Unsupported modulation"
    assert f(P, 7, 2, P, NULL) == C.ERR_ARG          # no multiple of Q_m
    assert f(P, 10, 4, P, NULL) == C.ERR_ARG
    assert f(P, -8, 8, P, NULL) == C.ERR_ARG         # negative size
    assert f(NULL, 8, 2, P, NULL) == C.ERR_ARG       # null pointer with a non-zero size
    assert f(P, 8, 2, NULL, NULL) == C.ERR_ARG
    for Q_m in (1, 2, 4, 6, 8):                      # nothing to do: OK without a launch, null pointers included
        assert f(NULL, 0, Q_m, NULL, NULL) == C.OK
    with pytest.raises(pkg.UnsupportedParameters, match="Unsupported modulation"):
        pkg.modulate_dev(0x1000, 30, 3, 0x1000)
    with pytest.raises(pkg.NRLDPCError):
        pkg.modulate_dev(0x1000, 7, 2, 0x1000)


def test_demodulate_refusals_come_before_any_device_call(pkg):
    C = pkg._capi
    f = pkg.load().nrldpc_demodulate_dev
    ok = dict(rx=P, n=64, Q_m=4, method=C.DEMOD_LLR, variance=0.5, var=NULL, out=P, dt=C.LLR_F32)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["rx"], a["n"], a["Q_m"], a["method"], a["variance"], a["var"], a["out"], a["dt"], NULL)

    for Q_m in (0, 3, 5, 7, 16, -1):
        assert call(Q_m=Q_m) == C.ERR_UNSUPPORTED, Q_m
        assert pkg.load().nrldpc_last_error() == b"Unsupported modulation"
    for method in (-1, 3, 99):
        assert call(method=method) == C.ERR_UNSUPPORTED, method
    assert call(dt=C.LLR_F64) == C.ERR_UNSUPPORTED
    assert call(dt=C.LLR_F64, method=C.DEMOD_APPROX_LLR) == C.ERR_UNSUPPORTED
    assert call(n=-1) == C.ERR_ARG
    assert call(rx=NULL) == C.ERR_ARG and call(out=NULL) == C.ERR_ARG
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert call(variance=v) == C.ERR_ARG, v
        assert call(variance=v, n=0) == C.ERR_ARG, v
    # nothing to do: OK without a launch -- for every method, with null data pointers, and with a variance array in place of the scalar
    for method in (C.DEMOD_LLR, C.DEMOD_APPROX_LLR, C.DEMOD_HARD):
        for dt in (C.LLR_F32, C.LLR_F16):
            assert call(n=0, method=method, dt=dt, rx=NULL, out=NULL) == C.OK
    assert call(n=0, variance=0.0, var=P) == C.OK
    assert call(n=0, method=C.DEMOD_HARD, dt=C.LLR_F64) == C.OK  # out_dtype is not read for hard decisions
    with pytest.raises(pkg.UnsupportedParameters, match="Unsupported modulation"):
        pkg.demodulate_dev(0x1000, 10, 3, 0x1000)
    with pytest.raises(pkg.NRLDPCError):
        pkg.demodulate_dev(0x1000, 10, 2, 0x1000, variance=0.0)


def test_system_objects_refuse_what_the_reference_refuses(pkg):
    """Construction and the dependent properties need no device (NRModulator.m:29-63, NRDemodulator.m:31-65)."""
    for name, q in (("BPSK", 1), ("QPSK", 2), ("16QAM", 4), ("64QAM", 6), ("256QAM", 8)):
        m, d = pkg.NRModulator(Modulation=name), pkg.NRDemodulator(Modulation=name, DecisionMethod="Hard decision", Variance=0.25)
        assert (m.Q_m, m.ModulationOrder, d.Q_m, d.ModulationOrder) == (q, 1 << q, q, 1 << q)
        assert d.DecisionMethod == "Hard decision" and d.Variance == 0.25
    assert pkg.NRModulator().Modulation == "BPSK" and pkg.NRDemodulator().DecisionMethod == "Log-likelihood ratio"
    for cls in (pkg.NRModulator, pkg.NRDemodulator):
        with pytest.raises(pkg.UnsupportedParameters, match="Unsupported modulation"):
            cls(Modulation="8PSK")
    m = pkg.NRModulator(Modulation="QPSK")
    with pytest.raises(pkg.UnsupportedParameters):
        m.Modulation = "8PSK"
    with pytest.raises(pkg.UnsupportedParameters):
        pkg.NRDemodulator(DecisionMethod="Soft decision")
    with pytest.raises(pkg.UnsupportedParameters):
        pkg.NRDemodulator(OutputDataType="float64")

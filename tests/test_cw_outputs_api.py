"""The boundary of the whole-codeword / final-parity-check outputs (nrldpc_decode_cw, nrldpc_decode_cw_dev, nrldpc_cw_out):
declared, exported, bound with the structure size the header states -- and added without touching what the min-sum kernels are
compiled from.  All without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrldpc_decode_cw", "nrldpc_decode_cw_dev")


def _header():
    return open(os.path.join(ROOT, "include", "nrldpc.h")).read()


def test_header_declares_both_entry_points_and_the_output_structure():
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+nrldpc_decode_cw_dev\s*\(\s*nrldpc_handle\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*const\s+nrldpc_cw_out\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", code)
    assert re.search(r"int\s+nrldpc_decode_cw\s*\(\s*nrldpc_handle\s+\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*uint8_t\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*const\s+nrldpc_cw_out\s*\*\s*\w+\s*\)", code)
    st = re.search(r"typedef struct nrldpc_cw_out \{(.*?)\} nrldpc_cw_out;", code, re.S).group(1)
    fields = re.findall(r"(\w+\s*\*?)\s*(\w+)\s*;", st)
    assert [(t.replace(" ", ""), n) for t, n in fields] == [("uint32_t", "struct_size"), ("uint8_t*", "cw_packed"),
                                                            ("int32_t*", "unsatisfied"), ("uint8_t*", "checks_packed")]
    assert re.search(r"#define\s+NRLDPC_CW_SCRATCH_BYTES\s+\(64u\s*<<\s*20\)", txt)
    # added by symbol, not by a revision bump
    assert re.search(r"#define\s+NRLDPC_ABI_VERSION\s+6\b", txt)
    # the semantics are part of the header
    for phrase in ("nrldpc_last_layers", "NRLDPC_LAYERS_AUTO", "NRLDPC_ERR_UNSUPPORTED", "nrldpc_decode_multi_dev variants do not exist"):
        assert phrase in txt.split("whole-codeword hard decisions and final parity checks")[1].split("typedef struct nrldpc_cw_out")[0], phrase


def test_library_exports_both_entry_points(pkg):
    lib = pkg.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg._capi.EXPORTS
    assert lib.nrldpc_abi_version() == 6


def test_binding_structure_has_the_size_the_header_states(pkg):
    """The header's comment gives sizeof(nrldpc_cw_out) (the library static_asserts it); the ctypes structure must agree."""
    m = re.search(r"sizeof\(nrldpc_cw_out\)\s*==\s*(\d+)", _header())
    assert m
    CwOut = pkg._capi.CwOut
    assert ctypes.sizeof(CwOut) == int(m.group(1))
    capi = open(os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc", "nrldpc_capi.hip")).read()
    assert re.search(r"static_assert\(sizeof\(nrldpc_cw_out\)\s*==\s*%s\b" % m.group(1), capi)
    assert [f[0] for f in CwOut._fields_] == ["struct_size", "cw_packed", "unsatisfied", "checks_packed"]
    o = CwOut(None, 8, None)
    assert o.struct_size == ctypes.sizeof(CwOut) and o.cw_packed is None and o.unsatisfied == 8 and o.checks_packed is None
    assert pkg.CwOut is CwOut and hasattr(pkg.Codec, "decode_cw") and hasattr(pkg.Codec, "decode_cw_dev")


def test_the_min_sum_kernels_identity_is_untouched(pkg):
    """The new units are sources of the library, not of the decoder kernels: nrldpc_kernel_id() of the built library is the hash
    of KERNEL_SOURCES in the tree, which lists neither of them (the committed profiles are pinned to that hash by
    test_capi_symbols.py)."""
    bld = pkg._capi._build
    assert "nrldpc_cwout.hip" in bld.SOURCES and "nrldpc_cwout.h" in bld.HEADERS
    assert not {"nrldpc_cwout.hip", "nrldpc_cwout.h", "nrldpc_bp.h", "nrldpc_decode_bp.hip", "nrldpc_capi.hip"} & set(bld.KERNEL_SOURCES)
    assert pkg.load().nrldpc_kernel_id().decode() == bld.kernel_id()
    # nothing the decoder kernels are compiled from includes the new header
    csrc = os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc")
    for f in bld.KERNEL_SOURCES:
        assert "nrldpc_cwout" not in open(os.path.join(csrc, f)).read(), f


def test_mex_gateway_has_the_whole_codeword_command():
    src = open(os.path.join(ROOT, "matlab", "nrldpc_mex.cpp")).read()
    assert '"decode_cw"' in src and "nrldpc_decode_cw(" in src and "mxCreateLogicalMatrix(" in src

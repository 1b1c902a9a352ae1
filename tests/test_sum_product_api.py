"""The sum-product mode's boundary (NRLDPC_ALG_*): declared, exported, bound, and an unknown name refused -- all without a GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrldpc_set_algorithm", "nrldpc_get_algorithm", "nrldpc_pool_set_algorithm")


def _header():
    return open(os.path.join(ROOT, "include", "nrldpc.h")).read()


def test_header_declares_the_algorithm_selector():
    txt = _header()
    assert re.search(r"#define\s+NRLDPC_ALG_MIN_SUM\s+0\b", txt)
    assert re.search(r"#define\s+NRLDPC_ALG_SUM_PRODUCT\s+1\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+nrldpc_set_algorithm\s*\(\s*nrldpc_handle\s+\w+\s*,\s*int32_t\s+\w+\s*\)", code)
    assert re.search(r"int\s+nrldpc_get_algorithm\s*\(\s*nrldpc_handle\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)", code)
    assert re.search(r"int\s+nrldpc_pool_set_algorithm\s*\(\s*nrldpc_pool_handle\s+\w+\s*,\s*int32_t\s+\w+\s*\)", code)
    # added by symbol, not by a revision bump, and not as a field of nrldpc_cfg
    assert re.search(r"#define\s+NRLDPC_ABI_VERSION\s+6\b", txt)
    cfg = re.search(r"typedef struct nrldpc_cfg \{(.*?)\} nrldpc_cfg;", code, re.S).group(1)
    assert "algorithm" not in cfg


def test_library_exports_the_algorithm_selector(pkg):
    lib = pkg.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg._capi.EXPORTS


def test_binding_constants(pkg):
    C = pkg._capi
    assert (C.ALG_MIN_SUM, C.ALG_SUM_PRODUCT) == (0, 1)
    assert C.ALGORITHMS == {"min-sum": 0, "sum-product": 1}
    assert C.algorithm_code("sum-product") == C.ALG_SUM_PRODUCT and C.algorithm_name(0) == "min-sum"


@pytest.mark.parametrize("bad", ["bogus", "Sum-Product", "", None, 1])
def test_unknown_algorithm_is_refused_before_any_device_call(pkg, bad):
    """(Nothing here reaches nrldpc_create: the names are checked first.)"""
    with pytest.raises(pkg.UnsupportedParameters):
        pkg.Codec(1, 384, algorithm=bad)
    with pytest.raises(pkg.UnsupportedParameters):
        pkg.CodecPool(1, 384, [0], algorithm=bad)
    with pytest.raises(pkg.UnsupportedParameters):
        pkg.NRLDPCDecoder(A=100, BG=2, G=300, Q_m=2, algorithm=bad)


def test_mex_gateway_selects_the_algorithm():
    src = open(os.path.join(ROOT, "matlab", "nrldpc_mex.cpp")).read()
    assert '"set_algorithm"' in src and "nrldpc_set_algorithm(" in src
    assert "'sum-product'" in src and '"sum-product"' in src

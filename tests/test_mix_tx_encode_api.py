"""The one-launch mixed encoder (nrldpc_mix_tx_encode_all_dev) at the C ABI and in the binding, without a device: the function is
declared, exported and bound; its unit is built and stays out of the decoder kernels' identity; every refusal comes back before any
HIP call (this file runs where there is no GPU); a census on the plans' real offsets shows that the plan P_enc of
tests/test_mix_tx_encode_gpu.py reaches every path class of the encoder body (tests/tx_cases.py); and the records, the workgroup
mapping and the LDS carve-up (csrc/nrldpc_mix_tx.h) are walked on the CPU by a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import ctypes
import importlib
import inspect
import os
import re
import shutil
import subprocess

import pytest

import mix_cases as M
import mix_tx_enc_cases as E
import tx_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
NAME = "nrldpc_mix_tx_encode_all_dev"


def test_symbol_is_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    assert NAME in C.EXPORTS and hasattr(lib, NAME) and re.search(r"\bint %s\(" % NAME, hdr)
    assert len(getattr(lib, NAME).argtypes) == 4  # plan, c, cw, stream: no handle array
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    # declared below the transmit block, in a block of its own that says the per-configuration call remains
    assert hdr.index("typedef struct nrldpc_mix_tx*") < hdr.index("int nrldpc_mix_tx_rate_match_dev(") < hdr.index("int %s(" % NAME)
    block = hdr[hdr.index("the transmit plan's encode stage in ONE launch"):hdr.index("int %s(" % NAME)]
    for phrase in ("nrldpc_mix_tx_encode_dev remains", "no handle array", "never written again", "ONE launch whatever n"):
        assert phrase in block, phrase
    assert callable(C.MixTxPlan.encode_all)
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    sig = inspect.signature(DC.MixedEncodeChain.__init__)
    assert sig.parameters["one_launch_encode"].default is False  # the default chain stays the per-configuration loop


def test_new_unit_is_built_and_is_not_part_of_the_decoder_kernels_identity(pkg):
    bld = pkg._capi._build
    assert "nrldpc_mix_tx_enc.hip" in bld.SOURCES and "nrldpc_mix_tx_enc.hip" not in bld.KERNEL_SOURCES
    assert os.path.exists(os.path.join(bld.CSRC, "nrldpc_mix_tx_enc.hip"))
    kernels_h = open(os.path.join(bld.CSRC, "nrldpc_kernels.h")).read()
    assert "Mix" not in kernels_h  # the argument structures stay out of the decoder's identity
    assert bld.kernel_id() == pkg.load().nrldpc_kernel_id().decode() == "a54d4abae9865fdf"  # the parent commit's value
    # the single-configuration encoder's unit does not know the new one, and the new one does not take its arguments
    assert "mix" not in open(os.path.join(bld.CSRC, "nrldpc_encode.hip")).read().lower()
    assert "nrldpc_kernels.h" not in open(os.path.join(bld.CSRC, "nrldpc_mix_tx_enc.hip")).read()


def test_refusals_come_before_any_device_call(pkg):
    C = pkg._capi
    lib = pkg.load()
    fn = getattr(lib, NAME)
    assert fn(None, P, P, None) == C.ERR_ARG and b"null mix plan" in lib.nrldpc_last_error()
    assert fn(None, None, None, None) == C.ERR_ARG
    with pytest.raises(pkg.NRLDPCError):
        pkg.MixTxPlan(M.mix(pkg), list(M.N_TB)[:3])  # (a plan that cannot be made is refused as before)


def test_the_empty_plan_needs_no_device_and_does_nothing(pkg):
    ps = M.mix(pkg)
    for plan in (pkg.MixTxPlan([], []), pkg.MixTxPlan(ps, [0] * 9)):
        for d in (None, 0x1000):
            plan.encode_all(d, d)
        plan.close()
        with pytest.raises(pkg.NRLDPCError, match="null mix plan"):
            plan.encode_all(0x1000, 0x1000)  # a closed plan is a null plan
    DC = importlib.import_module("ldpc-3gpp-matlab_amd.device_chain")
    chain = DC.MixedEncodeChain(ps, [0] * 9, one_launch_encode=True)
    assert chain.one_launch_encode and chain.codecs == [None] * 9 and chain.plan.totals()["cw"] == 0
    chain.close()


def test_too_large_for_one_launch_is_refused_at_create(pkg):
    """2^31 - 1 transport blocks of a one-wave size would be 2^29 encode workgroups, but the count itself is refused first, with the
    text of the other prefix tables; nrldpc_mix_tx_layout and nrldpc_mix_tx_create still agree."""
    C = pkg._capi
    lib = pkg.load()
    ps = M.mix(pkg)[:2]
    ts = (C.TbParams * 2)()
    for i, p in enumerate(ps):
        ctypes.memmove(ctypes.byref(ts[i]), ctypes.byref(C.tb_params(p)), ctypes.sizeof(C.TbParams))
    cnt = (ctypes.c_int32 * 2)(2 ** 31 - 1, 1)
    a_off = (ctypes.c_int64 * 3)()
    h = ctypes.c_void_p()
    assert lib.nrldpc_mix_tx_layout(2, ts, cnt, a_off) == C.ERR_UNSUPPORTED and b"too large for one launch" in lib.nrldpc_last_error()
    assert lib.nrldpc_mix_tx_create(2, ts, cnt, 0, ctypes.byref(h)) == C.ERR_UNSUPPORTED and h.value is None


# ---- census: what P_enc reaches -------------------------------------------------------------------------------------------------------
def test_census_p_enc_reaches_every_class_of_the_encoder_body(pkg):
    want = T.enc_universe()
    assert len(want) == 48
    ps, n_tb = E.p_enc(pkg)
    sizes = [(p.BG, p.Z_c) for p in ps]
    assert len(ps) == 15 and sorted(sizes) == sorted((bg, Z) for bg in T.ENC_SIZES for Z in T.ENC_SIZES[bg])
    assert all(p.C == 1 for p in ps) and n_tb == [max(T.enc_batches(p.BG, p.Z_c)) for p in ps]
    # every one-wave configuration ends in a ragged workgroup; the two bodies alternate in configuration order
    nwc = [T.enc_nwc(bg, Z) for bg, Z in sizes]
    assert all(k % T.ENC_WAVES for k, w in zip(n_tb, nwc) if w == 1)
    four = [i for i, w in enumerate(nwc) if w == 4]
    assert len(four) == 3 and all(0 < i < len(ps) - 1 and nwc[i - 1] == 1 and nwc[i + 1] == 1 for i in four)
    # segment offsets are multiples of 16: the classes are those of tx_cases.enc_reached()
    off = pkg.mix_layout(ps, n_tb)
    assert all(o.c_hat % 16 == 0 and o.cw % 16 == 0 for o in off)
    seen = E.plan_census(pkg, ps, n_tb)
    missing = sorted(want - set(seen), key=repr)
    assert not missing, "P_enc at the seven base-offset pairs leaves unreached: %r" % missing
    assert set(seen) == set(T.enc_reached())
    # an aligned base alone reaches little, and every base-offset pair of the list is kept for a class of its own or for the odd phases
    assert len(set(E.plan_census(pkg, ps, n_tb, offsets=((0, 0),)))) < len(want)
    # ... and a size dropped from the list shows: without the three sizes tx_cases keeps for their size alone the plan still reaches
    # everything, and then every remaining size is the only one that reaches some class
    core = {b: tuple(z for z in T.ENC_SIZES[b] if z not in T.ENC_SIZES_FOR_SIZE[b]) for b in T.ENC_SIZES}
    qs, cnt = E.p_enc(pkg, core)
    assert len(qs) == 12 and not want - set(E.plan_census(pkg, qs, cnt))
    for bg in core:
        for Z in core[bg]:
            fewer = {b: tuple(z for z in core[b] if (b, z) != (bg, Z)) for b in core}
            qs, cnt = E.p_enc(pkg, fewer)
            assert want - set(E.plan_census(pkg, qs, cnt)), (bg, Z)


# ---- the host walk under sanitizers -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/mix_host/mix_tx_enc_check.cpp built once with the sanitizers (their runtimes linked statically: the program needs nothing
    preloaded)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path_factory.mktemp("mix_host") / "mix_tx_enc_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mix_host", "mix_tx_enc_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", ["P9", "P_enc", "zero-first-and-last"])
def test_records_mapping_and_lds_walked_on_the_cpu_under_sanitizers(pkg, checker, tmp_path, name):
    """tests/mix_host/mix_tx_enc_check.cpp (its own main, -fsanitize=address,undefined) over P9 and P_enc at the seven base-offset
    pairs: every codeword served exactly once, reads inside the code block, every output byte written by one thread and no gap byte
    touched, every slot's LDS region inside the launch's size, table offsets inside the table bytes."""
    if name == "P9":
        ps, n_tb = M.mix(pkg), list(M.N_TB)
    elif name == "P_enc":
        ps, n_tb = E.p_enc(pkg)
    else:
        ps, n_tb = M.mix(pkg)[:4], [0, 2, 1, 0]
    src = tmp_path / "mix_tx_enc.txt"
    src.write_text(E.walk_input(pkg, ps, n_tb))
    out = subprocess.run([checker, str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and "mix_tx_enc_check ok" in out.stdout, out.stdout + out.stderr
    if name == "P_enc":  # the largest case of the LDS arithmetic: four one-wave codewords of BG2 Z = 384
        assert "LDS 21056" in out.stdout and "15 tables" in out.stdout, out.stdout
    if name == "P9":  # two configurations share (BG, Z): one table for both
        distinct = len({(p.BG, p.Z_c) for p, k in zip(ps, n_tb) if k})
        assert "%d tables" % distinct in out.stdout and distinct < sum(1 for k in n_tb if k), out.stdout

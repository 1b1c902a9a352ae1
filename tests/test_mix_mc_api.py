"""Mixed transport-block batches, the Monte-Carlo loop's own two stages (nrldpc_mix_tx_payload_dev, nrldpc_mix_tx_outcome_dev) and the
mixed sweep, without a device: the functions are declared, exported and bound; the new unit and the shared headers are built and stay
out of the decoder kernels' identity; the single payload kernel and the mixed one share one copy of the hash and the chunk rule; the
draw record is 16 bytes; every refusal comes back before any HIP call (this file runs where there is no GPU); the empty plan needs no
device; the payload mapping, the chunk stores and the outcome rule (csrc/nrldpc_mix_mc.h, csrc/nrldpc_payload_bits.h) are walked on
the CPU by a stand-alone program built with the address and undefined-behaviour sanitizers, against harness.payload_bits_np; and
plot_SNR_vs_A(mixed=True) writes what mixed=False writes, with a deterministic hook in place of the simulation."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mix_mc_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc")
P = ctypes.c_void_p(0x1000)  # a non-null address nothing may dereference: every call below is refused, or has nothing to do
NULL = None
NAMES = ("nrldpc_mix_tx_payload_dev", "nrldpc_mix_tx_outcome_dev")


def test_symbols_are_declared_exported_and_bound(pkg):
    C = pkg._capi
    lib = pkg.load()
    hdr = open(os.path.join(ROOT, "include", "nrldpc.h")).read()
    for name in NAMES:
        assert name in C.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, hdr), name
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [4, 10]
    assert "#define NRLDPC_ABI_VERSION 6" in hdr and lib.nrldpc_abi_version() == C.ABI_VERSION == 6  # added without a revision bump
    assert "} nrldpc_mix_draw;" in hdr and "sizeof == 16" in hdr[hdr.index("typedef struct nrldpc_mix_draw"):hdr.index("} nrldpc_mix_draw;") + 80]
    assert ctypes.sizeof(C.MixDraw) == 16 and [(f, getattr(C.MixDraw, f).offset) for f, _ in C.MixDraw._fields_] == [("seed", 0), ("first_block", 8)]
    assert pkg.MixDraw is C.MixDraw
    for method in ("draws", "payload", "outcome"):
        assert callable(getattr(C.MixTxPlan, method))
    H = importlib.import_module("ldpc-3gpp-matlab_amd.harness")
    assert callable(H.simulate_point_mixed)
    # the note that listed the mixed payload draw as missing now says where it is
    block = hdr[hdr.index("mixed transport-block batches, the channel leg"):hdr.index("typedef struct nrldpc_mix_chan*")]
    assert "nrldpc_mix_tx_payload_dev" in block


def test_new_unit_is_built_and_is_not_part_of_the_decoder_kernels_identity(pkg):
    bld = pkg._capi._build
    units, headers = {"nrldpc_mix_mc.hip"}, {"nrldpc_mix_mc.h", "nrldpc_payload_bits.h"}
    assert units <= set(bld.SOURCES) and headers <= set(bld.HEADERS)
    assert not (units | headers) & set(bld.KERNEL_SOURCES)
    for f in units | headers:
        assert os.path.exists(os.path.join(CSRC, f)), f
    assert "Mix" not in open(os.path.join(CSRC, "nrldpc_kernels.h")).read()
    assert bld.kernel_id() == pkg.load().nrldpc_kernel_id().decode() == "a54d4abae9865fdf"  # the parent commit's value
    # one copy of the hash and of the chunk rule: the single kernel's unit includes the header and no longer defines them
    shared = open(os.path.join(CSRC, "nrldpc_payload_bits.h")).read()
    for unit in ("nrldpc_channel.hip", "nrldpc_mix_mc.hip", "nrldpc_mix_mc.h"):
        text = open(os.path.join(CSRC, unit)).read()
        for fn in ("uint64_t splitmix64", "0xBF58476D1CE4E5B9", "0x00204081u"):
            assert fn in shared and fn not in text, (unit, fn)
    assert '#include "nrldpc_payload_bits.h"' in open(os.path.join(CSRC, "nrldpc_channel.hip")).read()
    assert '#include "nrldpc_payload_bits.h"' in open(os.path.join(CSRC, "nrldpc_mix_mc.h")).read()


def test_draw_records_broadcast_and_refuse(pkg):
    ps, n_tb, seeds, first = MC.plan(pkg, "P_small")
    plan = pkg.MixTxPlan(ps, [0] * 7)  # an empty plan: no device
    d = plan.draws(seeds, first)
    assert len(d) == 7 and [(x.seed, x.first_block) for x in d] == list(zip(seeds, first))
    assert np.frombuffer(d, np.uint8).size == 7 * 16
    one = plan.draws(-1, 3)  # a seed is taken modulo 2^64, as payload_bits_dev takes it
    assert {(x.seed, x.first_block) for x in one} == {((1 << 64) - 1, 3)}
    assert [x.first_block for x in plan.draws(5)] == [0] * 7
    for bad in (dict(seed=[1, 2]), dict(seed=0, first_block=[0] * 8), dict(seed=0, first_block=-1), dict(seed=0, first_block=1 << 64)):
        with pytest.raises(pkg.NRLDPCError):
            plan.draws(**bad)
    plan.close()


def test_null_plan_is_refused_and_the_empty_plan_does_nothing(pkg):
    C = pkg._capi
    lib = pkg.load()
    assert lib.nrldpc_mix_tx_payload_dev(None, P, P, NULL) == C.ERR_ARG and lib.nrldpc_last_error() == b"null mix plan"
    assert lib.nrldpc_mix_tx_outcome_dev(None, P, P, P, 1, P, P, P, P, NULL) == C.ERR_ARG and lib.nrldpc_last_error() == b"null mix plan"
    ps, _ = MC.small(pkg)
    left = np.full(7, -7, np.int32)
    for plan in (pkg.MixTxPlan([], []), pkg.MixTxPlan(ps, [0] * 7)):
        assert plan.totals()["a"] == 0
        for d in (None, 0x1000):  # OK without a launch, null pointers included; nothing is dereferenced or written
            plan.payload(d, d)
            for first in (0, 1):
                plan.outcome(d, d, d, first, d, d, d, d_left=d)
                plan.outcome(d, d, d, first, d, d, d, d_left=left.ctypes.data)
        assert (left == -7).all()  # d_left included
        plan.close()
        plan.close()


def test_null_pointers_of_a_non_empty_plan_are_refused_before_any_device_call(pkg):
    """The pointer checks need a plan with transport blocks, and such a plan needs a device; where there is none the creation is refused
    with the library's no-device text and the checks are those of tests/test_mix_mc_gpu.py."""
    C = pkg._capi
    lib = pkg.load()
    ps, n_tb = MC.small(pkg)
    try:
        plan = pkg.MixTxPlan(ps, n_tb)
    except pkg.NRLDPCError as e:
        assert "no HIP device available" in str(e)
        return
    h = plan._h
    null = (C.ERR_ARG, b"null pointer")
    calls = [(lambda: lib.nrldpc_mix_tx_payload_dev(h, P, None, NULL), null),
             (lambda: lib.nrldpc_mix_tx_payload_dev(h, None, P, NULL), (C.ERR_ARG, b"null draw records"))]
    for k in range(6):  # each of the six arrays in turn; d_left alone may be null
        args = [P, P, P, P, P, P]
        args[k] = None
        calls.append((lambda a=args: lib.nrldpc_mix_tx_outcome_dev(h, a[0], a[1], a[2], 0, a[3], a[4], a[5], None, NULL), null))
    for k, (call, want) in enumerate(calls):
        assert (call(), lib.nrldpc_last_error()) == want, k
    plan.close()


# ---- the host walk under sanitizers -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/mix_host/mix_mc_check.cpp built once with the sanitizers (their runtimes linked statically: the program needs nothing
    preloaded)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path_factory.mktemp("mix_host") / "mix_mc_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "mix_host", "mix_mc_check.cpp"), "-o", exe])
    return exe


def _case_file(pkg, tmp_path, name, move=None, flip=None):
    H = importlib.import_module("ldpc-3gpp-matlab_amd.harness")
    ps, n_tb, seeds, first = MC.plan(pkg, name)
    off, a_off = pkg.mix_layout(ps, n_tb), pkg.mix_tx_layout(ps, n_tb)
    n = len(ps)
    lines = [str(n)]
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        lines.append(" ".join(str(int(x)) for x in [k, p.A, p.B, seeds[i], first[i], a_off[i] + (16 if move == i else 0), off[i].b_hat, off[i].tb]))
    lines.append("%d %d %d" % (a_off[n], off[n].b_hat, off[n].tb))
    for i, (p, k) in enumerate(zip(ps, n_tb)):
        bits = H.payload_bits_np(seeds[i], first[i], k, p.A).reshape(-1)
        if flip == i:
            bits[-1] ^= 1
        lines.append("".join("01"[b] for b in bits) if k else "-")
    src = tmp_path / ("%s.txt" % name)
    src.write_text("\n".join(lines) + "\n")
    return str(src)


@pytest.mark.parametrize("name", ["P_small", "P_two"])
def test_mapping_stores_and_outcome_rule_walked_on_the_cpu_under_sanitizers(pkg, checker, tmp_path, name):
    """csrc/nrldpc_mix_mc.h and csrc/nrldpc_payload_bits.h exercised by tests/mix_host/mix_mc_check.cpp (its own main,
    -fsanitize=address,undefined) over both test plans, thread by thread, at base addresses +0 ... +3: every byte of every segment is
    written exactly once with the bit harness.payload_bits_np defines -- first_block = 2^32 + 5 and a block range across 2^32
    included -- whichever store form the address picks; no gap or guard byte is touched; the outcome rule over three attempts equals a
    ten-line reference loop; and the offsets the library reports are the headers'."""
    assert (1 << 32) + 5 in MC.PLANS[name][2]
    out = subprocess.run([checker, _case_file(pkg, tmp_path, name)], capture_output=True, text=True)
    assert out.returncode == 0 and "mix_mc_check ok" in out.stdout, out.stdout + out.stderr


def test_the_walk_notices_a_wrong_offset_and_a_wrong_bit(pkg, checker, tmp_path):
    """The checker is not vacuous: with one library offset moved by a segment's alignment, or one expected bit flipped, it fails."""
    out = subprocess.run([checker, _case_file(pkg, tmp_path, "P_small", move=4)], capture_output=True, text=True)
    assert out.returncode == 1 and "library offset differs" in out.stderr
    out = subprocess.run([checker, _case_file(pkg, tmp_path, "P_small", flip=6)], capture_output=True, text=True)
    assert out.returncode == 1 and "wrong bit" in out.stderr


# ---- the mixed sweep against the sequential one, with a hook in place of the simulation ----------------------------------------------------
def _hook(pkg, calls):
    """Deterministic outcomes from (A, EsN0, global block index): a block fails when a hash of the three falls below a rate that drops
    with Es/N0, faster for A = 200 (its ladder is rounds shorter); A = 300 is refused."""
    def simulate(A, EsN0, n, first_block):
        calls.setdefault(A, []).append((A, EsN0, n, first_block))
        if A == 300:
            raise pkg.UnsupportedParameters("refused by the hook")
        rate = min(1.0, 10.0 ** (-(EsN0 + 1.0) * (3.0 if A == 200 else 1.0)))
        idx = np.arange(first_block, first_block + n, dtype=np.uint64)
        with np.errstate(over="ignore"):
            h = (idx + np.uint64(A)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(round(EsN0 * 10)) % 1000) * np.uint64(0xBF58476D1CE4E5B9)
            h ^= h >> np.uint64(29)
            h *= np.uint64(0x94D049BB133111EB)
            h ^= h >> np.uint64(32)
        return (h >> np.uint64(40)).astype(np.float64) / float(1 << 24) >= rate
    return simulate


def test_mixed_sweep_equals_the_sequential_one_with_a_hook(pkg, tmp_path):
    """plot_SNR_vs_A(mixed=True, simulate=hook) against mixed=False with the same hook: three lengths that finish rounds apart and one
    the hook refuses; the files are byte-identical, the returns equal, and each length's list of hook calls is the sequential one.
    (Fails on the parent commit: no such keyword.)"""
    H = importlib.import_module("ldpc-3gpp-matlab_amd.harness")
    kw = dict(A=(100, 200, 300, 400), R=(1 / 3, 1 / 2), BG=2, iterations=8, target_block_errors=6, target_BLER=1e-2, EsN0_start=-2.0,
              EsN0_delta=0.25, seed=3, batch=32, max_points=60)
    got = {}
    for mixed in (False, True):
        calls = {}
        d = tmp_path / ("mixed" if mixed else "sequential")
        ret = H.plot_SNR_vs_A(results_dir=str(d), simulate=_hook(pkg, calls), mixed=mixed, **kw)
        files = {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}
        got[mixed] = (ret, files, calls)
    (ret0, files0, calls0), (ret1, files1, calls1) = got[False], got[True]
    assert len(files0) == 2 and files0 == files1
    assert ret0.keys() == ret1.keys()
    for r in ret0:
        assert [a for a, _ in ret0[r]] == [100, 200, 400]  # the refused length has no row
        assert all(x == y or (x[1] != x[1] and y[1] != y[1] and x[0] == y[0]) for x, y in zip(ret0[r], ret1[r])) and len(ret0[r]) == len(ret1[r])
        assert any(es == es for _, es in ret0[r])  # a crossing was found: the ladders did run
    assert calls0 == calls1 and sorted(calls0) == [100, 200, 300, 400]
    assert len(calls0[300]) == 2 and len(calls0[200]) < len(calls0[100])  # refused once per rate; one ladder is rounds shorter
    # mixed=True without a way to simulate on one device is refused
    for bad in (dict(), dict(device=True, devices=[0, 0])):
        with pytest.raises(pkg.UnsupportedParameters):
            H.plot_SNR_vs_A(results_dir=str(tmp_path / "bad"), mixed=True, **bad)

"""The host half of the host-pointer decode path -- csrc/nrldpc_host_quant.cpp and the piece walk of HostPool::quantise_rows_start --
under AddressSanitizer and UBSan, without a GPU: tests/host_quant/host_quant_check.cpp (its own main, the unit compiled into it,
-fsanitize=address,undefined with the runtimes linked statically: nothing is loaded into Python, nothing is preloaded) compares every
quantiser path the CPU offers with the plain one at every length 0..200 and element offset 0..3 on exact-size heap blocks, walks the
compact ranges of the planned chunks of tests/host_cases.py for every worker count 1..16, and holds nrldpc_top_block against a
plain scan."""
import os
import shutil
import subprocess

import pytest

import host_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {"f32": 0, "f16": 1, "f64": 2}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the sanitizer run"
    exe = str(tmp_path_factory.mktemp("host_quant") / "host_quant_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "ldpc-3gpp-matlab_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_quant", "host_quant_check.cpp"), "-o", exe])
    return exe


def planned_ranges():
    """(act, pitch, rows, lo, hi, kind) of the first and the last int8 chunk of every pipelined planned call, each piece and the whole"""
    out = []
    for c in H.HOST_PLAN:
        p = H.plan(c)
        if p["route"] != "pipeline" or not p["i8"]:
            continue
        for ch in (p["chunks"][0], p["chunks"][-1]):
            for lo, hi in sorted(set(ch["pieces"]) | {(0, ch["n"] * p["act"])}):
                out.append((p["act"], p["ncw"], ch["n"], lo, hi, KIND[c.dtype]))
    return sorted(set(out))


def test_quantiser_paths_piece_walk_and_layer_scan(checker, tmp_path):
    ranges = planned_ranges()
    assert {(a, pch) for a, pch, *_ in ranges} >= {(440, 1040), (600, 1040), (112, 416), (128, 416), (4136, 5984), (364, 364), (26112, 26112)}
    assert any(r[2] == 1 for r in ranges) and any(r[3] > 0 for r in ranges)  # a chunk of one codeword; pieces that start past 0
    src = tmp_path / "ranges.txt"
    src.write_text("%d\n" % len(ranges) + "".join(" ".join(map(str, r)) + "\n" for r in ranges))
    out = subprocess.run([checker, str(src)], capture_output=True, text=True)
    assert out.returncode == 0 and "host_quant_check ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[0].startswith("paths ok: %d comparisons" % (3 * 201 * 4 * 8 * 2))
    assert lines[1].startswith("walk ok: %d ranges" % len(ranges)) and int(lines[1].split()[-7]) > 0
    assert lines[2].startswith("top_block ok: %d calls" % (3 * 5 * 12 * 136))

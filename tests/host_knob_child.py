"""One process under one value of a host-path knob the library reads once per process (NRLDPC_HOST_CHUNK_MB=1, NRLDPC_HOST_THREADS=1 or
=3, NRLDPC_HOST_PIPELINE=0, NRLDPC_HOST_ZEROCOPY_KB=0): the calls tests/host_cases.py assigns to that value, each through
host_cases.run_call (poisoned staging, guard rows, the oracle and one device launch, the library's own report of the pipeline).
tests/test_host_paths_gpu.py starts this script.  A plain script, not a test module: `python tests/host_knob_child.py MODE` with the
environment already set; prints one line of JSON and exits 0 (all equal) or 1."""
import importlib
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for path in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if path not in sys.path:
        sys.path.insert(0, path)
import oracle as orc  # noqa: E402
import host_cases as H  # noqa: E402


def main(argv):
    mode = argv[1]
    rec = dict(mode=mode, ok=False, calls=[])
    try:
        for name in H.KNOBS:
            assert os.environ.get(name) == H.MODE_ENV[mode].get(name), "%s is not what mode %s needs" % (name, mode)
        calls = [c for c in H.HOST_PLAN if c.mode == mode]
        # what this process is there to reach, from the census: the classes its knob forces
        forced = set()
        for c in calls:
            forced |= H.census(c)
            assert H.FORCED[mode] <= H.executed(c), (c.name, H.FORCED[mode])
        assert forced == H.FORCED[mode], forced
        if mode == "chunk1":
            p = H.plan(calls[0])
            assert p["chunk"] == (H.MiB // 2) // p["ncw"] == 87 and len(p["chunks"]) == 24  # 512 KiB of int8 at 5984 LLRs a codeword
        if mode in ("pipe0", "zc0"):
            assert all(H.plan(c)["route"] == "one-copy" for c in calls)
            assert all(H.plan(c._replace(mode="default"))["route"] == ("pipeline" if mode == "pipe0" else "zero-copy") for c in calls)
        pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
        orc.lib().orc_set_threads(min(16, os.cpu_count() or 1))
        for c in calls:
            r = H.run_call(pkg, orc, c)
            assert r["route"] == H.plan(c)["route"]
            rec["calls"].append(c.name)
            rec[c.name] = r
        rec["ok"] = True
    except Exception:
        rec["error"] = traceback.format_exc()[-3000:]
    print(json.dumps(rec))
    return 0 if rec["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))

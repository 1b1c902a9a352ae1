#!/usr/bin/env python
"""Record which kernel every planned call of tests/decode_cases.py runs: profiles/decode_routes.json.

The library has no report of the decoder kernel it launched; the profiler sees kernel names, which carry the template arguments.
This tool starts itself as a child under `rocprofv3 --kernel-trace` (no counters, no other tracing, the program after `--`), in
which every planned call is launched once through nrldpc_decode_dev in plan order, reads the trace, and writes per planned call the
kernel name, the grid (in workgroups) and the workgroup size, stamped with nrldpc_kernel_id, pair_search_id and nrldpc_build_id.
tests/test_decode_cases.py holds the record against the model.

    python tools/trace_decode_routes.py [--out profiles/decode_routes.json] [--timeout 900]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import signal
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child():
    """every planned call once, in plan order: the routing does not read the data, so the LLRs are noise"""
    import numpy as np
    import torch
    import decode_cases as D
    pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
    rng = np.random.default_rng(1)
    for c in D.plan():
        rows, cols, kb = D.BG_DIMS[c.bg]
        tdt = torch.float16 if c.dtype == "f16" else torch.float32
        llr = torch.from_numpy(rng.standard_normal((c.batch, cols * c.Z)).astype(np.float32)).to(tdt).cuda()
        hard = torch.empty(c.batch * kb * c.Z, dtype=torch.uint8, device="cuda")
        it = torch.empty(c.batch, dtype=torch.int32, device="cuda")
        app = torch.empty(c.batch * cols * c.Z, dtype=torch.float32, device="cuda") if c.soft else None
        codec = pkg.Codec(c.bg, c.Z, max_iter=c.iters, n_layers=c.nl, early_term=bool(c.et), llr_dtype=np.float16 if c.dtype == "f16" else np.float32,
                          crc=D.crc_of(c))
        if c.refill_grid:
            os.environ["NRLDPC_REFILL_GRID"] = str(c.refill_grid)
        try:
            codec.decode_dev(llr.data_ptr(), c.batch, hard.data_ptr(), it.data_ptr(), app.data_ptr() if c.soft else None,
                             torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            if c.refill_grid:
                del os.environ["NRLDPC_REFILL_GRID"]
            codec.close()
    print("launched %d planned calls" % len(D.plan()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_routes.json"))
    ap.add_argument("--timeout", type=int, default=900)
    a = ap.parse_args()
    if a.child:
        return child()
    import decode_cases as D
    bld = importlib.import_module("ldpc-3gpp-matlab_amd.build")
    pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
    L = pkg.load()
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, NRLDPC_TEST_HOOKS="1")
        env.pop("NRLDPC_REFILL_GRID", None)
        # a process group of its own: on the time limit the profiler AND the child it started are killed, not the profiler alone
        proc = subprocess.Popen(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "routes", "--",
                                 sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=tmp, start_new_session=True)
        try:
            rc = proc.wait(timeout=a.timeout)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.wait()
            raise SystemExit("the traced child did not finish within %d s: killed with its process group" % a.timeout)
        if rc:
            raise SystemExit("rocprofv3 exit %d" % rc)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        assert len(files) == 1, files
        rows = [r for r in csv.DictReader(open(files[0])) if "nrldpc::" in r["Kernel_Name"] and "nrldpc_decode" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    plan = D.plan()
    assert len(rows) == len(plan), "%d decoder launches in the trace, %d planned calls" % (len(rows), len(plan))
    kernels, calls = [], {}
    for c, r in zip(plan, rows):
        name = r["Kernel_Name"]
        if name not in kernels:
            kernels.append(name)
        wg = int(r["Workgroup_Size_X"])
        gx = int(r["Grid_Size_X"])
        assert gx % wg == 0
        calls[c.name] = [kernels.index(name), gx // wg, wg]  # the dispatch packet's grid is in work-items
    rec = {"nrldpc_kernel_id": L.nrldpc_kernel_id().decode(), "pair_search_id": bld.pair_search_id(),
           "nrldpc_build_id": L.nrldpc_build_id().decode(), "source": "rocprofv3 --kernel-trace of tools/trace_decode_routes.py --child",
           "columns": ["kernel (index into kernels)", "grid in workgroups", "workgroup size"], "kernels": kernels, "calls": calls}
    with open(a.out, "w") as f:  # one kernel and one call per line
        f.write("{\n")
        for k in ("nrldpc_kernel_id", "pair_search_id", "nrldpc_build_id", "source", "columns"):
            f.write("%s: %s,\n" % (json.dumps(k), json.dumps(rec[k])))
        f.write('"kernels": [\n' + ",\n".join(json.dumps(k) for k in kernels) + '\n],\n"calls": {\n')
        f.write(",\n".join("%s: %s" % (json.dumps(n), json.dumps(calls[n])) for n in sorted(calls)) + "\n}\n}\n")
    print("wrote %s: %d calls, %d kernels" % (a.out, len(calls), len(kernels)))


if __name__ == "__main__":
    main()

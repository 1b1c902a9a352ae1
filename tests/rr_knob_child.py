"""One process under one value of the rate-recovery switches (NRLDPC_RR_GENERAL=1, NRLDPC_RR_SCATTER=1 or NRLDPC_RR_SCATTER=0, which
the library reads once per process): every set of tests/rr_cases.py through nrldpc_rate_recover_dev (f32) and through
nrldpc_rate_recover_ex_dev with f16 input, buffer and output, against the model of tests/test_rate_recover_paths_gpu.py, which
starts this script.  A plain script, not a test module: `python tests/rr_knob_child.py general|scatter1|scatter0` with the
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
import rr_cases as R  # noqa: E402


def main(argv):
    mode = argv[1]
    rec = dict(mode=mode, ok=False, sets=0, elements=0)
    try:
        for name in ("NRLDPC_RR_GENERAL", "NRLDPC_RR_SCATTER"):
            assert os.environ.get(name) == R.MODE_ENV[mode].get(name), "%s is not what mode %s needs" % (name, mode)
        # what this process is there to reach, from the census: the forms the switch forces
        refs = [R.derive(kw) for kw in R.RR_SETS]
        forms = {(ref["Q_m"], R.launch_form(ref, buf, mode)) for ref in refs for buf in (False, True)}
        if mode == "general":
            assert forms == {(q, "general") for q in R.QMS}, forms
        if mode == "scatter0":
            assert not any(f == "scatter" for _, f in forms), forms
        if mode == "scatter1":
            calls = [c for c in R.plan_single()[0] if c[4] == mode]
            reached = set()
            for ref in refs:
                reached |= R.census(ref, calls, R.N_TB)
            want = {c for c in R.universe() if c[1] == "scatter" and c[2] in (4, 6, 8)}
            assert want and want <= reached, sorted(want - reached)
        pkg = importlib.import_module("ldpc-3gpp-matlab_amd")
        orc.lib()
        for k in range(len(R.RR_SETS)):
            rec["elements"] += R.run_single(pkg, orc, k, "f32", (R.F32, R.F32, R.F32), R.OFFSETS[0])
            rec["elements"] += R.run_single(pkg, orc, k, "ex", (R.F16, R.F16, R.F16), R.OFFSETS[0])
            rec["sets"] += 1
        rec["ok"] = True
    except Exception:
        rec["error"] = traceback.format_exc()[-3000:]
    print(json.dumps(rec))
    return 0 if rec["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))

"""Every call of tests/host_cases.py::HOST_PLAN through nrldpc_decode / nrldpc_decode_packed: the handle's staging buffers and pinned
slots are poisoned first (the same shape with every finite LLR negated and every infinity 0), the caller's arrays are prefilled and
carry guard rows, and the result is compared bit for bit -- hard decisions and iteration counts -- with the CPU oracle on every
codeword and with one nrldpc_decode_dev launch on the same LLRs.  After each pipelined call nrldpc_last_host_phases must report the
chunk count, the codewords per chunk and the layer count the census predicted, so that the claim about which path ran rests on the
library's own report.  Knobs the library reads once per process run in fresh children (tests/host_knob_child.py)."""
import json
import os
import subprocess
import sys

import pytest

import host_cases as H

pytestmark = pytest.mark.gpu

DEFAULT = [c.name for c in H.HOST_PLAN if c.mode == "default"]


@pytest.fixture(scope="module", autouse=True)
def oracle_threads(orc):
    orc.lib().orc_set_threads(min(16, os.cpu_count() or 1))


@pytest.mark.parametrize("name", DEFAULT)
def test_planned_call(pkg, orc, name):
    assert not any(k in os.environ for k in H.KNOBS), "a host-path knob is set in the test process"
    c = H.BY_NAME[name]
    rec = H.run_call(pkg, orc, c)
    print(rec)
    p = H.plan(c)
    assert rec["route"] == p["route"] and rec["compared"] == c.batch
    if p["route"] == "pipeline":
        assert (rec["chunks"], rec["codewords_per_chunk"]) == (len(p["chunks"]), p["chunk"])


def test_auto_equals_the_explicit_count(pkg, orc):
    """AUTO at Z = 20: settled by the first chunk (12 rows), and lifted by the last codeword (20 rows, the call starts again with a
    full scan): both equal what the explicit count returns on the same handle and what count_layers reads off the array."""
    for name in ("z20_auto_first", "z20_auto_restart"):
        c = H.BY_NAME[name]
        llr, info, _ = H.build_input(orc, c)
        want = H.plan(c)["nl"]
        assert pkg._capi.count_layers(c.bg, c.Z, llr) == want
        codec = pkg.Codec(c.bg, c.Z, max_iter=H.MAX_ITER, n_layers=H.AUTO, early_term=True, alpha=H.ALPHA, llr_dtype=H.NP_DT[c.dtype])
        h_auto, it_auto, _ = H.raw_decode(pkg, codec, c, llr)
        assert codec.last_layers() == want and codec.last_host_phases()["layers"] == want
        codec.set_layers(want)
        h_exp, it_exp, _ = H.raw_decode(pkg, codec, c, llr)
        codec.close()
        assert (h_auto == h_exp).all() and (it_auto == it_exp).all(), name


# Each child: import torch, load the library, one planned call with its oracle comparison -- about two seconds; the limit is that
# with a wide margin for a cold machine.
CHILD_TIMEOUT = 120
STOPPED = []  # the mode whose child timed out or ended on a signal: no further child is started


@pytest.mark.parametrize("mode", H.MODES[1:])
def test_knob_in_a_fresh_child(pkg, mode):
    """NRLDPC_HOST_CHUNK_MB=1, NRLDPC_HOST_THREADS=1 and =3, NRLDPC_HOST_PIPELINE=0, NRLDPC_HOST_ZEROCOPY_KB=0: the calls the census
    assigns to each value, in a child of its own per value, one at a time; after a child that ended on a signal or its time limit
    no further child is started."""
    assert not STOPPED, "the %s child ended on a signal or its time limit: no further child is started" % STOPPED[0]
    pkg.load()
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_knob_child.py")
    env = {k: v for k, v in os.environ.items() if k not in H.KNOBS}
    env.update(H.MODE_ENV[mode])
    try:
        p = subprocess.run([sys.executable, child, mode], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        STOPPED.append(mode)
        pytest.fail("the %s child did not end within %d s (%s)" % (mode, CHILD_TIMEOUT, e))
    if p.returncode < 0 or p.returncode > 1:
        STOPPED.append(mode)
        pytest.fail("the %s child ended with status %d\n%s" % (mode, p.returncode, p.stdout[-2000:] + p.stderr[-2000:]))
    assert p.returncode == 0, (mode, p.stdout[-3000:], p.stderr[-3000:])
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(rec)
    want = [c.name for c in H.HOST_PLAN if c.mode == mode]
    assert rec["mode"] == mode and rec["ok"] and rec["calls"] == want and want

"""The device-pointer decode entries on buffers laid out by the test: every planned call of tests/decode_cases.py (each kernel
instantiation nrldpc_decode_dev can launch in the default process, and the cross of every route kind's data-path classes) runs with
its LLRs inside a larger allocation at the planned byte offset, with hard decisions, iteration counts and soft output between guards
at least one workgroup's rows long, everything prefilled with patterns no correct output contains (0xA5 bytes, 0x5A5A5A5A ints, a NaN
payload).  After the call the guards and the whole LLR allocation are bit for bit what they were, every hard byte is 0 or 1, every
count is in 1..max_iter, and all of it equals the oracle.  The host entry cannot see any of this: its staging buffers are aligned,
sized for max_batch and reused from call to call."""
import os

import numpy as np
import pytest

import decode_cases as D
from conftest import BG_DIMS, awgn_llr, rule_kw

pytestmark = pytest.mark.gpu

HARD_FILL, ITERS_FILL, APP_FILL = 0xA5, 0x5A5A5A5A, 0x7FC5A5A5
NP_DT = {"f16": np.float16, "f32": np.float32}


class Guarded:
    """`body` elements of dtype `dt` at byte offset `off` behind a front guard, a back guard of `back` elements behind them, all
    prefilled from `fill` (a scalar bit pattern, or an array for the whole allocation)"""

    def __init__(self, torch, dt, body, back, off, fill, front=64):
        dt = np.dtype(dt)
        assert off % dt.itemsize == 0 or dt.itemsize == 1
        self.front = (front + 255) // 256 * 256 + off          # bytes; the allocation itself is 256-byte aligned
        self.n = body * dt.itemsize
        total = self.front + self.n + back * dt.itemsize + 64
        if np.isscalar(fill):
            host = np.frombuffer(np.full((total + 3) // 4, fill, np.uint32).tobytes(), np.uint8)[:total].copy() if dt.itemsize != 1 \
                else np.full(total, fill, np.uint8)
            if dt.itemsize != 1 and off % 4:
                raise AssertionError("pattern words must stay aligned")
        else:
            host = fill(total, self.front)
        self.before = host
        self.dev = torch.from_numpy(host.copy()).cuda()
        assert self.dev.data_ptr() % 256 == 0
        self.ptr = self.dev.data_ptr() + self.front
        self.dt = dt

    def read(self):
        after = self.dev.cpu().numpy()
        lo, hi = self.front, self.front + self.n
        assert (after[:lo] == self.before[:lo]).all(), "front guard written"
        assert (after[hi:] == self.before[hi:]).all(), "back guard written"
        return after[lo:hi].view(self.dt)

    def unchanged(self):
        return (self.dev.cpu().numpy() == self.before).all()


def llr_alloc(torch, llr, ncw, off, seed):
    """the LLR array inside a larger allocation: pads of at least one full workgroup of codewords, strong finite values of random sign"""
    dt = llr.dtype
    pad = ncw * llr.shape[1]

    def fill(total, front):
        rng = np.random.default_rng(seed ^ 0x5EED)
        n = total // dt.itemsize + 1
        v = (np.where(rng.integers(0, 2, n) == 1, 24.0, -24.0)).astype(dt)
        host = np.frombuffer(v.tobytes(), np.uint8)[:total].copy()
        host[front: front + llr.size * dt.itemsize] = np.frombuffer(llr.tobytes(), np.uint8)
        return host
    return Guarded(torch, dt, llr.size, pad, off, fill, front=pad * dt.itemsize)


def outputs(torch, c, r):
    rows, cols, kb = BG_DIMS[c.bg]
    K, N = kb * c.Z, cols * c.Z
    hard = Guarded(torch, np.uint8, c.batch * K, max(64, r.ncw * K), c.hard_off, HARD_FILL)
    iters = Guarded(torch, np.int32, c.batch, max(16, r.ncw), 0, ITERS_FILL) if c.want_iters else None
    app = Guarded(torch, np.float32, c.batch * N, max(16, r.ncw * N), 0, APP_FILL) if c.soft else None
    return hard, iters, app


def check(c, ref, hard, iters, app, llr_buf):
    rows, cols, kb = BG_DIMS[c.bg]
    h = hard.read().reshape(c.batch, kb * c.Z)
    assert llr_buf.unchanged(), "the LLR allocation was written"
    assert (h <= 1).all(), "a hard byte is neither 0 nor 1 (%d of them keep the prefill)" % int((h == HARD_FILL).sum())
    assert (h == ref[0]).all(), "hard decisions differ"
    if iters is not None:
        it = iters.read()
        assert ((it >= 1) & (it <= c.iters)).all(), "an iteration count is outside 1..max_iter"
        assert (it == ref[1]).all(), "iteration counts differ"
    if app is not None:
        a = app.read().reshape(c.batch, cols * c.Z)
        assert not np.isnan(a).any(), "a soft output keeps the prefill"
        assert (a == ref[2]).all(), "soft outputs differ"


def run_planned(pkg, orc, c):
    import torch
    r = D.call_route(c)
    info, llr = D.inputs(c, orc, awgn_llr)
    codec = pkg.Codec(c.bg, c.Z, max_iter=c.iters, n_layers=c.nl, early_term=bool(c.et), llr_dtype=NP_DT[c.dtype], crc=D.crc_of(c))
    try:
        assert rule_kw(codec) == D.rule(c)
        ref = D.reference(c, orc, llr, rule_kw(codec))
        llr_buf = llr_alloc(torch, llr, r.ncw, c.llr_off, c.seed)
        hard, iters, app = outputs(torch, c, r)
        assert llr_buf.ptr % 16 == c.llr_off % 16 and hard.ptr % 4 == c.hard_off
        if c.refill_grid:
            os.environ["NRLDPC_REFILL_GRID"] = str(c.refill_grid)
        try:
            codec.decode_dev(llr_buf.ptr, c.batch, hard.ptr, iters.ptr if iters else None, app.ptr if app else None,
                             torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            if c.refill_grid:
                del os.environ["NRLDPC_REFILL_GRID"]
    finally:
        codec.close()
    check(c, ref, hard, iters, app, llr_buf)


def _chunks():
    """route kind x base graph x what the calls are there for, cut so that no id runs for more than a few seconds"""
    groups = {}
    for c in D.plan():
        groups.setdefault((c.why[0][:4], D.call_route(c).kind, c.bg), []).append(c)
    out = []
    for (why, kind, bg), calls in sorted(groups.items()):
        cost, cur, k = 0, [], 0
        for c in calls:
            w = c.batch * c.Z * c.iters + 20000
            if cur and cost + w > 1500000:
                out.append(("%s-%s-bg%d-%02d" % (why, kind, bg, k), cur))
                cost, cur, k = 0, [], k + 1
            cur.append(c)
            cost += w
        out.append(("%s-%s-bg%d-%02d" % (why, kind, bg, k), cur))
    return out


CHUNKS = _chunks()


@pytest.mark.parametrize("calls", [c for _, c in CHUNKS], ids=[n for n, _ in CHUNKS])
def test_planned_calls(pkg, orc, calls):
    failed = []
    for c in calls:
        try:
            run_planned(pkg, orc, c)
        except AssertionError as e:
            failed.append("%s [%s]: %s" % (c.name, D.call_route(c).kernel, str(e).split("\n")[0]))
    assert not failed, "\n".join(failed)


def test_every_planned_call_is_in_a_chunk():
    assert sorted(c.name for _, cs in CHUNKS for c in cs) == sorted(c.name for c in D.plan())


# bg, Z, early_term, dtype, batch, llr offset, hard offset: both base graphs and LLR types; workgroups of 128 ... 512 threads, which
# fall in the classes "up to 256" and "up to 512" (the third class, above 512, is empty in the default process: the run-time-Z
# schedule caps a workgroup at 512 threads -- test_multi_call_model_of_the_planned_configurations); BG1 Z = 144 (448 threads) runs
# inside the 512-thread workgroups of Z = 7 and BG2 Z = 88 (192) inside the 256-thread ones of Z = 36; an empty configuration; one
# handle listed twice; one CRC-stop handle, routed to a launch of its own
MULTI = [(1, 7, 1, "f16", 80, 0, 1), (1, 144, 1, "f16", 4, 2, 0), (2, 88, 1, "f32", 5, 4, 2), (2, 36, 1, "f32", 9, 0, 3),
         (1, 384, 1, "f32", 3, 8, 0), (2, 384, 0, "f16", 3, 0, 1), (2, 160, 1, "f16", 0, 0, 0), (1, 40, 0, "f32", 7, 0, 2),
         (2, 36, 2, "f16", 10, 2, 0)]
TWICE = 3  # this configuration's handle is listed a second time, with other data and buffers


def test_multi_call_model_of_the_planned_configurations():
    shared, own, bp = D.multi_groups([(bg, Z, et, dt, B, False) for bg, Z, et, dt, B, lo, ho in MULTI])
    assert own == [8] and not bp
    assert shared[(1, "f16", 512)][:2] == ([0, 1], 512) and D.rtz_schedule(1, 144)[1] == 448   # 448 inside 512
    assert shared[(2, "f32", 256)][:2] == ([2, 3], 256) and D.rtz_schedule(2, 88)[1] == 192    # 192 inside 256
    assert {k[2] for k in shared} == {256, 512}
    assert max(D.rtz_schedule(bg, Z)[1] for bg in (1, 2) for Z in D.ALL_Z) == 512              # the class above 512 is empty


def test_mixed_call_on_guarded_buffers(pkg, orc):
    """nrldpc_decode_multi_dev: nine configurations and a repeated handle in one call, every output guarded and prefilled, some
    pointers misaligned, once with d_iters and once without, the second call on another stream before the first is synchronised;
    everything against the oracle"""
    import torch
    work, codecs = [], []
    for i, (bg, Z, et, dt, B, lo, ho) in enumerate(MULTI + [MULTI[TWICE]]):
        c = D._call("multi-%d" % i, bg, Z, 0, et, False, dt, max(B, 1), 14 if et else 3, 0.2 if et else -2.5, bool(et), lo, ho, True, 0,
                    ("multi",))
        if i < len(MULTI):
            codecs.append(pkg.Codec(bg, Z, max_iter=c.iters, early_term=bool(et), llr_dtype=NP_DT[dt], crc=D.crc_of(c)))
        codec = codecs[i] if i < len(MULTI) else codecs[TWICE]
        info, llr = D.inputs(c, orc, awgn_llr)
        ref = D.reference(c, orc, llr, rule_kw(codec))
        # guards as long as one workgroup of whichever kernel serves it: the shared launch's run-time-Z schedule, or its own route
        r = D.call_route(c)
        r = r._replace(ncw=max(r.ncw, D.rtz_schedule(bg, Z)[0]))
        work.append((c._replace(batch=B), codec, llr, ref, r))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    try:
        for k, with_iters in enumerate((True, False)):
            bufs = []
            for c, codec, llr, ref, r in work:
                cc = c._replace(want_iters=with_iters)
                bufs.append((cc, ref, llr_alloc(torch, llr, r.ncw, c.llr_off, c.seed + k)) + outputs(torch, cc, r)[:2])
            runs.append(bufs)
        torch.cuda.synchronize()
        for k, with_iters in enumerate((True, False)):  # the second call goes out on the other stream before the first is synchronised
            bufs = runs[k]
            pkg.decode_multi_dev([w[1] for w in work], [b[2].ptr for b in bufs], [w[0].batch for w in work], [b[3].ptr for b in bufs],
                                 [b[4].ptr for b in bufs] if with_iters else None, streams[k].cuda_stream)
        torch.cuda.synchronize()
    finally:
        for codec in codecs:
            codec.close()
    for bufs in runs:
        for cc, ref, lb, hard, iters in bufs:
            if cc.batch == 0:  # the empty configuration: nothing of its buffers is touched
                assert hard.unchanged() and lb.unchanged() and (iters is None or iters.unchanged())
            else:
                check(cc, ref, hard, iters, None, lb)

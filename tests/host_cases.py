"""A census of decode_host (csrc/nrldpc_capi.hip), the host-pointer entry behind nrldpc_decode / nrldpc_decode_packed: a model of
its decisions that maps one call to the set of classes it executes, the universe of those classes with every exclusion's reason,
the calls of tests/test_host_paths_gpu.py (HOST_PLAN), the host-pointer calls the older test files make (OLDER_CALLS), the inputs of
the planned calls with the positions at which a helper kernel's mistake must change a decision (witnesses), and the routine that
runs one planned call on a GPU and compares it.  Plain Python; nothing here needs a GPU except run_call.

A class is a tuple whose first element names its dimension:
  ("route", ...)   zero-copy | one-copy + why | pipeline
  ("input", ...)   f16 | f32 | f64 + where the doubles are narrowed
  ("wire", ...)    format of a chunk of the pipeline
  ("expand", ...)  which branch of nrldpc_expand_i8_kernel / nrldpc_expand_i8_rows_kernel a chunk runs
  ("rows", ...)    act == pitch or compact rows, form of the expansion, act % 64
  ("split", ...)   whether a copy thread's piece starts inside a row, for EVERY worker count 1..16
  ("chunk", ...), ("first", ...), ("nchunks", ...), ("last", ...)   the chunk plan
  ("layers", ...)  where the layer count comes from
  ("out", route, ...) / ("iters", route, ...)   how the hard decisions leave, with or without iteration counts
  ("workers", ...) copy threads asked for (NRLDPC_HOST_THREADS)
  ("soft-output", ...) soft output wanted, by the size band of the input (it always goes by one copy)
A call under a knob that is read once per process (MODES but "default") is counted only for the classes its knob forces: it runs in
a child of its own, and whatever else it executes is counted where the default process executes it.
"""
from collections import namedtuple

import numpy as np

MiB = 1 << 20
BG_DIMS = {1: (46, 68, 22), 2: (42, 52, 10)}  # rows, columns, kb
AUTO = -1
NS = 4                     # staging slots (nrldpc_codec::kSlots)
GRID_THREADS = 8192 * 256  # the expand kernels' largest grid: one trip of the grid-stride loop
DEV_EB = {"f16": 2, "f32": 4, "f64": 4}   # on the device (doubles are narrowed to f32)
HOST_EB = {"f16": 2, "f32": 4, "f64": 8}
NP_DT = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
PIPE_MIN = 8 * MiB
ZC_MAX = 2 * MiB

KNOBS = ("NRLDPC_HOST_CHUNK_MB", "NRLDPC_HOST_THREADS", "NRLDPC_HOST_PIPELINE", "NRLDPC_HOST_ZEROCOPY_KB")
MODE_ENV = {"default": {}, "chunk1": {"NRLDPC_HOST_CHUNK_MB": "1"}, "threads1": {"NRLDPC_HOST_THREADS": "1"},
            "threads3": {"NRLDPC_HOST_THREADS": "3"}, "pipe0": {"NRLDPC_HOST_PIPELINE": "0"}, "zc0": {"NRLDPC_HOST_ZEROCOPY_KB": "0"}}
MODES = tuple(MODE_ENV)

# nl: 0 = every row, 4..rows, AUTO.  call_nl: decode_packed(n_layers=) of this call only.  neg: (codeword, element) of every -inf.
# auto: (count the data of every codeword shows, None | (codeword, count that one codeword shows)).  i8: False = NRLDPC_HOST_I8=0
# around the call (read per call).  esn0: operating point of the input.
Call = namedtuple("Call", "name bg Z batch nl dtype packed iters app timing neg auto mode i8 alg call_nl esn0 seed")


def call(name, bg, Z, batch, nl=0, dtype="f32", packed=False, iters=True, app=False, timing=False, neg=(), auto=None, mode="default",
         i8=True, alg="min-sum", call_nl=None, esn0=1.0, seed=0):
    return Call(name, bg, Z, batch, nl, dtype, packed, iters, app, timing, tuple(neg), auto, mode, i8, alg, call_nl, esn0, seed)


def dims(c):
    rows, cols, kb = BG_DIMS[c.bg]
    return rows, cols, kb, cols * c.Z, kb * c.Z


def data_layers(c, n_cw):
    """what NRLDPC_LAYERS_AUTO finds in the first n_cw codewords of the call's input"""
    base, late = c.auto
    return max(base, late[1]) if late and late[0] < n_cw else base


def pieces(total, parts):
    """the compact ranges [lo, hi) a chunk is quantised and sent in"""
    return [((total * p // parts) & ~63, total if p + 1 == parts else (total * (p + 1) // parts) & ~63) for p in range(parts)]


def worker_ranges(lo, hi, nw):
    """quantise_rows_start: the range of each of nw copy threads within [lo, hi)"""
    n = hi - lo
    per = ((n + nw - 1) // nw + 63) & ~63
    out = []
    for w in range(nw):
        a = lo + min(n, per * w)
        out.append((a, min(hi, a + per)))
    return out


def row_walk(a, b, act, pitch):
    """the (compact position, source element, length) pieces one copy thread quantises for its range [a, b)"""
    out, pos = [], a
    while pos < b:
        r, in_row = divmod(pos, act)
        ln = min(b - pos, act - in_row)
        out.append((pos, r * pitch + in_row, ln))
        pos += ln
    return out


def plan(c, full_scan=False):
    """decode_host's decisions for one call: route, reason, chunk plan, layer count, per-chunk wire format and expansion"""
    rows, cols, kb, ncw, K = dims(c)
    eb = DEV_EB[c.dtype]
    in_bytes = c.batch * ncw * eb
    i8 = c.i8 and c.alg == "min-sum"
    nl = c.call_nl if c.call_nl is not None else c.nl
    nl = rows if nl == 0 else nl
    p = dict(in_bytes=in_bytes, ncw=ncw, K=K, KO=(K + 7) // 8 if c.packed else K, restarted=full_scan)
    if c.mode != "pipe0" and in_bytes >= PIPE_MIN and not c.app and not c.timing:
        wire_eb = 1 if i8 else eb
        cap = ((1 if c.mode == "chunk1" else 32) << 20) // (2 if i8 else 1)
        quarter = c.batch * ncw * wire_eb // 4
        chunk = max(1, min(c.batch, min(cap, quarter) // (ncw * wire_eb)))
        p["chunk_from"] = "knob" if cap < quarter else "quarter"
        p["rounded"] = chunk >= 512
        if chunk >= 512:
            chunk -= chunk % 512
        starts = list(range(0, c.batch, chunk)) + [c.batch]
        scan_first = min(c.batch, chunk)
        layers = "per-call" if c.call_nl is not None else "explicit"
        if nl == AUTO:
            lazy = not full_scan and scan_first < c.batch
            nl = data_layers(c, scan_first if lazy else c.batch)
            layers = "auto-restart" if full_scan else "auto-first-chunk"
            if lazy and nl < rows and data_layers(c, c.batch) > nl:
                return plan(c, full_scan=True)  # (the chunks before the lifting codeword ran once with too few rows)
        act = min(ncw, (kb + nl) * c.Z) if i8 else ncw
        chunks = []
        for k in range(len(starts) - 1):
            c0, n = starts[k], starts[k + 1] - starts[k]
            total = n * act
            parts = 4 if i8 and k == 0 and total >= MiB else 1
            ch = dict(k=k, c0=c0, n=n, parts=parts, pieces=pieces(total, parts), slot=k % NS, stream=k & 1)
            negs = sorted((cw - c0) * act + e for cw, e in c.neg if c0 <= cw < c0 + n and e < act)
            ch["neg_above_act"] = any(c0 <= cw < c0 + n and e >= act for cw, e in c.neg)
            if not i8:
                ch["wire"] = "native-sum-product" if c.alg != "min-sum" else "native-i8off"
            elif negs:
                hit = next(i for i, (lo, hi) in enumerate(ch["pieces"]) if any(lo <= x < hi for x in negs))
                ch["wire"] = ("native-neg-after-sent" if hit > 0 else "native-later-chunk" if k else
                              "native-neg-nothing-sent" if parts == 4 else "native-neg-first-chunk-one-piece")
            else:
                ch["wire"] = "int8"
            if ch["wire"] == "int8":
                aligned = (c0 * ncw * eb) % 16 == 0  # d_q = s_q + slot * q_slot, q_slot a multiple of 256: always aligned
                if act == ncw:
                    ch["expand"] = "flat-vec" if aligned else "flat-scalar"
                    ch["tail"] = total % 16 if aligned else 0
                    ch["trip2"] = (total >> 4 if aligned else total) > GRID_THREADS
                else:
                    vec = act % 16 == 0 and ncw % 8 == 0 and aligned
                    ch["expand"] = "rows-vec" if vec else "rows-scalar"
                    ch["tail"] = 0
                    ch["trip2"] = (total >> 4 if vec else total) > GRID_THREADS
            chunks.append(ch)
        p.update(route="pipeline", why=None, chunk=chunk, starts=starts, nl=nl, act=act, chunks=chunks, layers=layers, i8=i8)
        return p
    layers = "per-call" if c.call_nl is not None else "explicit"
    if nl == AUTO:
        nl, layers = data_layers(c, c.batch), "auto-caller-thread"
    zc = 0 if c.mode == "zc0" else ZC_MAX
    if not c.app and not c.timing and in_bytes <= zc:
        p.update(route="zero-copy", why=None, nl=nl, layers=layers)
        return p
    if in_bytes >= PIPE_MIN:
        why = "soft-output" if c.app else "timing" if c.timing else "pipeline-off"
    elif in_bytes > ZC_MAX:
        why = "size"
    else:
        why = "soft-output" if c.app else "timing" if c.timing else "zerocopy-off"
    p.update(route="one-copy", why=why, nl=nl, layers=layers)
    return p


def split_in_row(p, nw):
    """does a piece of some copy thread start inside a row (so that the walk's first step is a partial row)?"""
    act = p["act"]
    for ch in p["chunks"]:
        if "expand" not in ch:
            continue
        for lo, hi in ch["pieces"]:
            if any(a % act and a < b for a, b in worker_ranges(lo, hi, nw)):
                return True
    return False


FORCED = {"chunk1": {("chunk", "capped-by-knob")}, "threads1": {("workers", "1")}, "threads3": {("workers", "3")},
          "pipe0": {("route", "one-copy", "pipeline-off")}, "zc0": {("route", "one-copy", "zerocopy-off")}}


def census(c):
    """the classes one call is counted for"""
    S = executed(c)
    return S if c.mode == "default" else S & FORCED[c.mode]


def executed(c):
    """the classes one call executes"""
    p = plan(c)
    rows, cols, kb, ncw, K = dims(c)
    route = p["route"]
    S = {("route", route) if route != "one-copy" else ("route", route, p["why"]), ("layers", p["layers"])}
    if c.packed:
        if route == "zero-copy":
            S.add(("out", route, "cpu-pack-partial" if K % 8 else "cpu-pack-whole"))
        else:
            S.add(("out", route, "pack-kernel-narrow" if K % 8 else "pack-kernel-wide"))  # d_hard = s_hard + c0 * K: aligned with K
    else:
        S.add(("out", route, "bytes"))
    S.add(("iters", route, "yes" if c.iters else "no"))
    if c.app:
        S.add(("soft-output", "<=2MiB" if p["in_bytes"] <= ZC_MAX else "2-8MiB" if p["in_bytes"] < PIPE_MIN else ">=8MiB"))
    if route != "pipeline":
        S.add(("input", "f64", "caller-thread") if c.dtype == "f64" else ("input", c.dtype))
        return S
    S.add(("workers", {"threads1": "1", "threads3": "3"}.get(c.mode, "default")))
    S.add(("chunk", "rounded512" if p["rounded"] else "below512"))
    S.add(("chunk", "capped-by-knob" if p["chunk_from"] == "knob" else "quarter-of-batch"))
    S.add(("nchunks", ">4" if len(p["chunks"]) > NS else "<=4"))
    last = p["chunks"][-1]["n"]
    S.add(("last", "single" if last == 1 and p["chunk"] > 1 else "full" if last == p["chunk"] else "short"))
    wires = {ch["wire"] for ch in p["chunks"]}
    for ch in p["chunks"]:
        w = ch["wire"]
        S.add(("wire", w))
        if ch["k"] == 0 and p["i8"]:
            S.add(("first", "four-pieces" if ch["parts"] == 4 else "one-piece"))
        if c.dtype == "f64":
            S.add(("input", "f64", "quantiser" if w == "int8" or w == "native-neg-after-sent" else "move-narrow"))
            if w.startswith("native-neg") or w == "native-later-chunk":
                S.add(("input", "f64", "move-narrow"))
        else:
            S.add(("input", c.dtype))
        if w != "int8":
            continue
        if ch["neg_above_act"]:
            S.add(("wire", "int8", "neg-above-act"))
        e = ch["expand"]
        S.add(("expand", e) if not ch["trip2"] else ("expand", e, "trip2"))
        if ch["trip2"]:
            S.add(("expand", e))
        if ch["tail"]:
            S.add(("expand", "flat-tail", ch["tail"]))
        if p["act"] == ncw:
            S.add(("rows", "full"))
        else:
            S.add(("rows", "compact", e, "act%64==0" if p["act"] % 64 == 0 else "act%64!=0"))
    if p["i8"] and p["act"] != ncw and "int8" in wires:
        S.add(("split", "in-row" if all(split_in_row(p, nw) for nw in range(1, 17)) else "row-aligned-for-some-worker-count"))
    return S


# ---- the universe ------------------------------------------------------------------------------------------------------------------------
ROUTES = ("zero-copy", "one-copy", "pipeline")


def product():
    U = [("route", "zero-copy"), ("route", "pipeline")]
    U += [("route", "one-copy", w) for w in ("size", "soft-output", "timing", "pipeline-off", "zerocopy-off")]
    U += [("input", "f16"), ("input", "f32")] + [("input", "f64", w) for w in ("caller-thread", "move-narrow", "quantiser")]
    U += [("wire", w) for w in ("int8", "native-i8off", "native-sum-product", "native-neg-nothing-sent", "native-neg-after-sent",
                                "native-neg-first-chunk-one-piece", "native-later-chunk")] + [("wire", "int8", "neg-above-act")]
    for e in ("flat-vec", "flat-scalar", "rows-vec", "rows-scalar"):
        U += [("expand", e), ("expand", e, "trip2")]
    U += [("expand", "flat-tail", t) for t in range(1, 16)]
    U += [("rows", "full")] + [("rows", "compact", e, m) for e in ("rows-vec", "rows-scalar") for m in ("act%64==0", "act%64!=0")]
    U += [("split", "in-row"), ("split", "row-aligned-for-some-worker-count")]
    U += [("chunk", x) for x in ("rounded512", "below512", "capped-by-knob", "quarter-of-batch")]
    U += [("first", "four-pieces"), ("first", "one-piece"), ("nchunks", "<=4"), ("nchunks", ">4")]
    U += [("last", x) for x in ("full", "short", "single")]
    U += [("layers", x) for x in ("explicit", "per-call", "auto-first-chunk", "auto-restart", "auto-caller-thread")]
    for r in ROUTES:
        U += [("out", r, k) for k in ("bytes", "pack-kernel-wide", "pack-kernel-narrow", "cpu-pack-whole", "cpu-pack-partial")]
        U += [("iters", r, "yes"), ("iters", r, "no")]
    U += [("workers", "default"), ("workers", "1"), ("workers", "3")]
    U += [("soft-output", b) for b in ("<=2MiB", "2-8MiB", ">=8MiB")]
    return U


ALL_Z = sorted(a * 2 ** j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a * 2 ** j <= 384)


def misaligned_chunk_shapes():
    """Every (bg, Z, dtype, knob) whose chunk start c0 * ncols * Z * eb can miss a multiple of 16 -- the flat kernel's vec == 0
    launch and the rows kernel's scalar form for want of alignment.  A start misses only when ncols * Z * eb is no multiple of 16:
    68 Z eb and 52 Z eb are multiples of 16 for eb = 4 and for even Z, so fp16 at an odd Z (at most 15) is left.  Such a codeword
    holds at most 68 * 15 = 1020 LLRs, the pipeline starts at 8 MiB = 4 Mi fp16 LLRs, a chunk is min(knob, a quarter of the
    batch) / ncw codewords and the knob is at least 1 MiB / 2 of int8: at least 512 Ki / 1020 = 514 codewords, so the chunk is rounded
    down to a multiple of 512 and every start is a multiple of 512 codewords.  Enumerated, not assumed: the list comes back empty."""
    bad = []
    for bg in (1, 2):
        for Z in ALL_Z:
            for dt in ("f16", "f32", "f64"):
                ncw = BG_DIMS[bg][1] * Z
                if ncw * DEV_EB[dt] % 16 == 0:
                    continue
                bmin = -(-PIPE_MIN // (ncw * DEV_EB[dt]))
                for mode in ("default", "chunk1"):
                    for i8 in (True, False):
                        # the chunk grows with the batch up to the knob's cap: the smallest batch and the cap bound it from both sides
                        for batch in (bmin, bmin + 1, bmin + 2, bmin + 3, 4 * bmin, 64 * bmin):
                            ch = plan(call("probe", bg, Z, batch, dtype=dt, mode=mode, i8=i8))["chunk"]
                            if ch * ncw * DEV_EB[dt] % 16:
                                bad.append((bg, Z, dt, mode, i8, batch, ch))
    return bad


IMPOSSIBLE = [
    ("a tail of the flat kernel is n_rows * ncols * Z mod 16 and ncols * Z = 4 * (17 Z or 13 Z): only 4, 8 and 12 occur",
     lambda c: c[:2] == ("expand", "flat-tail") and c[2] % 4 != 0),
    ("the CPU packs only on the zero-copy route and the pack kernel runs only on the other two",
     lambda c: c[0] == "out" and ((c[1] == "zero-copy") != c[2].startswith("cpu-pack")) and c[2] != "bytes"),
]
OUTSIDE_THE_CALLS = [
    ("a second trip of a vector form needs more than 8192 * 256 * 16 = 32 Mi int8 LLRs in one chunk; a chunk is capped at "
     "NRLDPC_HOST_CHUNK_MB / 2, 16 MiB of int8 at the default of 32: reachable through the C ABI with the knob at 65 or more and "
     "a batch of 128 Mi LLRs, larger than any array the suite builds -- it exists and is not planned",
     lambda c: c in (("expand", "flat-vec", "trip2"), ("expand", "rows-vec", "trip2"))),
    ("the flat kernel's vec == 0 launch (and its second trip) needs a chunk start c0 * ncols * Z * eb off a multiple of 16: "
     "misaligned_chunk_shapes() enumerates every lifting size, type and knob value and finds none -- launch_expand_i8 keeps the "
     "branch for callers other than decode_host, and there are none in the C ABI",
     lambda c: c[:2] == ("expand", "flat-scalar")),
    ("the pack kernel's narrow branch at K % 8 == 0 needs an unaligned d_hard; decode_host passes s_hard + c0 * K, a multiple of 8 "
     "from a 256-byte-aligned base (not a class of its own here: the narrow class is K % 8 != 0)", lambda c: False),
    ("NRLDPC_HOST_THREADS values other than the default, 1 and 3 exist and are not planned", lambda c: False),
]


def universe():
    return {c for c in product() if not any(t(c) for _, t in IMPOSSIBLE + OUTSIDE_THE_CALLS)}


def reached(calls):
    S = set()
    for c in calls:
        S |= census(c)
    return S


def missing(calls):
    return sorted(universe() - reached(calls), key=repr)


# ---- the planned calls -------------------------------------------------------------------------------------------------------------------
# Each is the smallest batch that reaches its class: the pipeline starts at batch * ncols * Z * eb >= 8 MiB (f64 counts 4 bytes), the
# chunk is floor(batch / 4) codewords, rounded down to a multiple of 512 from 512 on.
Z20 = dict(bg=2, Z=20, batch=2017, nl=12, esn0=3.0)          # the reference's default operating point: act = 440, 5 chunks of 504 + 1
Z7 = dict(bg=2, Z=7, esn0=-4.0)                              # ncw = 364 = 12 mod 16, K = 70; 6 chunks of 1024 (slot reuse)
HOST_PLAN = [
    # rows scalar; compact rows with act % 64 = 56; a last chunk of one codeword, which holds a -inf (native beside int8 neighbours);
    # one -inf above act in chunk 1, which must neither force the fall-back nor change a result
    call("z20_rows_scalar", neg=((2016, 7 * 20 + 3), (700, 440 + 5)), seed=1, **Z20),
    # the same shape as doubles: narrowed inside the quantiser, and by move(narrow) in the chunks that hold a -inf -- the first, which
    # goes in one piece, and the third; packed, K = 200
    call("z20_f64_packed", dtype="f64", packed=True, neg=((2, 439), (1100, 3 * 20 + 1)), seed=2, **Z20),
    # AUTO settled by the first chunk / lifted by the last codeword (restart with a full scan): act = 440 / 600, both scalar
    call("z20_auto_first", auto=(12, None), seed=3, **dict(Z20, nl=AUTO)),
    call("z20_auto_restart", auto=(12, (2016, 20)), seed=4, **dict(Z20, nl=AUTO)),
    # a per-call count on a handle made with every row, no iteration counts
    call("z20_call_layers", packed=True, iters=False, call_nl=12, seed=5, **dict(Z20, nl=0)),
    # NRLDPC_HOST_I8=0 and sum-product: every chunk in the handle's own format
    call("z20_i8off", i8=False, seed=6, **Z20),
    call("z20_sum_product", alg="sum-product", seed=7, **Z20),
    # the one-copy route forced by set_timing on the pipelined shape
    call("z20_timing", timing=True, seed=1, **Z20),
    # flat tails of 12, 8 and 4 in the last chunk; the narrow pack kernel in the pipeline; more chunks than slots
    call("z7_tail12", batch=5765, seed=11, **Z7),
    call("z7_tail8", batch=5762, iters=False, seed=12, **Z7),
    call("z7_tail4_packed", batch=5763, packed=True, seed=13, **Z7),
    # rows vector with act = 112 (48 mod 64): sixteen-element stores either side of every row end
    call("z8_rows_vec", bg=2, Z=8, batch=5042, nl=4, esn0=5.0, seed=21),
    # rows vector with act = 128, fp16 input
    call("z8_rows_vec_64", bg=2, Z=8, batch=10083, nl=6, dtype="f16", esn0=4.0, seed=22),
    # rows scalar for want of an 8-element pitch (odd Z) while act = 64 Z: BG1 with 42 rows, kb + 42 = 64
    call("z3_rows_scalar_64", bg=1, Z=3, batch=10281, nl=42, esn0=-2.0, seed=23),
    # the first chunk in four pieces (41 * 26112 >= 1 MiB): a -inf in its first piece (nothing sent yet) / in its third (two
    # pieces queued: the stream is synchronised before the fall-back overwrites the pinned slot); a last chunk that is full
    call("z384_neg_piece0", bg=1, Z=384, batch=164, neg=((3, 5 * 384 + 9),), esn0=-1.0, seed=31),
    call("z384_neg_piece2", bg=1, Z=384, batch=164, neg=((25, 30 * 384 + 2),), esn0=-1.0, seed=32),
    # the scalar rows kernel's second grid-stride trip: 508 * 4136 > 8192 * 256 >= 507 * 4136 (batch 2032, not the 2040 first worked by hand)
    call("z88_trip2", bg=1, Z=88, batch=2032, nl=25, dtype="f16", esn0=1.0, seed=41),
    # one copy: between 2 and 8 MiB, packed at K % 8 == 0 and != 0, and with soft output
    call("one_copy_wide", bg=2, Z=20, batch=505, nl=12, packed=True, esn0=3.0, seed=51),
    call("one_copy_narrow", batch=1441, packed=True, iters=False, seed=52, **Z7),
    call("one_copy_app", bg=2, Z=20, batch=505, nl=12, app=True, esn0=3.0, seed=51),
    call("small_app", bg=2, Z=20, batch=5, nl=12, app=True, esn0=3.0, seed=53),
    call("z20_app", app=True, seed=1, **Z20),
    # zero copy: the CPU packs, with and without a last partial byte; AUTO on the caller's thread; doubles narrowed there
    call("zero_copy_partial", batch=33, packed=True, seed=61, **Z7),
    call("zero_copy_whole", bg=2, Z=20, batch=5, packed=True, iters=False, dtype="f64", nl=AUTO, auto=(12, None), esn0=3.0, seed=62),
    call("zero_copy_bytes", bg=2, Z=20, batch=5, nl=12, dtype="f16", iters=False, esn0=3.0, seed=63),
    # knobs read once per process: each runs in a fresh child (tests/host_knob_child.py)
    call("chunk1_z88", bg=1, Z=88, batch=2032, nl=25, dtype="f16", mode="chunk1", esn0=1.0, seed=41),
    call("threads1_z20", mode="threads1", neg=((2016, 7 * 20 + 3), (700, 440 + 5)), seed=1, **Z20),
    call("threads3_z8", bg=2, Z=8, batch=5042, nl=4, mode="threads3", esn0=5.0, seed=21),
    call("pipe0_z20", mode="pipe0", packed=True, seed=2, **Z20),
    call("zc0_z7", batch=33, packed=True, mode="zc0", iters=False, seed=61, **Z7),
]
BY_NAME = {c.name: c for c in HOST_PLAN}
assert len(BY_NAME) == len(HOST_PLAN)

# ---- the host-pointer calls of the older test files, their shapes copied as data ---------------------------------------------------------
_E = dict(esn0=0.0)
OLDER_CALLS = (
    # test_full_size_gpu.py: round trips, host against device, the pipelined path (with NRLDPC_HOST_I8=0 as well)
    [call("cfg2", 1, 384, 4096, dtype="f16"), call("cfg5", 1, 384, 8192, nl=5, dtype="f16"), call("hostdev", 2, 384, 4096, nl=22, dtype="f16")]
    + [call("cfg3_%d" % n, 2, 384, 4096, nl=n, dtype="f16") for n in (42, 32, 22, 17, 12, 9, 7)]
    + [call("pipe_%s_%d%s%s" % (dt, B, "" if i8 else "_native", "" if it else "_noit"), bg, Z, B, dtype=dt, i8=i8, iters=it,
            neg=((B // 3, 9 * Z + 3), (B // 3, 40 * Z + 1)))
       for dt, B, bg, Z in (("f64", 1237, 1, 384), ("f32", 1001, 1, 384), ("f16", 2049, 1, 384), ("f32", 9001, 2, 20), ("f64", 3001, 1, 36))
       for i8, it in ((True, True), (True, False), (False, True))]
    # test_layers_gpu.py::test_auto_on_the_pipelined_host_path (the grid test and the pool decode small batches, zero-copy)
    + [c for dt in ("f16", "f64") for c in (
        call("auto_%s" % dt, 1, 384, 700, nl=AUTO, auto=(5, None), dtype=dt, neg=((695, 2 * 384 + 3),)),
        call("auto_pk_%s" % dt, 1, 384, 700, nl=AUTO, auto=(5, None), dtype=dt, neg=((695, 2 * 384 + 3),), packed=True, iters=False),
        call("junk_%s" % dt, 1, 384, 700, nl=5, dtype=dt, neg=((695, 2 * 384 + 3),)),
        call("auto8_%s" % dt, 1, 384, 8, nl=AUTO, auto=(46, None), dtype=dt, iters=False),
        call("late_%s" % dt, 1, 384, 700, nl=AUTO, auto=(5, (699, 19)), dtype=dt, neg=((695, 2 * 384 + 3),)))]
    + [call("grid_%d_%d" % (bg, Z), bg, Z, 6, nl=n, dtype="f16", auto=(8, None)) for bg in (1, 2) for Z in (2, 20, 384) for n in (AUTO, 8)]
    # test_decode_gpu.py::test_bit_packed_hard_output
    + [call("pk_%d_%d_%s_%d" % (bg, Z, dt, pk), bg, Z, B, dtype=dt, packed=bool(pk))
       for bg, Z, B in ((1, 384, 700), (2, 7, 33), (1, 3, 5), (2, 96, 9000), (1, 64, 1)) for dt in ("f16", "f64") for pk in (0, 1)]
    # test_sum_product_gpu.py: small batches, soft output, one batch large enough for the pipeline
    + [call("sp_small", 1, 20, 24, dtype="f32", alg="sum-product", app=True), call("sp_small2", 2, 20, 48, dtype="f16", alg="sum-product"),
       call("sp_pk", 1, 64, 96, nl=20, alg="sum-product", packed=True), call("sp_pk_nl", 1, 64, 96, nl=0, call_nl=20, alg="sum-product", packed=True),
       call("sp_f64", 1, 64, 96, nl=20, dtype="f64", alg="sum-product"), call("sp_big", 1, 64, 600, alg="sum-product"),
       call("ms_app", 2, 20, 16, nl=12, app=True)]
)


# ---- critical positions: where a helper kernel's mistake lands ---------------------------------------------------------------------------
SPECIALS = (np.nan, np.inf, -0.0, 0.0625, 1e4, 0.0)  # NaN, a +inf filler, -0, a rounding tie, a clamped value, +0
STRONG = 15.875                                      # 127 grid units: the largest value that is not clamped


def critical(c):
    """{class: [(codeword, element), ...]} for the helper classes of a pipelined call, and the first inactive element of compact rows
    under 'inactive' (the opposite case: junk there must change nothing)"""
    p = plan(c)
    out = {}
    if p["route"] != "pipeline":
        return out
    act, ncw = p["act"], p["ncw"]
    for ch in p["chunks"]:
        if ch["wire"] != "int8":
            continue
        c0, n = ch["c0"], ch["n"]
        if ch["tail"]:
            out.setdefault(("expand", "flat-tail", ch["tail"]), []).extend((c0 + n - 1, ncw - ch["tail"] + j) for j in range(ch["tail"]))
        rws = sorted({0, 1, n // 2, n - 1} & set(range(n)))
        if ch["expand"] == "rows-scalar":
            # under AUTO with a lifting codeword only that codeword holds anything above the first chunk's count (else the first
            # scan would find the whole batch's count and nothing would restart): the others end at the first count's last element
            base = act if not (c.auto and c.auto[1]) else min(act, (BG_DIMS[c.bg][2] + c.auto[0]) * c.Z)
            out.setdefault(("expand", "rows-scalar"), []).extend(
                (c0 + r, e) for r in rws for e in (0, (act if c.auto and c.auto[1] and c0 + r == c.auto[1][0] else base) - 1))
            if not c.auto:
                out.setdefault("inactive", []).extend((c0 + r, act) for r in rws)
            if ch["trip2"]:
                r, e = divmod(GRID_THREADS, act)
                out.setdefault(("expand", "rows-scalar", "trip2"), []).extend((c0 + r, e + j) for j in range(2))
        if ch["expand"] == "rows-vec":
            for r in rws[:-1]:
                out.setdefault(("expand", "rows-vec"), []).extend([(c0 + r, act - 16 + j) for j in range(16)] + [(c0 + r + 1, j) for j in range(16)])
            out.setdefault("inactive", []).extend((c0 + r, act) for r in rws)
    return out


def build_input(orc, c):
    """(llr [batch][ncw] in the call's type, info bits, {class: positions}): noisy codewords below the waterfall; strong values of the
    transmitted sign at every critical position but those whose index is 2 mod 3 within their class (the last excepted), which carry NaN, +inf, -0, a
    tie, a clamped value and +0 in turn; the columns no active layer reads hold junk under an explicit count and zeros under AUTO;
    the -inf of the call."""
    rows, cols, kb, ncw, K = dims(c)
    rng = np.random.default_rng(7000 + c.seed)
    n_src = min(c.batch, 64)
    info = rng.integers(0, 2, (n_src, K), dtype=np.uint8)
    cw = np.tile(orc.encode(c.bg, c.Z, info), (-(-c.batch // n_src), 1))[:c.batch]
    info = np.tile(info, (-(-c.batch // n_src), 1))[:c.batch]
    mu = 2.0 * 10.0 ** (c.esn0 / 10.0)
    llr = (1 - 2.0 * cw) * mu
    llr += np.sqrt(2 * mu) * rng.standard_normal(cw.shape, dtype=np.float32)
    llr[:, :2 * c.Z] = 0
    p = plan(c)
    nl = p["nl"]
    top = (kb + nl) * c.Z
    if c.auto:
        llr[:, (kb + c.auto[0]) * c.Z:] = 0
        if c.auto[1]:
            b, n = c.auto[1]
            llr[b, (kb + n) * c.Z - 1] = 0.5
    elif top < ncw:
        llr[:, top:] = 5 * rng.standard_normal((c.batch, ncw - top), dtype=np.float32)
    crit = critical(c)
    for cls, pos in crit.items():
        for i, (b, e) in enumerate(pos):
            if cls == "inactive":
                llr[b, e] = (STRONG, -1e4, np.nan)[i % 3]
            elif i % 3 == 2 and i != len(pos) - 1:  # (the last position of a class stays strong: a loop that ends one early shows)
                llr[b, e] = SPECIALS[(i // 3) % len(SPECIALS)]
            else:
                llr[b, e] = (1 - 2.0 * cw[b, e]) * STRONG
    for b, e in c.neg:
        llr[b, e] = -np.inf
    llr = llr.astype(NP_DT[c.dtype])
    if c.auto:  # the data really is what the model was told: the first chunk shows the base count, the whole batch the final one
        first = min(c.batch, p.get("chunk", c.batch))
        assert np_count_layers(c, llr[:first]) == c.auto[0] and np_count_layers(c, llr) == nl == data_layers(c, c.batch), \
            (c.name, np_count_layers(c, llr[:first]), np_count_layers(c, llr))
        if c.auto[1]:
            assert p["restarted"] == (np_count_layers(c, llr[:first]) < np_count_layers(c, llr)), c.name
    return llr, info, crit


def np_count_layers(c, llr):
    """NRLDPC_LAYERS_AUTO's count, by a plain scan: the highest column block from kb + 4 up that holds anything but +-0 and NaN"""
    rows, cols, kb, ncw, K = dims(c)
    x = np.asarray(llr, np.float64).reshape(-1, cols, c.Z)
    live = (np.nan_to_num(x, nan=0.0, posinf=1.0, neginf=-1.0) != 0).any((0, 2))
    top = max([b for b in range(kb + 4, cols) if live[b]], default=kb + 3)
    return max(4, top - kb + 1)


def poison_of(c, llr):
    """the poison array of a call: every finite LLR negated, every infinity and NaN 0; under AUTO with a lifting codeword its lifting
    value is 0 too, so that the poison call settles on the first chunk's count and does not restart"""
    rows, cols, kb, ncw, K = dims(c)
    poison = np.where(np.isfinite(llr), -llr, 0).astype(llr.dtype)
    if c.auto and c.auto[1]:
        poison[c.auto[1][0], (kb + c.auto[0]) * c.Z:] = 0
        assert np_count_layers(c, poison) == c.auto[0], c.name
    return poison


MAX_ITER = 3
ALPHA = 0.625


def oracle_decode(orc, c, llr, nl):
    return orc.decode_nmsq(c.bg, c.Z, np.asarray(llr, np.float64), MAX_ITER, n_layers=nl, early_term=True, alpha=ALPHA)


def witnesses(orc, c, llr, positions, nl):
    """the positions at which negating that one LLR changes the oracle's hard decisions or iteration count of its codeword"""
    out = []
    for b, e in positions:
        x = np.array(llr[b], np.float64)
        h0, i0 = oracle_decode(orc, c, x, nl)
        x[e] = -x[e]
        h1, i1 = oracle_decode(orc, c, x, nl)
        if (h0 != h1).any() or i0[0] != i1[0]:
            out.append((b, e))
    return out


# ---- one planned call on the GPU ----------------------------------------------------------------------------------------------------------
GUARD = 3
PATTERN = 0xA5


def raw_decode(pkg, codec, c, llr, poison=False):
    """nrldpc_decode / nrldpc_decode_packed[_layers] on arrays this routine owns: outputs prefilled with a pattern, GUARD rows either
    side; returns (hard [batch][KO], iters or None, app or None) after checking the guards"""
    capi = pkg._capi
    B, KO = llr.shape[0], (codec.K + 7) // 8 if c.packed else codec.K
    hard = np.full((B + 2 * GUARD, KO), PATTERN, np.uint8)
    iters = np.full(B + 2 * GUARD, -0x5A5A5A5B, np.int32) if c.iters else None
    app = np.full((B + 2 * GUARD, codec.N_cw), -77.25, np.float32) if c.app else None
    ptr = lambda a: capi._ptr(a[GUARD:]) if a is not None else None  # noqa: E731
    L, h = codec._lib, codec._h
    if c.packed and c.call_nl is not None:
        capi.check(L.nrldpc_decode_packed_layers(h, capi._ptr(llr), B, ptr(hard), ptr(iters), int(c.call_nl)))
    elif c.packed:
        capi.check(L.nrldpc_decode_packed(h, capi._ptr(llr), B, ptr(hard), ptr(iters)))
    else:
        capi.check(L.nrldpc_decode(h, capi._ptr(llr), B, ptr(hard), ptr(iters), ptr(app)))
    for a, v in ((hard, PATTERN), (iters, -0x5A5A5A5B), (app, -77.25)):
        if a is not None:
            assert (a[:GUARD] == v).all() and (a[-GUARD:] == v).all(), (c.name, "guard rows overwritten", "poison" if poison else "")
    return hard[GUARD:-GUARD], None if iters is None else iters[GUARD:-GUARD], None if app is None else app[GUARD:-GUARD]


def dev_decode(pkg, c, llr, nl, want_app=False):
    """one nrldpc_decode_dev launch on the same LLRs (doubles narrowed to f32): a different route to the same decoder kernels"""
    import torch
    dt = np.float32 if c.dtype == "f64" else NP_DT[c.dtype]
    cd = pkg.Codec(c.bg, c.Z, max_iter=MAX_ITER, n_layers=nl, early_term=True, alpha=ALPHA, llr_dtype=dt, algorithm=c.alg)
    B = llr.shape[0]
    d_llr = torch.from_numpy(llr.astype(dt)).cuda()
    d_h = torch.full((B, cd.K), 7, dtype=torch.uint8, device="cuda")
    d_it = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    d_app = torch.zeros((B, cd.N_cw), dtype=torch.float32, device="cuda") if want_app else None
    cd.decode_dev(d_llr.data_ptr(), B, d_h.data_ptr(), d_it.data_ptr(), d_app.data_ptr() if want_app else None,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cd.close()
    return d_h.cpu().numpy(), d_it.cpu().numpy(), d_app.cpu().numpy() if want_app else None


def run_call(pkg, orc, c, env=None):
    """Poison the handle's staging, make the call, compare bit for bit with the oracle and with one device launch, and hold the
    library's own report of the pipeline against the model.  Returns a record of what was compared."""
    import os
    rows, cols, kb, ncw, K = dims(c)
    p = plan(c)
    llr, info, crit = build_input(orc, c)
    nl_handle = c.nl
    codec = pkg.Codec(c.bg, c.Z, max_iter=MAX_ITER, n_layers=nl_handle, early_term=True, alpha=ALPHA, llr_dtype=NP_DT[c.dtype],
                      algorithm=c.alg)
    if not c.i8:
        os.environ["NRLDPC_HOST_I8"] = "0"
    try:
        if c.timing:  # the pipelined result of the same handle first, timing off
            twin = c._replace(timing=False)
            assert plan(twin)["route"] == "pipeline"
            raw_decode(pkg, codec, twin, poison_of(c, llr), poison=True)
            piped = raw_decode(pkg, codec, twin, llr)
            codec.set_timing(True)
        poison = poison_of(c, llr)
        raw_decode(pkg, codec, c, poison, poison=True)
        if c.auto:
            assert codec.last_layers() == c.auto[0] == pkg._capi.count_layers(c.bg, c.Z, poison), (c.name, "poison call's layer count")
        before = llr.copy()
        hard, iters, app = raw_decode(pkg, codec, c, llr)
        assert llr.tobytes() == before.tobytes(), (c.name, "the caller's LLRs were written")
        ph = codec.last_host_phases()
        last_nl = codec.last_layers()
        if c.timing:
            codec.set_timing(False)
            assert (piped[0] == hard).all() and (piped[1] == iters).all(), (c.name, "one-copy under timing differs from the pipeline")
    finally:
        if not c.i8:
            del os.environ["NRLDPC_HOST_I8"]
        codec.close()
    nl = p["nl"]
    rec = dict(name=c.name, route=p["route"], layers=nl, compared=c.batch)
    assert last_nl == nl, (c.name, "layer count", last_nl, nl)
    if c.auto:
        assert pkg._capi.count_layers(c.bg, c.Z, llr) == nl, (c.name, "count_layers")
    if p["route"] != "pipeline" and not c.timing:  # a handle that never ran the pipeline has no phases to report
        assert ph is None, (c.name, "the model says", p["route"], "but the library reports a pipelined call", ph)
    if c.auto:
        first = min(c.batch, p.get("chunk", c.batch))
        assert pkg._capi.count_layers(c.bg, c.Z, llr[:first]) == c.auto[0], (c.name, "count_layers of the first chunk")
        if c.auto[1]:  # the restart: the first chunk alone shows fewer rows than the batch
            assert p["restarted"] and c.auto[0] < nl
    if p["route"] == "pipeline":
        assert ph is not None and (ph["chunks"], ph["codewords_per_chunk"], ph["layers"]) == (len(p["chunks"]), p["chunk"], nl), \
            (c.name, "the library reports", ph, "the model", len(p["chunks"]), p["chunk"], nl)
        rec.update(chunks=ph["chunks"], codewords_per_chunk=ph["codewords_per_chunk"])
    if c.packed:
        bits = np.unpackbits(hard, axis=1, bitorder="little")
        assert not bits[:, K:].any(), (c.name, "unused bits of the last byte are set")
        hard = bits[:, :K]
        if K % 8:  # every bit of the last partial byte takes both values somewhere in the batch: a dropped bit shows
            tail = hard[:, K - K % 8:]
            assert tail.any(0).all() and not tail.all(0).any(), (c.name, "the last partial byte's bits are constant over the batch")
    d_h, d_it, d_app = dev_decode(pkg, c, llr, nl, want_app=c.app)
    bad = np.flatnonzero((d_h != hard).any(1))
    assert bad.size == 0, (c.name, "hard decisions differ from one device launch at codewords", bad[:8].tolist())
    if c.iters:
        bad = np.flatnonzero(d_it != iters)
        assert bad.size == 0, (c.name, "iteration counts differ from one device launch at codewords", bad[:8].tolist())
    if c.app:
        assert app.tobytes() == d_app.tobytes(), (c.name, "soft output differs from one device launch")
    if c.alg == "min-sum":  # (sum-product has no bit-exact CPU twin: the device launch is its reference)
        ho, io = oracle_decode(orc, c, llr, nl)
        bad = np.flatnonzero((ho != hard).any(1))
        assert bad.size == 0, (c.name, "hard decisions differ from the oracle at codewords", bad[:8].tolist())
        if c.iters:
            bad = np.flatnonzero(io != iters)
            assert bad.size == 0, (c.name, "iteration counts differ from the oracle at codewords", bad[:8].tolist())
        rec["errors"] = float((ho != info).any(1).mean())
        rec["iters"] = sorted(set(io.tolist()))
    return rec

"""A census of the decoder's dispatch behind nrldpc_decode_dev / nrldpc_decode_multi_dev: a model, restated from the source, of which
kernel one decode launch runs (launch_decode in csrc/nrldpc_decode.hip and the launchers of nrldpc_decode_z64.h / _z64s.h / _z64p.h),
the universe of kernel instantiations and data-path classes the default process can reach, the device-pointer calls the older tests
make (older_calls()), and the plan of calls tests/test_decode_dev_contract_gpu.py runs on buffers of its own.  Plain Python: no torch,
no GPU; the oracle is asked only by inputs() / reference().

A route is the launcher family ("kind") and, inside it, the build:
  ilv             interleaved block geometry (NRLDPC_Z64I_LIST), PLAIN | ETP, every row | NL_RT, with the mode bit that admitted it
  packed          packed geometry (NRLDPC_Z64P_LIST; NRLDPC_Z64P_NL_LIST for a layer count of its own), PLAIN | ETP, rows | NL_RT | NL
  packed_general  BG2's general kernel of the packed geometry (any layer count, soft output)
  split           block geometry, two threads per check row, PLAIN | ETP | ETP + CRC, rows | NL_RT | a pruned-count unit
  row             block geometry, one thread per check row, PLAIN | ETP | ETP + CRC, rows | NL_RT | a pruned-count unit
  general         block geometry, the unpipelined kernel (soft output)
  rtz             the run-time-Z kernel, with or without the CRC fold; the LLR type is a template argument here and only here
An instantiation is (unit name space, kernel name with its template arguments) -- what a profiler prints for the launch.

Excluded from the universe, and why (EXCLUDED): routes behind knobs read once per process, the -DNRLDPC_Z64_AB and
NRLDPC_BUILD_ALLMODES builds, the sum-product kernel and nrldpc_decode_cw_dev (tests of their own), NRLDPC_Z64PR_LIST (empty).
"""
import zlib
from collections import namedtuple

import numpy as np

BG_DIMS = {1: (46, 68, 22), 2: (42, 52, 10)}  # rows, columns, kb
ALL_Z = sorted(a * 2 ** j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a * 2 ** j <= 384)
NL_RT = 0  # nrldpc_device.h:53 -- the template value of "layer count read at run time"

# ---- the lists, as build.py mirrors them (tests/test_capi_symbols.py holds build.py to the headers; test_decode_cases.py holds these
# to build.py) -------------------------------------------------------------------------------------------------------------------
Z64_BG1 = (60, 64, 104, 112, 120, 128, 144, 176, 192, 208, 224, 240, 256, 288, 320, 352, 384)
Z64_BG2 = (52, 60, 64, 88, 96, 104, 112, 120, 128, 144, 192, 208, 224, 240, 256, 288, 320, 352, 384)
Z64_PAIRS = [(1, z) for z in Z64_BG1] + [(2, z) for z in Z64_BG2]
Z64P_BG1 = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 26, 28, 30, 32, 36, 40, 44, 48, 52, 56, 72, 80, 88, 96,
            176, 352)
Z64P_BG2 = Z64P_BG1[:-4]
Z64P_PAIRS = [(1, z) for z in Z64P_BG1] + [(2, z) for z in Z64P_BG2]
Z64P_NL = [(2, 20, 12)]
Z64PR = []
Z64I = [
    (1, 2, 128, 5), (1, 3, 128, 7), (1, 4, 64, 5), (1, 5, 48, 7), (1, 6, 64, 7), (1, 7, 32, 5), (1, 8, 32, 5), (1, 9, 28, 5),
    (1, 10, 24, 5), (1, 11, 20, 5), (1, 12, 32, 1), (1, 13, 16, 1), (1, 14, 16, 1), (1, 15, 16, 1), (1, 16, 16, 5), (1, 18, 14, 5),
    (1, 20, 12, 1), (1, 22, 10, 1), (1, 24, 16, 1), (1, 26, 8, 1), (1, 28, 8, 1), (1, 30, 8, 1), (1, 32, 8, 5), (1, 36, 7, 7),
    (1, 40, 6, 5), (1, 44, 5, 7), (1, 48, 8, 1), (1, 52, 4, 5), (1, 56, 4, 5), (1, 60, 4, 7), (1, 64, 4, 7), (1, 72, 5, 1),
    (1, 80, 3, 7), (1, 96, 4, 7), (1, 104, 2, 7), (1, 112, 2, 3), (1, 120, 2, 3), (1, 128, 2, 7), (1, 160, 1, 6), (1, 192, 2, 1),
    (2, 2, 128, 3), (2, 4, 64, 7), (2, 5, 48, 7), (2, 7, 32, 6), (2, 8, 32, 7), (2, 9, 28, 7), (2, 10, 24, 7), (2, 11, 20, 7),
    (2, 13, 16, 5), (2, 14, 16, 5), (2, 15, 16, 5), (2, 16, 16, 5), (2, 18, 14, 5), (2, 20, 12, 5), (2, 22, 10, 5), (2, 26, 8, 5),
    (2, 28, 8, 5), (2, 30, 8, 5), (2, 32, 8, 5), (2, 36, 7, 7), (2, 40, 6, 5), (2, 44, 5, 7), (2, 52, 4, 1), (2, 56, 4, 1),
    (2, 60, 4, 1), (2, 64, 4, 1), (2, 80, 3, 7), (2, 88, 5, 1), (2, 96, 4, 1), (2, 104, 2, 1), (2, 112, 2, 1), (2, 120, 2, 1),
    (2, 128, 2, 1), (2, 160, 3, 1), (2, 176, 1, 1),
]
Z64_NL = [(1, 384, 5), (1, 384, 13), (1, 384, 24), (2, 384, 32), (2, 384, 22), (2, 384, 17), (2, 384, 12), (2, 384, 9), (2, 384, 7),
          (2, 208, 21)]
Z64_PAIR = [(1, 384)]
Z64P_NOT_ET = [(2, 52), (1, 176)]  # nrldpc_kernels.h:70 NRLDPC_Z64P_NOT_ET

# packed units that are compiled but that no call of the default process reaches (an interleaved entry takes every call they serve)
SHADOWED_PACKED = [(1, 3), (1, 5), (1, 6), (1, 36), (1, 44), (1, 80), (1, 96), (2, 52)]
SHADOWED_PACKED_NL = [(2, 20, 12)]

EXCLUDED = {
    "NRLDPC_FORCE_GENERIC": "A/B knob read once per process: every call on the run-time-Z kernel (nrldpc_decode.hip:353)",
    "NRLDPC_NO_ILV": "A/B knob read once per process (nrldpc_decode.hip:385)",
    "NRLDPC_NO_PACKED": "A/B knob read once per process (nrldpc_decode.hip:366,379)",
    "NRLDPC_NO_PACKED_ROW": "A/B knob read once per process; its list is empty anyway (nrldpc_decode.hip:401)",
    "NRLDPC_NO_PACKED_GENERAL": "A/B knob read once per process (nrldpc_decode.hip:418)",
    "NRLDPC_NO_RT": "A/B knob read once per process: pruned counts on the general kernels (nrldpc_decode.hip:409, nrldpc_decode_z64.h:1401)",
    "NRLDPC_SPLIT": "read only by a -DNRLDPC_Z64_AB library (nrldpc_decode_z64.h:1345)",
    "NRLDPC_NO_PRUNED_PIPELINE": "A/B knob read once per process (nrldpc_decode_z64.h:1391)",
    "NRLDPC_NO_REFILL / NRLDPC_REFILL_MASK": "A/B knobs read once per process (nrldpc_decode_z64p.h:395,398)",
    "NRLDPC_MULTI_*": "A/B knobs of nrldpc_decode_multi_dev read once per process (nrldpc_capi.hip:1051-1069,1152)",
    "-DNRLDPC_Z64_AB": "the A/B build with both forms of every pair: a library of its own",
    "NRLDPC_BUILD_ALLMODES": "the experiment build in which every interleaved entry serves every mode: a library of its own",
    "NRLDPC_Z64PR_LIST": "empty at this commit: no unit is compiled, launch_z64pr is instantiated nowhere",
    "sum-product": "nrldpc_decode_bp.hip has tests of its own (tests/test_sum_product_gpu.py)",
    "nrldpc_decode_cw_dev": "tests of its own (tests/test_cw_outputs_gpu.py)",
    "multi: batch*Z >= 512*384 on a block-geometry size": "the workload's size, not a test's: stays with "
                                                          "test_cfg4_mixed_batch_in_one_call_matches_the_oracle",
}


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def z64_blk(Z, ilv=False):
    """nrldpc_decode_z64.h:159 z64_blk for the block geometry (ilv: an interleaved unit's virtual size)"""
    if Z % 64 == 0:
        return 64
    if ilv:
        for b in range(63, 3, -1):
            if Z % b == 0:
                return b
    for b in range(60, 3, -4):
        if Z % b == 0:
            return b
    return 0


def z64_nwv(Z):
    return Z // z64_blk(Z)


def z64_ncwg(bg, Z):
    """nrldpc_decode_z64.h:177"""
    n = z64_nwv(Z)
    if bg == 1:
        return {8: 2, 6: 2, 5: 3, 4: 2, 3: 1}.get(n, 2)
    return {8: 1, 6: 2, 5: 1, 4: 3, 3: 4, 2: 2}.get(n, 4)


def z64_ncwg_et(bg, Z):
    """nrldpc_decode_z64.h:204"""
    return 1 if bg == 1 and z64_nwv(Z) == 4 else z64_ncwg(bg, Z)


def z64_ncwg_nl(bg, Z, nl):
    """nrldpc_decode_z64.h:189"""
    return 1 if (bg == 1 and z64_nwv(Z) == 6 and nl != NL_RT and nl <= 6) else z64_ncwg(bg, Z)


def z64p_rw(bg, Z):
    """nrldpc_decode_z64.h:131 for a packed unit"""
    if bg == 1 and Z in (88, 96, 176, 352):
        return 6
    best, fill = 1, -1
    for rw in (1, 2, 4):
        f = (64 * rw // Z) * Z * 1000 // (64 * rw)
        if f >= 800:
            return rw
        if f > fill:
            fill, best = f, rw
    return best


def rtz_schedule(bg, Z):
    """nrldpc_sched.h:113-131 build_schedule: codewords per workgroup and threads of the run-time-Z kernel"""
    kb = BG_DIMS[bg][2]
    ncp = (kb + 4) | 1
    slots, tmax = 4 * (4 if bg == 1 else 6), 512
    ncw, best, n = 1, -1.0, 1
    while n * Z <= tmax or n == 1:
        if not (n > 4 and n % 2 == 0):
            waves = (n * Z + 63) // 64
            lds = Z * n * ncp * 4 + 4 * (n + 1) + 16
            wgs = max(1, min(slots // waves, (160 * 1024) // lds))
            score = (n * Z) / (waves * 64.0) * min(slots, waves * wgs) / slots
            if waves % 4:
                score *= 0.85 if waves > 4 else 0.97
            if waves < 4:
                score *= 0.97
            if score >= best - 1e-9:
                best, ncw = score, n
            if n * Z > tmax:
                break
        n += 1
    return ncw, ((ncw * Z + 63) // 64) * 64


def split_default(bg, Z, nl):
    """nrldpc_decode_z64.h:1325 z64_split_default; nl = the template value (rows, a pruned-count unit's count)"""
    if nl != BG_DIMS[bg][0]:
        return (bg == 1 and Z == 384) or (bg == 2 and Z == 208)  # :1332
    if bg == 1:
        return Z in (60, 64, 104, 112, 120, 128, 176, 208, 224, 240, 256, 288, 384)  # :1334
    return Z in (52, 60, 64, 88, 96, 104, 112, 120, 128, 208, 224, 240, 256)  # :1336


def split_usable(bg, Z):
    """nrldpc_decode_z64s.h:50 Z64S::usable: THREADS <= 1024 (NG >= 2 holds for every layer count >= 4: rows 0..3 are two groups)"""
    return 2 * z64_nwv(Z) * 64 <= 1024


def has_split(bg, Z, nl):
    """nrldpc_decode_z64.h:1348 z64_has_split in the shipped build (z64_ab false)"""
    return split_usable(bg, Z) and split_default(bg, Z, nl)


def has_z64p(bg, Z, et):
    """nrldpc_decode.hip:365 has_z64p_kernel"""
    if et and (bg, Z) in Z64P_NOT_ET:
        return False
    return (bg, Z) in Z64P_PAIRS


def z64pg_serves(bg):
    """nrldpc_decode_z64p.h:429"""
    return bg == 2


Route = namedtuple("Route", "kind build unit kernel ncw threads ptr refills soft_ok admitted")
# ptr: the kernel branches on the alignment of llr / hard; refills: a parity-stop build with slots (DecArgs::work)


def _b(x):
    return "true" if x else "false"


def route(bg, Z, nl, et, soft, dtype="f16"):
    """The kernel one launch_decode call runs in the default process.  nl: resolved layer count (4..rows); et: 0 | 1 | 2 (CRC-aided
    stop); soft: soft output asked for.  Soft output with the CRC-aided stop is refused by the C ABI before any launch."""
    rows = BG_DIMS[bg][0]
    assert 4 <= nl <= rows and Z in ALL_Z and et in (0, 1, 2) and not (soft and et == 2)
    crc, stop, allrows = et == 2, et != 0, nl == rows
    nlt = rows if allrows else NL_RT
    if not soft and not crc:  # nrldpc_decode.hip:386-394
        want = 1 if not stop else 2 if allrows else 4
        for b, z, ncw, mode in Z64I:
            if b == bg and z == Z and (mode & want):
                ZC = z * ncw
                rw = ZC // z64_blk(ZC, ilv=True)
                return Route("ilv", ("ETP" if stop else "PLAIN", "rows" if allrows else "NL_RT"), "u_z64i_%d_%d" % (bg, Z),
                             "nrldpc_decode_z64p_kernel<%d, %d, %s, %d, %d>" % (bg, ZC, _b(stop), nlt, 1000 + ncw),
                             ncw, 2 * rw * 64, False, stop, False, want)
        for b, z, n in Z64P_NL:  # :396-399
            if b == bg and z == Z and n == nl:
                rw = z64p_rw(bg, Z)
                return Route("packed", ("ETP" if stop else "PLAIN", "NL%d" % nl), "u_z64p_%d_%d_nl%d" % (bg, Z, nl),
                             "nrldpc_decode_z64p_kernel<%d, %d, %s, %d, 0>" % (bg, Z, _b(stop), nl), 64 * rw // Z, 2 * rw * 64, False, stop,
                             False, None)
        # (:402-405 NRLDPC_Z64PR_LIST is empty)
        if (allrows or not (bg == 2 and stop)) and has_z64p(bg, Z, stop):  # :413
            rw = z64p_rw(bg, Z)
            return Route("packed", ("ETP" if stop else "PLAIN", "rows" if allrows else "NL_RT"), "u_z64p_%d_%d" % (bg, Z),
                         "nrldpc_decode_z64p_kernel<%d, %d, %s, %d, 0>" % (bg, Z, _b(stop), nlt), 64 * rw // Z, 2 * rw * 64, False, stop,
                         False, None)
    if bg == 2 and not crc and (bg, Z) not in Z64_PAIRS and (bg, Z) in Z64P_PAIRS and z64pg_serves(bg):  # :419-424
        rw = z64p_rw(bg, Z)
        return Route("packed_general", ("general",), "u_z64p_%d_%d" % (bg, Z), "nrldpc_decode_z64pg_kernel<%d, %d, 0, %d>" % (bg, Z, rows),
                     64 * rw // Z, rw * 64, False, False, True, None)
    if (bg, Z) in Z64_PAIRS:  # :426 -> launch_z64, nrldpc_decode_z64.h:1375
        unit = "u_z64_%d_%d" % (bg, Z)
        tpc = z64_nwv(Z) * 64

        def split(etp, n, c=False, u=unit):
            return Route("split", (("ETP+CRC" if c else "ETP") if etp else "PLAIN", "rows" if n == rows else "NL_RT" if n == NL_RT else "NL%d" % n),
                         u, "nrldpc_decode_z64s_kernel<%d, %d, %s, %d, %s>" % (bg, Z, _b(etp), n, _b(c)), 1, 2 * tpc, True, False, False, None)

        def rowf(ncwg, full, plain, etp, n, c=False, u=unit):
            kind = "row" if full else "general"
            build = ("general",) if not full else (("ETP+CRC" if c else "ETP") if etp else "PLAIN",
                                                   "rows" if n == rows else "NL_RT" if n == NL_RT else "NL%d" % n)
            return Route(kind, build, u, "nrldpc_decode_z64_kernel<%d, %d, %d, %s, %s, %s, %d, %s>"
                         % (bg, Z, ncwg, _b(full), _b(plain), _b(etp), n, _b(c)), ncwg, ncwg * tpc, True, False, not full, None)

        if crc and not soft:  # :1377-1386
            if has_split(bg, Z, rows):
                return split(True, nlt, True)
            return rowf(z64_ncwg_et(bg, Z), True, False, True, nlt, True)
        if has_split(bg, Z, rows) and allrows and not soft:  # :1387-1390
            return split(stop, rows)
        if not soft:  # :1392-1398 -> launch_z64_pruned, :1364
            for b, z, n in Z64_NL:
                if b == bg and z == Z and n == nl:
                    u = "u_z64_%d_%d_nl%d" % (bg, Z, nl)
                    if has_split(bg, Z, n):
                        return split(stop, n, u=u)
                    g = z64_ncwg_nl(bg, Z, n)
                    return rowf(g, True, not stop, stop, n, u=u)
        if not allrows and not soft:  # :1402-1410
            if has_split(bg, Z, rows):
                return split(stop, NL_RT)
            if stop:
                return rowf(z64_ncwg_et(bg, Z), True, False, True, NL_RT)
            return rowf(z64_ncwg(bg, Z), True, True, False, NL_RT)
        if not allrows or soft:  # :1412
            return rowf(z64_ncwg(bg, Z), False, False, False, rows)
        if stop:  # :1414
            return rowf(z64_ncwg_et(bg, Z), True, False, True, rows)
        return rowf(z64_ncwg(bg, Z), True, True, False, rows)  # :1415
    ncw, threads = rtz_schedule(bg, Z)  # :429-442
    return Route("rtz", ("CRC" if crc else "plain", dtype), "", "nrldpc_decode_kernel<%d, %d, %s>" % (bg, 1 if dtype == "f16" else 0, _b(crc)),
                 ncw, threads, False, False, True, None)


def instantiation(r):
    return (r.unit, r.kernel)


def grid(r, batch, refill_grid=0):
    g = -(-batch // r.ncw)
    if r.refills and refill_grid and g > refill_grid:  # nrldpc_decode_z64p.h:404-409 (the test hook; the resident cap is far above a test's)
        g = refill_grid
    return g


# ---- data-path classes --------------------------------------------------------------------------------------------------------
def llr_class(off):
    """nrldpc_decode_z64.h:981 / nrldpc_decode_z64s.h:213: wide when (llr & 15) == 0; else narrow, by how far off"""
    off &= 15
    return "wide" if off == 0 else "narrow%d" % (off & -off if (off & -off) < 16 else 16)


def hard_class(off, soft):
    """nrldpc_decode_z64.h:1265 (!app_row && (hard & 3) == 0) / nrldpc_decode_z64s.h:443"""
    return "dword" if (off & 3) == 0 and not soft else "byte"


def tail_class(ncw, batch):
    if batch < ncw:
        return "small"
    return "full" if batch % ncw == 0 else "partial"


Call = namedtuple("Call", "name bg Z nl et soft dtype batch iters esn0_off straggle llr_off hard_off want_iters refill_grid seed why")


def call_route(c):
    return route(c.bg, c.Z, c.nl or BG_DIMS[c.bg][0], c.et, c.soft, c.dtype)


def classes(c):
    """the data-path classes one call executes; only routes that have a branch carry its classes"""
    r = call_route(c)
    out = {(r.kind, "iters", "set" if c.want_iters else "null"), (r.kind, "tail", tail_class(r.ncw, c.batch))}
    if r.ptr:
        out.add((r.kind, "llr", llr_class(c.llr_off)))
        out.add((r.kind, "hard", hard_class(c.hard_off, c.soft)))
    if r.soft_ok:
        out.add((r.kind, "soft", "yes" if c.soft else "no"))
    if r.kind in ("ilv", "packed"):
        out.add((r.kind, "refill", "active" if r.refills and c.refill_grid and -(-c.batch // r.ncw) > c.refill_grid else "none"))
    return out


def universe_classes():
    u = set()
    for kind in ("ilv", "packed", "packed_general", "split", "row", "general", "rtz"):
        for v in ("set", "null"):
            u.add((kind, "iters", v))
        for v in ("full",) if kind == "split" else ("full", "partial", "small"):  # the split form holds one codeword per workgroup
            u.add((kind, "tail", v))
        if kind in ("split", "row", "general"):
            for v in ("wide", "narrow2", "narrow4", "narrow8"):
                u.add((kind, "llr", v))
            # (the general kernel runs in the default process only for soft output, and then stores bytes: nrldpc_decode_z64.h:1265)
            for v in ("byte",) if kind == "general" else ("dword", "byte"):
                u.add((kind, "hard", v))
        for soft in (True, False):
            if (kind, soft) in soft_shapes() and kind in ("packed_general", "general", "rtz"):
                u.add((kind, "soft", "yes" if soft else "no"))
        if kind in ("ilv", "packed"):
            for v in ("active", "none"):
                u.add((kind, "refill", v))
    return u


_SOFT = None


def soft_shapes():
    """{(kind, soft): [(Z, bg, nl, et), ...]}: every shape of the default process by route kind, with and without soft output"""
    global _SOFT
    if _SOFT is None:
        _SOFT = {}
        for bg in (1, 2):
            for Z in ALL_Z:
                for nl in pruned_counts(bg, Z):
                    for et in (0, 1):
                        for soft in (False, True):
                            _SOFT.setdefault((route(bg, Z, nl, et, soft).kind, soft), []).append((Z, bg, nl, et))
    return _SOFT


def pruned_counts(bg, Z):
    """layer counts that can change the route of (bg, Z): every count a list names for it, and one that no list names"""
    rows = BG_DIMS[bg][0]
    named = [n for b, z, n in Z64_NL + Z64P_NL if (b, z) == (bg, Z)]
    return [rows] + named + [19 if bg == 1 else 14]


def universe():
    """{instantiation: (Route, (bg, Z, nl, et, soft, dtype))}: every kernel instantiation launch_decode can launch in the default
    process, with the first call shape that reaches it"""
    u = {}
    for bg in (1, 2):
        for Z in ALL_Z:
            for nl in pruned_counts(bg, Z):
                for et in (0, 1, 2):
                    for soft in (False, True):
                        if soft and et == 2:
                            continue
                        for dt in ("f16", "f32"):
                            r = route(bg, Z, nl, et, soft, dt)
                            u.setdefault(instantiation(r), (r, (bg, Z, nl, et, soft, dt)))
    return u


# ---- the plan -----------------------------------------------------------------------------------------------------------------
# (test_decode_cases.py holds this table to test_decode_gpu._waterfall_esn0)
WATERFALL = {1: [(4, 8.0), (5, 6.2), (8, 4.6), (13, 3.0), (17, 2.0), (24, 1.0), (30, 0.2), (46, -0.8)],
             2: [(4, 7.0), (7, 4.5), (9, 2.6), (12, 1.3), (17, 0.0), (22, -0.7), (32, -1.8), (42, -2.5)]}  # = test_decode_gpu._waterfall_esn0
CRC16 = (0x11021, 16)
STOP_ITERS, FIXED_ITERS = 14, 2


def waterfall(bg, nl):
    pts = WATERFALL[bg]
    return float(np.interp(nl, [p[0] for p in pts], [p[1] for p in pts]))


# seeds changed where the oracle did not meet a condition of test_decode_cases.py with the default seed (crc32 of the name)
# (tests/decode_seeds.py, written by tools/find_decode_seeds.py: the first later seed that meets it)
from decode_seeds import SEEDS  # noqa: E402


def _call(name, bg, Z, nl, et, soft, dtype, batch, iters, esn0_off, straggle, llr_off, hard_off, want_iters, refill_grid, why):
    seed = SEEDS.get(name, zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return Call(name, bg, Z, nl, et, soft, dtype, batch, iters, esn0_off, straggle, llr_off, hard_off, want_iters, refill_grid, seed, why)


def _fixed(name, bg, Z, nl, soft, dt, batch, llr_off, hard_off, want_iters, why):
    return _call(name, bg, Z, nl, 0, soft, dt, batch, FIXED_ITERS, -2.5, False, llr_off, hard_off, want_iters, 0, why)


def _stop(name, bg, Z, nl, et, soft, dt, batch, llr_off, hard_off, want_iters, why, refill_grid=0):
    return _call(name, bg, Z, nl, et, soft, dt, batch, STOP_ITERS, 0.2, True, llr_off, hard_off, want_iters, refill_grid, why)


def _tag(bg, Z, nl, et, soft, dt):
    return "bg%d-z%d-nl%d-et%d%s-%s" % (bg, Z, nl, et, "-soft" if soft else "", dt)


def build_plan():
    plan, flip, turn = [], 0, 0
    eb = {"f16": 2, "f32": 4}
    uni = universe()
    for inst in sorted(uni):
        r, (bg, Z, nl, et, soft, dt0) = uni[inst]
        why = ("instantiation",) + inst
        serves_fixed = r.kind in ("packed_general", "general", "rtz") and r.build[0] != "CRC" or r.build[0] == "PLAIN"
        serves_stop = r.kind in ("packed_general", "general", "rtz") or r.build[0] != "PLAIN"
        t = "%s-%s" % (r.kind, _tag(bg, Z, nl, et, soft, dt0))
        template_dt = r.kind == "rtz"

        def dt():
            nonlocal flip
            if template_dt:
                return dt0
            flip += 1
            return ("f16", "f32")[flip & 1]
        if serves_fixed:
            d = dt()
            plan.append(_fixed(t + "-fix-a", bg, Z, nl, soft, d, r.ncw + 1, 0, 0, True, why))
            d = dt()
            plan.append(_fixed(t + "-fix-u", bg, Z, nl, soft, d, max(1, r.ncw - 1), eb[d], 1, True, why))
        if serves_stop:
            e = et if et else 1
            d = dt()
            plan.append(_stop(t + "-stop", bg, Z, nl, e, soft, d, 2 * r.ncw + 1, 0, 2, True, why))
            if r.refills:
                d = dt()
                plan.append(_stop(t + "-refill", bg, Z, nl, e, soft, d, 5 * r.ncw + 3, 0, 2, True, why, refill_grid=1))
            if r.ptr and not soft:
                # the parity-stop and CRC twins are kernels of their own: each also takes the dword store (everything aligned) and
                # the narrow LLR path, whose offset (one element / 4 bytes for fp16 / 8 bytes) and `hard` offset (0..3) go round
                # from instantiation to instantiation, so that narrow LLR with the dword store occurs in every fourth
                d = dt()
                plan.append(_stop(t + "-stop-a", bg, Z, nl, e, soft, d, 2 * r.ncw + 1, 0, 0, True, why))
                d = dt()
                turn += 1
                lo = ((eb[d], 8, 4) if d == "f16" else (4, 8))[turn % (3 if d == "f16" else 2)]
                plan.append(_stop(t + "-stop-u", bg, Z, nl, e, soft, d, 2 * r.ncw + 1, lo, turn % 4, True, why))
    # every route kind: the cross of its data-path classes at one small and one large lifting size of the kind
    by_kind = {}
    for inst in sorted(uni):
        r, shape = uni[inst]
        # (a fixed-iteration build of the kind: a batch of one codeword cannot hold an early leaver and a straggler, which every
        # planned parity-stop call must; the pointer branches and the tail handling are the same code in the PLAIN and ETP builds)
        if r.build[0] in ("PLAIN", "general", "plain"):
            by_kind.setdefault(r.kind, []).append((shape[1], shape[0], inst))
    for kind in sorted(by_kind):
        sizes = sorted(by_kind[kind])
        picks = [sizes[0][2], sizes[-1][2]]
        for inst in picks:
            r, (bg, Z, nl, et, soft, dt0) = uni[inst]
            why = ("classes", kind)
            t = "x-%s-%s" % (kind, _tag(bg, Z, nl, et, soft, dt0))
            batches = sorted({1, r.ncw, r.ncw + 1, 3 * r.ncw - 1})
            stop = r.build[0] in ("ETP", "ETP+CRC", "CRC")
            for bi, batch in enumerate(batches):
                for wi in (True, False):
                    if r.ptr:  # LLR offset 0 / one element / 4 bytes (fp16 only) / 8 bytes, both types
                        lo = [("f16", 0), ("f16", 2), ("f16", 4), ("f16", 8), ("f32", 0), ("f32", 4), ("f32", 8)]
                    else:      # no pointer branch in this kernel: the types alternate
                        lo = [(dt0 if kind == "rtz" else ("f16", "f32")[(bi + wi) & 1], 0)]
                    for d, lo_off in lo:
                        for ho in ((0, 1, 2, 3) if r.ptr else (0,)):
                            n = "%s-b%d-%s-l%d-h%d-%s" % (t, batch, d, lo_off, ho, "it" if wi else "noit")
                            if stop:
                                plan.append(_stop(n, bg, Z, nl, et or 1, soft, d, batch, lo_off, ho, wi, why))
                            else:
                                plan.append(_fixed(n, bg, Z, nl, soft, d, batch, lo_off, ho, wi, why))
    # soft-output routes: every row and a pruned count, fixed and stop, soft output between guards
    for kind in ("rtz", "general", "packed_general"):
        sizes = sorted(set((Z, bg) for Z, bg, nl, et in soft_shapes()[(kind, True)]))
        for Z, bg in (sizes[0], sizes[-1]):
            rows = BG_DIMS[bg][0]
            for nl in (rows, 19 if bg == 1 else 14):
                for soft in (True, False):  # ... and the same shapes without it, where they stay on this kind
                    r = route(bg, Z, nl, 0, soft, "f32")
                    r1 = route(bg, Z, nl, 1, soft, "f16")
                    t = "soft-%s-%s" % (kind, _tag(bg, Z, nl, 0, soft, "f32"))
                    if r.kind == kind:
                        plan.append(_fixed(t + "-fix", bg, Z, nl, soft, "f32", r.ncw + 1, 0, 0, True, ("soft", kind)))
                    if r1.kind == kind:
                        plan.append(_stop(t + "-stop", bg, Z, nl, 1, soft, "f16", 2 * r1.ncw + 1, 0, 2, True, ("soft", kind)))
        if (kind, False) in soft_shapes():  # the kind without soft output, wherever it is first met
            Z, bg, nl, et = soft_shapes()[(kind, False)][0]
            r = route(bg, Z, nl, et, False, "f32")
            t = "nosoft-%s-%s" % (kind, _tag(bg, Z, nl, et, False, "f32"))
            if et:
                plan.append(_stop(t, bg, Z, nl, 1, False, "f32", 2 * r.ncw + 1, 0, 2, True, ("soft", kind)))
            else:
                plan.append(_fixed(t, bg, Z, nl, False, "f32", r.ncw + 1, 0, 0, True, ("soft", kind)))
    names = [c.name for c in plan]
    assert len(set(names)) == len(names)
    return plan


_PLAN = None


def plan():
    global _PLAN
    if _PLAN is None:
        _PLAN = build_plan()
    return _PLAN


def reason(c):
    """what a planned call is there for"""
    return c.why


# ---- inputs and the oracle's answer -------------------------------------------------------------------------------------------
def crc_of(c):
    """the CRC a CRC-stop call protects its whole information word with: CRC16, K' = K (no fillers)"""
    return (CRC16[0], CRC16[1], BG_DIMS[c.bg][2] * c.Z) if c.et == 2 else None


def inputs(c, orc, awgn_llr):
    """(info, llr in the call's dtype): QPSK/AWGN at the call's operating point; a stop call scales a twentieth of its codewords,
    at least one, by 0.05 so that they run to the cap"""
    rows, cols, kb = BG_DIMS[c.bg]
    rng = np.random.default_rng(c.seed)
    K = kb * c.Z
    info = rng.integers(0, 2, (c.batch, K), dtype=np.uint8)
    if c.et == 2:
        poly, L = CRC16
        for b in range(c.batch):
            rem = orc.crc(poly, L, info[b, : K - L])
            info[b, K - L:] = (rem >> np.arange(L - 1, -1, -1)) & 1
    cw = orc.encode(c.bg, c.Z, info)
    dt = np.float16 if c.dtype == "f16" else np.float32
    llr = awgn_llr(rng, cw, waterfall(c.bg, c.nl or rows) + c.esn0_off, dt, c.Z)
    if c.straggle:
        idx = rng.choice(c.batch, max(1, c.batch // 20), replace=False)
        llr[idx] = (llr[idx].astype(np.float32) * np.float32(0.05)).astype(dt)
    return info, llr


def rule(c):
    """nrldpc_sched.h:70 default_rule as oracle keywords (beta in grid units at the default llr_scale 8); the GPU test holds the
    rule its Codec resolved against this"""
    rows = BG_DIMS[c.bg][0]
    frac = (c.nl or rows) / rows
    beta = (0.375 if frac > 0.2 else 0.25) if c.bg == 1 else (0.3125 if frac > 0.25 else 0.25)
    return {"alpha": 0.875, "beta": beta * 8}


def conditions(c, orc, awgn_llr):
    """the conditions a planned call's input must meet, asked of the oracle: returns a list of what does not hold (empty = good)"""
    info, llr = inputs(c, orc, awgn_llr)
    hard, it, _ = reference(c, orc, llr, rule(c))
    bad = []
    if c.et:
        if not it.min() < c.iters:
            bad.append("no codeword leaves before the cap")
        if not it.max() == c.iters:
            bad.append("no codeword runs to the cap")
    else:
        if not hard.any(axis=1).all():
            bad.append("a codeword's decisions are the all-zero word")
        if not (hard != info).any(axis=1).all():
            bad.append("a codeword has converged to the transmitted word")
    return bad


def reference(c, orc, llr, rule):
    """(hard, iters, app or None) of the oracle for a planned call; rule = rule_kw(codec) or the default rule's keywords"""
    if c.et == 2:
        h, it = orc.decode_nmsq_crc(c.bg, c.Z, llr.astype(np.float64), c.iters, crc_of(c), n_layers=c.nl, **rule)
        return h, it, None
    out = orc.decode_nmsq(c.bg, c.Z, llr.astype(np.float64), c.iters, n_layers=c.nl, early_term=bool(c.et), want_app=c.soft, **rule)
    return out[0], out[1], (out[2] if c.soft else None)


# ---- nrldpc_decode_multi_dev --------------------------------------------------------------------------------------------------
def multi_groups(configs, min_rows=512 * 384):
    """configs: (bg, Z, et, dtype, batch, sum_product) per configuration.  Returns (shared, own, out_of_scope): shared maps
    (bg, dtype, thread class) to (indices, threads of the launch, grid); own lists the indices routed to launches of their own
    (nrldpc_capi.hip:1096-1113); configurations with batch 0 are in none."""
    edges = (256, 512, 768)
    shared, own, bp = {}, [], []
    for i, (bg, Z, et, dt, batch, sp) in enumerate(configs):
        if batch == 0:
            continue
        if sp:
            bp.append(i)
            continue
        if et == 2 or (batch * Z >= min_rows and (bg, Z) in Z64_PAIRS):
            own.append(i)
            continue
        ncw, threads = rtz_schedule(bg, Z)
        cls = next(e for e in edges if threads <= e)
        idx, th, g = shared.get((bg, dt, cls), ([], 0, 0))
        shared[(bg, dt, cls)] = (idx + [i], max(th, threads), g + -(-batch // ncw))
    return shared, own, bp


# ---- the device-pointer calls of the older tests (shapes copied as data) ----------------------------------------------------------
def _old(name, bg, Z, nl, et, dt, batch, llr_off=0, hard_off=0, soft=False, test=""):
    rows = BG_DIMS[bg][0]
    return _call("old-" + name, bg, Z, 0 if nl == rows else nl, et, soft, dt, batch, 10, 0.0, False, llr_off, hard_off, True, 0, ("older", test))


def _cfg4_buckets():
    """the buckets of test_full_size_gpu.py::test_cfg4_mixed_batch_in_one_call_matches_the_oracle, generated as the test does"""
    rng = np.random.default_rng(44)
    draws = [(int(rng.integers(1, 3)), int(rng.choice(ALL_Z))) for _ in range(8192)]
    buckets = {}
    for key in draws:
        buckets[key] = buckets.get(key, 0) + 1
    buckets[(1, 7)] = 1
    buckets[(1, 384)] = 600
    buckets[(2, 256)] = 800
    out = []
    for k, ((bg, Z), n) in enumerate(sorted(buckets.items())):
        rows = BG_DIMS[bg][0]
        out.append((bg, Z, rows if k % 3 else max(4, rows - (k % 11)), 1 if k % 4 else 0, "f16" if k % 3 else "f32", n))
    return out


def older_calls():
    """every call of the suite, before this census, that hands nrldpc_decode_dev (or the pool's device entry, which launches through
    the same decode_launch) buffers the test allocated -- all of them aligned except test_unaligned_device_pointers', all with
    iteration counts, none with guards or a poison fill (host_cases.dev_decode prefills 7 / -3 without guards).  Sum-product handles
    are out of scope."""
    out = []
    for bg, Z, dt in ((1, 384, "f16"), (2, 256, "f32"), (1, 320, "f16"), (1, 240, "f16"), (2, 104, "f32")):  # test_decode_gpu.py
        for et in (1, 0):
            out.append(_old("unaligned-%d-%d-%d" % (bg, Z, et), bg, Z, BG_DIMS[bg][0], et, dt, 9, 2 if dt == "f16" else 4, 1,
                            test="test_unaligned_device_pointers"))
    out.append(_old("dev-entry", 1, 384, 46, 1, "f16", 64, test="test_device_pointer_entry_and_timing"))
    for bg in (1, 2):  # test_layers_gpu.py::test_auto_equals_explicit_on_the_layer_count_grid (AUTO resolves to the same count)
        rows = BG_DIMS[bg][0]
        for Z in (8, 20, 64, 96, 144, 208, 352, 384):
            for nl in (4, 10, 13, 24, rows - 1, rows):
                out.append(_old("layers-%d-%d-%d" % (bg, Z, nl), bg, Z, nl, 1, "f16" if Z % 3 else "f32", 3 + (300 // Z if Z < 64 else 0),
                                test="test_auto_equals_explicit_on_the_layer_count_grid"))
    for nl, dt in ((5, "f16"), (19, "f16"), (5, "f32"), (19, "f32")):
        out.append(_old("layers-pipe-%d-%s" % (nl, dt), 1, 384, nl, 1, dt, 700, test="test_auto_on_the_pipelined_host_path"))
    for n in (300, 350, 250):
        out.append(_old("layers-pool-%d" % n, 2, 384, 9, 1, "f16", n, test="test_auto_in_the_pool_and_in_the_mixed_batch_call"))
    for et in (0, 1):  # test_full_size_gpu.py
        out.append(_old("cfg1-%d" % et, 1, 384, 46, et, "f16", 4096, test="test_cfg1_full_batch_every_codeword"))
    out.append(_old("host-dev-agree", 2, 384, 22, 1, "f16", 4096, test="test_host_and_device_entry_points_agree"))
    for dt, B, bg, Z in (("f32", 1237, 1, 384), ("f32", 1001, 1, 384), ("f16", 2049, 1, 384), ("f32", 9001, 2, 20), ("f32", 3001, 1, 36)):
        out.append(_old("pipelined-%d" % B, bg, Z, BG_DIMS[bg][0], 1, dt, B, test="test_pipelined_host_path_equals_one_device_launch"))
    for bg, Z, nl, et, dt, n in _cfg4_buckets():
        out.append(_old("cfg4-%d-%d" % (bg, Z), bg, Z, nl, et, dt, n, test="test_cfg4_mixed_batch_in_one_call_matches_the_oracle"))
    for n in (500, 600, 100):
        out.append(_old("pool-dev-%d" % n, 2, 384, 42, 1, "f16", n, test="test_pool_decode_dev_shards_device_resident_batches"))
    out.append(_old("half-soft-chain", 2, 208, 42, 1, "f16", 16, test="test_chain_with_f16_llrs_and_f16_buffer"))
    out.append(_old("sum-product-ms", 2, 52, 20, 1, "f32", 96, test="test_api_entries_take_the_sum_product_handle (its min-sum handle)"))
    import host_cases as H  # tests/test_host_paths_gpu.py: one device launch beside every planned host call (host_cases.run_call)
    for c in H.HOST_PLAN:
        if c.alg == "min-sum":
            out.append(_old("host-" + c.name, c.bg, c.Z, H.plan(c)["nl"], 1, "f32" if c.dtype == "f64" else c.dtype, c.batch, soft=c.app,
                            test="test_host_paths_gpu.py"))
    return out


def older_multi():
    """the nrldpc_decode_multi_dev calls of the suite before this census, as multi_groups() configurations per call.  The calls of
    test_mix_skip_gpu.py::settled_step are not listed shape by shape: none of its nine configurations has the CRC-aided stop or
    batch * Z >= 196608, so whatever their lifting sizes they share launches of the multi kernel."""
    cfg4 = [(bg, Z, et, dt, n, False) for bg, Z, nl, et, dt, n in _cfg4_buckets()]
    cfg4_nl = [nl for bg, Z, nl, et, dt, n in _cfg4_buckets()]
    return {
        "cfg4": (cfg4, cfg4_nl, True),   # True: the call is also made without d_iters
        "crc-mixed": ([(2, 36, 2, "f16", 9, False), (1, 24, 1, "f16", 9, False), (2, 384, 2, "f16", 9, False)], [42, 46, 42], False),
        "layers-auto": ([(1, 64, 1, "f16", 40, False), (2, 20, 1, "f16", 40, False), (1, 384, 1, "f16", 40, False)], [13, 12, 46], False),
        "sum-product": ([(2, 52, 1, "f32", 96, True), (2, 52, 1, "f32", 96, False), (1, 20, 1, "f32", 40, True)], [20, 20, 46], False),
    }


def older_reached():
    """(instantiations of launch_decode, data-path classes, (bg, dtype) of the shared multi kernel, thread classes of the shared
    launches) the older tests reached on buffers of their own"""
    calls = older_calls()
    inst = {instantiation(call_route(c)) for c in calls}
    cls = set().union(*(classes(c) for c in calls))
    multi, tcls = set(), set()
    for cfg, nls, no_iters in older_multi().values():
        shared, own, bp = multi_groups(cfg)
        for i in own:  # a launch of its own goes through launch_decode: aligned
            bg, Z, et, dt, n, sp = cfg[i]
            c = _old("multi-own", bg, Z, nls[i], et, dt, n)
            inst.add(instantiation(call_route(c)))
            cls |= classes(c) | (classes(c._replace(want_iters=False)) if no_iters else set())
        for (bg, dt, t) in shared:
            multi.add((bg, dt))
            tcls.add(t)
    return inst, cls, multi, tcls

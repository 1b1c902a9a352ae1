"""The cases the rate-recovery path tests share (tests/test_rate_recover_paths_gpu.py, tests/rr_knob_child.py) and a census of what
they reach (tests/test_rr_cases.py, CPU): the receive-side twin of tests/tx_cases.py.

Rate recovery exists in three units -- "f32": csrc/nrldpc_ratematch.hip (nrldpc_rate_recover_dev, a lane owns a PAIR of positions),
"ex": csrc/nrldpc_ratematch_ex.hip (nrldpc_rate_recover_ex_dev, a QUAD), "mix": csrc/nrldpc_mix.hip
(nrldpc_mix_rate_recover[_harq]_dev, quads from a table) -- and each picks its kernel, and inside it its code path, from sizes,
from where a group of positions lies relative to the boundaries of a code block (the 2Z punctured columns, the filler gap, the end
of the circular buffer, the end of E, the wrap at k_0, a change of interleaver row) and from the ALIGNMENT of the addresses it is
given.  The conditions the units share live once, in csrc/nrldpc_rm_core.h: the geometry (RmGeom), the launch rule (rm_launch_rule
-- tests/test_rm_rule_host.py holds launch_form and mix_form below to it on the CPU), the general gather of ex and mix
(gather_general; the f32 unit's general kernel keeps a copy of the walk) and the tail finish4 with its access widths; the
branch-free gather, the scatter's input part, the fill loops and the f32 unit's tail are in the units.  The census below restates
those conditions from the sources -- no part of it runs a kernel -- so that the list of sets can be held to "every class is
reached" on the CPU.  Derived parameters come from testbench_ref.derive through tx_cases.derive.  The last section ("the device
side") is what the GPU test and the switch child share to run a set on the device and compare it with the model; the census does
not use it, and it imports torch only when called.

A class is (unit, form, Q_m, feature).  Forms: "general" (the repetition walk), "fast" (the no-repetition gather), "scatter" (the
input-driven form, units f32 and ex).  Features:
  gather forms     all:<kind>, <kind>><kind> between neighbours of a group, wrapk0, rowchg; general also depth1, depth2, depth3+,
                   carry, nocarry (the walk's row-overflow step taken / not taken);
  scatter          in:J<J>:run|tail|endP|gap, in:J<J>:tail:endP, in:J<J>:tail:gap (input part, the kernel's precedence);
                   fill:tile:skipped|plain|mixed, fill:all:<kind>, fill:<kind>><kind>, fill:E0 (fill part);
  access width     acc:<array>:<element type>:<which form the access takes>, followed per code block row (odd G, N_cb).
"""
import itertools

import numpy as np

import tx_cases as T
from tx_cases import derive  # noqa: F401  (the tests take it from here)

QMS = (1, 2, 4, 6, 8)
UNITS = ("f32", "ex", "mix")
WIDTH = {"f32": 2, "ex": 4, "mix": 4}      # positions a lane owns
F32, F16 = "f32", "f16"
# (g_tilde, buffer, output) element offsets from a 256-byte boundary
OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))
COMBOS = tuple(itertools.product((F32, F16), repeat=3))  # (input, buffer, output)
N_TB = 2                                     # transport blocks of a single-configuration call of the new tests
MODES = ("default", "general", "scatter1", "scatter0")  # no switch, NRLDPC_RR_GENERAL=1, NRLDPC_RR_SCATTER=1, NRLDPC_RR_SCATTER=0
MODE_ENV = {"general": {"NRLDPC_RR_GENERAL": "1"}, "scatter1": {"NRLDPC_RR_SCATTER": "1"}, "scatter0": {"NRLDPC_RR_SCATTER": "0"}}


# ---- the launch rules --------------------------------------------------------------------------------------------------------------
def launch_form(ref, buffer, mode="default"):
    """launch_rate_recover / launch_rate_recover_ex: the general kernel when a code block has more bits than the buffer has
    non-filler positions (or NRLDPC_RR_GENERAL is set); else the scatter with a buffer at Q_m <= 2 and N >= 4096 (or wherever
    NRLDPC_RR_SCATTER says); else the plain gather."""
    P = T.rm_geometry(ref)[2]
    if mode == "general" or any(e > P for e in ref["E_r"]):
        return "general"
    if mode == "scatter1":
        return "scatter"
    if mode == "scatter0":
        return "fast"
    return "scatter" if buffer and ref["Q_m"] <= 2 and ref["N"] >= 4096 else "fast"


def mix_form(ref):
    """(form, echo) of a configuration as nrldpc_mix_create sets them: the rule above without its switches; echo where the single
    call would run its input-driven form."""
    P = T.rm_geometry(ref)[2]
    rep = any(e > P for e in ref["E_r"])
    return ("general" if rep else "fast"), (not rep and ref["Q_m"] <= 2 and ref["N"] >= 4096)


def scatter_J(unit, Qm):
    """interleaver columns per lane of the input part: RrJ (f32 unit), RRX_J (ex)"""
    return 4 if unit == "ex" else {1: 4, 2: 2, 4: 1, 6: 2, 8: 1}[Qm]


# ---- one code block ------------------------------------------------------------------------------------------------------------------
PUNCT, FILL, BEYOND, LIVE, DEAD, KEPT = range(6)
KIND = ("punct", "fill", "beyond", "live", "dead", "kept")
FKIND = {PUNCT: "punct", FILL: "fill", BEYOND: "beyond", LIVE: "covered"}  # fill part: DEAD -> echo / zero by the buffer


class Block:
    """Position arrays over the 2Z + N positions of code block r: kind, q (index among the buffer's non-filler positions from
    k_0), the interleaver row i, as every kernel computes them."""

    def __init__(self, ref, r):
        Z, N, K, Qm = ref["Z_c"], ref["N"], ref["K"], ref["Q_m"]
        self.N_cb = N_cb = ref["N_cb"]
        self.lo_f, self.F, self.P, self.nfk0 = lo_f, F, P, nfk0 = T.rm_geometry(ref)
        hi_f = K - 2 * Z
        self.Z, self.Qm, self.ncwz, self.E = Z, Qm, 2 * Z + N, ref["E_r"][r]
        E = self.E
        p = np.arange(self.ncwz) - 2 * Z
        fill = (p >= lo_f) & (p < hi_f)
        self.inb = inb = (p >= 0) & (p < N_cb) & ~fill
        q = p - np.clip(p - lo_f, 0, F) - nfk0
        self.q = q = np.where(q < 0, q + P, q)
        self.live = live = inb & (q < E)
        self.rows = rows = E // Qm if E > 0 else 1
        self.i = np.minimum(q // rows, Qm - 1)
        kind = np.full(self.ncwz, DEAD)
        kind[p < 0] = PUNCT
        kind[fill] = FILL
        kind[(p >= N_cb) & ~fill] = BEYOND
        kind[live] = LIVE
        self.kind = kind
        self._memo = {}

    def cached(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]


def block(ref, r):
    """Block(ref, r), kept with the derived set"""
    memo = ref.setdefault("_blocks", {})
    if r not in memo:
        memo[r] = Block(ref, r)
    return memo[r]


def _names(kind, W, names, prefix=""):
    """all:<kind> of the groups of W whose positions agree, a>b between neighbours that do not"""
    k = kind.reshape(-1, W)
    out = set()
    same = (k == k[:, :1]).all(axis=1)
    out |= {prefix + "all:" + names[v] for v in np.unique(k[same, 0]).tolist()}
    a, b = k[:, :-1], k[:, 1:]
    d = a != b
    out |= {prefix + names[x] + ">" + names[y] for x, y in set(zip(a[d].tolist(), b[d].tolist()))}
    return out


def gather_features(b, W, general, kept):
    kind = np.where(b.kind == DEAD, KEPT, b.kind) if kept else b.kind
    out = _names(kind, W, KIND)
    q, inb, live, i = (x.reshape(-1, W) for x in (b.q, b.inb, b.live, b.i))
    for s in range(W):
        for t in range(s + 1, W):
            if (inb[:, s] & inb[:, t] & (q[:, t] < q[:, s])).any():
                out.add("wrapk0")
    if (live[:, :-1] & live[:, 1:] & (i[:, :-1] != i[:, 1:])).any():
        out.add("rowchg")
    if general and b.live.any():
        # the walk: k = q + P, q + 2P, ... < E; jj += Pr, ii += Pq, and the row-overflow step when jj >= rows
        ql = b.q[b.live]
        depth = -(-(b.E - ql) // b.P)
        out |= {"depth1" for _ in [0] if (depth == 1).any()} | {"depth2" for _ in [0] if (depth == 2).any()}
        if (depth >= 3).any():
            out.add("depth3+")
        Pr = b.P - (b.P // b.rows) * b.rows
        jj = ql - b.i[b.live] * b.rows
        for step in range(1, int(depth.max())):
            act = depth > step
            jj = jj + Pr
            carry = act & (jj >= b.rows)
            jj = np.where(jj >= b.rows, jj - b.rows, jj)
            if carry.any():
                out.add("carry")
            if (act & ~carry).any():
                out.add("nocarry")
    return out


def scatter_input(b, J):
    """(feature, j0 array) per run class of the input part: columns j0 .. j0 + J - 1 of every interleaver row i"""
    out = {}
    if b.E == 0:
        return out
    j0 = np.arange(0, b.rows, J)
    nj = np.minimum(b.rows - j0, J)
    for i in range(b.Qm):
        n = i * b.rows + j0 + b.nfk0
        n = np.where(n >= b.P, n - b.P, n)
        tail = nj < J
        endP = ~tail & (n + J > b.P)
        gap = ~tail & ~endP & ~((n >= b.lo_f) | (n + J <= b.lo_f))
        run = ~tail & ~endP & ~gap
        for name, m in (("run", run), ("tail", tail), ("endP", endP), ("gap", gap), ("tail:endP", tail & (n + nj > b.P)),
                        ("tail:gap", tail & (n < b.lo_f) & (n + nj > b.lo_f))):
            if m.any():
                out.setdefault("in:J%d:%s" % (J, name), []).append((i, j0[m], n[m]))
    return out


FILL_TILE = 512  # RR_FILL_TILE, RRX_FILL_TILE


def scatter_fill(b, W, buffer):
    """features of the fill part and the mask of positions whose tile is not skipped"""
    out = set()
    hi_f = b.lo_f + (b.kind == FILL).sum()  # (= K - 2Z: every filler position lies inside the 2Z + N positions)
    ran = np.zeros(b.ncwz, bool)
    for x0 in range(0, b.ncwz, FILL_TILE):
        x1 = min(x0 + FILL_TILE, b.ncwz) - 1
        p0, p1 = x0 - 2 * b.Z, x1 - 2 * b.Z
        plain = p0 >= 0 and p1 < b.N_cb and not (p1 >= b.lo_f and p0 < hi_f)
        if plain and b.q[x0] < b.E and b.q[x1] < b.E and b.q[x1] - b.q[x0] == p1 - p0:
            out.add("fill:tile:skipped")
            continue
        out.add("fill:tile:plain" if plain else "fill:tile:mixed")
        ran[x0:x1 + 1] = True
    names = dict(FKIND)
    names[DEAD] = "echo" if buffer else "zero"
    groups = ran.reshape(-1, W)[:, 0]
    if groups.any():
        out |= _names(b.kind.reshape(-1, W)[groups].reshape(-1), W, names, "fill:")
    if b.E == 0:
        out.add("fill:E0")
    return out, ran


# ---- access width -------------------------------------------------------------------------------------------------------------------
def _odd(t, x):
    """an f16 address `x` elements above a 4-byte boundary fails quad_ok; f32 never does"""
    return t == F16 and x % 2 == 1


def access_features(ref, unit, form, types, offs, buffer, n_tb, fresh=(), echo=False):
    """_access_features, memoised on the derived set"""
    memo = ref.setdefault("_access", {})
    key = (unit, form, types, offs, buffer, n_tb, tuple(sorted(fresh)), bool(echo))
    if key not in memo:
        memo[key] = _access_features(ref, unit, form, types, offs, buffer, n_tb, fresh, echo)
    return memo[key]


def _access_features(ref, unit, form, types, offs, buffer, n_tb, fresh=(), echo=False):
    """acc:* features of one call: types = (input, buffer, output) element types, offs = element offsets of the three base
    pointers, fresh = the transport blocks that start a new HARQ process (mix, HARQ call)."""
    idt, hdt, odt = types
    go, ho, oo = offs
    C_, G, Qm = ref["C"], ref["G"], ref["Q_m"]
    roff = T.rm_offsets(ref)
    out = set()
    for r in range(C_):
        b = block(ref, r)
        for tb in range(n_tb):
            blk = tb * C_ + r
            o_el, h_el, g_el = oo + blk * b.ncwz, ho + blk * b.N_cb, go + tb * G + roff[r]
            if unit == "f32" and form != "scatter":
                out.add("acc:out:%s:%s" % (odt, "wide" if (oo * (4 if odt == F32 else 2)) % 8 == 0 else "elem"))
            elif form != "scatter":  # ex, mix: finish4
                out.add("acc:out:%s:%s" % (odt, "elem" if _odd(odt, o_el) else "wide"))  # pos0 is a multiple of 4
                if buffer:
                    inb = b.inb.reshape(-1, 4)
                    full, some = inb.all(axis=1), inb.any(axis=1)
                    kept = (~b.live & b.inb).reshape(-1, 4).any(axis=1) if (echo and form == "fast") else np.zeros(len(full), bool)
                    if unit == "mix" and tb in fresh:
                        if full.any():
                            out.add("acc:hb:%s:fresh-quad-%s" % (hdt, "elem" if _odd(hdt, h_el) else "wide"))
                        if (some & ~full).any():
                            out.add("acc:hb:%s:fresh-single" % hdt)
                    else:
                        if (full & ~kept).any():  # p0 = pos0 - 2Z is even
                            out.add("acc:hb:%s:quad-%s" % (hdt, "elem" if _odd(hdt, h_el) else "wide"))
                        if (some & ~full & ~kept).any():
                            out.add("acc:hb:%s:single" % hdt)
                        if kept.any():
                            out.add("acc:hb:%s:kept-single" % hdt)
            else:
                J = scatter_J(unit, Qm)
                for name, hits in b.cached(("in", J), lambda: scatter_input(b, J)).items():
                    kind = name.split(":", 2)[2]
                    if ":" in kind:
                        continue
                    for i, j0, n in hits:
                        p = np.where(n < b.lo_f, n, n + b.F)
                        if unit == "f32":
                            if i == 0:
                                out.add("acc:g:%s:%s" % (idt, "elem" if kind == "tail" else "wide"))
                            if kind == "run":
                                al = (o_el + 2 * b.Z + p) % J == 0
                                out |= {"acc:out:%s:run-%s" % (odt, "elem" if J == 1 else w) for w, m in (("wide", al), ("elem", ~al)) if m.any()}
                            else:
                                out.add("acc:out:%s:run-elem" % odt)
                        else:
                            if i == 0:
                                if kind == "tail":
                                    out.add("acc:g:%s:elem-tail" % idt)
                                else:
                                    odd = (g_el + j0 * Qm) % 2 == 1 if idt == F16 else np.zeros(len(j0), bool)
                                    out |= {"acc:g:%s:%s" % (idt, w) for w, m in (("wide", ~odd), ("elem-odd", odd)) if m.any()}
                            if kind == "run":
                                odd = (o_el + 2 * b.Z + p) % 2 == 1 if odt == F16 else np.zeros(len(p), bool)
                                out |= {"acc:out:%s:run-%s" % (odt, w) for w, m in (("wide", ~odd), ("elem", odd)) if m.any()}
                                if buffer:
                                    odd = (h_el + p) % 2 == 1 if hdt == F16 else np.zeros(len(p), bool)
                                    out |= {"acc:hb:%s:run-%s" % (hdt, w) for w, m in (("wide", ~odd), ("elem", odd)) if m.any()}
                            else:
                                out.add("acc:out:%s:run-single" % odt)
                                if buffer:
                                    out.add("acc:hb:%s:run-single" % hdt)
                W = WIDTH[unit]
                _, ran = b.cached(("fill", W, buffer), lambda: scatter_fill(b, W, buffer))
                write = (ran & ~b.live).reshape(-1, W)
                full, some = write.all(axis=1), write.any(axis=1)
                if unit == "f32":
                    vec = (oo * (4 if odt == F32 else 2)) % 8 == 0
                    if full.any():
                        out.add("acc:out:%s:fill-%s" % (odt, "wide" if vec else "elem"))
                    if (some & ~full).any():
                        out.add("acc:out:%s:fill-elem" % odt)
                else:
                    if full.any():
                        out.add("acc:out:%s:fill-%s" % (odt, "elem" if _odd(odt, o_el) else "wide"))
                    if (some & ~full).any():
                        out.add("acc:out:%s:fill-single" % odt)
                    if buffer:
                        echo_m = (ran & b.inb & ~b.live).reshape(-1, W)
                        efull, esome = echo_m.all(axis=1), echo_m.any(axis=1)
                        if efull.any():
                            out.add("acc:hb:%s:echo-%s" % (hdt, "elem" if _odd(hdt, h_el) else "wide"))
                        if (esome & ~efull).any():
                            out.add("acc:hb:%s:echo-single" % hdt)
    return out


# ---- what one set reaches under a plan of calls ------------------------------------------------------------------------------------
# a call: (unit, (input, buffer, output) types, offsets, with a buffer, mode); the mix adds which transport blocks are new
def plan_single(n_tb=N_TB):
    """The calls of tests/test_rate_recover_paths_gpu.py and tests/rr_knob_child.py on one set."""
    calls = []
    for odt in (F32, F16):
        for offs in OFFSETS:
            calls += [("f32", (F32, F32, odt), offs, buf, "default") for buf in (False, True)]
    for combo in COMBOS:
        for offs in (OFFSETS if combo in ((F16, F16, F16), (F32, F16, F16)) else OFFSETS[:1]):
            calls += [("ex", combo, offs, buf, "default") for buf in (False, True)]
    for mode in MODES[1:]:
        for buf in (False, True):
            calls += [("f32", (F32, F32, F32), OFFSETS[0], buf, mode), ("ex", (F16, F16, F16), OFFSETS[0], buf, mode)]
    return calls, n_tb


MIX_CALLS = [((F16, F16, F16), offs) for offs in OFFSETS] + [((F32, F32, F32), OFFSETS[0]), ((F32, F32, F32), OFFSETS[4])]


def mix_n_tb(k):
    """transport blocks of set k inside the mix of the new tests: 0 .. 3, cycling (an empty configuration every fourth)"""
    return (3, 1, 2, 0)[k % 4]


def mix_new(k, n):
    """the `is_new` flags of set k's transport blocks in the HARQ call: both values inside a configuration wherever n >= 2"""
    return [(tb + k) % 2 for tb in range(n)]


def _features(ref, key):
    """gather / scatter features of a set, per (unit width, form, buffer, kept): cached, they do not depend on types or offsets"""
    memo = ref.setdefault("_features", {})
    if key not in memo:
        W, form, buffer, kept, unit = key
        out = set()
        for r in range(ref["C"]):
            b = block(ref, r)
            if form == "scatter":
                J = scatter_J(unit, ref["Q_m"])
                out |= set(b.cached(("in", J), lambda: scatter_input(b, J)))
                out |= b.cached(("fill", W, buffer), lambda: scatter_fill(b, W, buffer))[0]
            else:
                out |= gather_features(b, W, form == "general", kept)
        memo[key] = out
    return memo[key]


def census(ref, calls, n_tb, mix=None):
    """{(unit, form, Q_m, feature)} one set reaches under the calls `calls` (plan_single) and, with mix = (calls, n_tb, new), as a
    configuration of the mix calls (plain with and without a buffer; HARQ with the flags `new`)."""
    Qm = ref["Q_m"]
    out = set()
    for unit, types, offs, buf, mode in calls:
        form = launch_form(ref, buf, mode)
        feats = _features(ref, (WIDTH[unit], form, buf, False, unit)) | access_features(ref, unit, form, types, offs, buf, n_tb)
        out |= {(unit, form, Qm, f) for f in feats}
    if mix is not None and mix[1] > 0:
        mcalls, n, new = mix
        form, echo = mix_form(ref)
        fresh = {tb for tb, f in enumerate(new) if f}
        for types, offs in mcalls:
            for buf, fr in ((False, ()), (True, ()), (True, fresh)):
                feats = _features(ref, (4, form, buf, bool(echo and buf and form == "fast"), "mix"))
                feats = feats | access_features(ref, "mix", form, types, offs, buf, n, fresh=fr, echo=echo)
                out |= {("mix", form, Qm, f) for f in feats}
    return out


# ---- the universe ------------------------------------------------------------------------------------------------------------------
FORMS = {"f32": ("general", "fast", "scatter"), "ex": ("general", "fast", "scatter"), "mix": ("general", "fast")}
TRANSITIONS = ("punct>live", "punct>dead", "punct>kept", "live>dead", "dead>live", "live>kept", "kept>live", "live>fill", "dead>fill",
               "kept>fill", "fill>live", "fill>dead", "fill>kept", "live>beyond", "dead>beyond", "kept>beyond", "fill>beyond")
FILL_KINDS = ("covered", "echo", "zero", "fill", "punct", "beyond")
FILL_TRANSITIONS = tuple("%s>%s" % (a, b) for a in ("punct",) for b in ("covered", "echo", "zero")) + \
    tuple("%s>%s" % (a, b) for a in ("covered", "echo", "zero") for b in ("covered", "echo", "zero", "fill", "beyond") if a != b) + \
    tuple("fill>%s" % b for b in ("covered", "echo", "zero", "beyond"))


def _product(unit, form, Qm):
    """every feature the dimensions allow for (unit, form, Q_m), before the exclusions"""
    types = (F32, F16)
    if form != "scatter":
        kinds = KIND if (unit == "mix" and form == "fast") else KIND[:5]
        out = ["all:" + k for k in kinds] + [t for t in TRANSITIONS if "kept" not in t or "kept" in kinds] + ["wrapk0", "rowchg"]
        if form == "general":
            out += ["depth1", "depth2", "depth3+", "carry", "nocarry"]
        if unit == "f32":
            out += ["acc:out:%s:%s" % (t, w) for t in types for w in ("wide", "elem")]
        else:
            out += ["acc:out:f32:wide", "acc:out:f16:wide", "acc:out:f16:elem"]
            pre = ("", "fresh-") if unit == "mix" else ("",)
            for x in pre:
                out += ["acc:hb:f32:%squad-wide" % x, "acc:hb:f32:%ssingle" % x]
                out += ["acc:hb:f16:%squad-wide" % x, "acc:hb:f16:%squad-elem" % x, "acc:hb:f16:%ssingle" % x]
            if "kept" in kinds:
                out += ["acc:hb:f32:kept-single", "acc:hb:f16:kept-single"]
        return out
    J = scatter_J(unit, Qm)
    out = ["in:J%d:%s" % (J, c) for c in ("run", "tail", "endP", "gap", "tail:endP", "tail:gap")]
    out += ["fill:tile:" + c for c in ("skipped", "plain", "mixed")] + ["fill:all:" + k for k in FILL_KINDS]
    out += ["fill:" + t for t in FILL_TRANSITIONS] + ["fill:E0"]
    if unit == "f32":
        out += ["acc:g:f32:wide", "acc:g:f32:elem"]
        out += ["acc:out:%s:%s" % (t, w) for t in types for w in ("run-wide", "run-elem", "fill-wide", "fill-elem")]
    else:
        for t in types:
            odd = t == F16
            out += ["acc:g:%s:wide" % t, "acc:g:%s:elem-tail" % t] + (["acc:g:%s:elem-odd" % t] if odd else [])
            for arr, part in (("out", "run"), ("out", "fill"), ("hb", "run"), ("hb", "echo")):
                out += ["acc:%s:%s:%s-wide" % (arr, t, part), "acc:%s:%s:%s-single" % (arr, t, part)]
                out += ["acc:%s:%s:%s-elem" % (arr, t, part)] if odd else []
    return out


# Classes the product names that cannot exist: (reason, test on (unit, form, Q_m, feature)).  Throughout: 2Z + N = 52 Z or 68 Z is a
# multiple of 4, so no group is ragged at the end of a code block (there is no kind "off"), and the f32 unit's `vec` test depends on
# the output base alone; N >= 4096 means Z >= 64, where every lifting size is a multiple of 4.
def _echo_only_at_big_Z(u, f, q, x):
    return x in ("punct>kept", "kept>live", "fill>kept")


IMPOSSIBLE = (
    ("Q_m = 1 has one interleaver row: no row change, and the walk's jj = q + nP < E = rows never overflows",
     lambda u, f, q, x: q == 1 and x in ("rowchg", "carry")),
    ("a pair never straddles the even positions 2Z and K (the end of the punctured columns, the end of the filler gap)",
     lambda u, f, q, x: u == "f32" and (x.startswith(("punct>", "fill>", "fill:punct>", "fill:fill>")))),
    ("the mix keeps buffer entries only where the single call scatters: Q_m <= 2",
     lambda u, f, q, x: u == "mix" and q > 2 and "kept" in x),
    ("echo needs N >= 4096, where 4 | Z: the punctured columns, the end of the gap and k_0 fall between quads",
     _echo_only_at_big_Z),
    ("the f32 unit's scatter owns one column per lane at Q_m = 4, 8: every run is whole, element stores only",
     lambda u, f, q, x: u == "f32" and f == "scatter" and q in (4, 8) and (x.startswith("in:J1:") and x != "in:J1:run" or x in ("acc:g:f32:elem",) or x.endswith("run-wide"))),
    ("the tail of two columns per lane is one column: it crosses nothing",
     lambda u, f, q, x: x in ("in:J2:tail:endP", "in:J2:tail:gap")),
    ("a dead block under the mix's general form is one with E_r = 0 beside a repeating one: C >= 2, where 4 | Z",
     lambda u, f, q, x: u == "mix" and f == "general" and x in ("punct>dead", "fill>dead")),
    ("under the mix's general form a block has dead positions beside live ones only when E_r lie on both sides of P, so C >= 2 and "
     "4 | Z; the dead ones are the last before k_0, a multiple of Z (or before the end of the buffer): dead>live falls between quads",
     lambda u, f, q, x: u == "mix" and f == "general" and x == "dead>live"),
    ("no buffer position is 'zero' and 'echo' in one call",
     lambda u, f, q, x: x in ("fill:echo>zero", "fill:zero>echo")),
)
# Classes that exist -- real instantiations, e.g. nrldpc_rate_recover_scatter_kernel<__half, 4> -- but lie outside the calls these
# tests make: they are not part of the universe the sets are held to, and nothing here claims they are reached.
OUTSIDE_THE_CALLS = (
    ("Q_m >= 4 scatters only under NRLDPC_RR_SCATTER=1, and the process that sets it makes the f32 call with f32 output and the "
     "f16/f16/f16 ex call at base offsets (0, 0, 0): the access forms of other element types and of odd bases are not run there",
     lambda u, f, q, x: f == "scatter" and q > 2 and x.startswith("acc:") and
     (":f32:" in x if u == "ex" else ":f16:" in x) or (f == "scatter" and q > 2 and x in ("acc:g:f16:elem-odd", "acc:out:f16:fill-elem"))),
)


def product():
    """every (unit, form, Q_m, feature) the dimensions allow"""
    return {(unit, form, Qm, x) for unit in UNITS for form in FORMS[unit] for Qm in QMS for x in _product(unit, form, Qm)}


def universe():
    """The product of the dimensions less IMPOSSIBLE and less OUTSIDE_THE_CALLS"""
    return {c for c in product() if not any(test(*c) for _, test in IMPOSSIBLE + OUTSIDE_THE_CALLS)}


# ---- the space the sets were searched in ---------------------------------------------------------------------------------------------
# (BG, A): Z_c = 6, 9, 20, 20, 88, 88 (BG2; N = 4400 at Z = 88) and BG1 Z_c = 64 (N = 4224, the smallest the scatter rule accepts);
# K' odd at A = 101, 801, 1385.  Then the shapes with C = 2 under a tight LBRM, whole or with one block not transmitted.
SPACE_SHAPES = ((2, 20), (2, 38), (2, 100), (2, 101), (2, 800), (2, 801), (1, 1384), (1, 1385))
SPACE_LBRM = (None, 1.0, 1.5, 2.5)   # TBS_LBRM / A
SPACE_FRACTIONS = (0.3, 0.55, 0.8, 0.97, 1.0, 1.03, 1.6, 2.1, 2.4, 3.3)  # G / P, then +-0, 1, 2 symbols
SPACE_G_MAX = 9000


def space(step=1):
    """The parameter sets of the search, every step-th of them: every shape x LBRM x rv_id x Q_m, G around the listed multiples of
    the buffer's non-filler positions P; C = 2 (A = 3842, TBS_LBRM = 2700) with and without CBGTI; and C = 2 with G around 2 P, so
    that E_r lie on both sides of P (TBS_LBRM = 2700 and 2702: P = 1902 and 1903; N_L = 1 and 2: E_r differ by Q_m N_L)."""
    out = []
    for BG, A in SPACE_SHAPES:
        for lbrm in SPACE_LBRM:
            for rv in range(4):
                for Qm in QMS:
                    base = dict(BG=BG, A=A, Q_m=Qm, rv_id=rv, G=Qm)
                    if lbrm:
                        base.update(I_LBRM=1, TBS_LBRM=int(A * lbrm))
                    P = T.rm_geometry(derive(base))[2]
                    gs = set()
                    for fr in SPACE_FRACTIONS:
                        g0 = int(fr * P) // Qm * Qm
                        gs |= {g0 + d * Qm for d in (-2, -1, 0, 1, 2)}
                    out += [dict(base, G=G) for G in sorted(gs) if 0 < G <= SPACE_G_MAX]
    for rv in range(4):
        for Qm in QMS:
            for cbgti in ((), (1,), (0,)):
                base = dict(BG=2, A=3842, Q_m=Qm, rv_id=rv, G=Qm, I_LBRM=1, TBS_LBRM=2700)
                if cbgti:
                    base["CBGTI"] = list(cbgti)
                P = T.rm_geometry(derive(base))[2]
                n = 2 - len(cbgti)
                out += [dict(base, G=int(fr * n * P) // (2 * Qm) * 2 * Qm + d * Qm) for fr in (0.5, 1.03, 2.2) for d in (0, 1)]
    for tbs in (2700, 2702):
        for N_L in (1, 2):
            for rv in range(4):
                for Qm in QMS:
                    base = dict(BG=2, A=3842, Q_m=Qm, rv_id=rv, G=Qm * N_L, N_L=N_L, I_LBRM=1, TBS_LBRM=tbs)
                    P = T.rm_geometry(derive(base))[2]
                    sym = Qm * N_L
                    out += [dict(base, G=(2 * P // sym + d) * sym) for d in (-2, -1, 0, 1, 2)]
    return out[::step]


# ---- the sets ----------------------------------------------------------------------------------------------------------------------
# The first three are kept for a property of their own (RR_PROPERTIES); the rest is what a greedy search over space() needs for the
# classes those three leave (most new classes first, the smaller shape on a tie), pruned until every set is the only one that
# reaches some class.  Z_c = 9 (A = 38: 2Z, K - 2Z and k_0 are no multiples of 4), 20 and, for C = 2, 208.
RR_PROPERTIES = ("C=3 with unequal E_r and an odd G", "a middle and a trailing code block with E_r=0", "BG1 Z=384")
RR_SETS = [
    dict(BG=2, A=7701, G=3335, Q_m=1),
    dict(BG=2, A=7701, G=1112, Q_m=2, CBGTI=[1, 2]),
    dict(BG=1, A=8424, G=8000, Q_m=2),
    dict(BG=2, A=38, G=10, Q_m=1, rv_id=2, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=12, Q_m=1, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=24, Q_m=1, rv_id=1, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=37, Q_m=1, rv_id=1, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=50, Q_m=1, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=101, G=21, Q_m=1, rv_id=2, I_LBRM=1, TBS_LBRM=101),
    dict(BG=2, A=3842, G=950, Q_m=1, rv_id=3, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=3842, G=4184, Q_m=1, rv_id=0, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=38, G=10, Q_m=2, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=20, Q_m=2, rv_id=2, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=22, Q_m=2, rv_id=1, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=38, Q_m=2, rv_id=1, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=50, Q_m=2, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=101, G=18, Q_m=2, rv_id=2, I_LBRM=1, TBS_LBRM=101),
    dict(BG=2, A=3842, G=950, Q_m=2, rv_id=3, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=3842, G=4184, Q_m=2, rv_id=0, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=38, G=16, Q_m=4, rv_id=2, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=20, Q_m=4, rv_id=3, I_LBRM=1, TBS_LBRM=95),
    dict(BG=2, A=38, G=28, Q_m=4, rv_id=1, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=52, Q_m=4, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=76, Q_m=4, rv_id=1, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=100, G=264, Q_m=4, rv_id=3),
    dict(BG=2, A=3842, G=948, Q_m=4, rv_id=2, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=3842, G=1952, Q_m=4, rv_id=0, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=38, G=12, Q_m=6, rv_id=2, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=18, Q_m=6, rv_id=3, I_LBRM=1, TBS_LBRM=95),
    dict(BG=2, A=38, G=18, Q_m=6, rv_id=2, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=54, Q_m=6, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=78, Q_m=6, rv_id=1, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=100, G=258, Q_m=6, rv_id=3),
    dict(BG=2, A=3842, G=954, Q_m=6, rv_id=2, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=3842, G=1956, Q_m=6, rv_id=0, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=38, G=8, Q_m=8, rv_id=3, I_LBRM=1, TBS_LBRM=95),
    dict(BG=2, A=38, G=16, Q_m=8, rv_id=2, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=16, Q_m=8, rv_id=2, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=38, G=56, Q_m=8, rv_id=0, I_LBRM=1, TBS_LBRM=57),
    dict(BG=2, A=38, G=80, Q_m=8, rv_id=1, I_LBRM=1, TBS_LBRM=38),
    dict(BG=2, A=100, G=488, Q_m=8, rv_id=3),
    dict(BG=2, A=3842, G=944, Q_m=8, rv_id=2, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    dict(BG=2, A=3842, G=1952, Q_m=8, rv_id=0, I_LBRM=1, TBS_LBRM=2700, CBGTI=[1]),
    # E_r on both sides of P = 1902 / 1903 (C = 2, G next to 2 P): a repeating block beside one with dead positions
    dict(BG=2, A=3842, G=3806, Q_m=1, N_L=2, I_LBRM=1, TBS_LBRM=2702),
    dict(BG=2, A=3842, G=3804, Q_m=2, N_L=2, I_LBRM=1, TBS_LBRM=2700),
    dict(BG=2, A=3842, G=3804, Q_m=4, I_LBRM=1, TBS_LBRM=2700),
    dict(BG=2, A=3842, G=3804, Q_m=6, N_L=2, I_LBRM=1, TBS_LBRM=2700),
    dict(BG=2, A=3842, G=3800, Q_m=8, I_LBRM=1, TBS_LBRM=2700),
]
N_PROPERTY_SETS = len(RR_PROPERTIES)
# configurations of the mix of the new tests: (set, transport blocks); every set with 3 or 2, then one set once more with none
# (twice, in the middle and at the end) and one with a single block
MIX_CONFIGS = [(k, 3 - k % 2) for k in range(len(RR_SETS))]
MIX_CONFIGS[5:5] = [(0, 0)]
MIX_CONFIGS += [(3, 1), (1, 0)]


def rr_properties(refs):
    have = set()
    for ref in refs:
        E = ref["E_r"]
        if ref["C"] == 3 and len(set(E)) > 1 and 0 not in E and ref["G"] % 2:
            have.add(RR_PROPERTIES[0])
        if ref["C"] == 3 and E[0] > 0 and E[1] == 0 and E[2] == 0:
            have.add(RR_PROPERTIES[1])
        if ref["BG"] == 1 and ref["Z_c"] == 384:
            have.add(RR_PROPERTIES[2])
    return have


_DERIVED = {}


def derived(kw):
    """derive(kw) of a listed set, kept by its parameters with what the census memoises on it (the sweep does not come through here)"""
    key = tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))
    if key not in _DERIVED:
        _DERIVED[key] = derive(kw)
    return _DERIVED[key]


def rr_reached(sets, mix_configs=None):
    """class -> the first set of `sets` that reaches it, under the calls of the new tests"""
    calls, n_tb = plan_single()
    refs = [derived(kw) for kw in sets]
    if mix_configs is None:
        mix_configs = [(k, 3 - k % 2) for k in range(len(sets))]
    seen = {}
    for k, ref in enumerate(refs):
        for c in census(ref, calls, n_tb):
            seen.setdefault(c, k)
    for pos, (k, n) in enumerate(mix_configs):
        for c in census(refs[k], (), 0, mix=(MIX_CALLS, n, mix_new(pos, n))):
            seen.setdefault(c, k)
    return seen


def rr_missing(sets, mix_configs=None):
    """What `sets` leaves unreached: classes of the universe and properties, sorted; empty when it reaches everything."""
    have = set(rr_reached(sets, mix_configs))
    props = set(RR_PROPERTIES) - rr_properties([derive(kw) for kw in sets])
    return sorted(universe() - have) + sorted(props)


# ---- what the suite reached before these lists --------------------------------------------------------------------------------------
def reached_before(half_soft_sets, half_soft_n_tb, chain_sets):
    """The classes of the universe that the two older lists reach under the calls of their tests: the nine sets of
    tests/test_half_soft_path_gpu.py::CASES (f32 call with both outputs; all eight combinations of the ex call at offset 0 and
    f16/f16/f16 one element in; the mix at aligned bases with n_tb = half_soft_n_tb, plain and HARQ with flags mixed) and the ten of
    tests/test_chain_gpu.py::CASES (f32 call only); three transport blocks, no switch."""
    base, one = OFFSETS[0], OFFSETS[4]
    calls = [("f32", (F32, F32, o), base, buf, "default") for o in (F32, F16) for buf in (False, True)]
    both = calls + [("ex", c, base, buf, "default") for c in COMBOS for buf in (False, True)]
    both += [("ex", (F16, F16, F16), one, buf, "default") for buf in (False, True)]
    mcalls = [(c, base) for c in COMBOS]
    have = set()
    for k, (kw, n) in enumerate(zip(half_soft_sets, half_soft_n_tb)):
        have |= census(derive(kw), both, 3, mix=(mcalls, n, [(tb + k + 1) % 2 for tb in range(n)]))
    for kw in chain_sets:
        have |= census(derive(kw), calls[:3], 3)
    return have & universe()


# ---- the device side (GPU tests and tests/rr_knob_child.py only) ----------------------------------------------------------------------
NP = {F32: np.dtype(np.float32), F16: np.dtype(np.float16)}
GUARD = 32  # bytes checked either side of an array (the slots keep 256)


def bits(x):
    """a float array as integers: comparisons are bit for bit (-0 is not +0, +inf equals +inf)"""
    return np.ascontiguousarray(x).view(np.int32 if x.dtype == np.float32 else np.int16)


class ElemSlot:
    """n elements of type t, `off` elements above a 256-byte boundary inside a larger device tensor that holds NaN -- which no call
    produces from finite input -- everywhere else.  ptr is the raw address of element 0."""

    def __init__(self, n, t, off, data=None):
        import torch
        dt = torch.float16 if t == F16 else torch.float32
        pad = 256 // NP[t].itemsize
        self.n, self.lo = n, pad + off
        self.buf = torch.full((self.lo + n + pad,), float("nan"), dtype=dt, device="cuda")
        assert self.buf.data_ptr() % 256 == 0 and pad * NP[t].itemsize >= GUARD
        if data is not None:
            self.set(data)
        self.ptr = self.buf.data_ptr() + self.lo * NP[t].itemsize

    def set(self, data):
        import torch
        self.buf[self.lo:self.lo + self.n] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1).copy()).cuda()

    def data(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def guards_intact(self):
        w = self.buf.cpu().numpy()
        return bool(np.isnan(w[:self.lo]).all() and np.isnan(w[self.lo + self.n:]).all())


class Shape:
    """What tests/test_half_soft_path_gpu.py::model_step reads of a parameter object, from testbench_ref.derive"""

    def __init__(self, ref):
        self.Z_c, self.C, self.K, self.K_prime, self.N, self.N_cb = ref["Z_c"], ref["C"], ref["K"], ref["K_prime"], ref["N"], ref["N_cb"]
        self.k_0, self.Q_m, self.G, self.E_r = ref["k_0"], ref["Q_m"], ref["G"], list(ref["E_r"])


def product_params(pkg, kw, ref):
    """the product's parameter object of a set, which must derive what testbench_ref.derive derives"""
    p = pkg.NRLDPC(**kw)
    p.validate()
    s = Shape(ref)
    for k, v in vars(s).items():
        got = getattr(p, k)
        assert (list(got) if k == "E_r" else int(got)) == v, (kw, k, got, v)
    return p


def filler_mask(ref):
    """the filler positions of a buffer row [N_cb]"""
    lo_f = T.rm_geometry(ref)[0]
    pos = np.arange(ref["N_cb"])
    return (pos >= lo_f) & (pos < ref["K"] - 2 * ref["Z_c"])


def sequence_inputs(ref, seed, n_tb, hdt):
    """three transmissions (f32, 4 randn) and the contents of the non-zero buffer of the third call: 3 randn in hdt, no zero among
    them, filler positions included"""
    rng = np.random.default_rng(seed)
    gs = [(4 * rng.standard_normal((n_tb, ref["G"]))).astype(np.float32) for _ in range(3)]
    h = (3 * rng.standard_normal((n_tb, ref["C"], ref["N_cb"]))).astype(NP[hdt])
    h[h == 0] = 1
    return gs, h


_MODEL = {}


def model_sequence(orc, ref, seed, n_tb, types, new=None):
    """Expected (outputs [3], buffers after call 1 and 2) of the sequence no buffer / a zero buffer / the non-zero buffer, from
    oracle.rate_recover widened by model_step and narrow of tests/test_half_soft_path_gpu.py.  new: flags per transport block for
    the third call -- a flagged block's rows count as +0.0.  Computed once per argument tuple and never modified."""
    shape = tuple(tuple(v) if isinstance(v, list) else v for k, v in sorted(ref.items()) if not k.startswith("_"))
    key = (shape, seed, n_tb, types, None if new is None else tuple(new))
    if key not in _MODEL:
        from test_half_soft_path_gpu import model_step
        idt, hdt, odt = (NP[t] for t in types)
        p = Shape(ref)
        gs, h2 = sequence_inputs(ref, seed, n_tb, types[1])
        outs, bufs = [], []
        if n_tb:
            outs.append(model_step(orc, p, gs[0].astype(idt), None, hdt, odt))
            h = np.zeros((n_tb, p.C, p.N_cb), hdt)
            outs.append(model_step(orc, p, gs[1].astype(idt), h, hdt, odt))
            bufs.append(h)
            h = h2.copy()
            for tb, f in enumerate(new or ()):
                if f:
                    h[tb] = 0
            outs.append(model_step(orc, p, gs[2].astype(idt), h, hdt, odt))
            bufs.append(h)
            for x in outs + bufs:
                x.setflags(write=False)
        _MODEL[key] = (outs, bufs)
    return _MODEL[key]


def code(pkg, t):
    return pkg._capi.LLR_F16 if t == F16 else pkg._capi.LLR_F32


def call_single(pkg, p, unit, types, g, n_tb, h, o):
    """nrldpc_rate_recover_dev (unit f32) or the symbol nrldpc_rate_recover_ex_dev itself on raw addresses"""
    C = pkg._capi
    if unit == "f32":
        assert types[:2] == (F32, F32)
        pkg.rate_recover_dev(p, g, n_tb, h, o, out_dtype=code(pkg, types[2]))
    else:
        t = C.tb_params(p)
        C.check(pkg.load().nrldpc_rate_recover_ex_dev(C.C.byref(t), C._ptr(g), code(pkg, types[0]), n_tb, C._ptr(h), code(pkg, types[1]),
                                                      C._ptr(o), code(pkg, types[2]), None))


def check_buffer(got, want, before, filler, tag):
    """the buffer equals the model bit for bit off the filler positions and is untouched at them"""
    got, want, before = (bits(x).reshape(-1, filler.size) for x in (got, want, before))
    bad = np.argwhere(got[:, ~filler] != want[:, ~filler])
    assert bad.size == 0, tag + ("buffer (row, non-filler index)", bad[:4].tolist())
    assert (got[:, filler] == before[:, filler]).all(), tag + ("filler positions of the buffer",)


def run_single(pkg, orc, k, unit, types, offs, n_tb=N_TB):
    """Set k through one unit at the base offsets `offs`: the three-call sequence against the model, everything exact; the guards
    of every array intact and g_tilde unchanged.  Returns the number of elements compared."""
    import torch
    kw = RR_SETS[k]
    ref = _ref(k)
    p = product_params(pkg, kw, ref)
    want_o, want_h = model_sequence(orc, ref, 4000 + k, n_tb, types)
    gs, h2 = sequence_inputs(ref, 4000 + k, n_tb, types[1])
    filler = filler_mask(ref)
    ncwz = 2 * ref["Z_c"] + ref["N"]
    hs = ElemSlot(n_tb * ref["C"] * ref["N_cb"], types[1], offs[1])
    n = 0
    for c in range(3):
        tag = (kw, unit, types, offs, "call %d" % c)
        g = gs[c].astype(NP[types[0]])
        src = ElemSlot(g.size, types[0], offs[0], g)
        dst = ElemSlot(n_tb * ref["C"] * ncwz, types[2], offs[2])
        if c:
            hs.set(np.zeros(hs.n, NP[types[1]]) if c == 1 else h2)
        before = hs.data()
        call_single(pkg, p, unit, types, src.ptr, n_tb, hs.ptr if c else None, dst.ptr)
        torch.cuda.synchronize()
        got = dst.data().reshape(n_tb * ref["C"], ncwz)
        bad = np.argwhere(bits(got) != bits(want_o[c]))
        assert bad.size == 0, tag + ("output (code block, position)", bad[:4].tolist())
        assert np.isposinf(got[:, 2 * ref["Z_c"]:][:, :filler.size][:, filler].astype(np.float32)).all(), tag
        if c:
            check_buffer(hs.data(), want_h[c - 1], before, filler, tag)
        else:
            assert np.isnan(hs.data()).all(), tag + ("the buffer of a call that was given none",)
        assert (bits(src.data()) == bits(g.reshape(-1))).all(), tag + ("g_tilde changed",)
        assert src.guards_intact() and dst.guards_intact() and hs.guards_intact(), tag + ("guards",)
        n += got.size
    return n


def _ref(k):
    return derived(RR_SETS[k])

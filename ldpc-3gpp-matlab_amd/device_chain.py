"""Receive chain with every per-bit stage on the GPU: demodulator LLRs g_tilde in HBM -> rate recovery
(nrldpc_rate_recover_dev, row N1) -> LDPC decode (nrldpc_decode_dev, the hot path) -> CRC stages
(nrldpc_crc_check_dev, row N2) -> a_hat + ok flags.  The reference runs these as six interpreted stages
per transport block (NRLDPCDecoder.m:133-140); here one transport-block batch is three kernel launches
with no host loop and no PCIe traffic in between.  torch is used for device memory only.
"""
import copy

import numpy as np

from ._capi import LLR_F16, LLR_F32, MIX_FIELDS, MIX_SKIP_SETTLED, MIX_SKIP_UNSCHEDULED, Codec, MixChanPlan, MixPlan, MixTxPlan, MultiCall, NRLDPCError, UnsupportedParameters, algorithm_code, crc_check_harq_dev, demod_method_code, rate_recover_dev, tb_params
from .nrldpc import NRLDPC


class _Derived:
    """What a chain step needs of the parameter object's Dependent properties (NRLDPC.m:297-543), computed once per setting of the
    settable ones: the mirror re-derives every Dependent property on every access, as the reference does, and a step reads a dozen
    of them -- 1 ms of Python per step, a fifth of a small code's Monte-Carlo sweep."""
    __slots__ = ("t", "C", "Z_c", "N", "K", "B", "N_cb", "A", "G", "BG", "act", "flags")

    def __init__(self, p):
        self.t = tb_params(p)
        self.C, self.Z_c, self.N, self.K, self.B, self.N_cb, self.A, self.G, self.BG = p.C, p.Z_c, p.N, p.K, p.B, p.N_cb, p.A, p.G, p.BG
        self.act = p.active_layers()
        self.flags = list(p.CBGTI_flags)


def _derived(chain):
    p = chain.p
    key = (p.BG, p.A, p.I_LBRM, p.TBS_LBRM, p.rv_id, p.G, p.Q_m, p.N_L, tuple(p.CBGTI))  # every settable property (NRLDPC.m:28-84)
    if getattr(chain, "_dkey", None) != key:
        chain._dval, chain._dkey = _Derived(p), key
    return chain._dval


class DeviceDecodeChain:
    """Batched NRLDPCDecoder.step on device tensors.  `params` is an NRLDPC parameter object (or any
    NRLDPCDecoder).  The DiscreteState of the reference (NRLDPCDecoder.m:64-95) lives in HBM, one row per transport
    block of the batch: d_tilde_buffer (`harq`, only when I_HARQ), b_hat_buffer (`b_hat`) and the sticky
    code_block_CRC_passed flags (`cb_pass`); reset() clears them (:343-356).  CBGTI of `params` is honoured (:304)."""

    def __init__(self, params: NRLDPC, iterations=50, I_HARQ=0, alpha=None, llr_scale=0, prune_layers=True,
                 llr_dtype=None, device_id=0, beta=0.0, crc_stop=False, algorithm="min-sum", harq_dtype=None):
        """llr_dtype: of the LLRs rate recovery hands the decoder; None = fp16 for "min-sum" (its kernels quantise to an int8 grid
        anyway), f32 for "sum-product" (flooding sum-product, the reference's comm.LDPCDecoder: it ingests the values unquantised).
        harq_dtype: of the soft buffer (only with I_HARQ): None / np.float32 = the reference's accumulation in f32, np.float16 = half
        the memory; the buffer then saturates at +-65504 and the decoder sees exactly what it holds (nrldpc_rate_recover_ex_dev)."""
        algorithm_code(algorithm)  # UnsupportedParameters for an unknown name, before any device work
        try:
            self.harq_dtype = np.dtype(np.float32 if harq_dtype is None else harq_dtype)
        except TypeError:
            self.harq_dtype = None
        if self.harq_dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
            raise UnsupportedParameters("harq_dtype should be numpy float32 or float16, not %r." % (harq_dtype,))
        import torch
        self.torch = torch
        params.validate()
        self.p = params
        self.crc_stop = bool(crc_stop)  # nrldpc_cfg.early_term = 2: a code block also stops when its CRC holds
        self.iterations, self.I_HARQ = int(iterations), int(I_HARQ)
        self.alpha, self.beta, self.llr_scale, self.prune = alpha, beta, llr_scale, prune_layers
        self.algorithm = algorithm
        self.llr_dtype = np.dtype(llr_dtype if llr_dtype is not None else np.float32 if algorithm == "sum-product" else np.float16)
        self.dev = torch.device("cuda", device_id)
        self.device_id = device_id
        self._codec, self._codec_layers, self._codec_code = None, None, None
        self._layers_seen = 4
        self.harq = self.b_hat = self.cb_pass = None

    def reset(self):
        """reset(hDec): clears d_tilde_buffer, b_hat_buffer and code_block_CRC_passed (NRLDPCDecoder.m:343-356)."""
        self.harq = self.b_hat = self.cb_pass = None  # re-allocated zeroed (for any batch size) by the next step
        self._layers_seen = 4

    def close(self):
        if self._codec is not None:
            self._codec.close()
            self._codec = None

    def _codec_for(self, n_layers):
        """One codec for the chain's lifetime; the layer count is a property of the call (nrldpc_set_layers, ABI revision 5)."""
        if self._codec is not None and self._codec_code != (self.p.BG, self.p.Z_c):
            # A changed on a plain parameter object between steps: Z_c (or BG) moved, and a codec built for the old pair would read
            # and write tensors sized for the new one out of bounds -- a new code is a new codec
            self._codec.close()
            self._codec = None
        if self._codec is None:
            self._codec_code = (self.p.BG, self.p.Z_c)
            self._codec_layers = None
            self._codec = Codec(self.p.BG, self.p.Z_c, max_iter=self.iterations, n_layers=n_layers, early_term=True,
                                alpha=self.alpha or 0.0, beta=self.beta, llr_scale=self.llr_scale, llr_dtype=self.llr_dtype, device_id=self.device_id,
                                crc=self.p.code_block_check() if self.crc_stop else None, algorithm=self.algorithm)
        elif self._codec_layers != n_layers:
            self._codec.set_layers(n_layers)
        self._codec_layers = n_layers
        return self._codec

    def step(self, g_tilde):
        """g_tilde: torch float32 or float16 tensor [n_tb][G] on the device (positive = bit 0).
        Returns (a_hat uint8 [n_tb][A], ok bool [n_tb], iters int32 [n_tb][C]) as device tensors."""
        torch, p = self.torch, self.p
        if g_tilde.dim() != 2 or g_tilde.shape[1] != p.G or g_tilde.dtype not in (torch.float32, torch.float16) or not g_tilde.is_cuda:
            raise NRLDPCError("g_tilde should be a float32 or float16 device tensor of shape [n_tb][G].")
        if g_tilde.device != self.dev:
            raise NRLDPCError("g_tilde lives on %s, this chain on %s." % (g_tilde.device, self.dev))
        with torch.cuda.device(self.dev):  # the stateless stage kernels launch on the current HIP device
            return self._step(g_tilde.contiguous())

    def _step(self, g_tilde):
        torch, d = self.torch, _derived(self)
        n_tb, C_ = g_tilde.shape[0], d.C
        t = d.t
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        ncwz = 2 * d.Z_c + d.N
        if self.cb_pass is not None and self.cb_pass.shape[0] != n_tb:
            # see NRLDPCDecoder.step_batch: only HARQ state that is really pending makes a new batch size an error
            # (the check synchronises, but only on this rare path); without it a new batch size starts a new set
            if self.I_HARQ and (bool(self.cb_pass.any()) or bool(self.harq.any())):
                raise NRLDPCError("batch size changed from %d to %d transport blocks with HARQ state pending "
                                  "(I_HARQ ~= 0); call reset() first." % (self.cb_pass.shape[0], n_tb))
            self.cb_pass = self.b_hat = self.harq = None
        if self.cb_pass is not None and (self.cb_pass.shape[1] != C_ or self.b_hat.shape[1] != d.B or
                                         (self.harq is not None and self.harq.shape[2] != d.N_cb)):
            # another code on the same parameter object (A changed between steps): buffers of the old one's sizes hold nothing that
            # belongs to these transport blocks -- a new set, as after reset() (the codec itself: _codec_for)
            self.cb_pass = self.b_hat = self.harq = None
            self._layers_seen = 4
        if self.cb_pass is None:
            self.cb_pass = torch.zeros((n_tb, C_), dtype=torch.int32, device=self.dev)
            self.b_hat = torch.zeros((n_tb, d.B), dtype=torch.uint8, device=self.dev)
            if self.I_HARQ:
                self.harq = torch.zeros((n_tb, C_, d.N_cb), dtype=torch.float16 if self.harq_dtype == np.float16 else torch.float32, device=self.dev)
        tdt = torch.float16 if self.llr_dtype == np.float16 else torch.float32
        cw_llr = torch.empty((n_tb * C_, ncwz), dtype=tdt, device=self.dev)
        rate_recover_dev(t, g_tilde.data_ptr(), n_tb, self.harq.data_ptr() if self.I_HARQ else None,
                         cw_llr.data_ptr(), LLR_F16 if tdt == torch.float16 else LLR_F32, stream,
                         in_dtype=LLR_F16 if g_tilde.dtype == torch.float16 else LLR_F32,
                         harq_dtype=LLR_F16 if self.harq_dtype == np.float16 else LLR_F32)
        rows = 46 if d.BG == 1 else 42
        n_layers = rows
        if self.prune:
            act = d.act
            self._layers_seen = max(self._layers_seen, act) if self.I_HARQ else act
            n_layers = self._layers_seen
        codec = self._codec_for(n_layers)
        c_hat = torch.empty((n_tb * C_, d.K), dtype=torch.uint8, device=self.dev)
        iters = torch.empty(n_tb * C_, dtype=torch.int32, device=self.dev)
        codec.decode_dev(cw_llr.data_ptr(), n_tb * C_, c_hat.data_ptr(), iters.data_ptr(), None, stream)
        ok = torch.empty(n_tb, dtype=torch.int32, device=self.dev)
        crc_check_harq_dev(t, c_hat.data_ptr(), n_tb, self.b_hat.data_ptr(), ok.data_ptr(), self.cb_pass.data_ptr(),
                           d.flags, self.I_HARQ != 0, stream)
        return self.b_hat[:, : d.A].clone(), ok != 0, iters.view(n_tb, C_)


class MixedDecodeChain:
    """The receive chain for a MIX of configurations: n parameter sets (NRLDPC objects) with n_tb[i] transport blocks each, from
    demodulator LLRs to b_hat in a number of launches that does not depend on n -- mix rate recovery (one launch), the mixed-batch
    decoder (nrldpc_decode_multi_dev: a handful), the mix CRC stage (one launch).  Every array is PACKED: configuration i's segment
    starts at plan.offsets[i].<field> elements and is exactly the array DeviceDecodeChain uses for that configuration;
    views() / pack() convert.  One codec per configuration (its layer count from active_layers() when prune_layers) and one
    MultiCall, both built once.

    I_HARQ = 0 (the default): no state, every step stands alone.  I_HARQ != 0: the chain owns the DiscreteState of the reference's
    decoder (NRLDPCDecoder.m:64-95) for every transport block of the mix, packed and zero-initialised -- `harq` (d_tilde_buffer, f32
    or f16 by harq_dtype), `cb_pass` (the sticky code_block_CRC_passed), `cbgti` (CBGTI_flags of each parameter object, filled once)
    and `b_hat`, which becomes in/out (b_hat_buffer) -- and step() takes the redundancy version(s) and a per-transport-block "starts
    a new HARQ process" flag array; reset() clears the state of every block (:343-356), a flag that of one block.  A plan is immutable
    and rv_id only moves k_0, so the chain holds one MixPlan per distinct tuple of redundancy versions over the same arrays.

    skip (only with I_HARQ != 0; None, the default, is the chain described so far, on the same code path): a step decodes only the code
    blocks still PENDING -- MixPlan.pending turns the state into an index list and a count per configuration, the counts come to the
    host (the one synchronisation the mode adds), and unless every block is pending MixPlan.gather_cw packs the pending LLR rows, the
    decoder runs on counts[i] rows and MixPlan.scatter_hard puts the hard decisions back.  "unscheduled": pending = the block's CBGTI
    flag; b_hat, ok and cb_pass are bit for bit those of skip=None.  "settled": also leaves out blocks whose CRC held in an earlier
    step and transport blocks already acknowledged (the rule: include/nrldpc.h); a settled block keeps the hard decisions of the step
    in which it settled instead of being decoded again -- a deviation from the reference -- and `ok` and `c_hat` become state, which
    reset() clears.  After a step last_decoded lists the code blocks decoded per configuration, `index` and `count` are the device
    arrays of MixPlan.pending, iters is 0 for a block that was not decoded."""

    _SKIP_RULES = {"unscheduled": MIX_SKIP_UNSCHEDULED, "settled": MIX_SKIP_SETTLED}
    _SHAPES = {"g": lambda t, n: (n, t.G), "harq": lambda t, n: (n, t.C, t.N_cb), "cw": lambda t, n: (n * t.C, 2 * t.Z + t.N),
               "c_hat": lambda t, n: (n * t.C, t.K), "cb": lambda t, n: (n, t.C), "b_hat": lambda t, n: (n, t.B), "tb": lambda t, n: (n,)}

    def __init__(self, params, n_tb, iterations=50, alpha=None, beta=0.0, llr_scale=0, prune_layers=True, llr_dtype=None,
                 algorithm="min-sum", device_id=0, I_HARQ=0, harq_dtype=None, skip=None):
        algorithm_code(algorithm)  # UnsupportedParameters for an unknown name, before any device work
        try:
            self.harq_dtype = np.dtype(np.float32 if harq_dtype is None else harq_dtype)
        except TypeError:
            self.harq_dtype = None
        if self.harq_dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
            raise UnsupportedParameters("harq_dtype should be numpy float32 or float16, not %r." % (harq_dtype,))
        self.I_HARQ = int(I_HARQ)
        if skip is not None and (not isinstance(skip, str) or skip not in self._SKIP_RULES):
            raise UnsupportedParameters("skip should be None, \"unscheduled\" or \"settled\", not %r." % (skip,))
        if skip is not None and not self.I_HARQ:
            raise UnsupportedParameters("skip=%r reads HARQ state: it needs I_HARQ ~= 0." % (skip,))
        self.skip = skip
        self.last_decoded = None
        self.index = self.count = self._count_host = self._dense = None
        import torch
        self.torch = torch
        params = list(params)
        for p in params:
            p.validate()
        self.params, self.n_tb = params, [int(x) for x in n_tb]
        self.algorithm = algorithm
        self.llr_dtype = np.dtype(llr_dtype if llr_dtype is not None else np.float32 if algorithm == "sum-product" else np.float16)
        if self.llr_dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
            raise UnsupportedParameters("llr_dtype should be numpy float32 or float16, not %r." % (llr_dtype,))
        self.dev = torch.device("cuda", device_id)
        self.device_id = device_id
        self.prune = bool(prune_layers)
        self.plan = MixPlan(params, self.n_tb, device_id=device_id)
        self._own_rv = tuple(int(p.rv_id) for p in params)
        self._plans = {self._own_rv: self.plan}  # one plan per tuple of redundancy versions (only I_HARQ steps add to it)
        self._acts = {self._own_rv: [p.active_layers() for p in params]}
        self.codecs = []
        self.harq = self.cb_pass = self.cbgti = None
        try:
            for p in params:
                rows = 46 if p.BG == 1 else 42
                self.codecs.append(Codec(p.BG, p.Z_c, max_iter=int(iterations), n_layers=p.active_layers() if prune_layers else rows,
                                         early_term=True, alpha=alpha or 0.0, beta=beta, llr_scale=llr_scale, llr_dtype=self.llr_dtype,
                                         device_id=device_id, algorithm=algorithm))
            tot, off = self.plan.totals, self.plan.offsets
            tdt = torch.float16 if self.llr_dtype == np.float16 else torch.float32
            # the chain's own packed arrays, allocated once (gaps stay zero: the kernels never touch them)
            self.cw_llr = torch.zeros(tot.cw, dtype=tdt, device=self.dev)
            self.c_hat = torch.zeros(tot.c_hat, dtype=torch.uint8, device=self.dev)
            self.iters = torch.zeros(tot.cb, dtype=torch.int32, device=self.dev)
            self.b_hat = torch.zeros(tot.b_hat, dtype=torch.uint8, device=self.dev)
            self.ok = torch.zeros(tot.tb, dtype=torch.int32, device=self.dev)
            n = len(params)
            # what each codec runs at now, and (I_HARQ, prune_layers) the sticky maximum over the redundancy versions since reset()
            self._codec_layers = [p.active_layers() if prune_layers else (46 if p.BG == 1 else 42) for p in params]
            self._layers_seen = [4] * n
            if self.I_HARQ:
                self.harq = torch.zeros(tot.harq, dtype=torch.float16 if self.harq_dtype == np.float16 else torch.float32, device=self.dev)
                self.cb_pass = torch.zeros(tot.cb, dtype=torch.int32, device=self.dev)
                self.cbgti = torch.ones(tot.cb, dtype=torch.uint8, device=self.dev)
                for v, p, k in zip(self.views(self.cbgti, "cb"), params, self.n_tb):
                    if k:
                        v.copy_(torch.tensor([1 if f else 0 for f in p.CBGTI_flags], dtype=torch.uint8).repeat(k, 1))
            self._multi = MultiCall(self.codecs, [self.cw_llr.data_ptr() + off[i].cw * self.llr_dtype.itemsize for i in range(n)],
                                    [self.n_tb[i] * params[i].C for i in range(n)], [self.c_hat.data_ptr() + off[i].c_hat for i in range(n)],
                                    [self.iters.data_ptr() + 4 * off[i].cb for i in range(n)]) if n else None
            if self.skip is not None and self._multi is not None:
                self.index = torch.zeros(tot.cb, dtype=torch.int32, device=self.dev)
                self.count = torch.zeros(n, dtype=torch.int32, device=self.dev)
                self._count_host = torch.zeros(n, dtype=torch.int32).pin_memory()
        except Exception:
            self.close()
            raise

    def close(self):
        for c in getattr(self, "codecs", []):
            c.close()
        self.codecs = []
        self._multi = self._dense = None
        for plan in getattr(self, "_plans", {}).values():
            plan.close()
        self._plans = {}
        if getattr(self, "plan", None) is not None:
            self.plan.close()

    def reset(self):
        """reset(hDec) for every transport block of the mix: clears d_tilde_buffer, b_hat_buffer and code_block_CRC_passed
        (NRLDPCDecoder.m:343-356), and the sticky layer counts."""
        for t in (self.harq, self.b_hat, self.cb_pass):
            if t is not None:
                t.zero_()
        if self.skip is not None:  # ok is the settled rule's state, c_hat holds the decisions settled blocks keep
            self.ok.zero_()
            self.c_hat.zero_()
        self._layers_seen = [4] * len(self.params)

    def new_batch(self):
        """reset() without a memset, for a caller whose next step flags EVERY transport block as new (step(..., new=all ones)): the flags
        make the kernels treat harq, cb_pass and b_hat as cleared, so only the sticky layer counts are left to forget.  (Not with skip:
        there ok and c_hat are state that only reset() clears.)"""
        if self.skip is not None:
            raise NRLDPCError("new_batch() is reset() without the memsets; with skip set, ok and c_hat are state: call reset().")
        self._layers_seen = [4] * len(self.params)

    def _plan_for(self, rv_id):
        """The plan (and the active layer counts) for a step's redundancy versions: None = the parameter objects' own, one int for
        every configuration, or a sequence of n.  Built on first use from copies of the parameter objects, then cached."""
        n = len(self.params)
        if rv_id is None:
            key = self._own_rv
        elif isinstance(rv_id, (int, np.integer)):
            key = (int(rv_id),) * n
        else:
            key = tuple(int(x) for x in rv_id)
            if len(key) != n:
                raise NRLDPCError("rv_id should be None, one value or one value per configuration (%d), got %d." % (n, len(key)))
        if key not in self._plans:
            ps = []
            for p, rv in zip(self.params, key):
                q = copy.copy(p)
                q.rv_id = rv  # (UnsupportedParameters for a value outside 0 ... 3)
                ps.append(q)
            plan = MixPlan(ps, self.n_tb, device_id=self.device_id)
            same = all(getattr(a, f) == getattr(b, f) for a, b in zip(plan.offsets, self.plan.offsets) for f in MIX_FIELDS)
            if not same or len(plan.offsets) != len(self.plan.offsets):
                plan.close()
                raise NRLDPCError("the layout of the plan for rv_id %r differs from the chain's: its packed arrays cannot be shared." % (key,))
            self._plans[key], self._acts[key] = plan, [q.active_layers() for q in ps]
        return self._plans[key], self._acts[key]

    def views(self, packed, field):
        """The per-configuration views of a packed tensor: field is one of "g", "harq", "cw", "c_hat", "cb" (iters, cb_pass), "b_hat",
        "tb" (ok); view i has the shape of the single-configuration array ([n_tb][G], [n_tb][C][N_cb], [n_tb*C][N_cw], [n_tb*C][K],
        [n_tb][C], [n_tb][B], [n_tb])."""
        if field not in MIX_FIELDS:
            raise NRLDPCError("unknown field %r (one of %s)" % (field, ", ".join(MIX_FIELDS)))
        flat = packed.reshape(-1)
        if flat.numel() < getattr(self.plan.totals, field):
            raise NRLDPCError("the packed %s array should hold at least %d elements." % (field, getattr(self.plan.totals, field)))
        out = []
        for i, t in enumerate(self.plan.params):
            shape = self._SHAPES[field](t, self.n_tb[i])
            o = getattr(self.plan.offsets[i], field)
            out.append(flat[o: o + int(np.prod(shape, dtype=np.int64))].view(shape))
        return out

    def pack(self, tensors, field):
        """A packed tensor (gaps zero) from one tensor per configuration, each of the single-configuration shape for `field`."""
        tensors = list(tensors)
        if len(tensors) != len(self.params):
            raise NRLDPCError("one tensor per configuration expected (%d), got %d." % (len(self.params), len(tensors)))
        dt = tensors[0].dtype if tensors else self.torch.float32
        packed = self.torch.zeros(getattr(self.plan.totals, field), dtype=dt, device=self.dev)
        for v, x in zip(self.views(packed, field), tensors):
            if tuple(x.shape) != tuple(v.shape) or x.dtype != dt:
                raise NRLDPCError("a tensor of shape %s and type %s expected for field %r, got %s %s." % (tuple(v.shape), dt, field, tuple(x.shape), x.dtype))
            v.copy_(x)
        return packed

    def step(self, g_tilde_packed, rv_id=None, new=None):
        """g_tilde_packed: the packed float32 or float16 demodulator LLRs on the device (plan.totals.g elements; pack(..., "g")).
        With I_HARQ != 0 only: rv_id = the redundancy version(s) of this transmission (None: the parameter objects' own; one int for
        all configurations; a sequence of n), new = None or a packed uint8 device tensor of plan.totals.tb elements (pack(..., "tb")),
        non-zero where a transport block starts a new HARQ process in this step: its soft-buffer rows count as zero and are not read,
        its code-block flags and b_hat segments start from nothing -- reset() followed by a step, for that block alone.
        Returns (b_hat_packed uint8, ok int32, iters int32): the chain's own packed device arrays, valid until the next step (clone
        what must live longer); views(b_hat_packed, "b_hat")[i][:, :A] is a_hat of configuration i, views(ok, "tb")[i] its flags
        (0 where the reference returns []), views(iters, "cb")[i] its iteration counts [n_tb][C]."""
        torch = self.torch
        g = g_tilde_packed
        if g.dim() != 1 or g.dtype not in (torch.float32, torch.float16) or not g.is_cuda or not g.is_contiguous() or g.numel() < self.plan.totals.g:
            raise NRLDPCError("g_tilde should be a contiguous 1-D float32 or float16 device tensor of at least %d elements." % self.plan.totals.g)
        if g.device != self.dev:
            raise NRLDPCError("g_tilde lives on %s, this chain on %s." % (g.device, self.dev))
        if not self.I_HARQ:
            if rv_id is not None or new is not None:
                raise NRLDPCError("rv_id and new belong to a chain with HARQ state (I_HARQ ~= 0).")
        else:
            return self._step_harq(g, rv_id, new)
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            self.plan.rate_recover(g.data_ptr() if g.numel() else None, None, self.cw_llr.data_ptr(), in_dtype=LLR_F16 if g.dtype == torch.float16 else LLR_F32,
                                   out_dtype=LLR_F16 if self.llr_dtype == np.float16 else LLR_F32, stream=stream)
            if self._multi is not None:
                self._multi(stream)
            self.plan.crc_check(self.c_hat.data_ptr(), self.b_hat.data_ptr(), self.ok.data_ptr(), None, stream=stream)
        return self.b_hat, self.ok, self.iters

    def _step_harq(self, g, rv_id, new):
        torch = self.torch
        if new is not None:
            if (new.dim() != 1 or new.dtype != torch.uint8 or not new.is_cuda or not new.is_contiguous() or new.numel() < self.plan.totals.tb
                    or new.device != self.dev):
                raise NRLDPCError("new should be a contiguous 1-D uint8 tensor of at least %d elements on %s." % (self.plan.totals.tb, self.dev))
        plan, acts = self._plan_for(rv_id)
        if self.prune:
            # a row that carried an LLR in an earlier redundancy version still does (the buffer holds it): the sticky maximum.
            # More rows than a block needs are exact, only slower (a flagged block does not lower its configuration's count).
            for i, codec in enumerate(self.codecs):
                self._layers_seen[i] = max(self._layers_seen[i], acts[i])
                if self._codec_layers[i] != self._layers_seen[i]:
                    codec.set_layers(self._layers_seen[i])
                    self._codec_layers[i] = self._layers_seen[i]
        f16 = torch.float16
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            d_new = new.data_ptr() if new is not None and new.numel() else None
            plan.rate_recover_harq(g.data_ptr() if g.numel() else None, self.harq.data_ptr() if self.harq.numel() else None,
                                   self.cw_llr.data_ptr(), d_new, in_dtype=LLR_F16 if g.dtype == f16 else LLR_F32,
                                   harq_dtype=LLR_F16 if self.harq_dtype == np.float16 else LLR_F32,
                                   out_dtype=LLR_F16 if self.llr_dtype == np.float16 else LLR_F32, stream=stream)
            if self.skip is not None:
                self._decode_pending(plan, d_new, stream)
            elif self._multi is not None:
                self._multi(stream)
            plan.crc_check_harq(self.c_hat.data_ptr(), self.b_hat.data_ptr(), self.ok.data_ptr(), self.cb_pass.data_ptr(),
                                self.cbgti.data_ptr(), d_new, stream=stream)
        return self.b_hat, self.ok, self.iters

    def _decode_pending(self, plan, d_new, stream):
        """The decoder stage of a step with skip set: the pending code blocks only (self.ok still holds the previous step's flags)."""
        torch, n = self.torch, len(self.params)
        totals = [k * p.C for k, p in zip(self.n_tb, self.params)]
        if self._multi is None or not any(totals):  # the empty mix
            self.last_decoded = [0] * n
            return
        plan.pending(self._SKIP_RULES[self.skip], self.cb_pass.data_ptr(), self.ok.data_ptr(), self.cbgti.data_ptr(), d_new,
                     self.index.data_ptr(), self.count.data_ptr(), stream=stream)
        self._count_host.copy_(self.count, non_blocking=True)
        torch.cuda.current_stream(self.dev).synchronize()  # the one synchronisation of the mode: the decoder's batch sizes are host arguments
        counts = self.last_decoded = [int(x) for x in self._count_host.tolist()]
        if counts == totals:  # everything is pending: the step of skip=None
            self._multi(stream)
            return
        if self._dense is None:  # the dense arrays (the layout and totals of the full ones) and their decoder call, on first need
            tot, off = self.plan.totals, self.plan.offsets
            cw = torch.zeros(tot.cw, dtype=self.cw_llr.dtype, device=self.dev)
            c_hat = torch.zeros(tot.c_hat, dtype=torch.uint8, device=self.dev)
            iters = torch.zeros(tot.cb, dtype=torch.int32, device=self.dev)
            multi = MultiCall(self.codecs, [cw.data_ptr() + off[i].cw * self.llr_dtype.itemsize for i in range(n)], [0] * n,
                              [c_hat.data_ptr() + off[i].c_hat for i in range(n)], [iters.data_ptr() + 4 * off[i].cb for i in range(n)])
            self._dense = (cw, c_hat, iters, multi)
        cw, c_hat, iters, multi = self._dense
        if any(counts):
            plan.gather_cw(self.cw_llr.data_ptr(), self.index.data_ptr(), self.count.data_ptr(), cw.data_ptr(),
                           dtype=LLR_F16 if self.llr_dtype == np.float16 else LLR_F32, stream=stream)
            for i, k in enumerate(counts):
                multi.bt[i] = k
            multi(stream)
        plan.scatter_hard(c_hat.data_ptr(), iters.data_ptr(), self.index.data_ptr(), self.count.data_ptr(), self.c_hat.data_ptr(),
                          self.iters.data_ptr(), stream=stream)


class DeviceEncodeChain:
    """Batched NRLDPCEncoder.step on device tensors: CRC attachment + segmentation
    (nrldpc_crc_attach_dev), LDPC encoding (nrldpc_encode_dev), rate matching (nrldpc_rate_match_dev).
    The reference runs these as six interpreted stages per transport block (NRLDPCEncoder.m:60-67)."""

    def __init__(self, params: NRLDPC, device_id=0):
        import torch
        from ._capi import crc_attach_dev, rate_match_dev
        self.torch, self._crc_attach, self._rate_match = torch, crc_attach_dev, rate_match_dev
        params.validate()
        self.p = params
        self.dev = torch.device("cuda", device_id)
        self._device_id = device_id
        self._codec_code = (params.BG, params.Z_c)
        self._codec = Codec(params.BG, params.Z_c, max_iter=1, llr_dtype=np.float32, device_id=device_id)

    def close(self):
        if self._codec is not None:
            self._codec.close()
            self._codec = None

    def step(self, a):
        """a: torch uint8 tensor [n_tb][A] on the device -> g: uint8 [n_tb][G]."""
        torch, p = self.torch, self.p
        if a.dim() != 2 or a.shape[1] != p.A or a.dtype != torch.uint8 or not a.is_cuda:
            raise NRLDPCError("a should be a uint8 device tensor of shape [n_tb][A].")
        if a.device != self.dev:
            raise NRLDPCError("a lives on %s, this chain on %s." % (a.device, self.dev))
        with torch.cuda.device(self.dev):
            return self._step(a.contiguous())

    def _step(self, a):
        torch, d = self.torch, _derived(self)
        n_tb = a.shape[0]
        t = d.t
        s = torch.cuda.current_stream(self.dev).cuda_stream
        c = torch.empty((n_tb * d.C, d.K), dtype=torch.uint8, device=self.dev)
        self._crc_attach(t, a.data_ptr(), n_tb, c.data_ptr(), s)
        cw = torch.empty((n_tb * d.C, 2 * d.Z_c + d.N), dtype=torch.uint8, device=self.dev)
        if self._codec_code != (d.BG, d.Z_c):  # A changed on the parameter object: another code, another codec (see DeviceDecodeChain)
            self._codec.close()
            self._codec_code = (d.BG, d.Z_c)
            self._codec = Codec(d.BG, d.Z_c, max_iter=1, llr_dtype=np.float32, device_id=self._device_id)
        self._codec.encode_dev(c.data_ptr(), n_tb * d.C, cw.data_ptr(), s)
        g = torch.empty((n_tb, d.G), dtype=torch.uint8, device=self.dev)
        self._rate_match(t, cw.data_ptr(), n_tb, g.data_ptr(), s)
        return g


class MixedEncodeChain:
    """The transmit chain for a MIX of configurations, the twin of MixedDecodeChain: n parameter sets (NRLDPC objects) with n_tb[i]
    transport blocks each, from payload bits to rate-matched bits -- mix CRC attach (one launch), the existing encoder once per
    non-empty configuration, mix rate matching (one launch).  Every array is PACKED: configuration i's segment of the payload starts
    at plan.a_off[i] bytes, its code blocks, codeword bytes and rate-matched bits at plan.off[i].c_hat / .cw / .g, and each segment
    is exactly the array DeviceEncodeChain uses for that configuration; views() / pack() convert.  The packed g is the layout of
    MixedDecodeChain's "g" field for the same (params, n_tb).  One Codec per distinct (BG, Z_c) among the non-empty configurations.
    one_launch_encode=True: the encode stage is MixTxPlan.encode_all -- one launch from the plan's own tables -- and the chain builds
    no Codec; the result is the same bit for bit.  The default stays the per-configuration loop.
    For a Monte-Carlo loop the chain also draws the payload (draw(): one launch) and keeps the loop's per-block bookkeeping against it
    (outcome(): at most two launches), and step(a, rv_id=) sends a retransmission (harness.simulate_point_mixed)."""

    _SHAPES = {"a": lambda t, n: (n, t.A), "c": lambda t, n: (n * t.C, t.K), "cw": lambda t, n: (n * t.C, 2 * t.Z + t.N), "g": lambda t, n: (n, t.G)}
    _OFF = {"c": "c_hat", "cw": "cw", "g": "g"}

    def __init__(self, params, n_tb, device_id=0, one_launch_encode=False):
        import torch
        self.torch = torch
        params = list(params)
        for p in params:
            p.validate()
        self.params, self.n_tb = params, [int(x) for x in n_tb]
        self.dev = torch.device("cuda", device_id)
        self.device_id = device_id
        self.one_launch_encode = bool(one_launch_encode)
        self._codecs = {}
        self.codecs = []
        self.c = self.cw = self.g = None
        # the Monte-Carlo stages' arrays (draw() / outcome()), allocated on first use
        self.a = self.a_hat = self.done = self.good = self.all_new = self.left = self._left_host = self._draw = self._draw_host = self._draw_done = None
        self.plan = MixTxPlan(params, self.n_tb, device_id=device_id)
        self._own_rv = tuple(int(p.rv_id) for p in params)
        self._plans = {self._own_rv: self.plan}  # one plan per tuple of redundancy versions (only step(..., rv_id=) adds to it)
        try:
            for p, k in zip(params, self.n_tb):
                key = (p.BG, p.Z_c)
                if k and not self.one_launch_encode and key not in self._codecs:
                    self._codecs[key] = Codec(p.BG, p.Z_c, max_iter=1, llr_dtype=np.float32, device_id=device_id)
                self.codecs.append(self._codecs[key] if k and not self.one_launch_encode else None)
            tot = self.plan.totals()
            if any(self.n_tb):
                # the chain's own packed arrays, allocated once at the plan's totals (gaps stay zero: the kernels never touch them)
                self.c = torch.zeros(tot["c"], dtype=torch.uint8, device=self.dev)
                self.cw = torch.zeros(tot["cw"], dtype=torch.uint8, device=self.dev)
                self.g = torch.zeros(tot["g"], dtype=torch.uint8, device=self.dev)
        except Exception:
            self.close()
            raise

    def close(self):
        for c in getattr(self, "_codecs", {}).values():
            c.close()
        self._codecs, self.codecs = {}, []
        for plan in getattr(self, "_plans", {}).values():
            plan.close()
        self._plans = {}
        if getattr(self, "plan", None) is not None:
            self.plan.close()

    def _plan_for(self, rv_id):
        """The plan for a step's redundancy versions, as MixedDecodeChain._plan_for: None = the parameter objects' own, one int for every
        configuration, or a sequence of n.  rv_id only moves k_0 and no layout field depends on it, so the plans share the chain's
        packed arrays.  Built on first use from copies of the parameter objects, then cached."""
        n = len(self.params)
        if rv_id is None:
            key = self._own_rv
        elif isinstance(rv_id, (int, np.integer)):
            key = (int(rv_id),) * n
        else:
            key = tuple(int(x) for x in rv_id)
            if len(key) != n:
                raise NRLDPCError("rv_id should be None, one value or one value per configuration (%d), got %d." % (n, len(key)))
        if key not in self._plans:
            ps = []
            for p, rv in zip(self.params, key):
                q = copy.copy(p)
                q.rv_id = rv  # (UnsupportedParameters for a value outside 0 ... 3)
                ps.append(q)
            plan = MixTxPlan(ps, self.n_tb, device_id=self.device_id)
            same = plan.a_off == self.plan.a_off and all(getattr(a, f) == getattr(b, f) for a, b in zip(plan.off, self.plan.off) for f in MIX_FIELDS)
            if not same:
                plan.close()
                raise NRLDPCError("the layout of the plan for rv_id %r differs from the chain's: its packed arrays cannot be shared." % (key,))
            self._plans[key] = plan
        return self._plans[key]

    def _mc_arrays(self):
        torch, n = self.torch, len(self.params)
        if self.a is None:
            tot_a, tot_tb = self.plan.totals()["a"], self.plan.off[n].tb
            # zeroed once, so that the gaps read as zero; the kernels never touch a gap and never read done / a_hat on a first attempt
            self.a = torch.zeros(tot_a, dtype=torch.uint8, device=self.dev)
            self.a_hat = torch.zeros(tot_a, dtype=torch.uint8, device=self.dev)
            self.done = torch.zeros(tot_tb, dtype=torch.uint8, device=self.dev)
            self.good = torch.zeros(tot_tb, dtype=torch.uint8, device=self.dev)
            self.all_new = torch.ones(tot_tb, dtype=torch.uint8, device=self.dev)  # MixedDecodeChain.step's `new` for a batch's first attempt
            self.left = torch.zeros(n, dtype=torch.int32, device=self.dev)
            self._left_host = torch.zeros(n, dtype=torch.int32).pin_memory()
            self._draw = torch.zeros(16 * n, dtype=torch.uint8, device=self.dev)
            self._draw_host = torch.zeros(16 * n, dtype=torch.uint8).pin_memory()

    def draw(self, seed, first_block=0):
        """The payload draw of the Monte-Carlo loop for every configuration in ONE launch (MixTxPlan.payload): configuration i gets the
        blocks first_block_i ... first_block_i + n_tb[i] - 1 of seed_i (scalars broadcast), bit for bit harness.payload_bits.  The n draw
        records go up with one non-blocking copy from a pinned tensor.  Returns the packed payload a: the chain's own device array, valid
        until the next draw() -- what step() takes and outcome() compares with."""
        torch = self.torch
        d = self.plan.draws(seed, first_block)
        if self.g is None:  # the empty plan: nothing to do
            return torch.zeros(0, dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            self._mc_arrays()
            if self._draw_done is not None:
                self._draw_done.synchronize()  # the pinned records of the previous draw have gone up
            self._draw_host.copy_(torch.from_numpy(np.frombuffer(d, np.uint8)[:16 * self.plan.n]))
            self._draw.copy_(self._draw_host, non_blocking=True)
            self._draw_done = torch.cuda.Event()
            self._draw_done.record()
            self.plan.payload(self._draw.data_ptr(), self.a.data_ptr(), stream=torch.cuda.current_stream(self.dev).cuda_stream)
        return self.a

    def outcome(self, b_hat_packed, ok_packed, first, want_left=True):
        """The HARQ loop's bookkeeping of one attempt (MixTxPlan.outcome) against the payload of the last draw(): b_hat_packed and
        ok_packed are MixedDecodeChain.step's results for the same (params, n_tb); first = the batch's first attempt (the state of an
        earlier batch is not read: no memset).  Returns (good, left): good = the chain's packed uint8 device array in the "tb" layout,
        1 where a block is acknowledged and its latched a_hat equals a; left = per configuration the number of blocks not yet
        acknowledged, read back to the host (one small copy and the call's one synchronisation), or None with want_left=False."""
        torch, n = self.torch, len(self.params)
        if self.g is None:
            return torch.zeros(0, dtype=torch.uint8, device=self.dev), ([0] * n if want_left else None)
        if self.a is None:
            raise NRLDPCError("outcome() compares with the payload of draw(): call draw() first.")
        need_b, need_tb = self.plan.off[n].b_hat, self.plan.off[n].tb
        for x, dt, need, what in ((b_hat_packed, torch.uint8, need_b, "b_hat"), (ok_packed, torch.int32, need_tb, "ok")):
            if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.dtype != dt or not x.is_contiguous() or not x.is_cuda or x.device != self.dev or x.numel() < need:
                raise NRLDPCError("%s should be a contiguous 1-D %s tensor of at least %d elements on %s." % (what, dt, need, self.dev))
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev)
            self.plan.outcome(self.a.data_ptr(), b_hat_packed.data_ptr(), ok_packed.data_ptr(), first, self.a_hat.data_ptr(), self.done.data_ptr(),
                              self.good.data_ptr(), self.left.data_ptr() if want_left else None, stream=stream.cuda_stream)
            if not want_left:
                return self.good, None
            self._left_host.copy_(self.left, non_blocking=True)
            stream.synchronize()
        return self.good, [int(x) for x in self._left_host.tolist()]

    def _offset(self, i, field):
        return self.plan.a_off[i] if field == "a" else getattr(self.plan.off[i], self._OFF[field])

    def views(self, packed, field):
        """The per-configuration views of a packed tensor: field is one of "a", "c", "cw", "g"; view i has the shape of the
        single-configuration array ([n_tb][A], [n_tb*C][K], [n_tb*C][N_cw], [n_tb][G])."""
        if field not in self._SHAPES:
            raise NRLDPCError("unknown field %r (one of %s)" % (field, ", ".join(self._SHAPES)))
        flat = packed.reshape(-1)
        if flat.numel() < self.plan.totals()[field]:
            raise NRLDPCError("the packed %s array should hold at least %d elements." % (field, self.plan.totals()[field]))
        out = []
        for i, t in enumerate(self.plan.params):
            shape = self._SHAPES[field](t, self.n_tb[i])
            o = self._offset(i, field)
            out.append(flat[o: o + int(np.prod(shape, dtype=np.int64))].view(shape))
        return out

    def pack(self, tensors, field):
        """A packed uint8 tensor (gaps zero) from one tensor per configuration, each of the single-configuration shape for `field`."""
        tensors = list(tensors)
        if len(tensors) != len(self.params):
            raise NRLDPCError("one tensor per configuration expected (%d), got %d." % (len(self.params), len(tensors)))
        if field not in self._SHAPES:
            raise NRLDPCError("unknown field %r (one of %s)" % (field, ", ".join(self._SHAPES)))
        packed = self.torch.zeros(self.plan.totals()[field], dtype=self.torch.uint8, device=self.dev)
        for v, x in zip(self.views(packed, field), tensors):
            if tuple(x.shape) != tuple(v.shape) or x.dtype != self.torch.uint8:
                raise NRLDPCError("a uint8 tensor of shape %s expected for field %r, got %s %s." % (tuple(v.shape), field, tuple(x.shape), x.dtype))
            v.copy_(x)
        return packed

    def step(self, a_packed, rv_id=None):
        """a_packed: the packed payload bits, a contiguous 1-D uint8 device tensor of at least plan.totals()["a"] elements
        (pack(..., "a")); only bit 0 of a byte is read.  rv_id: the redundancy version(s) of this transmission -- None (the parameter
        objects' own, the chain's plan), one int for every configuration, or a sequence of n (a HARQ retransmission: _plan_for).
        Returns g_packed: the chain's own packed uint8 device array of rate-matched
        bits, valid until the next step (clone what must live longer); views(g_packed, "g")[i] is configuration i's [n_tb][G]."""
        torch, a = self.torch, a_packed
        plan = self.plan if rv_id is None else self._plan_for(rv_id)
        need = self.plan.totals()["a"]
        if not isinstance(a, torch.Tensor) or a.dim() != 1 or a.dtype != torch.uint8 or not a.is_contiguous():
            raise NRLDPCError("a should be a contiguous 1-D uint8 device tensor of at least %d elements." % need)
        if not a.is_cuda or a.device != self.dev:
            raise NRLDPCError("a lives on %s, this chain on %s." % (a.device, self.dev))
        if a.numel() < need:
            raise NRLDPCError("a should be a contiguous 1-D uint8 device tensor of at least %d elements, got %d." % (need, a.numel()))
        if self.g is None:  # the empty plan: nothing to do
            return torch.zeros(0, dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            plan.crc_attach(a.data_ptr(), self.c.data_ptr(), stream=stream)
            if self.one_launch_encode:
                plan.encode_all(self.c.data_ptr(), self.cw.data_ptr(), stream=stream)
            else:
                plan.encode(self.codecs, self.c.data_ptr(), self.cw.data_ptr(), stream=stream)
            plan.rate_match(self.cw.data_ptr(), self.g.data_ptr() if self.g.numel() else None, stream=stream)
        return self.g


class MixedChannel:
    """The channel leg for a MIX of configurations, between MixedEncodeChain and MixedDecodeChain: n parameter sets (NRLDPC objects)
    with n_tb[i] transport blocks each, from the packed rate-matched bits g to the packed LLRs g_tilde, each configuration at its own
    modulation order, Es/N0, seed and first symbol.  Fused by default -- MixChanPlan.awgn_llr, ONE launch, the symbols never exist in
    memory -- or, with separate=True, mapper -> noise (in place) -> demapper, one launch each; that route alone offers the decision
    methods and f16 LLRs.  Both arrays are PACKED in field g of the receive layout: configuration i's segment starts at
    plan.off[i].g and is exactly the [n_tb][G] array of the single-configuration calls; symbols ("sym": [n_sym][2] floats) and
    per-symbol values ("var": [n_sym]) start at plan.sym_off[i] symbols; views() / pack() convert.  The n operating-point records go
    up with one non-blocking copy from a pinned tensor per step."""

    _SHAPES = {"g": lambda t, n: (n, t.G), "sym": lambda t, n: (n * t.G // t.Q_m, 2), "var": lambda t, n: (n * t.G // t.Q_m,)}

    def __init__(self, params, n_tb, device_id=0):
        import torch
        self.torch = torch
        params = list(params)
        for p in params:
            p.validate()
        self.params, self.n_tb = params, [int(x) for x in n_tb]
        self.dev = torch.device("cuda", device_id)
        self.device_id = device_id
        self.g_tilde = self.tx = self._pt = self._pt_host = self._pt_done = None
        self._out = {}
        self.plan = MixChanPlan(params, self.n_tb, device_id=device_id)
        try:
            if any(self.n_tb):
                # the chain's own packed arrays, allocated once at the plan's totals (gaps stay zero: the kernels never touch them)
                self.g_tilde = torch.zeros(self.plan.totals()["g"], dtype=torch.float32, device=self.dev)
                self._pt = torch.zeros(32 * self.plan.n, dtype=torch.uint8, device=self.dev)
                self._pt_host = torch.zeros(32 * self.plan.n, dtype=torch.uint8).pin_memory()
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "plan", None) is not None:
            self.plan.close()

    def _offset(self, i, field):
        return self.plan.off[i].g if field == "g" else self.plan.sym_off[i] * (2 if field == "sym" else 1)

    def _total(self, field):
        tot = self.plan.totals()
        return tot["g"] if field == "g" else tot["sym"] * (2 if field == "sym" else 1)

    def views(self, packed, field):
        """The per-configuration views of a packed tensor: field is one of "g" (bits, LLRs or hard bits: [n_tb][G]), "sym" (a float
        tensor of 2 * totals()["sym"] elements: [n_sym][2]) and "var" (one value per symbol: [n_sym])."""
        if field not in self._SHAPES:
            raise NRLDPCError("unknown field %r (one of %s)" % (field, ", ".join(self._SHAPES)))
        flat = packed.reshape(-1)
        if flat.numel() < self._total(field):
            raise NRLDPCError("the packed %s array should hold at least %d elements." % (field, self._total(field)))
        out = []
        for i, t in enumerate(self.plan.params):
            shape = self._SHAPES[field](t, self.n_tb[i])
            o = self._offset(i, field)
            out.append(flat[o: o + int(np.prod(shape, dtype=np.int64))].view(shape))
        return out

    def pack(self, tensors, field):
        """A packed tensor (gaps zero, the tensors' dtype) from one tensor per configuration, each of the shape views() gives for `field`."""
        tensors = list(tensors)
        if len(tensors) != len(self.params):
            raise NRLDPCError("one tensor per configuration expected (%d), got %d." % (len(self.params), len(tensors)))
        if field not in self._SHAPES:
            raise NRLDPCError("unknown field %r (one of %s)" % (field, ", ".join(self._SHAPES)))
        dtype = tensors[0].dtype if tensors else self.torch.uint8
        packed = self.torch.zeros(self._total(field), dtype=dtype, device=self.dev)
        for v, x in zip(self.views(packed, field), tensors):
            if tuple(x.shape) != tuple(v.shape) or x.dtype != dtype:
                raise NRLDPCError("a %s tensor of shape %s expected for field %r, got %s %s." % (dtype, tuple(v.shape), field, tuple(x.shape), x.dtype))
            v.copy_(x)
        return packed

    def step(self, g_packed, EsN0_dB, seed, first_symbol=0, separate=False, method="llr", llr_dtype=None):
        """g_packed: the packed rate-matched bits, a contiguous 1-D uint8 device tensor of at least plan.totals()["g"] elements
        (MixedEncodeChain.step's result); only bit 0 of a byte is read.  EsN0_dB, seed, first_symbol: one value per configuration, or
        scalars, which broadcast (first_symbol: the global index of the configuration's first symbol -- noise is a function of
        (seed, global symbol index) alone).  Returns the packed g_tilde in the layout of MixedDecodeChain's "g" field: the chain's own
        device array, valid until the next step (clone what must live longer) -- f32 LLRs, or with separate=True what `method`
        ("llr", "approx", "hard"; names as in demod_method_code) and llr_dtype (torch.float32 / torch.float16) ask for; "hard" gives
        uint8 bits."""
        torch, g = self.torch, g_packed
        code = demod_method_code(method)
        if llr_dtype not in (None, torch.float32, torch.float16):
            raise NRLDPCError("llr_dtype should be torch.float32 or torch.float16, got %s." % (llr_dtype,))
        if not separate and (code != demod_method_code("llr") or llr_dtype not in (None, torch.float32)):
            raise NRLDPCError("the fused route gives exact f32 LLRs; decision methods and f16 need separate=True.")
        pts = self.plan.points(EsN0_dB, seed, first_symbol)
        need = self.plan.totals()["g"]
        if not isinstance(g, torch.Tensor) or g.dim() != 1 or g.dtype != torch.uint8 or not g.is_contiguous():
            raise NRLDPCError("g should be a contiguous 1-D uint8 device tensor of at least %d elements." % need)
        if not g.is_cuda or g.device != self.dev:
            raise NRLDPCError("g lives on %s, this chain on %s." % (g.device, self.dev))
        if g.numel() < need:
            raise NRLDPCError("g should be a contiguous 1-D uint8 device tensor of at least %d elements, got %d." % (need, g.numel()))
        hard = code == demod_method_code("hard")
        out_dtype = torch.uint8 if hard else (llr_dtype or torch.float32)
        if self.g_tilde is None:  # the empty plan: nothing to do
            return torch.zeros(0, dtype=out_dtype, device=self.dev)
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            if self._pt_done is not None:
                self._pt_done.synchronize()  # the pinned records of the previous step have gone up
            self._pt_host.copy_(torch.from_numpy(np.frombuffer(pts, np.uint8)[:32 * self.plan.n]))
            self._pt.copy_(self._pt_host, non_blocking=True)
            self._pt_done = torch.cuda.Event()
            self._pt_done.record()
            if not separate:
                self.plan.awgn_llr(g.data_ptr(), self._pt.data_ptr(), self.g_tilde.data_ptr(), stream=stream)
                return self.g_tilde
            if self.tx is None:
                self.tx = torch.zeros(2 * self.plan.totals()["sym"], dtype=torch.float32, device=self.dev)
            out = self.g_tilde if out_dtype == torch.float32 else self._out.get(out_dtype)
            if out is None:
                out = self._out[out_dtype] = torch.zeros(need, dtype=out_dtype, device=self.dev)
            self.plan.modulate(g.data_ptr(), self.tx.data_ptr(), stream=stream)
            self.plan.awgn(self.tx.data_ptr(), self._pt.data_ptr(), self.tx.data_ptr(), stream=stream)
            self.plan.demodulate(self.tx.data_ptr(), self._pt.data_ptr(), out.data_ptr(), method=method,
                                 out_dtype=LLR_F16 if out_dtype == torch.float16 else LLR_F32, stream=stream)
        return out

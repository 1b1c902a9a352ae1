"""ctypes binding of the C ABI declared in include/nrldpc.h (libnrldpc_hip.so).

There is no CPU implementation behind this module: if the shared object is missing it is built
with hipcc; if that is impossible, import fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

OK, ERR_UNSUPPORTED, ERR_ARG, ERR_HIP, ERR_NOMEM = 0, 1, 2, 3, 4
LLR_F32, LLR_F16, LLR_F64 = 0, 1, 2
MIX_SKIP_UNSCHEDULED, MIX_SKIP_SETTLED = 1, 2  # NRLDPC_MIX_SKIP_* of include/nrldpc.h


class UnsupportedParameters(ValueError):
    """Mirror of the MATLAB identifier 'ldpc_3gpp_matlab:UnsupportedParameters'
    (e.g. NRLDPC.m:240-294, get_3gpp_set_index.m:10)."""
    identifier = "ldpc_3gpp_matlab:UnsupportedParameters"


class NRLDPCError(RuntimeError):
    """Mirror of the MATLAB identifier 'ldpc_3gpp_matlab:Error' (e.g. NRLDPCDecoder.m:149)."""
    identifier = "ldpc_3gpp_matlab:Error"


ABI_VERSION = 6  # NRLDPC_ABI_VERSION of include/nrldpc.h
LAYERS_ALL, LAYERS_AUTO = 0, -1  # NRLDPC_LAYERS_*
# NRLDPC_ALG_*: the layered offset-normalised min-sum kernels (default), or flooding sum-product -- the reference's
# comm.LDPCDecoder (NRLDPCDecoder.m:120) -- selected per handle by nrldpc_set_algorithm
ALG_MIN_SUM, ALG_SUM_PRODUCT = 0, 1
ALGORITHMS = {"min-sum": ALG_MIN_SUM, "sum-product": ALG_SUM_PRODUCT}


def algorithm_code(algorithm):
    """NRLDPC_ALG_* of an algorithm name ("min-sum" / "sum-product"); UnsupportedParameters for anything else (no device call)."""
    try:
        return ALGORITHMS[algorithm]
    except (KeyError, TypeError):
        raise UnsupportedParameters("unknown decoding algorithm %r (one of %s)" % (algorithm, ", ".join(ALGORITHMS))) from None


def algorithm_name(code):
    return {v: k for k, v in ALGORITHMS.items()}[int(code)]


class Cfg(C.Structure):
    """nrldpc_cfg; struct_size is filled in by the constructor (positional arguments start at bg)."""
    _fields_ = [("struct_size", C.c_uint32), ("bg", C.c_int32), ("Z", C.c_int32), ("n_layers", C.c_int32), ("max_iter", C.c_int32),
                ("early_term", C.c_int32), ("alpha", C.c_float), ("llr_scale", C.c_int32),
                ("llr_dtype", C.c_int32), ("device_id", C.c_int32), ("max_batch", C.c_int32), ("beta", C.c_float),
                ("crc_poly", C.c_uint32), ("crc_len", C.c_int32), ("crc_bits", C.c_int32)]


def _cfg_init(self, *args, **kw):
    C.Structure.__init__(self, C.sizeof(Cfg), *args, **kw)


Cfg.__init__ = _cfg_init


class Dims(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nrows", C.c_int32), ("ncols", C.c_int32), ("kb", C.c_int32), ("i_ls", C.c_int32),
                ("K", C.c_int32), ("N_cw", C.c_int32), ("n_layers", C.c_int32), ("alpha", C.c_float), ("beta", C.c_float)]


class CwOut(C.Structure):
    """nrldpc_cw_out: the extra outputs of nrldpc_decode_cw[_dev], each left out by a null pointer; struct_size is filled in by the
    constructor (positional arguments start at cw_packed)."""
    _fields_ = [("struct_size", C.c_uint32), ("cw_packed", C.c_void_p), ("unsatisfied", C.c_void_p), ("checks_packed", C.c_void_p)]


def _cw_out_init(self, *args, **kw):
    C.Structure.__init__(self, C.sizeof(CwOut), *args, **kw)


CwOut.__init__ = _cw_out_init

MAX_C = 160


class TbParams(C.Structure):
    _fields_ = [("bg", C.c_int32), ("Z", C.c_int32), ("A", C.c_int32), ("B", C.c_int32), ("C", C.c_int32),
                ("K", C.c_int32), ("K_prime", C.c_int32), ("N", C.c_int32), ("N_cb", C.c_int32), ("k_0", C.c_int32),
                ("Q_m", C.c_int32), ("G", C.c_int32), ("tb_crc_len", C.c_int32), ("cb_crc_len", C.c_int32),
                ("E_r", C.c_int32 * MAX_C)]


def tb_params(p):
    """nrldpc_tb_params from an NRLDPC parameter object (NRLDPC.m:297-543)."""
    if p.C > MAX_C:
        raise UnsupportedParameters("more than %d code blocks" % MAX_C)
    t = TbParams(p.BG, p.Z_c, p.A, p.B, p.C, p.K, int(p.K_prime), p.N, p.N_cb, p.k_0, p.Q_m, p.G,
                 p.transport_block_L, p.code_block_L)
    for r, e in enumerate(p.E_r):
        t.E_r[r] = e
    return t


class MixOffsets(C.Structure):
    """nrldpc_mix_offsets: element offsets of one configuration inside the packed arrays of a mix plan (entry [n]: the totals)."""
    _fields_ = [(k, C.c_int64) for k in ("g", "harq", "cw", "c_hat", "cb", "b_hat", "tb")]


MIX_FIELDS = tuple(k for k, _ in MixOffsets._fields_)


class MixChanPoint(C.Structure):
    """nrldpc_mix_chan_point: the operating point of one configuration of a channel plan (32 bytes; a device array of n of them goes
    to every stage call).  variance = N0 is what the stand-alone noise and demapper stages read; sigma = sqrt(N0/2) and inv_n0 = 1/N0
    what the fused stage reads; seed is the Philox key, first_symbol the global index of the configuration's local symbol 0."""
    _fields_ = [("variance", C.c_float), ("sigma", C.c_float), ("inv_n0", C.c_float), ("reserved", C.c_uint32),
                ("seed", C.c_uint64), ("first_symbol", C.c_uint64)]

class MixDraw(C.Structure):
    """nrldpc_mix_draw: the payload draw of one configuration of a transmit plan (16 bytes; a device array of n of them goes to
    nrldpc_mix_tx_payload_dev): the splitmix64 seed and the global index of the configuration's transport block 0."""
    _fields_ = [("seed", C.c_uint64), ("first_block", C.c_uint64)]


EXPORTS = ["nrldpc_awgn_llr_dev", "nrldpc_rate_recover_dev",  "nrldpc_crc_check_dev", "nrldpc_crc_check_harq_dev", "nrldpc_crc_attach_dev", "nrldpc_rate_match_dev", "nrldpc_create", "nrldpc_destroy", "nrldpc_get_dims", "nrldpc_decode", "nrldpc_decode_dev",
           "nrldpc_decode_multi_dev", "nrldpc_quantise_llr", "nrldpc_encode", "nrldpc_encode_dev", "nrldpc_set_timing", "nrldpc_last_kernel_ms",
           "nrldpc_set_index", "nrldpc_lifting_size", "nrldpc_default_rule", "nrldpc_strerror", "nrldpc_last_error",
           "nrldpc_version", "nrldpc_build_id", "nrldpc_kernel_id", "nrldpc_pool_create", "nrldpc_pool_decode", "nrldpc_pool_last_split",
           "nrldpc_pool_destroy", "nrldpc_pool_decode_dev", "nrldpc_pool_size", "nrldpc_abi_version", "nrldpc_decode_packed",
           "nrldpc_set_layers", "nrldpc_set_llr_dtype", "nrldpc_last_layers", "nrldpc_count_layers", "nrldpc_pool_set_layers", "nrldpc_pool_decode_packed",
           "nrldpc_decode_packed_layers", "nrldpc_pool_set_timing", "nrldpc_pool_last_kernel_ms", "nrldpc_last_host_phases", "nrldpc_payload_bits_dev",
           "nrldpc_set_algorithm", "nrldpc_get_algorithm", "nrldpc_pool_set_algorithm", "nrldpc_decode_cw", "nrldpc_decode_cw_dev",
           "nrldpc_modulate_dev", "nrldpc_demodulate_dev", "nrldpc_rate_recover_ex_dev", "nrldpc_awgn_dev",
           "nrldpc_mix_layout", "nrldpc_mix_create", "nrldpc_mix_destroy", "nrldpc_mix_rate_recover_dev", "nrldpc_mix_crc_check_dev",
           "nrldpc_mix_rate_recover_harq_dev", "nrldpc_mix_crc_check_harq_dev",
           "nrldpc_mix_pending_dev", "nrldpc_mix_gather_cw_dev", "nrldpc_mix_scatter_hard_dev",
           "nrldpc_mix_tx_layout", "nrldpc_mix_tx_create", "nrldpc_mix_tx_destroy", "nrldpc_mix_tx_crc_attach_dev", "nrldpc_mix_tx_encode_dev",
           "nrldpc_mix_tx_rate_match_dev", "nrldpc_mix_tx_encode_all_dev",
           "nrldpc_mix_chan_layout", "nrldpc_mix_chan_point_set", "nrldpc_mix_chan_create", "nrldpc_mix_chan_destroy",
           "nrldpc_mix_chan_awgn_llr_dev", "nrldpc_mix_chan_modulate_dev", "nrldpc_mix_chan_awgn_dev", "nrldpc_mix_chan_demodulate_dev",
           "nrldpc_mix_tx_payload_dev", "nrldpc_mix_tx_outcome_dev"]

_lib = None


def lib_path():
    return _build.LIB


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7; if this
    library pulled in /opt/rocm's copy first, torch would later find "No HIP GPUs".  Importing torch
    first (when it is installed) makes both use the same runtime; without torch nothing happens."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load():
    """Load (building first if needed) libnrldpc_hip.so.  Raises if it cannot be produced."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    path = _build.LIB
    if os.environ.get("NRLDPC_LIB"):
        pass  # an explicitly selected library (kernel experiments): used as it is
    elif _build._stale():  # missing, or built from other sources than the tree holds now (content hash)
        import fcntl
        with open(path + ".lock", "w") as lk:  # several ranks of one node may get here at once: one builds, the rest wait
            fcntl.flock(lk, fcntl.LOCK_EX)
            if _build._stale():
                path = _build.build_lib()
    L = C.CDLL(path)
    # the ABI revision first, before any symbol that only this revision exports is touched: a stale library (NRLDPC_LIB skips
    # the build-id check) must fail with this message, not with a ctypes AttributeError on a missing symbol
    abi = getattr(L, "nrldpc_abi_version", None)
    have = abi() if abi is not None else 0
    if have != ABI_VERSION:
        raise RuntimeError("libnrldpc_hip.so speaks ABI revision %s, this binding %d"
                           % (have if abi is not None else "< 3 (no nrldpc_abi_version)", ABI_VERSION))
    L.nrldpc_build_id.restype = C.c_char_p
    L.nrldpc_kernel_id.restype = C.c_char_p
    if not os.environ.get("NRLDPC_LIB") and L.nrldpc_build_id().decode() != _build.source_id():
        raise RuntimeError("libnrldpc_hip.so (build %s) does not match the sources in the tree (%s) and could not be "
                           "rebuilt" % (L.nrldpc_build_id().decode(), _build.source_id()))
    vp, i32 = C.c_void_p, C.c_int32
    L.nrldpc_create.argtypes = [C.POINTER(Cfg), C.POINTER(vp)]
    L.nrldpc_destroy.argtypes = [vp]
    L.nrldpc_destroy.restype = None
    L.nrldpc_get_dims.argtypes = [vp, C.POINTER(Dims)]
    L.nrldpc_decode.argtypes = [vp, vp, i32, vp, vp, vp]
    L.nrldpc_decode_packed.argtypes = [vp, vp, i32, vp, vp]
    L.nrldpc_decode_packed_layers.argtypes = [vp, vp, i32, vp, vp, i32]
    L.nrldpc_pool_set_timing.argtypes = [vp, i32]
    L.nrldpc_last_host_phases.argtypes = [vp, C.POINTER(C.c_double)]
    L.nrldpc_payload_bits_dev.argtypes = [C.c_uint64, C.c_uint64, i32, i32, vp, vp]
    L.nrldpc_pool_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nrldpc_decode_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.nrldpc_decode_cw.argtypes = [vp, vp, i32, vp, vp, C.POINTER(CwOut)]
    L.nrldpc_decode_cw_dev.argtypes = [vp, vp, i32, vp, vp, C.POINTER(CwOut), vp]
    L.nrldpc_quantise_llr.argtypes = [vp, vp, C.c_int64, i32, i32]
    L.nrldpc_decode_multi_dev.argtypes = [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), C.POINTER(vp), vp]
    L.nrldpc_encode.argtypes = [vp, vp, i32, vp]
    L.nrldpc_encode_dev.argtypes = [vp, vp, i32, vp, vp]
    L.nrldpc_rate_recover_dev.argtypes = [C.POINTER(TbParams), vp, i32, vp, vp, i32, vp]
    if hasattr(L, "nrldpc_rate_recover_ex_dev"):  # added without a revision bump: a library selected with NRLDPC_LIB may lack it
        L.nrldpc_rate_recover_ex_dev.argtypes = [C.POINTER(TbParams), vp, i32, i32, vp, i32, vp, i32, vp]
    L.nrldpc_crc_check_dev.argtypes = [C.POINTER(TbParams), vp, i32, vp, vp, vp, vp]
    L.nrldpc_crc_check_harq_dev.argtypes = [C.POINTER(TbParams), vp, i32, vp, vp, vp, vp, i32, vp]
    L.nrldpc_awgn_llr_dev.argtypes = [vp, C.c_int64, i32, C.c_float, C.c_uint64, C.c_uint64, vp, vp]
    L.nrldpc_modulate_dev.argtypes = [vp, C.c_int64, i32, vp, vp]
    L.nrldpc_demodulate_dev.argtypes = [vp, C.c_int64, i32, i32, C.c_float, vp, vp, i32, vp]
    if hasattr(L, "nrldpc_awgn_dev"):  # added without a revision bump: a library selected with NRLDPC_LIB may lack it
        L.nrldpc_awgn_dev.argtypes = [vp, C.c_int64, C.c_float, vp, C.c_uint64, C.c_uint64, vp, vp]
    if hasattr(L, "nrldpc_mix_create"):  # the mixed-batch stages, added without a revision bump: a library selected with NRLDPC_LIB may lack them
        L.nrldpc_mix_layout.argtypes = [i32, C.POINTER(TbParams), C.POINTER(i32), C.POINTER(MixOffsets)]
        L.nrldpc_mix_create.argtypes = [i32, C.POINTER(TbParams), C.POINTER(i32), i32, C.POINTER(vp)]
        L.nrldpc_mix_destroy.argtypes = [vp]
        L.nrldpc_mix_destroy.restype = None
        L.nrldpc_mix_rate_recover_dev.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp]
        L.nrldpc_mix_crc_check_dev.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(L, "nrldpc_mix_rate_recover_harq_dev"):  # the HARQ / CBGTI forms, again without a revision bump
        L.nrldpc_mix_rate_recover_harq_dev.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, vp]
        L.nrldpc_mix_crc_check_harq_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "nrldpc_mix_pending_dev"):  # HARQ steps that decode only the pending code blocks, again without a revision bump
        L.nrldpc_mix_pending_dev.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.nrldpc_mix_gather_cw_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.nrldpc_mix_scatter_hard_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "nrldpc_mix_tx_create"):  # the transmit side of the mixed batches, again without a revision bump
        L.nrldpc_mix_tx_layout.argtypes = [i32, C.POINTER(TbParams), C.POINTER(i32), C.POINTER(C.c_int64)]
        L.nrldpc_mix_tx_create.argtypes = [i32, C.POINTER(TbParams), C.POINTER(i32), i32, C.POINTER(vp)]
        L.nrldpc_mix_tx_destroy.argtypes = [vp]
        L.nrldpc_mix_tx_destroy.restype = None
        L.nrldpc_mix_tx_crc_attach_dev.argtypes = [vp, vp, vp, vp]
        L.nrldpc_mix_tx_encode_dev.argtypes = [vp, C.POINTER(vp), vp, vp, vp]
        L.nrldpc_mix_tx_rate_match_dev.argtypes = [vp, vp, vp, vp]
    if hasattr(L, "nrldpc_mix_tx_encode_all_dev"):  # the encode stage in one launch, found by symbol like the rest
        L.nrldpc_mix_tx_encode_all_dev.argtypes = [vp, vp, vp, vp]
    if hasattr(L, "nrldpc_mix_tx_payload_dev"):  # the Monte-Carlo loop's payload draw and outcome latch, found by symbol like the rest
        L.nrldpc_mix_tx_payload_dev.argtypes = [vp, vp, vp, vp]
        L.nrldpc_mix_tx_outcome_dev.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    if hasattr(L, "nrldpc_mix_chan_create"):  # the channel leg of the mixed batches, found by symbol like the rest
        L.nrldpc_mix_chan_layout.argtypes = [i32, C.POINTER(TbParams), C.POINTER(i32), C.POINTER(C.c_int64)]
        L.nrldpc_mix_chan_point_set.argtypes = [C.c_float, C.c_uint64, C.c_uint64, C.POINTER(MixChanPoint)]
        L.nrldpc_mix_chan_create.argtypes = [i32, C.POINTER(TbParams), C.POINTER(i32), i32, C.POINTER(vp)]
        L.nrldpc_mix_chan_destroy.argtypes = [vp]
        L.nrldpc_mix_chan_destroy.restype = None
        L.nrldpc_mix_chan_awgn_llr_dev.argtypes = [vp, vp, vp, vp, vp]
        L.nrldpc_mix_chan_modulate_dev.argtypes = [vp, vp, vp, vp]
        L.nrldpc_mix_chan_awgn_dev.argtypes = [vp, vp, vp, vp, vp, vp]
        L.nrldpc_mix_chan_demodulate_dev.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp]
    L.nrldpc_crc_attach_dev.argtypes = [C.POINTER(TbParams), vp, i32, vp, vp]
    L.nrldpc_rate_match_dev.argtypes = [C.POINTER(TbParams), vp, i32, vp, vp]
    L.nrldpc_pool_create.argtypes = [C.POINTER(Cfg), C.POINTER(i32), i32, i32, C.POINTER(vp)]
    L.nrldpc_pool_decode.argtypes = [vp, vp, i32, vp, vp]
    L.nrldpc_pool_decode_packed.argtypes = [vp, vp, i32, vp, vp]
    L.nrldpc_pool_set_layers.argtypes = [vp, i32]
    L.nrldpc_set_layers.argtypes = [vp, i32]
    L.nrldpc_set_llr_dtype.argtypes = [vp, i32]
    L.nrldpc_set_algorithm.argtypes = [vp, i32]
    L.nrldpc_get_algorithm.argtypes = [vp, C.POINTER(i32)]
    L.nrldpc_pool_set_algorithm.argtypes = [vp, i32]
    L.nrldpc_last_layers.argtypes = [vp, C.POINTER(i32)]
    L.nrldpc_count_layers.argtypes = [i32, i32, vp, i32, i32]
    L.nrldpc_pool_last_split.argtypes = [vp, C.POINTER(i32)]
    L.nrldpc_pool_decode_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp), C.POINTER(vp)]
    L.nrldpc_pool_size.argtypes = [vp]
    L.nrldpc_pool_destroy.argtypes = [vp]
    L.nrldpc_pool_destroy.restype = None
    L.nrldpc_set_timing.argtypes = [vp, i32]
    L.nrldpc_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nrldpc_set_index.argtypes = [i32]
    L.nrldpc_lifting_size.argtypes = [i32, i32]
    L.nrldpc_default_rule.argtypes = [i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for f in ("nrldpc_strerror", "nrldpc_last_error", "nrldpc_version", "nrldpc_build_id"):
        getattr(L, f).restype = C.c_char_p
    L.nrldpc_strerror.argtypes = [i32]
    _lib = L
    return L


def check(rc):
    if rc == OK:
        return
    L = load()
    msg = (L.nrldpc_last_error() or b"").decode() or L.nrldpc_strerror(rc).decode()
    if rc == ERR_UNSUPPORTED:
        raise UnsupportedParameters(msg)
    raise NRLDPCError(msg)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


_NP2DT = {np.dtype(np.float32): LLR_F32, np.dtype(np.float16): LLR_F16, np.dtype(np.float64): LLR_F64}


class Codec:
    """One (BG, Z) LDPC coding core on one GPU: the object that takes the place of
    comm.LDPCDecoder / comm.LDPCEncoder in the reference (NRLDPCDecoder.m:120, NRLDPCEncoder.m:49)."""

    def __init__(self, bg, Z, max_iter=50, n_layers=0, early_term=True, alpha=0.0, llr_scale=0,
                 llr_dtype=np.float32, device_id=0, max_batch=0, beta=0.0, crc=None, algorithm="min-sum"):
        """alpha = 0: the library picks the check-node rule (alpha, beta) by rate (nrldpc_default_rule);
        otherwise message magnitude = max(alpha*min - beta, 0), beta in LLR units.
        n_layers: 0 = every row, 4..rows, or LAYERS_AUTO (-1) = read off each call's LLRs; set_layers() changes it between calls.
        crc = (poly with its x^L term, L, K'): the CRC-aided stop (nrldpc_cfg.early_term = 2) on the first K' information bits.
        algorithm: "min-sum" (default) or "sum-product" (flooding, the reference's comm.LDPCDecoder; alpha, beta and
        llr_scale are not read; not with crc); set_algorithm() changes it between calls."""
        alg = algorithm_code(algorithm)
        L = load()
        self._lib = L
        self._h = C.c_void_p()
        self.llr_dtype = np.dtype(llr_dtype)
        cfg = Cfg(int(bg), int(Z), int(n_layers), int(max_iter), 2 if crc else int(bool(early_term)), float(alpha),
                  int(llr_scale), _NP2DT[self.llr_dtype], int(device_id), int(max_batch), float(beta),
                  *((int(crc[0]), int(crc[1]), int(crc[2])) if crc else (0, 0, 0)))
        check(L.nrldpc_create(C.byref(cfg), C.byref(self._h)))
        d = Dims(C.sizeof(Dims))
        check(L.nrldpc_get_dims(self._h, C.byref(d)))
        self.bg, self.Z = int(bg), int(Z)
        self.K, self.N_cw, self.kb, self.ncols, self.nrows = d.K, d.N_cw, d.kb, d.ncols, d.nrows
        self.i_ls, self.n_layers = d.i_ls, d.n_layers
        self.alpha, self.beta = float(d.alpha), float(d.beta)  # resolved check-node rule
        if alg != ALG_MIN_SUM:
            try:
                self.set_algorithm(algorithm)
            except Exception:
                self.close()
                raise

    def set_algorithm(self, algorithm):
        """nrldpc_set_algorithm: "min-sum" or "sum-product" for the calls that follow; no device work."""
        check(self._lib.nrldpc_set_algorithm(self._h, algorithm_code(algorithm)))

    @property
    def algorithm(self):
        """The handle's decoding algorithm ("min-sum" / "sum-product"), as the library reports it."""
        a = C.c_int32()
        check(self._lib.nrldpc_get_algorithm(self._h, C.byref(a)))
        return algorithm_name(a.value)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nrldpc_destroy(self._h)
            self._h = C.c_void_p()

    def set_layers(self, n_layers):
        """nrldpc_set_layers: active layer count of the calls that follow (0 all, 4..rows, LAYERS_AUTO); no device work."""
        check(self._lib.nrldpc_set_layers(self._h, int(n_layers)))
        d = Dims(C.sizeof(Dims))
        check(self._lib.nrldpc_get_dims(self._h, C.byref(d)))
        self.n_layers, self.alpha, self.beta = d.n_layers, float(d.alpha), float(d.beta)

    def set_llr_dtype(self, llr_dtype):
        """nrldpc_set_llr_dtype: element type of the arrays the calls that follow hand over (np.float32 / float16 / float64)."""
        dt = np.dtype(llr_dtype)
        check(self._lib.nrldpc_set_llr_dtype(self._h, _NP2DT[dt]))
        self.llr_dtype = dt

    def last_layers(self):
        """nrldpc_last_layers: the count the most recent decode call ran with (what LAYERS_AUTO found)."""
        n = C.c_int32()
        check(self._lib.nrldpc_last_layers(self._h, C.byref(n)))
        return int(n.value)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-pointer entry points (numpy arrays) -------------------------------------------------
    def decode(self, llr, want_iters=False, want_app=False, out=None):
        """out: a (B, K) uint8 array to decode into.  A caller that decodes batch after batch should pass one: a fresh 35 MB
        array per call is mmap'd, page-faulted by sixteen copy threads and munmap'd every time -- 3-5 ms on top of a 4 ms call and
        20-30 ms every few calls (profiles/r05_host_stall.txt; what round 4 recorded as a stall of this entry point)."""
        llr = np.ascontiguousarray(llr, self.llr_dtype)
        if llr.size % self.N_cw:
            raise NRLDPCError("llr should hold a whole number of codewords of length %d" % self.N_cw)
        B = llr.size // self.N_cw
        if out is not None and (out.shape != (B, self.K) or out.dtype != np.uint8 or not out.flags.c_contiguous):
            raise NRLDPCError("out should be a C-contiguous uint8 array of shape (%d, %d)" % (B, self.K))
        hard = out if out is not None else np.empty((B, self.K), np.uint8)
        iters = np.empty(B, np.int32) if want_iters else None
        app = np.empty((B, self.N_cw), np.float32) if want_app else None
        check(self._lib.nrldpc_decode(self._h, _ptr(llr), B, _ptr(hard), _ptr(iters), _ptr(app)))
        out = (hard,)
        if want_iters:
            out += (iters,)
        if want_app:
            out += (app,)
        return out[0] if len(out) == 1 else out

    def decode_cw(self, llr, want_checks=False):
        """nrldpc_decode_cw: (hard, iters, cw, unsatisfied[, checks]) -- decode()'s hard decisions and iteration counts, the whole
        codeword's hard decisions cw [B][N_cw] (uint8; cw[:, :K] == hard), the number of active parity checks that fail on them
        (0 = converged) and, with want_checks, every check as a uint8 [B][nrows*Z] (row l, shift z at l*Z + z; inactive rows 0)."""
        llr = np.ascontiguousarray(llr, self.llr_dtype)
        if llr.size % self.N_cw:
            raise NRLDPCError("llr should hold a whole number of codewords of length %d" % self.N_cw)
        B = llr.size // self.N_cw
        nchk = self.nrows * self.Z
        hard = np.empty((B, self.K), np.uint8)
        iters = np.empty(B, np.int32)
        cw = np.empty((B, (self.N_cw + 7) // 8), np.uint8)
        unsat = np.empty(B, np.int32)
        chk = np.empty((B, (nchk + 7) // 8), np.uint8) if want_checks else None
        o = CwOut(cw.ctypes.data, unsat.ctypes.data, chk.ctypes.data if want_checks else None)
        check(self._lib.nrldpc_decode_cw(self._h, _ptr(llr), B, _ptr(hard), _ptr(iters), C.byref(o)))
        out = (hard, iters, np.unpackbits(cw, axis=1, bitorder="little")[:, :self.N_cw], unsat)
        if want_checks:
            out += (np.unpackbits(chk, axis=1, bitorder="little")[:, :nchk],)
        return out

    def decode_packed(self, llr, want_iters=False, out=None, n_layers=None):
        """nrldpc_decode_packed: hard decisions as [B][ceil(K/8)] bytes, bit k of a codeword in byte k // 8 at bit k % 8
        (np.unpackbits(out, axis=1, bitorder="little")[:, :K] gives decode()'s array).  out: see decode().
        n_layers: the active layer count of THIS call only (nrldpc_decode_packed_layers: 0 all, 4..rows, LAYERS_AUTO); the
        handle's own count is untouched."""
        llr = np.ascontiguousarray(llr, self.llr_dtype)
        if llr.size % self.N_cw:
            raise NRLDPCError("llr should hold a whole number of codewords of length %d" % self.N_cw)
        B = llr.size // self.N_cw
        if out is not None and (out.shape != (B, (self.K + 7) // 8) or out.dtype != np.uint8 or not out.flags.c_contiguous):
            raise NRLDPCError("out should be a C-contiguous uint8 array of shape (%d, %d)" % (B, (self.K + 7) // 8))
        packed = out if out is not None else np.empty((B, (self.K + 7) // 8), np.uint8)
        iters = np.empty(B, np.int32) if want_iters else None
        if n_layers is None:
            check(self._lib.nrldpc_decode_packed(self._h, _ptr(llr), B, _ptr(packed), _ptr(iters)))
        else:
            check(self._lib.nrldpc_decode_packed_layers(self._h, _ptr(llr), B, _ptr(packed), _ptr(iters), int(n_layers)))
        return (packed, iters) if want_iters else packed

    def encode(self, info):
        info = np.ascontiguousarray(info, np.uint8)
        if info.size % self.K:
            raise NRLDPCError("info should hold a whole number of blocks of length %d" % self.K)
        B = info.size // self.K
        cw = np.empty((B, self.N_cw), np.uint8)
        check(self._lib.nrldpc_encode(self._h, _ptr(info), B, _ptr(cw)))
        return cw

    # -- device-pointer entry points (raw addresses, e.g. torch.Tensor.data_ptr()) ----------------
    def decode_dev(self, d_llr, batch, d_hard, d_iters=None, d_app=None, stream=0):
        check(self._lib.nrldpc_decode_dev(self._h, _ptr(d_llr), int(batch), _ptr(d_hard), _ptr(d_iters),
                                          _ptr(d_app), C.c_void_p(stream)))

    def decode_cw_dev(self, d_llr, batch, d_hard, d_iters=None, d_cw_packed=None, d_unsatisfied=None, d_checks_packed=None, stream=0):
        """nrldpc_decode_cw_dev on raw device addresses: d_cw_packed [batch][ceil(N_cw/8)], d_unsatisfied [batch] int32, d_checks_packed
        [batch][ceil(nrows*Z/8)], each optional (at least one); bit i of a row in byte i // 8 at bit i % 8."""
        o = CwOut(*[int(x) if x else None for x in (d_cw_packed, d_unsatisfied, d_checks_packed)])
        check(self._lib.nrldpc_decode_cw_dev(self._h, _ptr(d_llr), int(batch), _ptr(d_hard), _ptr(d_iters), C.byref(o), C.c_void_p(stream)))

    def encode_dev(self, d_info, batch, d_cw, stream=0):
        check(self._lib.nrldpc_encode_dev(self._h, _ptr(d_info), int(batch), _ptr(d_cw), C.c_void_p(stream)))

    def set_timing(self, on=True):
        check(self._lib.nrldpc_set_timing(self._h, int(on)))

    def last_host_phases(self):
        """nrldpc_last_host_phases as a dict (ms of the caller's thread in each phase of the last large host-pointer call), or None."""
        out = (C.c_double * 10)()
        if self._lib.nrldpc_last_host_phases(self._h, out) != 0:
            return None
        return {"chunks": int(out[0]), "codewords_per_chunk": int(out[1]), "layers": int(out[2]), "scan_ms": out[3],
                "copy_quantise_ms": out[4], "launch_enqueue_ms": out[5], "wait_device_ms": out[6], "copy_out_ms": out[7],
                "copy_threads_numa_node": int(out[8]), "caller_cpu": int(out[9])}

    def last_kernel_ms(self):
        ms = C.c_float()
        check(self._lib.nrldpc_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


class CodecPool:
    """One node, several GPUs (nrldpc_pool_*): one handle and one host thread per entry of device_ids, the batch cut
    into len(device_ids) * chunks_per_device chunks pulled from a queue -- no collective, results identical to one
    Codec.decode call.  A device ordinal may repeat (several logical shards on one GPU)."""

    def __init__(self, bg, Z, device_ids, chunks_per_device=3, max_iter=50, n_layers=0, early_term=True, alpha=0.0,
                 beta=0.0, llr_scale=0, llr_dtype=np.float32, algorithm="min-sum"):
        alg = algorithm_code(algorithm)
        L = load()
        self._lib = L
        self.llr_dtype = np.dtype(llr_dtype)
        self.device_ids = [int(d) for d in device_ids]
        cfg = Cfg(int(bg), int(Z), int(n_layers), int(max_iter), int(bool(early_term)), float(alpha), int(llr_scale),
                  _NP2DT[self.llr_dtype], 0, 0, float(beta))
        ids = (C.c_int32 * len(self.device_ids))(*self.device_ids)
        self._p = C.c_void_p()
        check(L.nrldpc_pool_create(C.byref(cfg), ids, len(self.device_ids), int(chunks_per_device), C.byref(self._p)))
        if alg != ALG_MIN_SUM:
            try:
                self.set_algorithm(algorithm)
            except Exception:
                self.close()
                raise
        rows, cols, kb = {1: (46, 68, 22), 2: (42, 52, 10)}[int(bg)]
        self.K, self.N_cw = kb * int(Z), cols * int(Z)

    def decode(self, llr, want_iters=False):
        llr = np.ascontiguousarray(llr, self.llr_dtype)
        if llr.size % self.N_cw:
            raise NRLDPCError("llr should hold a whole number of codewords of length %d" % self.N_cw)
        B = llr.size // self.N_cw
        hard = np.empty((B, self.K), np.uint8)
        iters = np.empty(B, np.int32) if want_iters else None
        check(self._lib.nrldpc_pool_decode(self._p, _ptr(llr), B, _ptr(hard), _ptr(iters)))
        return (hard, iters) if want_iters else hard

    def decode_packed(self, llr, want_iters=False):
        """nrldpc_pool_decode_packed: as decode(), hard decisions bit-packed [B][ceil(K/8)] (Codec.decode_packed)."""
        llr = np.ascontiguousarray(llr, self.llr_dtype)
        if llr.size % self.N_cw:
            raise NRLDPCError("llr should hold a whole number of codewords of length %d" % self.N_cw)
        B = llr.size // self.N_cw
        packed = np.empty((B, (self.K + 7) // 8), np.uint8)
        iters = np.empty(B, np.int32) if want_iters else None
        check(self._lib.nrldpc_pool_decode_packed(self._p, _ptr(llr), B, _ptr(packed), _ptr(iters)))
        return (packed, iters) if want_iters else packed

    def set_algorithm(self, algorithm):
        """nrldpc_pool_set_algorithm: "min-sum" or "sum-product" for every shard."""
        check(self._lib.nrldpc_pool_set_algorithm(self._p, algorithm_code(algorithm)))

    def set_layers(self, n_layers):
        """nrldpc_pool_set_layers (LAYERS_AUTO: found once per call over the whole batch)."""
        check(self._lib.nrldpc_pool_set_layers(self._p, int(n_layers)))

    def decode_dev(self, d_llr, batch, d_hard, d_iters=None):
        """nrldpc_pool_decode_dev: shard i decodes batch[i] codewords at device address d_llr[i] (memory of
        device_ids[i]) into d_hard[i]; returns when every shard's stream is idle.  No host copies.  Work already queued on a
        shard's device when the call is made (e.g. the torch kernel still producing d_llr[i]) completes before the decoder
        starts: each shard synchronizes its device first (nrldpc.h)."""
        n = len(self.device_ids)
        if not (len(d_llr) == len(batch) == len(d_hard) == n):
            raise NRLDPCError("one entry per shard expected")
        vp = C.c_void_p
        a_llr = (vp * n)(*[vp(int(x)) for x in d_llr])
        a_hard = (vp * n)(*[vp(int(x)) for x in d_hard])
        a_b = (C.c_int32 * n)(*[int(b) for b in batch])
        a_it = (vp * n)(*[vp(int(x) if x else None) for x in d_iters]) if d_iters is not None else None
        check(self._lib.nrldpc_pool_decode_dev(self._p, a_llr, a_b, a_hard, a_it))

    def set_timing(self, on=True):
        """nrldpc_pool_set_timing: event pairs around every shard's decode kernel, on the shard's own launch stream."""
        check(self._lib.nrldpc_pool_set_timing(self._p, int(on)))

    def last_kernel_ms(self):
        """Kernel time of every shard's last launch, ms (nrldpc_pool_last_kernel_ms; 0 for a shard without work)."""
        out = (C.c_float * len(self.device_ids))()
        check(self._lib.nrldpc_pool_last_kernel_ms(self._p, out))
        return [float(v) for v in out]

    def last_split(self):
        """Codewords each shard decoded in the last call (uneven under early termination: faster shards pull more)."""
        out = (C.c_int32 * len(self.device_ids))()
        check(self._lib.nrldpc_pool_last_split(self._p, out))
        return list(out)

    def close(self):
        if getattr(self, "_p", None) and self._p.value:
            self._lib.nrldpc_pool_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiCall:
    """The argument arrays of one nrldpc_decode_multi_dev call, built once: what a C caller holds anyway.  call(stream) is the
    library call and nothing else (marshalling 5 x 100 values through ctypes costs about as much as the call's host side)."""

    def __init__(self, codecs, d_llr, batch, d_hard, d_iters=None):
        n = self.n = len(codecs)
        vp = C.c_void_p
        self.codecs = list(codecs)  # keeps the handles alive
        self.hs = (vp * n)(*[c._h for c in codecs])
        self.llr = (vp * n)(*[int(x) for x in d_llr])
        self.hard = (vp * n)(*[int(x) for x in d_hard])
        self.its = (vp * n)(*[int(x) if x else None for x in d_iters]) if d_iters is not None else None
        self.bt = (C.c_int32 * n)(*[int(b) for b in batch])
        self.fn = load().nrldpc_decode_multi_dev

    def __call__(self, stream=0):
        check(self.fn(self.n, self.hs, self.llr, self.bt, self.hard, self.its, C.c_void_p(stream)))


def decode_multi_dev(codecs, d_llr, batch, d_hard, d_iters=None, stream=0):
    """One launch per base graph, LLR type and workgroup class for a mix of configurations (nrldpc_decode_multi_dev):
    codecs[i] decodes batch[i] codewords at device address d_llr[i] into d_hard[i] (and d_iters[i])."""
    MultiCall(codecs, d_llr, batch, d_hard, d_iters)(stream)


def rate_recover_dev(p, d_g_tilde, n_tb, d_harq, d_cw_llr, out_dtype=LLR_F32, stream=0, in_dtype=LLR_F32, harq_dtype=LLR_F32):
    """nrldpc_rate_recover_dev on raw device addresses (p: NRLDPC parameter object or TbParams).  in_dtype / harq_dtype: the element
    types at d_g_tilde and d_harq (LLR_F32 / LLR_F16); anything but f32 for both goes to nrldpc_rate_recover_ex_dev, which also
    clamps what it converts to f16 (include/nrldpc.h)."""
    t = p if isinstance(p, TbParams) else tb_params(p)
    L = load()
    if int(in_dtype) == LLR_F32 and (d_harq is None or int(harq_dtype) == LLR_F32):
        check(L.nrldpc_rate_recover_dev(C.byref(t), _ptr(d_g_tilde), int(n_tb), _ptr(d_harq), _ptr(d_cw_llr),
                                        int(out_dtype), C.c_void_p(stream)))
        return
    if not hasattr(L, "nrldpc_rate_recover_ex_dev"):
        raise NRLDPCError("%s has no nrldpc_rate_recover_ex_dev: f16 demodulator LLRs and the f16 HARQ buffer need a library "
                          "built from this tree (NRLDPC_LIB selects an older one?)" % lib_path())
    check(L.nrldpc_rate_recover_ex_dev(C.byref(t), _ptr(d_g_tilde), int(in_dtype), int(n_tb), _ptr(d_harq), int(harq_dtype),
                                       _ptr(d_cw_llr), int(out_dtype), C.c_void_p(stream)))


def _mix_args(params, n_tb):
    """(n, TbParams array, int32 array) of a mix: params are NRLDPC parameter objects or TbParams."""
    params, n_tb = list(params), [int(x) for x in n_tb]
    if len(params) != len(n_tb):
        raise NRLDPCError("a mix needs one transport-block count per parameter set (%d sets, %d counts)" % (len(params), len(n_tb)))
    n = len(params)
    ts = (TbParams * max(n, 1))()
    for i, p in enumerate(params):
        C.memmove(C.byref(ts[i]), C.byref(p if isinstance(p, TbParams) else tb_params(p)), C.sizeof(TbParams))
    return n, ts, (C.c_int32 * max(n, 1))(*n_tb)


def _mix_lib():
    L = load()
    if not hasattr(L, "nrldpc_mix_create"):
        raise NRLDPCError("%s has no nrldpc_mix_create: mixed transport-block batches need a library built from this tree "
                          "(NRLDPC_LIB selects an older one?)" % lib_path())
    return L


def mix_layout(params, n_tb):
    """nrldpc_mix_layout: the n + 1 offset records (MixOffsets) of the packed arrays of a mix; entry [n] holds the totals.
    Host function, no device needed."""
    n, ts, nt = _mix_args(params, n_tb)
    off = (MixOffsets * (n + 1))()
    check(_mix_lib().nrldpc_mix_layout(n, ts, nt, off))
    return list(off)


class MixPlan:
    """nrldpc_mix_*: an immutable plan for a batch whose transport blocks differ in (BG, A, G, Q_m, rv_id, LBRM, C) -- n parameter
    sets (NRLDPC objects or TbParams) with n_tb[i] transport blocks each.  It owns the device-side tables and defines one packed
    layout (.offsets, n + 1 MixOffsets records in elements; entry [n]: the totals) for every array of the receive chain;
    rate_recover() and crc_check() are one launch each, whatever n, and so are their HARQ / CBGTI forms rate_recover_harq() and
    crc_check_harq() (per-transport-block "new HARQ process" flags, per-code-block CBGTI flags, sticky cb_pass, b_hat in/out).
    rv_id only moves k_0 and no layout field depends on it: a HARQ receiver holds one plan per redundancy version over the same
    packed arrays.  Streams may share a plan."""

    def __init__(self, params, n_tb, device_id=0):
        self._h = C.c_void_p()
        self._lib = L = _mix_lib()
        self.n, ts, nt = _mix_args(params, n_tb)
        self.n_tb = [int(x) for x in n_tb]
        self.device_id = int(device_id)
        off = (MixOffsets * (self.n + 1))()
        check(L.nrldpc_mix_layout(self.n, ts, nt, off))
        self.offsets = list(off)
        self.params = [ts[i] for i in range(self.n)]
        self._ts = ts  # (the records above are views of this array)
        check(L.nrldpc_mix_create(self.n, ts, nt, self.device_id, C.byref(self._h)))

    @property
    def totals(self):
        """Elements to allocate for each packed array (MixOffsets)."""
        return self.offsets[self.n]

    def rate_recover(self, d_g_tilde, d_harq, d_cw_llr, in_dtype=LLR_F32, harq_dtype=LLR_F32, out_dtype=LLR_F32, stream=0):
        """nrldpc_mix_rate_recover_dev on raw device addresses of the packed arrays (d_harq None: no soft buffer)."""
        check(self._lib.nrldpc_mix_rate_recover_dev(self._h, _ptr(d_g_tilde), int(in_dtype), _ptr(d_harq), int(harq_dtype),
                                                    _ptr(d_cw_llr), int(out_dtype), C.c_void_p(stream)))

    def crc_check(self, d_c_hat, d_b_hat, d_ok, d_cb_pass=None, stream=0):
        """nrldpc_mix_crc_check_dev on raw device addresses of the packed arrays."""
        check(self._lib.nrldpc_mix_crc_check_dev(self._h, _ptr(d_c_hat), _ptr(d_b_hat), _ptr(d_ok), _ptr(d_cb_pass), C.c_void_p(stream)))

    def _harq_fn(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise NRLDPCError("%s has no %s: HARQ / CBGTI state on mixed transport-block batches needs a library built from this "
                              "tree (NRLDPC_LIB selects an older one?)" % (lib_path(), name))
        return fn

    def rate_recover_harq(self, d_g_tilde, d_harq, d_cw_llr, d_new=None, in_dtype=LLR_F32, harq_dtype=LLR_F32, out_dtype=LLR_F32, stream=0):
        """nrldpc_mix_rate_recover_harq_dev on raw device addresses: d_harq is required; d_new (uint8, one per transport block in
        the packed tb layout; None: no block is new) marks the transport blocks whose buffer rows count as +0.0 and are not read."""
        check(self._harq_fn("nrldpc_mix_rate_recover_harq_dev")(self._h, _ptr(d_g_tilde), int(in_dtype), _ptr(d_harq), int(harq_dtype),
                                                                _ptr(d_cw_llr), int(out_dtype), _ptr(d_new), C.c_void_p(stream)))

    def crc_check_harq(self, d_c_hat, d_b_hat, d_ok, d_cb_pass, d_cbgti=None, d_new=None, stream=0):
        """nrldpc_mix_crc_check_harq_dev on raw device addresses: d_b_hat and d_cb_pass are in/out; d_cbgti (uint8, one per code
        block in the packed cb layout; None: all 1) and d_new as in rate_recover_harq."""
        check(self._harq_fn("nrldpc_mix_crc_check_harq_dev")(self._h, _ptr(d_c_hat), _ptr(d_b_hat), _ptr(d_ok), _ptr(d_cb_pass),
                                                             _ptr(d_cbgti), _ptr(d_new), C.c_void_p(stream)))

    def _skip_fn(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise NRLDPCError("%s has no %s: HARQ steps that decode only the pending code blocks need a library built from this "
                              "tree (NRLDPC_LIB selects an older one?)" % (lib_path(), name))
        return fn

    def pending(self, rule, d_cb_pass, d_ok, d_cbgti, d_new, d_index, d_count, stream=0):
        """nrldpc_mix_pending_dev on raw device addresses: rule = MIX_SKIP_UNSCHEDULED (d_cb_pass and d_ok are not read) or
        MIX_SKIP_SETTLED (both required; d_ok is the previous step's ok array); d_cbgti / d_new as in crc_check_harq, nullable.
        Leaves in d_index (int32, packed cb layout) the local rows of each configuration's pending code blocks, ascending, and in
        d_count (int32 [n]) how many there are."""
        check(self._skip_fn("nrldpc_mix_pending_dev")(self._h, int(rule), _ptr(d_cb_pass), _ptr(d_ok), _ptr(d_cbgti), _ptr(d_new),
                                                      _ptr(d_index), _ptr(d_count), C.c_void_p(stream)))

    def gather_cw(self, d_cw_llr, d_index, d_count, d_cw_dense, dtype=LLR_F32, stream=0):
        """nrldpc_mix_gather_cw_dev on raw device addresses: dense row j of configuration i = row d_index[off[i].cb + j] of the packed
        codeword LLRs, bit for bit, for j < d_count[i]; the dense array has the layout and size of the full one."""
        check(self._skip_fn("nrldpc_mix_gather_cw_dev")(self._h, _ptr(d_cw_llr), int(dtype), _ptr(d_index), _ptr(d_count), _ptr(d_cw_dense),
                                                        C.c_void_p(stream)))

    def scatter_hard(self, d_c_hat_dense, d_iters_dense, d_index, d_count, d_c_hat, d_iters=None, stream=0):
        """nrldpc_mix_scatter_hard_dev on raw device addresses: row d_index[off[i].cb + j] of d_c_hat (in/out) = dense row j; rows of
        blocks that are not pending keep what they held, their d_iters entries become 0."""
        check(self._skip_fn("nrldpc_mix_scatter_hard_dev")(self._h, _ptr(d_c_hat_dense), _ptr(d_iters_dense), _ptr(d_index), _ptr(d_count),
                                                           _ptr(d_c_hat), _ptr(d_iters), C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nrldpc_mix_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _mix_tx_lib():
    L = _mix_lib()
    if not hasattr(L, "nrldpc_mix_tx_create"):
        raise NRLDPCError("%s has no nrldpc_mix_tx_create: the transmit side of mixed transport-block batches needs a library built "
                          "from this tree (NRLDPC_LIB selects an older one?)" % lib_path())
    return L


def mix_tx_layout(params, n_tb):
    """nrldpc_mix_tx_layout: the n + 1 byte offsets of the packed payload array a of a mix ([n]: the total).  Every other transmit
    array uses mix_layout's fields: code blocks = c_hat, codeword bytes = cw, rate-matched bits = g.  Host function, no device needed."""
    n, ts, nt = _mix_args(params, n_tb)
    a_off = (C.c_int64 * (n + 1))()
    check(_mix_tx_lib().nrldpc_mix_tx_layout(n, ts, nt, a_off))
    return [int(x) for x in a_off]


class MixTxPlan:
    """nrldpc_mix_tx_*: the transmit twin of MixPlan -- an immutable plan for a batch whose transport blocks differ in
    (BG, A, G, Q_m, rv_id, LBRM, C).  .a_off: the n + 1 byte offsets of the packed payload array; .off: the receive layout's n + 1
    MixOffsets records, of which the transmit arrays use c_hat (code blocks), cw (codeword bytes) and g (rate-matched bits);
    totals(): {"a", "c", "cw", "g"} -> elements to allocate.  crc_attach() and rate_match() are one launch each, whatever n; encode()
    launches the existing encoder once per non-empty configuration, encode_all() is the same stage in one launch from the plan's own
    tables.  Streams may share a plan."""

    def __init__(self, params, n_tb, device_id=0):
        self._h = C.c_void_p()
        self._lib = L = _mix_tx_lib()
        self.n, ts, nt = _mix_args(params, n_tb)
        self.n_tb = [int(x) for x in n_tb]
        self.device_id = int(device_id)
        a_off = (C.c_int64 * (self.n + 1))()
        check(L.nrldpc_mix_tx_layout(self.n, ts, nt, a_off))
        self.a_off = [int(x) for x in a_off]
        off = (MixOffsets * (self.n + 1))()
        check(L.nrldpc_mix_layout(self.n, ts, nt, off))
        self.off = list(off)
        self.params = [ts[i] for i in range(self.n)]
        self._ts = ts  # (the records above are views of this array)
        check(L.nrldpc_mix_tx_create(self.n, ts, nt, self.device_id, C.byref(self._h)))

    def totals(self):
        """Elements (bytes) to allocate for each packed transmit array."""
        t = self.off[self.n]
        return {"a": self.a_off[self.n], "c": t.c_hat, "cw": t.cw, "g": t.g}

    def crc_attach(self, d_a, d_c, stream=0):
        """nrldpc_mix_tx_crc_attach_dev on raw device addresses of the packed arrays."""
        check(self._lib.nrldpc_mix_tx_crc_attach_dev(self._h, _ptr(d_a), _ptr(d_c), C.c_void_p(stream)))

    def encode(self, codecs, d_c, d_cw, stream=0):
        """nrldpc_mix_tx_encode_dev: codecs[i] (a Codec, or None for an empty configuration) encodes configuration i's code blocks."""
        codecs = list(codecs)
        if len(codecs) != self.n:
            raise NRLDPCError("one codec per configuration expected (%d), got %d." % (self.n, len(codecs)))
        hs = (C.c_void_p * max(self.n, 1))(*[c._h if c is not None else None for c in codecs])
        check(self._lib.nrldpc_mix_tx_encode_dev(self._h, hs, _ptr(d_c), _ptr(d_cw), C.c_void_p(stream)))

    def encode_all(self, d_c, d_cw, stream=0):
        """nrldpc_mix_tx_encode_all_dev: the encode stage in ONE launch from the plan's own tables, no codecs; leaves cw as encode()
        leaves it."""
        if not hasattr(self._lib, "nrldpc_mix_tx_encode_all_dev"):
            raise NRLDPCError("%s has no nrldpc_mix_tx_encode_all_dev: the one-launch mixed encoder needs a library built from this "
                              "tree (NRLDPC_LIB selects an older one?)" % lib_path())
        check(self._lib.nrldpc_mix_tx_encode_all_dev(self._h, _ptr(d_c), _ptr(d_cw), C.c_void_p(stream)))

    def rate_match(self, d_cw, d_g, stream=0):
        """nrldpc_mix_tx_rate_match_dev on raw device addresses of the packed arrays."""
        check(self._lib.nrldpc_mix_tx_rate_match_dev(self._h, _ptr(d_cw), _ptr(d_g), C.c_void_p(stream)))

    def _mc_fn(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise NRLDPCError("%s has no %s: the Monte-Carlo stages of mixed transport-block batches need a library built from this "
                              "tree (NRLDPC_LIB selects an older one?)" % (lib_path(), name))
        return fn

    def draws(self, seed, first_block=0):
        """The n nrldpc_mix_draw records of one payload() call as a ctypes array (host only), as MixChanPlan.points makes the channel's:
        seed and first_block are sequences of n values or scalars, which broadcast.  Copy the array to the device (16 * n bytes;
        np.frombuffer(d, np.uint8) views it -- one non-blocking copy from a pinned tensor) and hand its address to payload()."""
        def spread(x, what):
            xs = list(x) if hasattr(x, "__len__") else [x] * self.n
            if len(xs) != self.n:
                raise NRLDPCError("one %s per configuration expected (%d), got %d." % (what, self.n, len(xs)))
            return xs
        sd, fb = spread(seed, "seed"), spread(first_block, "first_block")
        d = (MixDraw * max(self.n, 1))()
        for i in range(self.n):
            if not 0 <= int(fb[i]) < 1 << 64:
                raise NRLDPCError("first_block should lie in [0, 2^64)")
            d[i].seed, d[i].first_block = int(sd[i]) % (1 << 64), int(fb[i])
        return d

    def payload(self, d_draw, d_a, stream=0):
        """nrldpc_mix_tx_payload_dev on raw device addresses: the payload draw of every configuration in ONE launch; segment i of the
        packed a becomes what payload_bits_dev(seed_i, first_block_i, n_tb[i], A_i) leaves."""
        check(self._mc_fn("nrldpc_mix_tx_payload_dev")(self._h, _ptr(d_draw), _ptr(d_a), C.c_void_p(stream)))

    def outcome(self, d_a, d_b_hat, d_ok, first, d_a_hat, d_done, d_good, d_left=None, stream=0):
        """nrldpc_mix_tx_outcome_dev on raw device addresses: the HARQ loop's bookkeeping of one attempt for every transport block of
        the mix -- a_hat (packed a layout) latched from b_hat where the block's CRC holds for the first time, done |= ok, good = done
        and a_hat == a (bytes, packed tb layout), d_left[i] (int32 [n], optional) = blocks of configuration i not yet done.  first:
        the batch's first attempt -- the old contents of d_done and d_a_hat are not read."""
        check(self._mc_fn("nrldpc_mix_tx_outcome_dev")(self._h, _ptr(d_a), _ptr(d_b_hat), _ptr(d_ok), 1 if first else 0, _ptr(d_a_hat),
                                                      _ptr(d_done), _ptr(d_good), _ptr(d_left), C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nrldpc_mix_tx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def crc_check_dev(p, d_c_hat, n_tb, d_b_hat, d_ok, d_cb_pass=None, stream=0):
    """nrldpc_crc_check_dev on raw device addresses."""
    t = p if isinstance(p, TbParams) else tb_params(p)
    check(load().nrldpc_crc_check_dev(C.byref(t), _ptr(d_c_hat), int(n_tb), _ptr(d_b_hat), _ptr(d_ok),
                                      _ptr(d_cb_pass), C.c_void_p(stream)))


def crc_check_harq_dev(p, d_c_hat, n_tb, d_b_hat, d_ok, d_cb_pass, cbgti_flags=None, keep_b_hat=True, stream=0):
    """nrldpc_crc_check_harq_dev: the CRC stage with the reference's HARQ / CBGTI state (NRLDPCDecoder.m:283-316,337).
    d_b_hat and d_cb_pass are in/out device buffers owned by the caller; cbgti_flags is a host sequence of C flags."""
    t = p if isinstance(p, TbParams) else tb_params(p)
    flags = None
    if cbgti_flags is not None:
        flags = (C.c_uint8 * t.C)(*[1 if f else 0 for f in cbgti_flags])
    check(load().nrldpc_crc_check_harq_dev(C.byref(t), _ptr(d_c_hat), int(n_tb), _ptr(d_b_hat), _ptr(d_ok),
                                           _ptr(d_cb_pass), flags, int(bool(keep_b_hat)), C.c_void_p(stream)))


def awgn_llr_dev(d_g, n_bits, Q_m, EsN0_dB, seed, first_symbol, d_g_tilde, stream=0):
    """nrldpc_awgn_llr_dev: modulation + AWGN + exact LLRs in one kernel (plot_BLER_vs_SNR.m:130-132)."""
    check(load().nrldpc_awgn_llr_dev(_ptr(d_g), int(n_bits), int(Q_m), float(EsN0_dB), int(seed), int(first_symbol),
                                     _ptr(d_g_tilde), C.c_void_p(stream)))


# NRLDPC_DEMOD_*: the three DecisionMethod values of the reference's NRDemodulator.m:10
DEMOD_LLR, DEMOD_APPROX_LLR, DEMOD_HARD = 0, 1, 2
DEMOD_METHODS = {"llr": DEMOD_LLR, "approx": DEMOD_APPROX_LLR, "hard": DEMOD_HARD,
                 "Log-likelihood ratio": DEMOD_LLR, "Approximate log-likelihood ratio": DEMOD_APPROX_LLR, "Hard decision": DEMOD_HARD}


def demod_method_code(method):
    """NRLDPC_DEMOD_* of a method name ("llr" / "approx" / "hard" or the reference's DecisionMethod strings);
    UnsupportedParameters for anything else (no device call)."""
    try:
        return DEMOD_METHODS[method]
    except (KeyError, TypeError):
        raise UnsupportedParameters("unknown decision method %r (one of %s)" % (method, ", ".join(DEMOD_METHODS))) from None


def modulate_dev(d_g, n_bits, Q_m, d_tx, stream=0):
    """nrldpc_modulate_dev: n_bits bit bytes at d_g -> n_bits / Q_m complex64 symbols at d_tx (NRModulator.m:73-81)."""
    check(load().nrldpc_modulate_dev(_ptr(d_g), int(n_bits), int(Q_m), _ptr(d_tx), C.c_void_p(stream)))


def demodulate_dev(d_rx, n_sym, Q_m, d_out, method="llr", variance=1.0, d_variance=None, out_dtype=LLR_F32, stream=0):
    """nrldpc_demodulate_dev: n_sym complex64 symbols at d_rx -> n_sym * Q_m LLRs of out_dtype (LLR_F32 / LLR_F16; positive = bit 0)
    at d_out, or hard-bit bytes for method "hard" (NRDemodulator.m:76-96).  variance: the complex noise variance N0;
    d_variance: a device array of n_sym floats, one per symbol, that replaces it."""
    check(load().nrldpc_demodulate_dev(_ptr(d_rx), int(n_sym), int(Q_m), demod_method_code(method), float(variance),
                                       _ptr(d_variance), _ptr(d_out), int(out_dtype), C.c_void_p(stream)))


def awgn_dev(d_tx, n_sym, d_rx, variance=1.0, d_variance=None, seed=0, first_symbol=0, stream=None):
    """nrldpc_awgn_dev: n_sym complex64 symbols at d_tx + complex Gaussian noise -> d_rx (which may be d_tx): the noise
    nrldpc_awgn_llr_dev draws for the same (seed, first_symbol), first_symbol being the global index of the first symbol.
    variance: the complex noise variance N0; d_variance: a device array of n_sym floats, one per symbol, that replaces it."""
    L = load()
    if not hasattr(L, "nrldpc_awgn_dev"):
        raise NRLDPCError("%s has no nrldpc_awgn_dev: the stand-alone AWGN stage needs a library built from this tree "
                          "(NRLDPC_LIB selects an older one?)" % lib_path())
    if not 0 <= int(first_symbol) < 1 << 64:
        raise NRLDPCError("first_symbol should lie in [0, 2^64)")
    check(L.nrldpc_awgn_dev(_ptr(d_tx), int(n_sym), float(variance), _ptr(d_variance), int(seed) % (1 << 64), int(first_symbol),
                            _ptr(d_rx), C.c_void_p(stream or 0)))


def _mix_chan_lib():
    L = _mix_lib()
    if not hasattr(L, "nrldpc_mix_chan_create"):
        raise NRLDPCError("%s has no nrldpc_mix_chan_create: the channel leg of mixed transport-block batches needs a library built "
                          "from this tree (NRLDPC_LIB selects an older one?)" % lib_path())
    return L


def mix_chan_layout(params, n_tb):
    """nrldpc_mix_chan_layout: the n + 1 offsets, in SYMBOLS, of the packed symbol array of a mix ([n]: the total).  Symbol s of
    configuration i is the float pair at 2 * (sym_off[i] + s), its per-symbol variance the float at sym_off[i] + s.  Bits and LLRs use
    mix_layout's field g.  Host function, no device needed."""
    n, ts, nt = _mix_args(params, n_tb)
    sym_off = (C.c_int64 * (n + 1))()
    check(_mix_chan_lib().nrldpc_mix_chan_layout(n, ts, nt, sym_off))
    return [int(x) for x in sym_off]


class MixChanPlan:
    """nrldpc_mix_chan_*: the channel leg between MixTxPlan and MixPlan -- an immutable plan for a batch whose transport blocks differ
    in modulation order.  .sym_off: the n + 1 offsets of the packed symbol array, in symbols; .off: the receive layout's n + 1
    MixOffsets records, of which the bits and the LLRs use g; totals(): {"g", "sym"} -> elements to allocate (2 floats per symbol).
    points() makes the n operating-point records a stage call reads from DEVICE memory.  awgn_llr() (fused), modulate(), awgn() and
    demodulate() are one launch each, whatever n.  Streams may share a plan."""

    def __init__(self, params, n_tb, device_id=0):
        self._h = C.c_void_p()
        self._lib = L = _mix_chan_lib()
        self.n, ts, nt = _mix_args(params, n_tb)
        self.n_tb = [int(x) for x in n_tb]
        self.device_id = int(device_id)
        sym_off = (C.c_int64 * (self.n + 1))()
        check(L.nrldpc_mix_chan_layout(self.n, ts, nt, sym_off))
        self.sym_off = [int(x) for x in sym_off]
        off = (MixOffsets * (self.n + 1))()
        check(L.nrldpc_mix_layout(self.n, ts, nt, off))
        self.off = list(off)
        self.params = [ts[i] for i in range(self.n)]
        self._ts = ts  # (the records above are views of this array)
        check(L.nrldpc_mix_chan_create(self.n, ts, nt, self.device_id, C.byref(self._h)))

    def totals(self):
        """Elements to allocate: "g" bits / LLRs / hard bits, "sym" symbols (two floats each; one float each in a variance array)."""
        return {"g": self.off[self.n].g, "sym": self.sym_off[self.n]}

    def points(self, EsN0_dB, seed, first_symbol=0):
        """The n nrldpc_mix_chan_point records of one call as a ctypes array (nrldpc_mix_chan_point_set per configuration; host only):
        EsN0_dB, seed and first_symbol are sequences of n values or scalars, which broadcast.  Copy the array to the device (it is
        32 * n bytes; np.frombuffer(pts, np.uint8) views it) and hand its address to the stage calls."""
        def spread(x, what):
            xs = list(x) if hasattr(x, "__len__") else [x] * self.n
            if len(xs) != self.n:
                raise NRLDPCError("one %s per configuration expected (%d), got %d." % (what, self.n, len(xs)))
            return xs
        es, sd, fs = spread(EsN0_dB, "EsN0_dB"), spread(seed, "seed"), spread(first_symbol, "first_symbol")
        pts = (MixChanPoint * max(self.n, 1))()
        for i in range(self.n):
            if not 0 <= int(fs[i]) < 1 << 64:
                raise NRLDPCError("first_symbol should lie in [0, 2^64)")
            check(self._lib.nrldpc_mix_chan_point_set(float(es[i]), int(sd[i]) % (1 << 64), int(fs[i]), C.byref(pts[i])))
        return pts

    def awgn_llr(self, d_g, d_pt, d_g_tilde, stream=0):
        """nrldpc_mix_chan_awgn_llr_dev on raw device addresses: packed bits -> packed f32 LLRs, mapper + noise + exact demapper fused."""
        check(self._lib.nrldpc_mix_chan_awgn_llr_dev(self._h, _ptr(d_g), _ptr(d_pt), _ptr(d_g_tilde), C.c_void_p(stream)))

    def modulate(self, d_g, d_tx, stream=0):
        """nrldpc_mix_chan_modulate_dev on raw device addresses: packed bits -> packed symbols."""
        check(self._lib.nrldpc_mix_chan_modulate_dev(self._h, _ptr(d_g), _ptr(d_tx), C.c_void_p(stream)))

    def awgn(self, d_tx, d_pt, d_rx, d_variance=None, stream=0):
        """nrldpc_mix_chan_awgn_dev on raw device addresses: d_rx may be d_tx; d_variance (packed symbol layout, one float per symbol)
        replaces the records' variance."""
        check(self._lib.nrldpc_mix_chan_awgn_dev(self._h, _ptr(d_tx), _ptr(d_pt), _ptr(d_variance), _ptr(d_rx), C.c_void_p(stream)))

    def demodulate(self, d_rx, d_pt, d_out, method="llr", d_variance=None, out_dtype=LLR_F32, stream=0):
        """nrldpc_mix_chan_demodulate_dev on raw device addresses: packed symbols -> packed LLRs of out_dtype (LLR_F32 / LLR_F16), or
        hard-bit bytes for method "hard" (method names as in demod_method_code).  d_pt is not read for "hard" or with d_variance."""
        check(self._lib.nrldpc_mix_chan_demodulate_dev(self._h, _ptr(d_rx), demod_method_code(method), _ptr(d_pt), _ptr(d_variance),
                                                       _ptr(d_out), int(out_dtype), C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.nrldpc_mix_chan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def payload_bits_dev(seed, first_block, n_tb, A, d_a, stream=0):
    """nrldpc_payload_bits_dev: the Monte-Carlo loop's payload draw (plot_BLER_vs_SNR.m:118) for n_tb blocks in one kernel."""
    check(load().nrldpc_payload_bits_dev(int(seed) % (1 << 64), int(first_block), int(n_tb), int(A), _ptr(d_a), C.c_void_p(stream)))


def crc_attach_dev(p, d_a, n_tb, d_c, stream=0):
    t = p if isinstance(p, TbParams) else tb_params(p)
    check(load().nrldpc_crc_attach_dev(C.byref(t), _ptr(d_a), int(n_tb), _ptr(d_c), C.c_void_p(stream)))


def rate_match_dev(p, d_cw, n_tb, d_g, stream=0):
    t = p if isinstance(p, TbParams) else tb_params(p)
    check(load().nrldpc_rate_match_dev(C.byref(t), _ptr(d_cw), int(n_tb), _ptr(d_g), C.c_void_p(stream)))


def quantise_llr(llr, llr_scale=8):
    """The int8 form nrldpc_decode puts on the wire for large host batches (include/nrldpc.h): (q, saw_negative_infinity)."""
    llr = np.ascontiguousarray(llr)
    kind = {np.dtype(np.float32): LLR_F32, np.dtype(np.float16): LLR_F16, np.dtype(np.float64): LLR_F64}[llr.dtype]
    q = np.empty(llr.shape, np.int8)
    neg = load().nrldpc_quantise_llr(_ptr(q), _ptr(llr), llr.size, kind, int(llr_scale))
    return q, bool(neg)


def count_layers(bg, Z, llr):
    """nrldpc_count_layers: what LAYERS_AUTO finds for host LLRs [batch][ncols*Z] (f32 / f16 / f64).  No device needed."""
    llr = np.ascontiguousarray(llr)
    cols = {1: 68, 2: 52}[int(bg)]
    if llr.size % (cols * int(Z)):
        raise NRLDPCError("llr should hold a whole number of codewords")
    n = load().nrldpc_count_layers(int(bg), int(Z), _ptr(llr), llr.size // (cols * int(Z)), _NP2DT[llr.dtype])
    if n < 0:
        raise NRLDPCError((load().nrldpc_last_error() or b"").decode())
    return n


def default_rule(bg, n_layers=0):
    """(alpha, beta) nrldpc_create uses when cfg.alpha == 0 (beta in LLR units)."""
    a, b = C.c_float(), C.c_float()
    check(load().nrldpc_default_rule(int(bg), int(n_layers), C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def set_index(Z):
    return load().nrldpc_set_index(int(Z))


def lifting_size(K_b, K_prime):
    return load().nrldpc_lifting_size(int(K_b), int(K_prime))

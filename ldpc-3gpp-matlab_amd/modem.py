"""NRModulator / NRDemodulator: mirrors of the reference's two modulation System objects (NRModulator.m, NRDemodulator.m), and
AWGNChannel, the mirror of the comm.AWGNChannel between them (plot_BLER_vs_SNR.m:50,105,131).

step() runs the library's mapper / demapper / noise kernels (nrldpc_modulate_dev / nrldpc_demodulate_dev / nrldpc_awgn_dev) and nothing else: a torch device
tensor is used where it lies, on its device's current stream; a numpy array is staged through device 0 and comes back as a numpy
array.  Bits are bytes {0,1} along the last axis, symbols complex64 of unit average power, LLRs positive for bit 0.
"""
import numpy as np

from . import _capi
from ._capi import UnsupportedParameters

Q_M = {"BPSK": 1, "QPSK": 2, "16QAM": 4, "64QAM": 6, "256QAM": 8}           # ModulationSet (NRModulator.m:8)
DECISION_METHODS = ("Log-likelihood ratio", "Approximate log-likelihood ratio", "Hard decision")  # NRDemodulator.m:10
_OUT = {np.dtype(np.float32): _capi.LLR_F32, np.dtype(np.float16): _capi.LLR_F16}


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


class _Modem:
    def __init__(self, Modulation="BPSK"):
        self.Modulation = Modulation

    @property
    def Modulation(self):
        return self._modulation

    @Modulation.setter
    def Modulation(self, m):
        if m not in Q_M:
            raise UnsupportedParameters("Unsupported modulation")  # NRModulator.m:83
        self._modulation = m

    @property
    def Q_m(self):
        """Bits per symbol (NRModulator.m:47-63)."""
        return Q_M[self._modulation]

    @property
    def ModulationOrder(self):
        """Points of the constellation (NRModulator.m:29-45)."""
        return 1 << self.Q_m

    def __call__(self, *a, **kw):
        return self.step(*a, **kw)

    def reset(self):  # NRModulator.m:91: nothing to reset
        pass

    def release(self):
        pass

    @staticmethod
    def _to_device(x, dtype):
        """(device tensor of `dtype`, contiguous; whether the caller gave a numpy array)."""
        import torch
        if _is_tensor(x):
            if not x.is_cuda:
                raise _capi.NRLDPCError("a torch input should be a device tensor (host data: pass a numpy array)")
            return x.to(dtype).contiguous(), False
        return torch.from_numpy(np.ascontiguousarray(x, {torch.uint8: np.uint8, torch.complex64: np.complex64, torch.float32: np.float32}[dtype])).cuda(), True


class NRModulator(_Modem):
    """hMod = NRModulator('Modulation', 'QPSK'); tx = step(hMod, g)  (plot_BLER_vs_SNR.m:101,130)."""

    def step(self, bits):
        """bits [..., n] (0/1; n a multiple of Q_m) -> complex64 symbols [..., n / Q_m]."""
        import torch
        g, host = self._to_device(bits, torch.uint8)
        if g.ndim == 0 or g.shape[-1] % self.Q_m:
            raise _capi.NRLDPCError("the number of bits should be a multiple of Q_m")
        tx = torch.empty(g.shape[:-1] + (g.shape[-1] // self.Q_m,), dtype=torch.complex64, device=g.device)
        with torch.cuda.device(g.device):
            _capi.modulate_dev(g.data_ptr(), g.numel(), self.Q_m, tx.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return tx.cpu().numpy() if host else tx


class NRDemodulator(_Modem):
    """hDemod = NRDemodulator('Modulation', 'QPSK', 'Variance', N0); g_tilde = step(hDemod, rx)  (plot_BLER_vs_SNR.m:102,132).
    DecisionMethod: one of the reference's three strings (or "llr" / "approx" / "hard").  Variance: the complex noise variance,
    tunable between steps (NRDemodulator.m:13-15,94-96); a scalar, or one value per symbol (an array shaped like rx).
    OutputDataType: np.float32 or np.float16 for the two LLR methods (f16 clamped to +-65504); hard decisions are uint8."""

    def __init__(self, Modulation="BPSK", DecisionMethod="Log-likelihood ratio", Variance=1.0, OutputDataType=np.float32):
        super().__init__(Modulation)
        self._method = _capi.demod_method_code(DecisionMethod)
        self.DecisionMethod = DECISION_METHODS[self._method]
        try:
            self._out = _OUT[np.dtype(OutputDataType)]
        except (KeyError, TypeError):
            raise UnsupportedParameters("OutputDataType should be float32 or float16") from None
        self.OutputDataType = np.dtype(OutputDataType)
        self.Variance = Variance

    def step(self, rx):
        """rx [..., n] complex symbols -> [..., n * Q_m] LLRs (positive = bit 0) or hard bits."""
        import torch
        y, host = self._to_device(rx, torch.complex64)
        if y.ndim == 0:
            raise _capi.NRLDPCError("rx should be an array of symbols")
        hard = self._method == _capi.DEMOD_HARD
        odt = torch.uint8 if hard else {_capi.LLR_F32: torch.float32, _capi.LLR_F16: torch.float16}[self._out]
        out = torch.empty(y.shape[:-1] + (y.shape[-1] * self.Q_m,), dtype=odt, device=y.device)
        var, d_var = self.Variance, None
        if np.ndim(var) != 0 or _is_tensor(var):
            if _is_tensor(var):
                d_var = var.to(device=y.device, dtype=torch.float32).contiguous()
            else:
                d_var = torch.from_numpy(np.ascontiguousarray(var, np.float32)).to(y.device)
            if d_var.numel() != y.numel():
                raise _capi.NRLDPCError("a Variance array should hold one value per symbol")
            var = 1.0
        with torch.cuda.device(y.device):
            _capi.demodulate_dev(y.data_ptr(), y.numel(), self.Q_m, out.data_ptr(), method=self._method_name(), variance=float(var),
                                 d_variance=d_var.data_ptr() if d_var is not None else None, out_dtype=self._out,
                                 stream=torch.cuda.current_stream().cuda_stream)
        return out.cpu().numpy() if host else out

    def _method_name(self):
        return ("llr", "approx", "hard")[self._method]


NOISE_METHODS = ("Signal to noise ratio (Eb/No)", "Signal to noise ratio (Es/No)", "Signal to noise ratio (SNR)", "Variance")
VARIANCE_SOURCES = ("Property", "Input port")


class AWGNChannel:
    """hChan = comm.AWGNChannel('NoiseMethod', 'Signal to noise ratio (SNR)'); hChan.SNR = EsN0; rx = step(hChan, tx)
    (plot_BLER_vs_SNR.m:50,105,131).  Properties, defaults and the variance they give are comm.AWGNChannel's; every one of them is
    tunable between steps.  N0 (read-only, no device needed) is the complex noise variance in use, derived in float64:
        Eb/No:    EsNo = EbNo + 10 log10(BitsPerSymbol), then as Es/No
        Es/No:    SignalPower * SamplesPerSymbol / 10^(EsNo/10)
        SNR:      SignalPower / 10^(SNR/10)
        Variance: Variance (VarianceSource "Property"), or step(tx, var) (VarianceSource "Input port": a scalar, or one value per
                  symbol as an array shaped like tx)
    The noise is the library's counter-based draw (nrldpc_awgn_dev: the fused kernel's noise for the same seed and symbol index), keyed
    by Seed.  The object counts the symbols it has stepped -- the stream position of RandomStream = 'mt19937ar with seed': two steps
    draw what one step over the concatenation draws, and reset() rewinds.  step(tx, first_symbol=k) draws at global symbol index k and
    leaves the counter alone (a sharded caller).  Any shape; the symbol order is the flattened C order."""

    def __init__(self, NoiseMethod=NOISE_METHODS[0], EbNo=10.0, EsNo=10.0, SNR=10.0, BitsPerSymbol=1, SignalPower=1.0,
                 SamplesPerSymbol=1, VarianceSource="Property", Variance=1.0, Seed=0):
        self.NoiseMethod = NoiseMethod
        self.VarianceSource = VarianceSource
        self.EbNo, self.EsNo, self.SNR, self.BitsPerSymbol = EbNo, EsNo, SNR, BitsPerSymbol
        self.SignalPower, self.SamplesPerSymbol, self.Variance, self.Seed = SignalPower, SamplesPerSymbol, Variance, Seed
        self._count = 0

    @property
    def NoiseMethod(self):
        return self._noise_method

    @NoiseMethod.setter
    def NoiseMethod(self, m):
        if m not in NOISE_METHODS:
            raise UnsupportedParameters("unknown NoiseMethod %r (one of %s)" % (m, ", ".join(NOISE_METHODS)))
        self._noise_method = m

    @property
    def VarianceSource(self):
        return self._variance_source

    @VarianceSource.setter
    def VarianceSource(self, v):
        if v not in VARIANCE_SOURCES:
            raise UnsupportedParameters("unknown VarianceSource %r (one of %s)" % (v, ", ".join(VARIANCE_SOURCES)))
        self._variance_source = v

    @property
    def N0(self):
        """The complex noise variance the next step(tx) uses (float64)."""
        i = NOISE_METHODS.index(self._noise_method)
        if i == 3:
            return float(self.Variance)
        if i == 2:
            return float(self.SignalPower) / 10.0 ** (float(self.SNR) / 10.0)
        EsNo = float(self.EsNo) if i == 1 else float(self.EbNo) + 10.0 * np.log10(float(self.BitsPerSymbol))
        return float(self.SignalPower) * float(self.SamplesPerSymbol) / 10.0 ** (EsNo / 10.0)

    def __call__(self, *a, **kw):
        return self.step(*a, **kw)

    def reset(self):
        """Rewind the noise stream: the same steps then draw the same noise."""
        self._count = 0

    def release(self):
        pass

    def step(self, tx, var=None, first_symbol=None):
        """tx [...] complex symbols -> tx + noise, same shape (a new array; tx is left as it is)."""
        import torch
        port = self._noise_method == "Variance" and self._variance_source == "Input port"
        if port != (var is not None):
            raise _capi.NRLDPCError("step(tx, var) goes with NoiseMethod 'Variance' and VarianceSource 'Input port', step(tx) with "
                                    "everything else")
        y, host = _Modem._to_device(tx, torch.complex64)
        n0, d_var = self.N0, None
        if port:
            if (var.ndim if _is_tensor(var) else np.ndim(var)) != 0:
                if _is_tensor(var):
                    d_var = var.to(device=y.device, dtype=torch.float32).contiguous()
                else:
                    d_var = torch.from_numpy(np.ascontiguousarray(var, np.float32)).to(y.device)
                if d_var.numel() != y.numel():
                    raise _capi.NRLDPCError("a variance array should hold one value per symbol")
                n0 = 1.0
            else:
                n0 = float(var)
        rx = torch.empty_like(y)
        with torch.cuda.device(y.device):
            _capi.awgn_dev(y.data_ptr(), y.numel(), rx.data_ptr(), variance=n0, d_variance=d_var.data_ptr() if d_var is not None else None,
                           seed=self.Seed, first_symbol=self._count if first_symbol is None else first_symbol,
                           stream=torch.cuda.current_stream().cuda_stream)
        if first_symbol is None:
            self._count += y.numel()
        return rx.cpu().numpy() if host else rx

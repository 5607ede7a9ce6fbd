"""fp64 reference and derived bound for the sinc sample-rate conversion (``rst_resample_sinc`` / ``audio_resample.resample``).

The contract, for ``p = i % n`` and ``j = i // n``::

    y[i] = sum_{k < L} filt[p, k] * X[j * o + k - lead]        X[t] = x[t] inside [0, len), 0 outside (int16: v * 2^-15)

``contract64`` evaluates it in fp64 from the fp32 table and the fp32 / int16 input, together with ``a64 = sum |filt| * |X|``.
``bound = (L + 1) * 2^-24 * a64`` per element is the standard fp32 dot-product bound for ``L`` terms summed in any order, with or
without FMA (every partial sum is at most ``a64`` in magnitude and each of the ``L`` roundings, products included, costs at most
``2^-24`` relative; one more unit for the second-order terms): it is derived, not measured.  Where ``a64 == 0`` every term is an
exact zero and the result must be exactly 0.
"""
import math

import torch
import torch.nn.functional as F

from rstnet_amd.codec.audio_resample import sinc_kernel, stream_geometry

RATES_TO_24K = [8000, 16000, 32000, 44100, 48000, 22050, 11025]
RATES_FROM_24K = [8000, 11025, 16000, 44100, 48000]
PAIRS = [(r, 24000) for r in RATES_TO_24K] + [(24000, r) for r in RATES_FROM_24K]      # the twelve rate pairs


def reduced(orig, new):
    g = math.gcd(int(orig), int(new))
    return int(orig) // g, int(new) // g


def table(o, n):
    """-> (filt ``[n, L]`` fp32, width): exactly what ``sinc_kernel(o, n)`` returns, phase-major."""
    kernel, width = sinc_kernel(o, n)
    return kernel[:, 0, :].contiguous(), width


def as_f64(x):
    """fp32 samples as they are, int16 samples times 2^-15 (exact either way)."""
    return x.double() / 32768.0 if x.dtype == torch.int16 else x.double()


def contract64(x, filt, o, n, lead, T_out):
    """The contract for one row ``x [T]`` (already cut to its length) -> ``(y64 [T_out], a64 [T_out])``."""
    L = filt.shape[1]
    J = -(-T_out // n) if T_out > 0 else 0
    if J == 0:
        return torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    X = as_f64(x.reshape(-1))
    need = (J - 1) * o + L                               # samples of the left-padded signal the last stride reads
    X = F.pad(X, (lead, max(0, need - lead - X.numel())))[:max(need, 1)]
    w = filt.double()[:, None, :]
    y = F.conv1d(X[None, None], w, stride=o)[0].t().reshape(-1)[:T_out]
    a = F.conv1d(X.abs()[None, None], w.abs(), stride=o)[0].t().reshape(-1)[:T_out]
    return y, a


def ref64(x, orig, new):
    """Whole-signal conversion of one row ``x [T]`` (fp32 or int16) -> ``(y64, a64)`` of length ``ceil(n * T / o)``."""
    o, n = reduced(orig, new)
    filt, width = table(o, n)
    return contract64(x, filt, o, n, width, -(-n * x.numel() // o))


def bound(a64, L):
    return (L + 1) * 2.0 ** -24 * a64


def check(y, y64, a64, L, what=""):
    """``y`` (fp32) within the bound of ``y64`` element by element, exactly zero where ``a64`` is; -> worst ratio err / bound."""
    y = y.double().cpu()
    assert y.shape == y64.shape, (what, tuple(y.shape), tuple(y64.shape))
    assert torch.isfinite(y).all(), f"{what}: non-finite output"
    zero = a64 == 0
    assert (y[zero] == 0).all(), f"{what}: non-zero output where every term is zero"
    err, b = (y - y64).abs()[~zero], bound(a64, L)[~zero]
    worst = float((err / b).max()) if err.numel() else 0.0
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3f}"
    return worst


def violates(y, y64, a64, L):
    """Whether ``y`` breaks the bound (or the exact-zero rule) anywhere."""
    y = y.double()
    zero = a64 == 0
    return bool((y[zero] != 0).any() or ((y - y64).abs()[~zero] > bound(a64, L)[~zero]).any())


def stream_ref(whole, delay_out, emitted):
    """The streaming definition: ``concat(zeros(delay_out), whole)`` cut to the emitted length (last dimension)."""
    z = torch.zeros(*whole.shape[:-1], delay_out, dtype=whole.dtype, device=whole.device)
    return torch.cat([z, whole], -1)[..., :emitted]


class HostStream:
    """Host restatement (fp64) of ``StreamResampler``: one buffer ``[hist + frame_in]``, and per step the three operations --
    chunk behind the history, the contract with ``lead = 0`` over the buffer, last ``hist`` samples to the front.  The first
    ``delay_out`` outputs after a reset are zeroed: over the zero history they would hold the filter's response AHEAD of the signal's
    first sample (outputs at negative time), which the whole-signal form never computes."""

    def __init__(self, orig, new, frame_out):
        self.o, self.n, self.width, self.L, self.q, self.hist, self.frame_in, self.delay_out = stream_geometry(orig, new, frame_out)
        self.frame_out = frame_out
        self.filt = table(self.o, self.n)[0] if self.o != self.n else torch.ones(1, 1)
        self.buf = torch.zeros(self.hist + self.frame_in, dtype=torch.float64)
        self.fresh = True

    def step(self, chunk):
        self.buf[self.hist:] = chunk.double()
        y, _ = contract64(self.buf, self.filt, self.o, self.n, 0, self.frame_out)
        if self.fresh:
            y[:self.delay_out] = 0.0
        self.fresh = False
        if self.hist:
            self.buf[:self.hist] = self.buf[self.frame_in:].clone()
        return y

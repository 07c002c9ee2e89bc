"""Audio at any integer sample rate -> the 16 kHz every model of the project takes, on the GPU.

For an input rate r: g = gcd(16000, r), L = 16000 / g (up), M = r / g (down), and the filter is
scipy.signal.resample_poly's default design, ``firwin(2*half_len + 1, 1/max(L, M), window=("kaiser", 5.0)) * L`` with
half_len = 10*max(L, M), computed in float64 (``design_filter``, numpy only).  The output is causal, with zero history
before the first sample:

    y = upfirdn(h, x, L, M)[:ceil(N*L/M)]          y[n] = sum_j h[p + j*L] * x[i0 - j],  i0 = floor(n*M/L), p = n*M mod L

It lags resample_poly's centred output by ``delay`` = half_len / M output samples (20 at 8 kHz, 10 at 24 / 32 / 44.1 /
48 / 96 kHz; where that is an integer, y[delay:] IS resample_poly's output).  Causal on purpose: an output depends on
no future input, so a stream resampled hop by hop with carried history (``Resampler.stream``) is bit-identical to the
whole stream resampled at once, and the streaming scorers keep their bit-exact guarantees for audio at any rate
(``afx.streaming.ResamplingScorer``).  The kernels (``afx_k_resample`` / ``afx_k_resample_stream``) work in fp32: fp32
taps, one fma chain per output in ascending j.  r = 16000 is the identity: nothing is launched.
"""
import functools
import math
import numbers

import numpy as np
import torch

from ._lib import call_on, check, lib, ptr

TARGET_RATE = 16000
MIN_RATE, MAX_RATE = 8000, 192000
FILTER_ID = "kaiser5-hl10"  # the filter design above: StreamState meta of a resampling scorer


def _rate(rate):
    """``rate`` as an int in MIN_RATE..MAX_RATE, else ValueError."""
    if isinstance(rate, bool) or not isinstance(rate, numbers.Real) or not float(rate).is_integer():
        raise ValueError(f"sample rate {rate!r}: an integer number of Hz")
    r = int(rate)
    if not MIN_RATE <= r <= MAX_RATE:
        raise ValueError(f"sample rate {r}: outside {MIN_RATE}..{MAX_RATE} Hz")
    return r


def ratio(rate):
    """(L, M): up and down factors from ``rate`` to 16 kHz."""
    r = _rate(rate)
    g = math.gcd(TARGET_RATE, r)
    return TARGET_RATE // g, r // g


@functools.lru_cache(maxsize=None)
def _design(r):
    L, M = ratio(r)
    if L == M:
        return L, M, np.ones(1)
    mx = max(L, M)
    half_len = 10 * mx
    n = np.arange(2 * half_len + 1, dtype=np.float64) - half_len
    c = 1.0 / mx
    h = c * np.sinc(c * n)  # scipy.signal.firwin: ideal low-pass at cutoff c (Nyquist = 1) ...
    h *= np.kaiser(2 * half_len + 1, 5.0)  # ... windowed ...
    h /= h.sum()  # ... and scaled to unit gain at DC
    h *= L
    h.setflags(write=False)
    return L, M, h


def design_filter(rate):
    """-> (L, M, h): the up / down factors and the float64 filter (read-only) for ``rate``; identity: (1, 1, [1.0])."""
    return _design(_rate(rate))


def phase_taps(L, h):
    """(L, T) float64 polyphase table: taps[p][j] = h[p + j*L] (0 past the end of h), T = ceil(len(h) / L)."""
    T = -(-len(h) // L)
    hp = np.zeros(L * T)
    hp[: len(h)] = h
    return hp.reshape(T, L).T.copy()


class Resampler:
    """``rate`` Hz -> 16 kHz on ``device`` (see the module docstring for the function).

    ``resampler(x)``: (B, N) fp32 on the GPU -> (B, ceil(N*L/M)); ``resampler.clips(list)``: ragged 1-D clips in one
    launch -> list; ``resampler.stream(chunk, hist, slots)``: the next chunk of several streams with their carried samples.
    ``delay``: the output's lag behind resample_poly's, in 16 kHz samples."""

    def __init__(self, rate, device="cuda"):
        self.rate = _rate(rate)
        self.L, self.M, self.h = design_filter(self.rate)
        half_len = (len(self.h) - 1) // 2
        self.delay = half_len / self.M
        self.identity = self.L == self.M
        taps = phase_taps(self.L, self.h)
        self.T = taps.shape[1]
        self.taps = torch.from_numpy(taps).to(torch.float32).to(device)
        self.device = self.taps.device

    @property
    def history(self):
        """Samples a stream carries from one chunk to the next (T - 1)."""
        return self.T - 1

    def n_out(self, n):
        """Output samples of an n-sample input: ceil(n*L/M)."""
        return -(-int(n) * self.L // self.M)

    def __call__(self, x):
        if not isinstance(x, torch.Tensor) or x.ndim != 2 or not x.is_cuda:
            raise ValueError("expected a (B, N) CUDA tensor")
        if self.identity:
            return x
        x = x.to(self.device, torch.float32).contiguous()
        B, N = x.shape
        n = self.n_out(N)
        out = torch.empty(B, n, dtype=torch.float32, device=self.device)
        if B == 0 or N == 0:
            return out
        in_offs = torch.arange(B + 1, dtype=torch.int64, device=self.device) * N
        out_offs = torch.arange(B + 1, dtype=torch.int64, device=self.device) * n
        self._launch(x, in_offs, out_offs, B, n, out)
        return out

    def clips(self, clips):
        """Ragged 1-D clips (any device) -> list of their 16 kHz versions on this resampler's device, one launch."""
        clips = [c.reshape(-1) for c in clips]
        if self.identity:
            return [c.to(self.device, torch.float32) for c in clips]
        if not clips:
            return []
        lens = [int(c.numel()) for c in clips]
        outs = [self.n_out(n) for n in lens]
        x = torch.cat([c.to(torch.float32) for c in clips]).to(self.device)
        in_offs = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int64).to(self.device)
        out_offs = torch.tensor([0] + np.cumsum(outs).tolist(), dtype=torch.int64).to(self.device)
        out = torch.empty(sum(outs), dtype=torch.float32, device=self.device)
        if max(outs) > 0:
            self._launch(x, in_offs, out_offs, len(clips), max(outs), out)
        return list(out.split(outs))

    def _launch(self, x, in_offs, out_offs, B, max_out, out):
        check(call_on(x, lib().afx_k_resample, ptr(x), ptr(in_offs), ptr(out_offs), B, max_out, ptr(self.taps), self.L,
                      self.M, self.T, ptr(out)))

    def stream(self, chunk, hist, slots=None):
        """The next ``n_in`` samples of several streams: chunk (A, n_in) fp32 on the GPU, row i the continuation of the
        stream whose carried samples are hist[slots[i]] (hist (S, T-1) fp32 on the same GPU, zeros for a new stream; slots
        distinct row indices, None = row i of hist for chunk row i).  Returns (A, n_in*L/M) (n_in*L must be a multiple of
        M) and advances the named rows of hist; the other rows are untouched.  Output over successive chunks ==
        ``self(whole stream)``, bit for bit."""
        A, n_in = chunk.shape
        if (n_in * self.L) % self.M:
            raise ValueError(f"a chunk of {n_in} samples at {self.rate} Hz is not a whole number of 16 kHz samples")
        idx = list(range(A)) if slots is None else [int(i) for i in slots]
        if len(idx) != A or len(set(idx)) != A or any(not 0 <= i < hist.shape[0] for i in idx):
            raise ValueError(f"slots: {A} distinct rows of hist (0..{hist.shape[0] - 1})")
        if A == 0:
            return chunk.new_empty(0, n_in * self.L // self.M)
        if self.identity:
            return chunk
        if hist.shape[1] != self.T - 1 or hist.dtype != torch.float32 or not hist.is_contiguous() or hist.device != chunk.device:
            raise ValueError(f"hist: contiguous fp32 (S, {self.T - 1}) on the chunk's device")
        chunk = chunk.to(torch.float32).contiguous()
        rows = torch.tensor(idx, dtype=torch.int32).to(chunk.device)
        out = torch.empty(A, n_in * self.L // self.M, dtype=torch.float32, device=chunk.device)
        check(call_on(chunk, lib().afx_k_resample_stream, ptr(chunk), A, n_in, ptr(hist), ptr(rows), ptr(self.taps),
                      self.L, self.M, self.T, ptr(out)))
        return out

"""Resampling to 16 kHz (afx/resample.py) without a GPU: the filter is scipy.signal.resample_poly's default design, and a
float64 host restatement of the kernels' index plan (i0 = floor(n*M/L), phase p = n*M mod L, T taps per phase, T - 1
carried samples) computes upfirdn's causal output, resample_poly's output after the stated delay, and the same values hop
by hop as over the whole signal."""
import numpy as np
import pytest
from scipy import signal

RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000]
LM = {8000: (2, 1), 11025: (640, 441), 22050: (320, 441), 24000: (2, 3), 32000: (1, 2), 44100: (160, 441),
      48000: (1, 3), 96000: (1, 6)}
TAPS = {8000: 21, 44100: 56, 48000: 61, 96000: 121}


def _plan(x, L, M, taps, hist=None, n_out=None):
    """The kernels' index plan in float64: hist (T-1 carried samples, zeros = a new stream) ++ x, n_out outputs."""
    T = taps.shape[1]
    v = np.concatenate([np.zeros(T - 1) if hist is None else hist, x])
    n_out = -(-len(x) * L // M) if n_out is None else n_out
    y = np.empty(n_out)
    for n in range(n_out):
        i0, p = (n * M) // L, (n * M) % L
        y[n] = sum(taps[p, j] * v[i0 + T - 1 - j] for j in range(T))
    return y, v[len(v) - (T - 1):]


@pytest.mark.parametrize("rate", RATES)
def test_design_matches_scipy(rate):
    from afx.resample import design_filter, phase_taps
    L, M, h = design_filter(rate)
    assert (L, M) == LM[rate]
    mx = max(L, M)
    ref = signal.firwin(2 * 10 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)) * L
    assert h.dtype == np.float64 and h.shape == ref.shape
    assert np.abs(h - ref).max() <= 1e-12
    taps = phase_taps(L, h)
    if rate in TAPS:
        assert taps.shape == (L, TAPS[rate])


@pytest.mark.parametrize("rate", RATES)
def test_index_plan_is_upfirdn_and_resample_poly(rate):
    from afx.resample import Resampler, design_filter, phase_taps
    L, M, h = design_filter(rate)
    taps = phase_taps(L, h)
    x = np.random.default_rng(rate).standard_normal(rate // 40 + 7)
    y, _ = _plan(x, L, M, taps)
    assert len(y) == -(-len(x) * L // M)
    assert np.abs(y - signal.upfirdn(h, x, L, M)[: len(y)]).max() <= 1e-12
    D = (len(h) - 1) // 2 / M
    assert D == Resampler(rate, device="cpu").delay
    if D.is_integer():
        D = int(D)
        ref = signal.resample_poly(x, L, M)
        assert np.abs(y[D:] - ref[: len(y) - D]).max() <= 1e-12


@pytest.mark.parametrize("rate", [8000, 24000, 44100, 48000])
def test_index_plan_hop_by_hop_equals_whole(rate):
    from afx.resample import design_filter, phase_taps
    L, M, h = design_filter(rate)
    taps = phase_taps(L, h)
    hop = rate // 50  # 20 ms: a whole number of 16 kHz samples at every rate here
    x = np.random.default_rng(1).standard_normal(5 * hop)
    whole, _ = _plan(x, L, M, taps)
    hist, parts = None, []
    for k in range(5):
        y, hist = _plan(x[k * hop:(k + 1) * hop], L, M, taps, hist, n_out=hop * L // M)
        parts.append(y)
    assert np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("rate", [7999, 192001, 0, -16000, 44100.5, "48000", None, True])
def test_bad_rates_are_refused(rate):
    from afx.resample import Resampler, design_filter
    with pytest.raises(ValueError):
        design_filter(rate)
    with pytest.raises(ValueError):
        Resampler(rate, device="cpu")


def test_identity_and_delay():
    from afx.resample import Resampler, design_filter
    assert design_filter(16000)[:2] == (1, 1)
    assert Resampler(16000, device="cpu").delay == 0
    assert Resampler(48000.0, device="cpu").rate == 48000
    assert {r: Resampler(r, device="cpu").delay for r in (8000, 44100, 48000, 96000)} == {8000: 20, 44100: 10, 48000: 10,
                                                                                           96000: 10}


def test_wrapper_hop_rates_and_state_keys_on_the_host():
    """ResamplingScorer around a host-side SlidingWindowScorer: which rates a 4000-sample hop admits, the state keys it
    adds, and a bare scorer refusing a wrapped state (the library is built: a state records its build id)."""
    import __graft_entry__ as ge
    ge.build()
    from afx.streaming import ResamplingScorer, SlidingWindowScorer
    sc = SlidingWindowScorer(None, 2, window=16000, hop=4000, device="cpu")
    hops = {r: ResamplingScorer(sc, np.int64(r)).hop_in for r in (8000, 12000, 24000, 32000, 44100, 48000, 96000)}
    assert hops == {8000: 2000, 12000: 3000, 24000: 6000, 32000: 8000, 44100: 11025, 48000: 12000, 96000: 24000}
    for bad in (11025, 22050, 7999, 44100.5):
        with pytest.raises(ValueError):
            ResamplingScorer(sc, bad)
    w = ResamplingScorer(sc, 48000)
    st = w.export_slots([1])
    assert set(st.tensors) == {"samples", "resample_hist"} and tuple(st.tensors["resample_hist"].shape) == (1, 60)
    assert st.meta["input_rate"] == 48000 and st.meta["resampler"] == "kaiser5-hl10"
    with pytest.raises(ValueError):
        sc.import_slots([0], st)
    with pytest.raises(ValueError):
        w.import_slots([0], sc.export_slots([1]))
    w.import_slots([0], st)

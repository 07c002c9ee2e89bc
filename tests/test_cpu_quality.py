"""The input-quality layer on the host (afx/quality.py): ``QualityPolicy.step_reference`` against hand-worked cases for every
measurement and against a scalar restatement of the stated summation order and run rule, the ring and the window count,
``max_bad`` / ``mask`` / ``abstain``, argument validation, the entry point in the header, the ctypes table and the built
library, the placement of ``QualityScorer`` among the other layers, and session export / import on host tensors.  No GPU:
the kernel is held against ``step_reference`` in tests/test_gpu_quality.py.  Every comparison is exact (bits, counts, bytes)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
N_MAX = (1 << 31) - 1
QNAN = 0x7fc00000
f32 = np.float32
NONFINITE, CLIPPED, FLAT, QUIET, DC = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.int32))


def _loose(**kw):
    """A policy under which nothing is flagged unless the test asks for it."""
    from afx.quality import QualityPolicy
    return QualityPolicy(**dict(dict(clip=INF, clip_count=1, flat_run=N_MAX, quiet=0.0, dc=INF), **kw))


def _stream(p, hops, window=None, scores=None):
    """One fresh stream pushed hop by hop -> (list of meas rows, list of out values or None, the state)."""
    from afx.quality import QualityState, window_hops
    hops = [np.asarray(h, dtype=np.float32) for h in hops]
    h = hops[0].size
    st = QualityState(1, window_hops(h if window is None else window, h))
    meas, outs = [], []
    for j, x in enumerate(hops):
        out, m = p.step_reference([0], x[None, :], j + 1, None if scores is None else [scores[j]], st)
        meas.append(m[0].tolist())
        outs.append(None if out is None else out[0])
    return meas, outs, st


# ---- hand-worked measurements ------------------------------------------------------------------------------------------------
def test_a_run_crosses_a_hop_border_and_continues():
    p = _loose(flat_run=5)
    meas, _, st = _stream(p, [[1, 2, 2, 2], [2, 2, 3, 3], [3, 3, 3, 3], [3, 7, 7, 7]])
    assert [m[3] for m in meas] == [3, 5, 6, 7]            # 2 2 2 | 2 2 -> 5;  3 3 | 3 3 3 3 -> 6;  | 3 -> 7
    assert [m[0] for m in meas] == [0, FLAT, FLAT, FLAT]   # 3 < 5 <= 5
    assert st.st[0].tolist() == [_bits(7.0), 3, 1]         # the newest sample, the run it ends, the window's one (FLAT) hop
    # the first sample of a session has r = 1 whatever the new state's `last` (bits 0 = +0.0) says
    assert _stream(p, [[0.0, 1, 2, 3]])[0][0][3] == 1 and _stream(p, [[0.0, 0.0, 0.0, 1]])[0][0][3] == 3


def test_signed_zeros_differ_and_equal_bit_nans_are_equal():
    p = _loose(flat_run=4)
    assert _stream(p, [[0.0, -0.0, 0.0, -0.0]])[0][0][3] == 1
    assert _stream(p, [[-0.0, -0.0, -0.0, 0.0]])[0][0][3] == 3
    nan_a, nan_b = np.array([0x7fc00000, 0x7fc00001], dtype=np.uint32).view(np.float32)
    m = _stream(p, [[nan_a, nan_a, nan_a, nan_a]])[0][0]
    assert m[3] == 4 and m[0] == NONFINITE | FLAT and m[1] == 4
    assert _stream(p, [[nan_a, nan_b, nan_a, nan_b]])[0][0][3] == 1


def test_clip_count_edge_and_the_compare_is_fp32():
    p = _loose(clip=0.5, clip_count=3)
    below = np.nextafter(f32(0.5), f32(0))
    m = _stream(p, [[0.5, -0.5, below, 0.1, -below, 0.2]])[0][0]
    assert m[2] == 2 and m[0] == 0                         # clipped == clip_count - 1
    m = _stream(p, [[0.5, -0.5, below, 0.1, -0.75, 0.2]])[0][0]
    assert m[2] == 3 and m[0] == CLIPPED                   # clipped == clip_count
    m = _stream(p, [[NAN, INF, -INF, 0.1, 0.2, 0.3]])[0][0]
    assert m[2] == 2 and m[1] == 3                         # a NaN is not clipped; the infinities are
    # clip is rounded to fp32 once: 0.1 (double) rounds UP, so the sample fp32(0.1) reaches it
    assert _stream(_loose(clip=0.1), [[f32(0.1), 0, 0.05, 0.01]])[0][0][2] == 1
    # the first and the last element count
    assert _stream(_loose(clip=0.5, clip_count=2), [[0.9, 0, 0.1, -0.9]])[0][0][0] == CLIPPED


def test_quiet_and_dc_sit_exactly_on_their_bounds():
    from afx.quality import QualityPolicy
    p = _loose(quiet=0.0625, dc=0.25)                      # hop 4: E_quiet = 0.25, D = 1.0
    assert [float(v) for v in p.bounds(4)] == [0.25, 1.0]
    m = _stream(p, [[0.5, 0, 0.1, 0]])[0][0]               # e = 0.25 + 0.01: not below
    assert m[0] == 0
    m = _stream(p, [[0.5, 0, 0, 0]])[0][0]
    assert m[4] == _bits(0.25) and m[0] == 0               # e == E_quiet: not below it
    m = _stream(p, [[np.nextafter(f32(0.5), f32(0)), 0, 0, 0]])[0][0]
    assert m[0] == QUIET
    m = _stream(p, [[0.25, 0.25, 0.25, 0.25]])[0][0]
    assert m[5] == _bits(1.0) and m[0] == 0                # |s| == D: not above it (e = 0.25: not quiet either)
    assert _stream(p, [[0.25, 0.25, 0.25, 0.5]])[0][0][0] == DC
    m = _stream(p, [[-0.25, -0.25, -0.25, -0.5]])[0][0]
    assert m[0] == DC and m[5] == _bits(-1.25) and m[6] == _bits(0.5)
    # the bounds are products in float64 rounded once: fp32(fp32(1e-7) * 4000), not an fp32 product
    q = QualityPolicy()
    assert q.bounds(4000)[0] == f32(np.float64(f32(1e-7)) * 4000) and q.bounds(4000)[1] == f32(np.float64(f32(0.05)) * 4000)


def test_nan_and_inf_samples():
    p = _loose(quiet=1.0, dc=0.0)
    m = _stream(p, [[1.0, NAN, -3.0, 2.0]])[0][0]
    assert m[0] == NONFINITE and m[1] == 1 and m[4] == QNAN and m[5] == QNAN and m[6] == _bits(3.0)  # NaN e, s: neither QUIET nor DC
    neg_nan = np.array([0xffc00123], dtype=np.uint32).view(np.float32)[0]
    m = _stream(p, [[neg_nan, 0, 0, 0]])[0][0]
    assert m[4] == QNAN and m[5] == QNAN and m[6] == 0     # every NaN sum is recorded as THE quiet NaN; no sample for the peak but zeros
    m = _stream(p, [[INF, 1.0, -INF, 0]])[0][0]
    assert m[1] == 2 and m[4] == _bits(INF) and m[5] == QNAN and m[6] == _bits(INF) and m[0] == NONFINITE | CLIPPED  # (|inf| >= clip = inf)
    m = _stream(p, [[INF, 1.0, 0, 0]])[0][0]
    assert m[5] == _bits(INF) and m[0] == NONFINITE | CLIPPED | DC
    m = _stream(p, [[NAN, NAN, NAN, NAN]])[0][0]
    assert m[6] == 0 and m[1] == 4


def test_a_hop_of_zeros_is_quiet_and_flat_once_the_run_is_reached():
    from afx.quality import QualityPolicy
    p = QualityPolicy(flat_run=6)
    meas, _, _ = _stream(p, [np.zeros(4), np.zeros(4), [0.3, -0.2, 0.25, -0.35]])
    assert [m[0] for m in meas] == [QUIET, QUIET | FLAT, 0] and [m[3] for m in meas] == [4, 8, 1]
    assert meas[0][4:7] == [0, 0, 0]
    # -0.0 sums: the padding is +0.0, so a hop of -0.0 sums to +0.0
    m = _stream(p, [[-0.0, -0.0, -0.0, -0.0]])[0][0]
    assert m[5] == 0 and m[4] == 0


# ---- the summation order and the run rule against scalar restatements ----------------------------------------------------
def _sum_by_definition(v):
    """The stated order, one np.float32 scalar operation at a time."""
    h = v.size
    tiles = -(-h // 1024)
    y = np.zeros(tiles * 1024, dtype=np.float32)
    y[:h] = v
    with np.errstate(invalid="ignore", over="ignore"):
        r = []
        for t in range(256):
            q = [y[4 * t + c] for c in range(4)]
            for tile in range(1, tiles):
                q = [f32(q[c] + y[1024 * tile + 4 * t + c]) for c in range(4)]
            r.append(f32(f32(q[0] + q[1]) + f32(q[2] + q[3])))
        w = 128
        while w >= 1:
            for t in range(w):
                r[t] = f32(r[t] + r[t + w])
            w //= 2
    return r[0]


@pytest.mark.parametrize("h", [1, 3, 1023, 1024, 1025, 4000])
def test_the_summation_order_is_the_stated_one(h):
    from afx.quality import hop_sums
    g = np.random.default_rng(h)
    x = (g.standard_normal(h) * np.exp(g.uniform(-8, 2, h))).astype(np.float32)  # magnitudes spread: the order shows in the last bits
    e, s = hop_sums(x[None, :])
    with np.errstate(over="ignore"):
        want_e, want_s = _sum_by_definition((x * x).astype(np.float32)), _sum_by_definition(x)
    assert _bits(e[0]) == _bits(want_e) and _bits(s[0]) == _bits(want_s)
    m = _stream(_loose(), [x])[0][0]
    assert m[4] == _bits(want_e) and m[5] == _bits(want_s) and m[6] == _bits(np.abs(x).max())


def test_streams_cut_into_updates_at_random_hop_boundaries():
    """Three slots, each with its own stream; every update names a random subset in a random order.  Per slot the meas rows
    are ``run_reference``'s over that slot's stream alone, and the run at the end is the one a scalar pass over the whole
    stream finds."""
    from afx.quality import QualityPolicy, QualityState, window_hops
    g = np.random.default_rng(11)
    hop, window, n, S = 37, 150, 24, 3
    p = QualityPolicy(clip=0.9, clip_count=2, flat_run=7, quiet=1e-3, dc=0.2, max_bad=1)
    streams = []
    for s in range(S):
        x = g.choice(np.array([0.0, -0.0, 0.5, 0.95, -0.95, 0.01, NAN], dtype=np.float32), n * hop, p=[0.3, 0.05, 0.3, 0.1, 0.1, 0.13, 0.02])
        x[g.integers(0, n * hop - 80):][:80] = 0.25   # a run of 80 across borders
        x[(5 + s) * hop - 3:(7 + s) * hop + 3] = 0.0  # a gap of zeros: a whole quiet hop
        streams.append(x.astype(np.float32))
    st = QualityState(S, window_hops(window, hop))
    pos, got = [0] * S, [[] for _ in range(S)]
    while min(pos) < n:
        named = [int(s) for s in g.permutation(S)[:g.integers(1, S + 1)] if pos[s] < n]
        if not named:
            continue
        x = np.stack([streams[s][pos[s] * hop:(pos[s] + 1) * hop] for s in named])
        _, meas = p.step_reference(named, x, [pos[s] + 1 for s in named], None, st)
        for i, s in enumerate(named):
            got[s].append(meas[i].tolist())
            pos[s] += 1
    seen = set()
    for s in range(S):
        want, valid = p.run_reference(streams[s], hop, window)
        assert got[s] == want.tolist(), s
        assert valid.tolist() == [m[7] <= 1 for m in got[s]]
        bits = streams[s].view(np.uint32).tolist()
        r, last, best = 0, None, []
        for b in bits:
            r = r + 1 if b == last else 1
            last = b
            best.append(r)
        assert int(st.st[s, 1]) == r and [m[3] for m in got[s]] == [max(best[j * hop:(j + 1) * hop]) for j in range(n)]
        assert st.totals[s, 0] == n and st.totals[s, 1:].tolist() == [sum((m[0] >> b) & 1 for m in got[s]) for b in range(5)]
        seen |= {m[0] for m in got[s]}
    assert {f for v in seen for f in (1, 2, 4, 8, 16) if v & f} == {1, 2, 4, 8, 16}
    # a trailing part of a hop is left out, and an empty stream is an empty answer
    assert p.run_reference(streams[0][:hop * 3 + 5], hop, window)[0].tolist() == got[0][:3]
    assert p.run_reference([], hop, window)[0].shape == (0, 8)


def test_run_saturates_and_totals_saturate():
    from afx.quality import QualityState
    p = _loose(flat_run=2)
    st = QualityState(1, 1)
    st.st[0] = (_bits(0.5), N_MAX - 2, 0)
    st.totals[0] = (N_MAX - 1, N_MAX, 0, 5, 0, 0)
    _, m = p.step_reference([0], f32([[0.5, 0.5, 0.5, 0.5]]), 9, None, st)
    assert m[0, 3] == N_MAX and st.st[0].tolist() == [_bits(0.5), N_MAX, 1]
    assert st.totals[0].tolist() == [N_MAX, N_MAX, 0, 6, 0, 0]
    _, m = p.step_reference([0], f32([[0.5, 0.5, 0.25, 0.25]]), 10, None, st)
    assert m[0, 3] == N_MAX and st.st[0].tolist() == [_bits(0.25), 2, 1] and st.totals[0, 0] == N_MAX


# ---- the ring and the window count ---------------------------------------------------------------------------------------------
CLEAN, LOUD = f32([0.1, -0.2, 0.3, -0.1]), f32([0.9, -0.9, 0.3, -0.1])


@pytest.mark.parametrize("W", [1, 2, 16])
def test_the_window_counts_the_flagged_hops_of_the_last_w_and_never_before_the_first(W):
    from afx.quality import QualityState
    p = _loose(clip=0.8, clip_count=2, mask=CLIPPED, max_bad=0)
    g = np.random.default_rng(W)
    st = QualityState(2, W)
    st.ring[:] = 31                                         # what a previous session left: deliberately poisoned
    loud = (g.random(3 * W + 5) < 0.4).tolist()
    for k, is_loud in enumerate(loud, start=1):
        out, m = p.step_reference([1], (LOUD if is_loud else CLEAN)[None, :], k, [2.5], st)
        want = sum(loud[max(0, k - W):k])                   # hops max(1, k-W+1)..k: the poisoned entries are never counted
        assert m[0, 7] == want and m[0, 0] == (CLIPPED if is_loud else 0), (W, k)
        assert st.ring[1, (k - 1) % W] == m[0, 0] and st.st[1, 2] == want
        assert (_bits(out[0]) == QNAN) == (want > 0) and (want > 0 or out[0] == f32(2.5))
    assert st.ring[0].tolist() == [31] * W and st.st[0].tolist() == [0, 0, 0]  # the slot not named
    # a reset mid-stream: state and totals cleared, the ring left alone -- and the new session does not count the old entries
    st.ring[1] = 31
    st.reset([1])
    assert st.st[1].tolist() == [0, 0, 0] and st.totals[1].tolist() == [0] * 6 and st.ring[1].tolist() == [31] * W
    for k in range(1, W + 2):
        out, m = p.step_reference([1], CLEAN[None, :], k, [2.5], st)
        assert m[0, 7] == 0 and out[0] == f32(2.5), (W, k)
    # without the bound the same entries would count (what the bound is for)
    if W > 1:
        st.st[1], st.ring[1] = 0, 31
        assert p.step_reference([1], CLEAN[None, :], W + 7, None, st)[1][0, 7] == W - 1


def test_max_bad_mask_and_abstain():
    zeros = np.zeros(4, np.float32)
    seq = [LOUD, CLEAN, zeros, CLEAN, CLEAN, CLEAN, CLEAN]  # CLIPPED, -, QUIET|FLAT.., -
    sc = [f32(v) for v in (1, 2, 3, 4, 5, 6, 7)]
    kw = dict(clip=0.8, clip_count=2, quiet=1e-4, flat_run=4)
    # window of 3 hops, max_bad 0: one flagged hop withholds the score until it has left the window
    meas, outs, _ = _stream(_loose(**kw), seq, window=12, scores=sc)
    assert [m[0] for m in meas] == [CLIPPED, 0, QUIET | FLAT, 0, 0, 0, 0] and [m[7] for m in meas] == [1, 1, 2, 1, 1, 0, 0]
    assert [_bits(o) == QNAN for o in outs] == [True] * 5 + [False] * 2 and outs[5:] == [f32(6), f32(7)]
    # max_bad 1
    outs = _stream(_loose(max_bad=1, **kw), seq, window=12, scores=sc)[1]
    assert [_bits(o) == QNAN for o in outs] == [False, False, True, False, False, False, False]
    # the mask: only CLIPPED counts
    meas, outs, _ = _stream(_loose(mask=CLIPPED, **kw), seq, window=12, scores=sc)
    assert [m[7] for m in meas] == [1, 1, 1, 0, 0, 0, 0] and [m[0] for m in meas][2] == QUIET | FLAT  # still measured and flagged
    assert [_bits(o) == QNAN for o in outs] == [True] * 3 + [False] * 4
    # mask 0: nothing counts
    assert all(_bits(o) != QNAN for o in _stream(_loose(mask=0, **kw), seq, window=12, scores=sc)[1])
    # abstain off: measured, counted, and every score passes bit for bit -- a NaN score with a payload included
    odd = np.array([0x7fc00abc], dtype=np.uint32).view(np.float32)[0]
    meas, outs, _ = _stream(_loose(abstain=False, **kw), seq, window=12, scores=[odd] + sc[1:])
    assert [m[7] for m in meas] == [1, 1, 2, 1, 1, 0, 0] and _bits(outs[0]) == 0x7fc00abc and outs[1:] == sc[1:]
    # no scores: no out
    assert _stream(_loose(**kw), seq)[1] == [None] * 7


def test_rows_named_in_any_order_rows_skipped_and_refusals_of_the_reference():
    from afx.quality import QualityState
    p = _loose(clip=0.8, clip_count=2)
    st = QualityState(4, 2)
    x = np.stack([LOUD, CLEAN, LOUD])
    out, m = p.step_reference([3, 0, 2], x, [1, 0, 5], f32([1, 2, 3]), st)
    assert m[:, 0].tolist() == [CLIPPED, -1, CLIPPED] and m[1].tolist() == [-1] * 8 and out[1] == f32(2)  # k = 0: skipped whole
    assert st.st[0].tolist() == [0, 0, 0] and st.totals[:, 0].tolist() == [0, 0, 1, 1] and st.ring.tolist() == [[0, 0], [0, 0], [2, 0], [2, 0]]
    before = st.copy()
    for args in (([0, 0], x[:2], 1, None), ([4], x[:1], 1, None), ([0], x[:2], 1, None), ([0, 1], x[:2], [1, 2, 3], None),
                 ([0, 1], x[:2], 1.5, None), ([0, 1], x[:2], 1, f32([1])), ([0], x[0], 1, None)):
        with pytest.raises(ValueError):
            p.step_reference(*args, st)
    with pytest.raises(ValueError):
        p.step_reference([0], x[:1], 1, None, (st.ring, st.st, st.totals))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((st.ring, st.st, st.totals), (before.ring, before.st, before.totals)))


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_policy_and_window_arguments_are_validated():
    from afx.quality import Quality, QualityPolicy, window_hops
    p = QualityPolicy(np.float32(0.5), np.int64(3), np.int32(2), np.float64(0), 0, 0, np.int64(5), np.bool_(False))
    assert p.params() == dict(clip=0.5, clip_count=3, flat_run=2, quiet=0.0, dc=0.0, mask=0, max_bad=5, abstain=False)
    assert all(type(v) in (int, float, bool) for v in p.params().values())
    d = QualityPolicy().params()
    assert d == dict(clip=float(f32(0.98)), clip_count=8, flat_run=320, quiet=float(f32(1e-7)), dc=float(f32(0.05)), mask=31, max_bad=0, abstain=True)
    QualityPolicy(clip=INF, quiet=INF, dc=INF)
    for bad in (dict(clip=0.0), dict(clip=-1.0), dict(clip=NAN), dict(clip="1"), dict(clip=True), dict(clip=1e39), dict(clip=1e-50),
                dict(clip_count=0), dict(clip_count=1.0), dict(clip_count=True), dict(clip_count=1 << 31), dict(flat_run=1), dict(flat_run=0),
                dict(flat_run=2.0), dict(flat_run=1 << 31), dict(quiet=-1e-9), dict(quiet=NAN), dict(quiet=None), dict(quiet=1e39),
                dict(dc=-0.1), dict(dc=NAN), dict(dc="x"), dict(mask=-1), dict(mask=32), dict(mask=1.0), dict(mask=True), dict(max_bad=-1),
                dict(max_bad=0.0), dict(max_bad=1 << 31), dict(abstain=1), dict(abstain=None)):
        with pytest.raises(ValueError):
            QualityPolicy(**bad)
    assert [window_hops(w, 4000) for w in (1, 4000, 4001, 16000, 64000)] == [1, 1, 2, 4, 16] and window_hops(1024 * 160, 160) == 1024
    for w, h in ((0, 4000), (4000, 0), (1024 * 160 + 1, 160), (4000.0, 4000), (4000, True), (4000, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            window_hops(w, h)
    for args in ((0, p, 4, 4), (8193, p, 4, 4), (2.0, p, 4, 4), (2, None, 4, 4), (2, p, 0, 4), (2, p, 4, 5000)):
        with pytest.raises(ValueError):
            Quality(*args, device="cpu")
    q = Quality(3, QualityPolicy(), 4000, 64000, "cpu")
    assert (q.W, q.ring.shape, q.ring.dtype, q.st.shape, q.totals.shape) == (16, (3, 16), torch.uint8, (3, 3), (3, 6))
    assert q.valid.tolist() == [True] * 3 and q.bad.tolist() == [0] * 3 and q.flags_at([0, 1, 17]).tolist() == [0, 0, 0]
    assert {k: v.tolist() for k, v in q.stats().items()} == {k: [0, 0, 0] for k in ("hops", "nonfinite", "clipped", "flat", "quiet", "dc")}
    x = torch.zeros(3, 4000)
    for args, kw in (((x[:2],), dict(hop_index=1)), ((x.double(),), dict(hop_index=1)), ((x[:, :3999],), dict(hop_index=1)),
                     ((x[:1], [3]), dict(hop_index=1)), ((x[:2], [1, 1]), dict(hop_index=1)), ((x,), dict(hop_index=[1, 2])),
                     ((x,), dict(hop_index=1.5)), ((x,), dict(hop_index=0)), ((x,), dict(hop_index=1 << 31)),
                     ((x,), dict(hop_index=1, scores=torch.zeros(2))), ((x,), dict(hop_index=1, scores=torch.zeros(3, dtype=torch.float64)))):
        with pytest.raises(ValueError):
            q.update(*args, **kw)
    from afx._lib import AfxError
    with pytest.raises(AfxError):  # no CPU fallback
        q.update(x, hop_index=1)
    assert q.update(x[:0], [], hop_index=1)[1].shape == (0, 8)


def test_quality_entry_point_is_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bafx_k_quality\s*\(", src) and hasattr(lib, "afx_k_quality") and "afx_k_quality" in built.SIGNATURES
    l = built.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    #       x  stride A hop hdr scores sstride clip cc fr  e_q  dc  mask max_bad abstain ring W state totals S meas out
    good = [p, 4, 1, 4, p, p, 1, 0.98, 8, 320, 1e-4, 0.2, 31, 0, 1, p, 2, p, p, 2, p, p]
    cases = [(i, None) for i in (0, 4, 15, 17, 18, 20)]    # a NULL required pointer
    cases += [(21, None),                                  # scores without an output
              (6, 0), (6, -1), (2, 0), (2, 8193), (2, -1), (3, 0), (3, -4), (3, (1 << 24) + 1), (1, 3), (1, -4), (19, 0), (19, -1),
              (16, 0), (16, 1025), (16, -1), (7, 0.0), (7, -0.5), (7, NAN), (8, 0), (8, -1), (9, 1), (9, 0), (10, -1e-9), (10, NAN),
              (11, -0.5), (11, NAN), (12, -1), (12, 32), (13, -1), (14, 2), (14, -1)]
    # refused on the host, with pointers that would pass the NULL check never dereferenced: nothing is launched
    for i, v in cases:
        args = list(good)
        args[i] = v
        assert l.afx_k_quality(*args, None) != 0 and b"quality" in l.afx_last_error(), (i, v)


# ---- placement -----------------------------------------------------------------------------------------------------------------
H = 4000


def _bare(S=2, hop=H, window=16000):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=window, hop=hop, device="cpu")


class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


def test_every_chain_constructs_and_the_forbidden_nestings_raise(built):
    from afx._lib import AfxError
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.streaming import IncrementalScorer, KVCachedScorer, ResamplingScorer, SlidingWindowScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    qp, vp = QualityPolicy(), VerdictPolicy(0.0, 0.5, verifier_enter=-0.5)
    cascade = lambda: CascadeScorer(_bare(), _Model(), CascadePolicy(0.0, 2))  # noqa: E731
    qs = QualityScorer(_bare(S=3), qp)
    assert (qs.S, qs.hop, qs.window, qs.device.type, qs.quality.W) == (3, H, 16000, "cpu", 4)
    assert qs._slot_list([2, 0], ordered=True) == [2, 0] and qs.samples_seen.tolist() == [0, 0, 0]
    assert qs.valid.tolist() == [True] * 3 and qs.valid.dtype == torch.bool and qs.flags.tolist() == [0] * 3 and qs.last_meas.shape == (0, 8)
    assert QualityScorer(_bare()).policy.params() == qp.params()  # (the default policy)
    with pytest.raises(AfxError):  # no CPU fallback, and nothing moved
        qs.push(torch.zeros(3, H))
    assert qs.samples_seen.tolist() == [0, 0, 0]
    # the full chain of the issue, and the shorter ones
    full = JitterScorer(GatedScorer(EvidenceScorer(VerdictScorer(QualityScorer(cascade(), qp), vp), EvidencePolicy())), 8000, "mulaw", 4)
    meta = full.state_meta()
    assert meta["quality"] == 1 and meta["quality_window"] == dict(W=4, hop=H) and meta["verdict"] == 1 and meta["gate"] == 1 and meta["cascade"] == 1
    v = VerdictScorer(QualityScorer(cascade(), qp), vp)
    assert v._verified is True and VerdictScorer(QualityScorer(_bare(), qp), vp)._verified is False
    assert VerdictScorer(QualityScorer(cascade(), qp), VerdictPolicy(0.0))._verified is False and VerdictScorer(cascade(), vp)._verified is True
    for front in (GatedScorer(qs), GatedScorer(VerdictScorer(qs, vp)), PacketScorer(QualityScorer(_bare(), qp), 8000, "mulaw"),
                  ResamplingScorer(QualityScorer(_bare(), qp), 8000), JitterScorer(GatedScorer(QualityScorer(cascade(), qp)), 8000, "mulaw", 4),
                  PacketScorer(GatedScorer(VerdictScorer(QualityScorer(_bare(), qp), vp)), 8000, "mulaw")):
        assert front.state_meta()["quality"] == 1
    assert isinstance(_bare(), SlidingWindowScorer) and issubclass(IncrementalScorer, SlidingWindowScorer) and issubclass(KVCachedScorer, SlidingWindowScorer)
    # forbidden: the quality layer around a front, the gate, the verdict or evidence layer, or itself; anything else around it the wrong way
    for inner in (ResamplingScorer(_bare(), 8000), PacketScorer(_bare(), 8000, "mulaw"), GatedScorer(_bare()), VerdictScorer(_bare(), vp),
                  EvidenceScorer(VerdictScorer(_bare(), vp), EvidencePolicy()), qs, object(), None):
        with pytest.raises(ValueError):
            QualityScorer(inner, qp)
    with pytest.raises(ValueError):
        QualityScorer(_bare(), "default")
    with pytest.raises(ValueError):
        QualityScorer(_bare(S=8193, hop=400, window=400), qp)
    with pytest.raises(ValueError):
        QualityScorer(_bare(hop=10, window=16000), qp)  # 1600 hops of window
    with pytest.raises(ValueError):
        CascadeScorer(qs, _Model(), CascadePolicy(0.0, 2))  # the cascade goes inside
    with pytest.raises(ValueError):
        EvidenceScorer(qs, EvidencePolicy())  # evidence wraps the verdict layer
    with pytest.raises(ValueError):
        VerdictScorer(GatedScorer(qs), vp)
    # around a plain scorer there is no cascade to forward to
    with pytest.raises(AttributeError):
        qs.verified
    c = QualityScorer(cascade(), qp)
    assert torch.isnan(c.verified).all() and c.verified_at.tolist() == [-1, -1] and c.take_events() == [] and c.last_verified() is None


def test_export_and_import_on_the_host_and_every_refusal_leaves_the_scorer_unchanged(built):
    from afx.quality import QualityPolicy, QualityScorer
    from afx.streaming import StreamState
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    a = QualityScorer(_bare(S=3), QualityPolicy())
    a.scorer.ring[:] = torch.arange(3 * 16000, dtype=torch.float32).reshape(3, 16000)
    a.scorer._seen[:] = torch.tensor([8000, 20000, 0])
    a.quality.ring[:] = torch.tensor([[0, 2, 0, 0], [8, 12, 12, 0], [31, 31, 31, 31]], dtype=torch.uint8)
    a.quality.st[:] = torch.tensor([[_bits(0.5), 1, 1], [0, 7000, 2], [0, 0, 0]], dtype=torch.int32)  # slot 1: a run in progress
    a.quality.totals[:] = torch.tensor([[2, 0, 1, 0, 0, 0], [5, 0, 0, 2, 3, 0], [0] * 6], dtype=torch.int32)
    assert a.valid.tolist() == [False, False, True] and a.flags.tolist() == [2, 8, 0]  # hop 2 at ring[1]; hop 5 at ring[0]; none
    st = a.export_slots([1, 0])
    t = st.tensors
    assert t["quality_ring"].tolist() == [[8, 12, 12, 0], [0, 2, 0, 0]] and t["quality_ring"].dtype == torch.uint8
    assert t["quality_state"].tolist() == [[0, 7000, 2], [_bits(0.5), 1, 1]] and t["quality_state"].dtype == torch.int64
    assert t["quality_totals"].tolist() == [[5, 0, 0, 2, 3, 0], [2, 0, 1, 0, 0, 0]] and st.seen.tolist() == [20000, 8000]
    assert st.meta["quality"] == 1 and st.meta["quality_window"] == dict(W=4, hop=H)
    # the destination runs another clip, flat_run, mask and max_bad: the ring stores raw flags
    b = QualityScorer(_bare(S=4), QualityPolicy(clip=0.5, flat_run=100, mask=2, max_bad=2))
    b.quality.ring[:] = 16

    def snap(c):
        return [c.quality.ring.clone(), c.quality.st.clone(), c.quality.totals.clone(), c.scorer.ring.clone(), c.samples_seen]

    before = snap(b)
    with_state = lambda rows: dict(t, quality_state=torch.tensor(rows))  # noqa: E731
    foreign = [
        a.scorer.export_slots([1, 0]),                                                     # a bare state: no quality part
        GatedScorer(_bare(S=3)).export_slots([1, 0]),
        VerdictScorer(_bare(S=3), VerdictPolicy(0.0)).export_slots([1, 0]),
        st.tensors, None,
        StreamState(dict(st.meta, quality=2), st.seen, t),                                 # another format
        StreamState(dict(st.meta, quality_window=dict(W=5, hop=H)), st.seen, t),           # another W
        StreamState(dict(st.meta, quality_window=dict(W=4, hop=2000)), st.seen, t),        # another hop
        StreamState({k: v for k, v in st.meta.items() if k != "quality_window"}, st.seen, t),
        StreamState(st.meta, st.seen, {k: v for k, v in t.items() if k != "quality_ring"}),
        StreamState(st.meta, st.seen, with_state([[0, -1, 2], [_bits(0.5), 1, 1]])),       # a negative run
        StreamState(st.meta, st.seen, with_state([[0, 7000, 5], [_bits(0.5), 1, 1]])),     # bad > W
        StreamState(st.meta, st.seen, with_state([[0, 7000, -1], [_bits(0.5), 1, 1]])),
        StreamState(st.meta, st.seen, with_state([[1 << 32, 7000, 2], [_bits(0.5), 1, 1]])),
        StreamState(st.meta, st.seen, dict(t, quality_state=t["quality_state"].to(torch.int32))),
        StreamState(st.meta, st.seen, dict(t, quality_state=t["quality_state"][:, :2])),
        StreamState(st.meta, st.seen, dict(t, quality_ring=t["quality_ring"][:, :3])),
        StreamState(st.meta, st.seen, dict(t, quality_ring=t["quality_ring"].to(torch.int32))),
        StreamState(st.meta, st.seen, dict(t, quality_ring=t["quality_ring"] + 64)),       # a bit that is no flag
        StreamState(st.meta, st.seen, dict(t, quality_totals=torch.tensor([[5, 0, 0, 6, 3, 0], [2, 0, 1, 0, 0, 0]]))),  # a flag counted more often than hops
        StreamState(st.meta, st.seen, dict(t, quality_totals=torch.tensor([[-5, 0, 0, 0, 0, 0], [2, 0, 1, 0, 0, 0]]))),
        StreamState(st.meta, st.seen, dict(t, quality_totals=t["quality_totals"][:, :5])),
        StreamState(dict(st.meta, window=32000), st.seen, t),                              # the inner scorer's own refusal
    ]
    for i, f in enumerate(foreign):
        with pytest.raises(ValueError):
            b.import_slots([3, 1], f)
        assert all(torch.equal(u, v) for u, v in zip(before, snap(b))), i
    with pytest.raises(ValueError):
        b.import_slots([3], st)  # two sessions for one slot
    with pytest.raises(ValueError):
        b.scorer.import_slots([3, 1], st)  # a bare scorer refuses a quality state
    b.import_slots([3, 1], StreamState.from_state_dict(st.state_dict()))
    assert b.quality.ring.tolist() == [[16] * 4, [0, 2, 0, 0], [16] * 4, [8, 12, 12, 0]]
    assert b.quality.st.tolist() == [[0, 0, 0], [_bits(0.5), 1, 1], [0, 0, 0], [0, 7000, 2]] and b.samples_seen.tolist() == [0, 8000, 0, 20000]
    assert b.quality.totals[[3, 1]].tolist() == [[5, 0, 0, 2, 3, 0], [2, 0, 1, 0, 0, 0]]
    assert b.valid.tolist() == [True] * 4  # max_bad = 2 here
    back = b.export_slots([3, 1])
    assert all(torch.equal(back.tensors[k], st.tensors[k]) for k in st.tensors) and back.meta == st.meta
    # reset: the inner session, state and totals; the ring stays
    b.reset([1, 3])
    assert b.quality.st.tolist() == [[0, 0, 0]] * 4 and b.quality.totals.tolist() == [[0] * 6] * 4 and b.samples_seen.tolist() == [0] * 4
    assert b.quality.ring.tolist() == [[16] * 4, [0, 2, 0, 0], [16] * 4, [8, 12, 12, 0]]
    # through the verdict layer and the gate: every layer peels its own part
    mk = lambda: GatedScorer(VerdictScorer(QualityScorer(_bare(S=2), QualityPolicy()), VerdictPolicy(0.0)))  # noqa: E731
    g1, g2 = mk(), mk()
    g1.scorer.scorer.quality.st[1] = torch.tensor([7, 3, 1], dtype=torch.int32)
    g2.import_slots([0], g1.export_slots([1]))
    assert g2.scorer.scorer.quality.st.tolist() == [[7, 3, 1], [0, 0, 0]]
    with pytest.raises(ValueError):
        g2.import_slots([0], GatedScorer(VerdictScorer(_bare(S=2), VerdictPolicy(0.0))).export_slots([1]))

"""The verdict layer on the host (afx/verdict.py): ``VerdictPolicy.step_reference`` against a scalar row-by-row restatement
of the stated function and against hand-worked cases, argument validation of ``VerdictPolicy`` / ``Verdicts`` /
``VerdictScorer``, the entry point in the header, the ctypes table and the built library, session export / import on host
tensors, the host's log-bound bookkeeping with the launch replaced by ``step_reference``, and ``Timeline.alarms``.  No GPU:
the kernel is held against ``step_reference`` in tests/test_gpu_verdict.py.  Every comparison is exact, bits of m included."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000
INF, NAN = float("inf"), float("nan")
N_MAX = (1 << 31) - 1
f32 = np.float32


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.int32))


def _by_definition(p, slots, scores, ks, m, st, verified=None):
    """The function of the module docstring, written out row by row with scalar fp32 operations; m, st updated in place."""
    alpha, enter, exit_ = f32(p.alpha), f32(p.enter), f32(p.exit)
    events = []
    for i, b in enumerate(slots):
        s = f32(scores[i])
        v = f32(NAN) if verified is None or p.verifier_enter is None else f32(verified[i])
        if np.isnan(s):
            continue
        n, run, on, since = (int(x) for x in st[b])
        n1 = n if n == N_MAX else n + 1
        with np.errstate(invalid="ignore", over="ignore"):
            m1 = s if n == 0 else f32(m[b] + f32(alpha * f32(s - m[b])))
        kind = 0
        if on == 0:
            if not np.isnan(v) and v < f32(p.verifier_enter):
                on, run, since, kind = 1, 0, int(ks[i]), 2
            elif not np.isnan(v):
                run = 0
            elif n1 >= p.min_scores and m1 < enter:
                run += 1
                if run >= p.confirm:
                    on, run, since, kind = 1, 0, int(ks[i]), 1
            else:
                run = 0
        elif not p.latch:
            if m1 >= exit_:
                run += 1
                if run >= p.release:
                    on, run, since, kind = 0, 0, -1, 3
            else:
                run = 0
        m[b], st[b] = m1, (n1, run, on, since)
        if kind:
            events.append((int(b), kind, int(ks[i]), _bits(m1)))
    return events


def _run(p, scores, verified=None):
    """One stream: (kinds per score (0 = no event), on flags, final m, final st row)."""
    from afx.verdict import new_state
    m, st = new_state(1)
    kinds, on = [], []
    for j, s in enumerate(scores):
        ev = p.step_reference([0], [s], j + 1, m, st, None if verified is None else [verified[j]])
        assert all(e[0] == 0 and e[2] == j + 1 for e in ev) and len(ev) <= 1
        kinds.append(ev[0][1] if ev else 0)
        on.append(int(st[0, 2]))
    return kinds, on, m[0], st[0].tolist()


def test_step_reference_equals_the_definition_row_by_row():
    from afx.verdict import VerdictPolicy, new_state
    g = np.random.default_rng(3)
    values = np.array([-INF, -1.5, -0.25, -0.0, 0.0, 0.1, 0.25, 0.25, 0.5, 1.0, INF, NAN], dtype=np.float32)
    seen = set()
    for case in range(60):
        S = int(g.integers(1, 20))
        p = VerdictPolicy([-0.25, 0.1, 0.25][case % 3], [0.25, None, INF][case % 3] if case % 2 else None,
                          alpha=[1.0, 0.3, 0.5, 1e-3][case % 4], confirm=int(g.integers(1, 4)), release=int(g.integers(1, 4)),
                          min_scores=int(g.integers(1, 4)), latch=case % 7 == 0, verifier_enter=[None, -0.5, 0.3][case % 3])
        m, st = new_state(S)
        m2, st2 = m.copy(), st.astype(np.int64)
        for step in range(12):
            A = int(g.integers(1, S + 1))
            slots = g.permutation(S)[:A]
            sc = values[g.integers(0, values.size, A)] if step % 2 else g.standard_normal(A).astype(np.float32)
            ks = g.integers(0, 1000, A)
            ver = np.where(g.random(A) < 0.2, g.standard_normal(A), np.nan).astype(np.float32)
            ev = p.step_reference(slots, sc, ks, m, st, ver)
            want = _by_definition(p, slots.tolist(), sc, ks, m2, st2, ver)
            assert ev == want, (case, step)
            assert m.view(np.int32).tolist() == m2.view(np.int32).tolist() and st.tolist() == st2.tolist(), (case, step)
            seen |= {e[1] for e in ev}
    assert seen == {1, 2, 3}


def test_thresholds_compare_in_fp32_and_are_rounded_once():
    from afx.verdict import VerdictPolicy
    # a score equal to enter is not below it; the next fp32 below is
    below = float(np.nextafter(f32(0.5), f32(0)))
    assert _run(VerdictPolicy(0.5), [0.5, below])[0] == [0, 1]
    # an m1 equal to exit counts as >= exit; the next fp32 below does not
    assert _run(VerdictPolicy(0.25, 0.5), [0.0, below, 0.5])[0] == [1, 0, 3]
    # 0.1 (double) rounds UP to fp32(0.1): the score fp32(0.1) is not below enter = 0.1, and is >= exit = 0.1
    assert float(f32(0.1)) > 0.1 and _run(VerdictPolicy(0.1), [f32(0.1)])[0] == [0]
    assert _run(VerdictPolicy(0.0, 0.1), [-1.0, f32(0.1)])[0] == [1, 3]
    p = VerdictPolicy(0.1, 0.7, alpha=0.3, verifier_enter=0.2)
    assert p.params() == dict(enter=float(f32(0.1)), exit=float(f32(0.7)), alpha=float(f32(0.3)), confirm=1, release=1, min_scores=1,
                              latch=False, verifier_enter=float(f32(0.2)))
    assert all(type(v) in (int, float, bool) for v in p.params().values())
    assert VerdictPolicy(0.5).params()["exit"] == 0.5 and VerdictPolicy(0.5).params()["verifier_enter"] is None


def test_smoothing_is_three_roundings_and_the_first_score_is_taken_whole():
    from afx.verdict import VerdictPolicy
    p = VerdictPolicy(-10.0, alpha=0.3)
    s0, s1 = f32(0.7310586), f32(-0.4621172)
    _, _, m, st = _run(p, [s0])
    assert _bits(m) == _bits(s0) and st == [1, 0, 0, -1]
    _, _, m, st = _run(p, [s0, s1])
    want = f32(s0 + f32(f32(0.3) * f32(s1 - s0)))
    assert _bits(m) == _bits(want) and st[0] == 2
    # signed zeros: m + alpha * (s - m) with s = m = -0.0 is -0.0 + (+0.0) = +0.0
    assert _bits(_run(p, [-0.0, -0.0])[2]) == _bits(0.0) and _bits(_run(p, [-0.0])[2]) == _bits(-0.0)


def test_min_scores_confirm_release_and_latch():
    from afx.verdict import VerdictPolicy
    # min_scores delays the first raise: scores 1 and 2 do not count, the run starts at the third
    assert _run(VerdictPolicy(0.0, min_scores=3), [-1, -1, -1, -1])[0] == [0, 0, 1, 0]
    assert _run(VerdictPolicy(0.0, min_scores=3, confirm=2), [-1, -1, -1, -1, -1])[0] == [0, 0, 0, 1, 0]
    # confirm: the run is broken by one contrary score
    kinds, on, _, st = _run(VerdictPolicy(0.0, confirm=3), [-1, -1, 1, -1, -1, -1, -1])
    assert kinds == [0, 0, 0, 0, 0, 1, 0] and on == [0, 0, 0, 0, 0, 1, 1] and st == [7, 0, 1, 6]
    # release: the same on the way out; since is -1 again when cleared
    kinds, on, _, st = _run(VerdictPolicy(0.0, 0.5, release=2), [-1, 1, 0.25, 1, 1, 1])
    assert kinds == [1, 0, 0, 0, 3, 0] and on == [1, 1, 1, 1, 0, 0] and st == [6, 0, 0, -1]
    # between enter and exit nothing moves either way (hysteresis)
    assert _run(VerdictPolicy(0.0, 0.5), [0.25, -1, 0.25, 0.25, 0.5])[0] == [0, 1, 0, 0, 3]
    # mid-run state: two of three confirmations
    assert _run(VerdictPolicy(0.0, confirm=3), [-1, -1])[3] == [2, 2, 0, -1]
    # latch never clears, and the run is not touched while latched
    kinds, on, _, st = _run(VerdictPolicy(0.0, latch=True), [-1, 5, 5, 5, -1])
    assert kinds == [1, 0, 0, 0, 0] and on == [1] * 5 and st == [5, 0, 1, 1]
    # a raise and a clear can alternate
    assert _run(VerdictPolicy(0.0), [-1, 1, -1, 1])[0] == [1, 3, 1, 3]


def test_nan_rows_infinities_and_named_slots_only():
    from afx.verdict import VerdictPolicy, new_state
    p = VerdictPolicy(0.0, 0.5, alpha=0.5, confirm=2)
    # a NaN row changes nothing: the run of two is not broken, n does not count it, and it logs nothing
    kinds, _, m, st = _run(p, [-1, NAN, -1])
    assert kinds == [0, 0, 1] and st == [2, 0, 1, 3] and _bits(m) == _bits(-1.0)
    # -inf raises; +inf after -inf makes m1 = -inf + 0.5 * (inf - -inf) = NaN: neither < enter nor >= exit, so the alarm stays
    kinds, on, m, _ = _run(VerdictPolicy(0.0, 0.5, alpha=0.5), [-INF, INF, 1.0])
    assert kinds == [1, 0, 0] and on == [1, 1, 1] and np.isnan(m)
    # ... and while clear a NaN m1 breaks the run
    assert _run(VerdictPolicy(0.0, alpha=0.5, confirm=2), [INF, -INF, -1])[0] == [0, 0, 0]
    # +inf clears, alpha = 1
    assert _run(VerdictPolicy(0.0, INF), [-1, 3e38, INF])[0] == [1, 0, 3]
    # only named slots move
    m, st = new_state(4)
    m0, st0 = m.copy(), st.copy()
    ev = VerdictPolicy(0.0).step_reference([2, 0], f32([-1, 1]), [7, 9], m, st)
    assert ev == [(2, 1, 7, _bits(-1.0))] and st.tolist() == [[1, 0, 0, -1], [0, 0, 0, -1], [1, 0, 1, 7], [0, 0, 0, -1]]
    assert m.view(np.int32)[[1, 3]].tolist() == m0.view(np.int32)[[1, 3]].tolist()
    # n saturates
    st[0, 0] = N_MAX - 1
    for want in (N_MAX, N_MAX):
        VerdictPolicy(0.0).step_reference([0], f32([1]), 1, m, st)
        assert int(st[0, 0]) == want
    # refusals of the reference itself
    for args in (([0, 0], f32([1, 1]), 1), ([4], f32([1]), 1), ([0], f32([1, 1]), 1), ([0, 1], f32([1, 1]), [1, 2, 3])):
        with pytest.raises(ValueError):
            VerdictPolicy(0.0).step_reference(*args, m, st)
    assert (m0 is not m) and st0.dtype == np.int32


def test_the_verifier_raises_at_once_restarts_the_run_and_plays_no_part_in_an_alarm():
    from afx.verdict import VerdictPolicy
    p = VerdictPolicy(0.0, 0.5, confirm=3, min_scores=4, verifier_enter=-0.5)
    # raises immediately, unarmed (before min_scores, whatever the screen's score), kind 2
    kinds, on, _, st = _run(p, [5.0], [-1.0])
    assert kinds == [2] and st == [1, 0, 1, 1]
    # a verifier score equal to its threshold is not below it: it restarts the run instead
    assert _run(p, [5.0], [-0.5])[0] == [0]
    # the verifier restarts the confirm run: without it the third low score raises, with a clearing score in between it takes three more
    q = VerdictPolicy(0.0, confirm=3, verifier_enter=-0.5)
    assert _run(q, [-1] * 6, [NAN] * 6)[0] == [0, 0, 1, 0, 0, 0]
    assert _run(q, [-1] * 6, [NAN, NAN, 0.9, NAN, NAN, NAN])[0] == [0, 0, 0, 0, 0, 1]
    # while the alarm is on, the verifier plays no part: a high verifier score does not clear it, a low one logs nothing
    kinds, on, _, _ = _run(q, [-1, -1, -1, -1, -1, 1], [NAN, NAN, NAN, 0.9, -0.9, NAN])
    assert kinds == [0, 0, 1, 0, 0, 3] and on == [0, 0, 1, 1, 1, 0]
    # verifier_enter=None: the column is ignored
    assert _run(VerdictPolicy(0.0), [5.0], [-1.0])[0] == [0]


def test_run_reference_is_a_fresh_stream():
    from afx.verdict import VerdictPolicy
    p = VerdictPolicy(0.0, 0.5, alpha=0.5, confirm=2)
    sc = [-1, -1, NAN, 2, 2, -3, -3]
    ev, on = p.run_reference(sc)
    kinds, on2, _, _ = _run(p, sc)
    assert [(e[1], e[2]) for e in ev] == [(k, j + 1) for j, k in enumerate(kinds) if k] and on == [bool(o) for o in on2]
    assert [e[2] for e in p.run_reference(sc, hop_index=[10, 20, 30, 40, 50, 60, 70])[0]] == [20, 40, 70]
    assert p.run_reference([]) == ([], [])


def test_policy_arguments_are_validated():
    from afx.verdict import VerdictPolicy
    VerdictPolicy(np.float32(-2.5), np.float64(0), np.float32(0.5), np.int64(2), np.int32(1), 1, np.bool_(True), -INF)
    VerdictPolicy(-INF, INF)
    for bad in (dict(enter=NAN), dict(enter="0"), dict(enter=None), dict(enter=True), dict(enter=1e39), dict(exit=NAN), dict(exit=-0.1),
                dict(exit="1"), dict(exit=-1e39), dict(verifier_enter=NAN), dict(verifier_enter="x"), dict(verifier_enter=1e39),
                dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0001), dict(alpha=NAN), dict(alpha="1"), dict(alpha=1e-50), dict(alpha=True),
                dict(confirm=0), dict(confirm=1.0), dict(confirm=True), dict(confirm=1 << 31), dict(release=0), dict(release=-1),
                dict(release=1 << 31), dict(min_scores=0), dict(min_scores=2.5), dict(min_scores=1 << 31), dict(latch=1), dict(latch=None)):
        with pytest.raises(ValueError):
            VerdictPolicy(**dict(dict(enter=0.0), **bad))
    assert VerdictPolicy(0.0, confirm=N_MAX, release=N_MAX, min_scores=N_MAX).params()["confirm"] == N_MAX


def _bare(S=2, hop=H, window=16000):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=window, hop=hop, device="cpu")


class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


def test_verdict_scorer_refuses_what_it_cannot_wrap_and_presents_the_inner_surface(built):
    from afx._lib import AfxError
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    from afx.streaming import ResamplingScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, Verdicts, VerdictScorer
    pol = VerdictPolicy(0.0, 0.5, alpha=0.3, confirm=2, verifier_enter=-0.5)
    cascade = CascadeScorer(_bare(), _Model(), CascadePolicy(0.0, 2))
    vs = VerdictScorer(_bare(S=3), pol)
    for front in (ResamplingScorer(_bare(), 8000), PacketScorer(_bare(), 8000, "mulaw"), GatedScorer(_bare()), vs, object(), None):
        with pytest.raises(ValueError):
            VerdictScorer(front, pol)
    with pytest.raises(ValueError):
        VerdictScorer(_bare(), "default")
    with pytest.raises(ValueError):
        VerdictScorer(_bare(S=8193, hop=400, window=400), pol)
    for args in ((0, pol), (8193, pol), (2.0, pol), (2, None)):
        with pytest.raises(ValueError):
            Verdicts(*args, device="cpu")
    assert (vs.S, vs.hop, vs.window, vs.device.type) == (3, H, 16000, "cpu")
    assert vs._slot_list([2, 0], ordered=True) == [2, 0] and vs.samples_seen.tolist() == [0, 0, 0]
    assert vs.alarm.tolist() == [False] * 3 and vs.alarm.dtype == torch.bool and torch.isnan(vs.smoothed).all()
    assert vs.alarm_since.tolist() == [-1] * 3 and vs.verdicts.st.tolist() == [[0, 0, 0, -1]] * 3
    assert vs.verdicts.cap == 1024 and Verdicts(300, pol, "cpu").cap == 1200 and vs.verdicts.log.numel() == 1 + 4 * 1024
    assert [a.tolist() for a in vs.take_events()] == [[], [], [], []]
    # no CPU fallback: push and update raise, and nothing moved
    with pytest.raises(AfxError):
        vs.push(torch.zeros(3, H))
    with pytest.raises(AfxError):
        vs.verdicts.update(torch.zeros(3), hop_index=1)
    assert vs.verdicts._pending == 0 and vs.samples_seen.tolist() == [0, 0, 0]
    for args, kw in (((torch.zeros(2),), dict(hop_index=1)), ((torch.zeros(3, dtype=torch.float64),), dict(hop_index=1)),
                     ((torch.zeros(1), [3]), dict(hop_index=1)), ((torch.zeros(2), [1, 1]), dict(hop_index=1)),
                     ((torch.zeros(3),), dict(hop_index=[1, 2])), ((torch.zeros(3),), dict(hop_index=1.5)),
                     ((torch.zeros(3),), dict(hop_index=-1)), ((torch.zeros(3),), dict(hop_index=1, verified=torch.zeros(2)))):
        with pytest.raises(ValueError):
            vs.verdicts.update(*args, **kw)
    # the gate and the fronts accept it in place of a scorer, around a cascade too; the cascade keeps refusing it as a screen
    inner = VerdictScorer(cascade, pol)
    for front in (GatedScorer(vs), PacketScorer(GatedScorer(inner), 8000, "mulaw"), JitterScorer(GatedScorer(inner), 8000, "mulaw", 4)):
        meta = front.state_meta()
        assert meta["verdict"] == 1 and meta["verdict_policy"] == pol.params() and meta["gate"] == 1
    assert PacketScorer(GatedScorer(inner), 8000, "mulaw").state_meta()["cascade"] == 1
    with pytest.raises(ValueError):
        CascadeScorer(vs, _Model(), CascadePolicy(0.0, 2))
    with pytest.raises(ValueError):
        GatedScorer(GatedScorer(vs))
    with pytest.raises(ValueError):
        GatedScorer(object())


def test_export_and_import_on_the_host_and_every_refusal_leaves_the_scorer_unchanged(built):
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.streaming import StreamState
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    pol = VerdictPolicy(0.0, 0.5, alpha=0.3, confirm=3, release=2)
    a = VerdictScorer(_bare(S=3), pol)
    a.scorer.ring[:] = torch.arange(3 * 16000, dtype=torch.float32).reshape(3, 16000)
    a.scorer._seen[:] = torch.tensor([8000, 20000, 0])
    a.verdicts.m[:] = torch.tensor([-0.75, 0.125, NAN])
    a.verdicts.st[:] = torch.tensor([[2, 1, 1, 1], [5, 2, 0, -1], [0, 0, 0, -1]], dtype=torch.int32)  # in alarm mid-release, mid-confirm, new
    st = a.export_slots([1, 0])
    assert st.tensors["verdict_state"].tolist() == [[5, 2, 0, -1], [2, 1, 1, 1]] and st.tensors["verdict_state"].dtype == torch.int64
    assert st.tensors["verdict_m"].tolist() == [0.125, -0.75] and st.tensors["verdict_m"].dtype == torch.float32
    assert st.meta["verdict"] == 1 and st.meta["verdict_policy"] == pol.params() and st.seen.tolist() == [20000, 8000]
    b = VerdictScorer(_bare(S=4), pol)
    b.verdicts.log[:3] = torch.tensor([0, 7, 7], dtype=torch.int32)

    def snap(c):
        return [c.verdicts.m.clone().nan_to_num(-7.0), c.verdicts.st.clone(), c.verdicts.log.clone(), c.scorer.ring.clone(), c.samples_seen]

    before = snap(b)
    t = st.tensors
    state = lambda rows: dict(t, verdict_state=torch.tensor(rows))  # noqa: E731
    foreign = [
        a.scorer.export_slots([1, 0]),                                                     # a bare state: no verdict part
        GatedScorer(_bare(S=3)).export_slots([1, 0]),
        st.tensors, None,
        StreamState(dict(st.meta, verdict=2), st.seen, t),                                 # another format
        StreamState(dict(st.meta, verdict_policy=dict(st.meta["verdict_policy"], confirm=4)), st.seen, t),
        StreamState({k: v for k, v in st.meta.items() if k != "verdict_policy"}, st.seen, t),
        StreamState(st.meta, st.seen, {k: v for k, v in t.items() if k != "verdict_m"}),
        StreamState(st.meta, st.seen, state([[5, 2, 2, -1], [2, 1, 1, 1]])),               # on outside {0, 1}
        StreamState(st.meta, st.seen, state([[5, 2, -1, -1], [2, 1, 1, 1]])),
        StreamState(st.meta, st.seen, state([[-1, 2, 0, -1], [2, 1, 1, 1]])),              # n < 0
        StreamState(st.meta, st.seen, state([[5, 3, 0, -1], [2, 1, 1, 1]])),               # run = confirm while clear
        StreamState(st.meta, st.seen, state([[5, -1, 0, -1], [2, 1, 1, 1]])),
        StreamState(st.meta, st.seen, state([[5, 2, 0, -1], [2, 2, 1, 1]])),               # run = release while on
        StreamState(st.meta, st.seen, state([[5, 2, 0, 4], [2, 1, 1, 1]])),                # since set while clear
        StreamState(st.meta, st.seen, state([[5, 2, 0, -1], [2, 1, 1, -1]])),              # on without since
        StreamState(st.meta, st.seen, state([[0, 0, 0, -1], [2, 1, 1, 1]])),               # n == 0 with a number in m
        StreamState(st.meta, st.seen, dict(t, verdict_m=torch.tensor([NAN, -0.75]))),      # m NaN after scores
        StreamState(st.meta, st.seen, dict(t, verdict_m=torch.zeros(2, dtype=torch.float64))),
        StreamState(st.meta, st.seen, dict(t, verdict_state=t["verdict_state"].to(torch.int32))),
        StreamState(st.meta, st.seen, dict(t, verdict_state=t["verdict_state"][:, :3])),
        StreamState(dict(st.meta, window=32000), st.seen, t),                              # the inner scorer's own refusal
        VerdictScorer(_bare(S=3), VerdictPolicy(0.0, 0.5, alpha=0.3, confirm=3, release=3)).export_slots([1, 0]),
    ]
    for i, f in enumerate(foreign):
        with pytest.raises(ValueError):
            b.import_slots([3, 1], f)
        assert all(torch.equal(u, v) for u, v in zip(before, snap(b))), i
    with pytest.raises(ValueError):
        b.import_slots([3], st)  # two sessions for one slot
    with pytest.raises(ValueError):
        b.scorer.import_slots([3, 1], st)  # a bare scorer refuses a verdict state
    b.import_slots([3, 1], StreamState.from_state_dict(st.state_dict()))
    assert b.verdicts.st.tolist() == [[0, 0, 0, -1], [2, 1, 1, 1], [0, 0, 0, -1], [5, 2, 0, -1]] and b.samples_seen.tolist() == [0, 8000, 0, 20000]
    assert b.verdicts.m[[3, 1]].tolist() == [0.125, -0.75] and torch.isnan(b.verdicts.m[[0, 2]]).all()
    assert b.alarm.tolist() == [False, True, False, False] and b.alarm_since.tolist() == [-1, 1, -1, -1]
    assert torch.equal(b.verdicts.log, before[2])  # the log belongs to the scorer: it did not move
    back = b.export_slots([3, 1])
    assert all(torch.equal(back.tensors[k], st.tensors[k]) for k in st.tensors) and back.meta == st.meta
    # a new stream round-trips too (m NaN, n 0)
    b.import_slots([0], a.export_slots([2]))
    # reset: the inner session and the verdict state; the log stays
    b.reset([1, 3])
    assert b.verdicts.st.tolist() == [[0, 0, 0, -1]] * 4 and torch.isnan(b.verdicts.m).all() and b.samples_seen.tolist() == [0] * 4
    assert torch.equal(b.verdicts.log, before[2])
    # through a cascade and the gate: every layer peels its own part
    mk = lambda: GatedScorer(VerdictScorer(CascadeScorer(_bare(S=2), _Model(), CascadePolicy(0.0, 2)), pol))  # noqa: E731
    g1, g2 = mk(), mk()
    g1.scorer.verdicts.st[1] = torch.tensor([4, 0, 1, 3], dtype=torch.int32)
    g1.scorer.verdicts.m[1] = -2.0
    g2.import_slots([0], g1.export_slots([1]))
    assert g2.scorer.verdicts.st.tolist() == [[4, 0, 1, 3], [0, 0, 0, -1]] and float(g2.scorer.smoothed[0]) == -2.0
    with pytest.raises(ValueError):
        g2.import_slots([0], GatedScorer(CascadeScorer(_bare(S=2), _Model(), CascadePolicy(0.0, 2))).export_slots([1]))


def test_the_host_takes_events_itself_before_the_log_could_overflow(monkeypatch):
    """The launch replaced by step_reference on host tensors: the bookkeeping around it is the product's."""
    from afx.verdict import VerdictPolicy, Verdicts
    S = 300
    p = VerdictPolicy(0.0)  # alpha 1, confirm 1, release 1: a slot whose score changes sign logs an event
    vd = Verdicts(S, p, "cpu")
    assert vd.cap == 1200
    drains = []

    def launch(self, scores, verified, slots, hop_index):
        m, st, log = self.m.numpy(), self.st.numpy(), self.log.numpy()
        for e in p.step_reference(slots, scores.numpy(), hop_index, m, st):
            if log[0] < self.cap:
                log[1 + 4 * log[0]:5 + 4 * log[0]] = e
            log[0] += 1

    real_drain = Verdicts._drain

    def drain(self):
        drains.append(self._pending)
        return real_drain(self)

    monkeypatch.setattr(Verdicts, "_launch", launch)
    monkeypatch.setattr(Verdicts, "_drain", drain)
    m, st = np.full(S, np.nan, np.float32), np.tile(np.array([0, 0, 0, -1]), (S, 1))
    want = []
    for k in range(1, 12):  # every slot alternates: 300 events per update, 1200 fit
        sc = np.full(S, -1.0 if k % 2 else 1.0, np.float32)
        want += p.step_reference(np.arange(S), sc, k, m, st)
        vd.update(torch.from_numpy(sc), hop_index=k)
        assert vd._pending <= vd.cap and int(vd.log[0]) <= vd.cap
    # updates 1-4 filled the bound (1200); the 5th and the 9th made the host take the events itself
    assert drains == [1200, 1200] and len(vd._kept) == 2 and vd._pending == 900 and int(vd.log[0]) == 900
    got = vd.take_events()
    assert len(want) == 11 * S and list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].view(np.int32).tolist())) == want
    assert got[3].dtype == np.float32 and got[0].dtype == np.int32
    assert vd._pending == 0 and int(vd.log[0]) == 0 and vd._kept == [] and [a.size for a in vd.take_events()] == [0] * 4
    # a subset update counts its own rows only
    vd.update(torch.full((5,), 1.0), [9, 2, 7, 4, 0], hop_index=[1, 2, 3, 4, 5])  # (every slot is in alarm: these clear)
    assert vd._pending == 5
    got = vd.take_events()
    assert got[0].tolist() == [9, 2, 7, 4, 0] and got[1].tolist() == [3] * 5 and got[2].tolist() == [1, 2, 3, 4, 5]
    # a count beyond what the host allowed means events were lost: an error, not a silent truncation
    vd.update(torch.full((2,), 1.0), [0, 1], hop_index=1)
    vd.log[0] = 3
    with pytest.raises(RuntimeError):
        vd.take_events()
    assert vd._pending == 0 and int(vd.log[0]) == 0  # (the bound follows the cleared count)
    vd.update(torch.full((2,), -1.0), [0, 1], hop_index=2)
    assert vd.take_events()[1].tolist() == [1, 1]  # and the log goes on
    vd._pending = 2 * vd.cap
    vd.log[0] = vd.cap + 1
    with pytest.raises(RuntimeError):
        vd.take_events()


def test_timeline_alarms():
    from afx.timeline import Timeline
    from afx.verdict import VerdictPolicy
    n = 8
    ends = [(j + 1) * H for j in range(n)]
    starts = [max(e - 16000, 0) for e in ends]
    tl = Timeline([1, -1, -1, 1, 1, -1, 1, -1], starts, ends)
    assert tl.alarms(VerdictPolicy(0.0)) == [(0.5, 1.0, 1), (1.5, 1.75, 1), (2.0, None, 1)]
    assert tl.alarms(VerdictPolicy(0.0, confirm=2, release=2)) == [(0.75, 1.25, 1)]
    assert tl.alarms(VerdictPolicy(0.0, latch=True)) == [(0.5, None, 1)]
    assert tl.alarms(VerdictPolicy(-5.0)) == [] and Timeline([], [], []).alarms(VerdictPolicy(0.0)) == []
    # another input rate: the times are the windows' ends in seconds of the input
    assert Timeline([1, -1], [0, 0], [2000, 4000], sample_rate=8000).alarms(VerdictPolicy(0.0)) == [(0.5, None, 1)]


def test_verdict_entry_point_is_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bafx_k_verdict\s*\(", src) and hasattr(lib, "afx_k_verdict") and "afx_k_verdict" in built.SIGNATURES
    l = built.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = [p, 1, None, p, 1, p, p, 2, 0.5, 0.0, 0.5, -0.5, 1, 1, 1, 0, p, 4]
    bad = {0: None, 3: None, 5: None, 6: None, 16: None}  # a NULL required pointer
    cases = [(i, v) for i, v in bad.items()]
    cases += [(1, 0), (4, 0), (4, 8193), (4, -1), (7, 0), (8, 0.0), (8, 1.5), (8, NAN), (8, -0.5), (9, NAN), (10, NAN), (11, NAN),
              (9, 0.75), (12, 0), (13, 0), (14, 0), (12, -3), (15, 2), (15, -1), (17, -1)]
    # refused on the host, with pointers that would pass the NULL check never dereferenced: nothing is launched
    for i, v in cases:
        args = list(good)
        args[i] = v
        assert l.afx_k_verdict(*args, None) != 0 and b"verdict" in l.afx_last_error(), (i, v)

"""The verdict layer on the GPU (afx/verdict.py; afx_k_verdict).  Every comparison is exact, bits of the smoothed score
included: the kernel against ``VerdictPolicy.step_reference`` over consecutive launches that carry ``m``, ``st`` and the log
(the whole state and log after every launch, unnamed rows' bytes included); the log's edges; special values; bad rows and
bad arguments; ``VerdictScorer`` end to end for the four scorer kinds (its scores against a dry run of the bare scorer, its
events against ``run_reference`` applied to those scores per slot), around a cascade, behind the gate and the packet front,
sessions moved between scorers, and the one-slot stream against ``Timeline.alarms``.

Tiny engines as in tests/test_gpu_cascade.py: a 1-layer Conformer student scores, a 1-layer XLSR_AASIST teacher verifies,
H = 4000.  The exact scorers run a 1-s window, the KV-cached scorer its 4-s window."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
INF, NAN = float("inf"), float("nan")
SENT = -77


def fixture_stream():
    g = np.random.default_rng(0)
    x = (0.002 * g.standard_normal(128000)).astype(np.float32)
    t = np.arange(128000) / 16000
    for a, b in [(0.5, 1.3), (2.0, 2.15), (3.0, 5.0), (6.5, 6.52)]:
        m = (t >= a) & (t < b)
        x[m] += (0.2 * np.sin(2 * np.pi * 180 * t[m]) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t[m]))).astype(np.float32)
    x[112000:120000] = 0
    return x


FIX = fixture_stream()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- 1. the kernel against step_reference --------------------------------------------------------------------------------
class _Mirror:
    """The state and the log of one kernel-level run, on the device and in numpy."""

    def __init__(self, S, cap, policy, pad=8):
        from afx.verdict import new_state
        self.S, self.cap, self.p = S, cap, policy
        self.m, self.st = new_state(S)
        self.log = np.full(1 + 4 * cap + pad, SENT, dtype=np.int32)  # (pad: words past the log's end, never written)
        self.log[0] = 0
        self.d_m, self.d_st, self.d_log = (torch.from_numpy(a.copy()).cuda() for a in (self.m, self.st, self.log))

    def launch(self, slots, scores, ks, ver=None, strided=False, policy=None):
        """One launch (rows with a slot outside [0, S) are left out of the reference: the kernel skips them) -> the events
        of the reference."""
        from afx._lib import call_on, lib
        p = self.p if policy is None else policy
        slots, ks, A = np.asarray(slots), np.asarray(ks), len(slots)
        sc = np.asarray(scores, dtype=np.float32)
        mat = torch.full((A, 2), 9.0)
        mat[:, 1] = torch.from_numpy(sc)
        d_sc = mat.cuda()[:, 1] if strided else torch.from_numpy(sc).cuda()
        d_v = None if ver is None else torch.from_numpy(np.asarray(ver, dtype=np.float32)).cuda()
        hdr = torch.from_numpy(np.stack([slots, ks], axis=1).astype(np.int32)).cuda()
        rc = call_on(self.d_m, lib().afx_k_verdict, _p(d_sc), 2 if strided else 1, _p(d_v), _p(hdr), A, _p(self.d_m), _p(self.d_st),
                     self.S, p.alpha, p.enter, p.exit, 0.0 if p.verifier_enter is None else p.verifier_enter, p.confirm, p.release,
                     p.min_scores, int(p.latch), _p(self.d_log), self.cap)
        torch.cuda.synchronize()
        assert rc == 0, lib().afx_last_error()
        ok = (slots >= 0) & (slots < self.S)
        ev = p.step_reference(slots[ok], sc[ok], ks[ok], self.m, self.st, None if ver is None else np.asarray(ver, dtype=np.float32)[ok])
        for e in ev:
            if self.log[0] < self.cap:
                self.log[1 + 4 * self.log[0]:5 + 4 * self.log[0]] = e
            self.log[0] += 1
        return ev

    def check(self, what):
        assert self.d_m.cpu().numpy().tobytes() == self.m.tobytes(), what
        assert self.d_st.cpu().numpy().tobytes() == self.st.tobytes(), what
        assert self.d_log.cpu().numpy().tobytes() == self.log.tobytes(), what


def _issue_policy():
    from afx.verdict import VerdictPolicy
    return VerdictPolicy(-0.25, 0.25, alpha=0.3, confirm=2, release=2, min_scores=2, verifier_enter=-0.5)


@pytest.mark.parametrize("with_verifier", [True, False])
@pytest.mark.parametrize("A", [1, 63, 64, 65, 1023, 1024, 1025, 8192])
def test_kernel_equals_the_reference_launch_by_launch(A, with_verifier):
    """One row, both sides of a wave, both sides of the 1024-row chunk, the most one launch takes.  The A named slots are a
    random subset of S = 9000, named in a new random order at every launch; scores sin(phase + 0.9 k) + 0.3 N(0, 1) per slot
    over 16 launches, 10 % NaN rows and 10 % verifier rows."""
    S, launches = 9000, 16
    g = np.random.default_rng(1000 + A)
    subset = g.permutation(S)[:A]
    phase = g.uniform(0, 2 * np.pi, S)
    mir = _Mirror(S, 16 * A, _issue_policy())  # (a slot logs at most one event per launch)
    kinds = set()
    for k in range(launches):
        slots = g.permutation(subset)
        sc = (np.sin(phase[slots] + 0.9 * k) + 0.3 * g.standard_normal(A)).astype(np.float32)
        sc[g.random(A) < 0.1] = np.nan
        ver = np.where(g.random(A) < 0.1, g.standard_normal(A), np.nan).astype(np.float32) if with_verifier else None
        ev = mir.launch(slots, sc, np.full(A, k + 1), ver, strided=True)
        mir.check((A, k))
        kinds |= {e[1] for e in ev}
    assert int(mir.log[0]) <= mir.cap  # (nothing was dropped: the whole list was compared)
    if A >= 65:  # a condition on the fixture, checked on the reference
        assert kinds == ({1, 2, 3} if with_verifier else {1, 3}), (A, kinds)


def test_log_edges_a_base_that_is_not_zero_a_full_log_and_no_log():
    from afx.verdict import VerdictPolicy
    p = VerdictPolicy(0.0)  # every change of sign is an event
    S, A = 200, 130
    slots = np.arange(A)[::-1].copy()
    # events appended at a non-zero log[0]
    mir = _Mirror(S, 400, p)
    mir.log[0] = mir.d_log[0] = 5
    assert len(mir.launch(slots, np.full(A, -1.0), np.full(A, 1))) == A
    mir.check("base 5")
    assert int(mir.log[0]) == 5 + A and mir.log[1:21].tolist() == [SENT] * 20 and mir.log[21:25].tolist()[:3] == [A - 1, 1, 1]
    # cap below the events of a launch: the first cap are stored, log[0] is the total, state and later launches unaffected
    mir = _Mirror(S, 70, p)
    for k, v in enumerate([-1.0, 1.0, -1.0]):
        assert len(mir.launch(slots, np.full(A, v), np.full(A, k + 1))) == A
        mir.check(("cap 70", k))
    assert int(mir.log[0]) == 3 * A and mir.log[1 + 4 * 69:1 + 4 * 70].tolist()[:3] == [A - 70, 1, 1] and mir.st[:A, 2].tolist() == [1] * A
    # cap = 0: counted, never stored
    mir = _Mirror(S, 0, p)
    mir.launch(slots, np.full(A, -1.0), np.full(A, 1))
    mir.check("cap 0")
    assert mir.log.tolist() == [A] + [SENT] * 8


def test_special_values_signed_zeros_thresholds_infinities_and_an_all_nan_launch():
    from afx.verdict import VerdictPolicy
    values = np.array([-INF, -1.0, -0.25, np.nextafter(np.float32(-0.25), np.float32(-1)), -0.0, 0.0, 0.25,
                       np.nextafter(np.float32(0.25), np.float32(0)), 1.0, 3.0e38, INF, NAN, 1e-45, -1e-45], dtype=np.float32)
    S = 70
    for pi, p in enumerate((VerdictPolicy(-0.25, 0.25, verifier_enter=0.0), VerdictPolicy(0.0, 0.0, alpha=0.5, confirm=2, verifier_enter=-0.25),
                            VerdictPolicy(-0.25, 0.25, alpha=0.3, release=2, min_scores=3, latch=True, verifier_enter=INF),
                            VerdictPolicy(-INF, INF, alpha=1.0), VerdictPolicy(INF, INF, alpha=0.5))):
        g = np.random.default_rng(pi)
        mir = _Mirror(S, 4096, p)
        for k in range(14):
            slots = g.permutation(S)[:S - (k % 3)]
            A = slots.size
            sc = np.full(A, NAN, np.float32) if k == 5 else (np.roll(values, k)[np.arange(A) % values.size] if k < 5 else values[g.integers(0, values.size, A)])
            ver = np.where(g.random(A) < 0.3, values[g.integers(0, values.size, A)], np.float32(NAN)).astype(np.float32)
            before = (mir.m.copy(), mir.st.copy(), mir.log.copy())
            ev = mir.launch(slots, sc, np.full(A, k), ver if p.verifier_enter is not None else None, strided=bool(k % 2))
            mir.check((pi, k))
            if k == 5:  # the launch whose rows are all NaN changed nothing
                assert ev == [] and all(a.tobytes() == b.tobytes() for a, b in zip(before, (mir.m, mir.st, mir.log)))
        assert int(mir.log[0]) > 0 or pi == 3


def test_bad_rows_are_skipped_whole_and_bad_arguments_launch_nothing():
    from afx._lib import lib
    from afx.verdict import VerdictPolicy
    S = 6
    p = _issue_policy()
    mir = _Mirror(S, 64, VerdictPolicy(0.0))
    # slot -1 and slot S sit among good rows: no state change, no event, and the good rows' events keep their order
    slots = np.array([2, -1, 0, S, 5, 1 << 20, -(1 << 20)])
    for k, v in enumerate([-1.0, 1.0]):
        ev = mir.launch(slots, np.full(slots.size, v), np.arange(slots.size) + 10 * k)
        mir.check(("bad rows", k))
        assert [e[0] for e in ev] == [2, 0, 5] and [e[2] for e in ev] == [10 * k, 10 * k + 2, 10 * k + 4]
    assert mir.st[[1, 3, 4]].tolist() == [[0, 0, 0, -1]] * 3
    # bad arguments: an error, nothing launched, no byte of the state or the log changed
    l = lib()
    A = 4
    sc, v = torch.full((A,), -1.0, device="cuda"), torch.full((A,), -1.0, device="cuda")
    hdr = torch.tensor([[0, 1], [1, 1], [2, 1], [3, 1]], dtype=torch.int32, device="cuda")
    big_sc, big_hdr = torch.full((8193,), -1.0, device="cuda"), torch.zeros(8193, 2, dtype=torch.int32, device="cuda")
    good = [sc, 1, v, hdr, A, mir.d_m, mir.d_st, S, p.alpha, p.enter, p.exit, p.verifier_enter, 2, 2, 2, 0, mir.d_log, mir.cap]
    cases = [(0, None), (3, None), (5, None), (6, None), (16, None), (1, 0), (1, -1), (4, 0), (4, -1), (7, 0), (7, -1), (8, 0.0), (8, -0.5),
             (8, 1.5), (8, NAN), (8, INF), (9, NAN), (10, NAN), (11, NAN), (10, -0.5), (12, 0), (13, 0), (14, 0), (12, -1), (15, 2), (15, -1),
             (17, -1)]
    for i, val in cases:
        args = list(good)
        args[i] = val
        rc = l.afx_k_verdict(*[_p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], None)
        torch.cuda.synchronize()
        assert rc != 0 and b"verdict" in l.afx_last_error(), (i, val)
    args = list(good)
    args[0], args[3], args[4] = big_sc, big_hdr, 8193  # more rows than one launch takes
    assert l.afx_k_verdict(*[_p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], None) != 0
    assert b"verdict" in l.afx_last_error()
    torch.cuda.synchronize()
    mir.check("bad arguments")


# ---- engines and scorers -----------------------------------------------------------------------------------------------------
_ENGINES = {}
KINDS = ["sliding", "incremental", "kv", "kv-fp16x3"]


def _student(dtype):
    if dtype not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES[dtype] = (eng, sd)
    return _ENGINES[dtype]


def _teacher():
    if "teacher" not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype="fp16")
        eng.load_state_dict(sd)
        _ENGINES["teacher"] = (eng, sd)
    return _ENGINES["teacher"]


def _screen(kind, S):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    eng, sd = _student("fp16x3" if kind == "kv-fp16x3" else "fp16")
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _quartile_and_median(scores):
    s = np.sort(np.asarray(scores, dtype=np.float32))
    return float(s[s.size // 4]), float(s[s.size // 2])


def _events_of(vs):
    slot, kind, k, sm = vs.take_events()
    assert slot.dtype == kind.dtype == k.dtype == np.int32 and sm.dtype == np.float32
    return list(zip(slot.tolist(), kind.tolist(), k.tolist(), sm.view(np.int32).tolist()))


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------
_TICKS, _RESET_AT = 22, 9


def _schedule(t):
    """None: the lock-stepped push; else the named slots, in the order named (slot 1 sits out one tick in four)."""
    return [None, [2, 0, 1], [1, 2, 0], [0, 2]][t % 4]


def _run(front, streams, S, on_tick=None):
    """Pushes the schedule into ``front``, slot 1 reset before tick _RESET_AT -> per tick (slots in the order of the returned
    scores, the scores)."""
    pos, out = [0] * S, []
    for t in range(_TICKS):
        if t == _RESET_AT:
            front.reset([1])
        named = _schedule(t)
        order = list(range(S)) if named is None else named
        chunk = torch.from_numpy(np.stack([streams[s][pos[s]:pos[s] + H] for s in order])).cuda()
        sc = front.push(chunk) if named is None else front.push(chunk, named)
        assert sc.shape == (len(order),) and sc.dtype == torch.float32 and sc.is_cuda
        out.append((order, sc.clone()))
        if on_tick is not None:
            on_tick(t, order)
        for s in order:
            pos[s] += H
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_end_to_end_equals_the_bare_scorer_and_the_reference(kind):
    """Subsets and orders of named slots and a reset mid-run.  enter / exit: the lower quartile / the median of the bare
    scorer's own scores; the VerdictScorer runs the two thresholds alone, so the reference raises and clears, and the test
    asserts that it does.  A stand-alone ``Verdicts`` fed the same score tensors runs a smoothing policy with run lengths of
    2 beside it (an extra: no condition on its events)."""
    from afx.verdict import VerdictPolicy, Verdicts, VerdictScorer, new_state
    S = 3
    streams = [np.roll(FIX, -o)[:_TICKS * H].copy() for o in (0, 30000 + 57, 44000)]
    dry = _run(_screen(kind, S), streams, S)
    enter, exit_ = _quartile_and_median(torch.cat([sc for _, sc in dry]).cpu().numpy())  # from the bare scorer's own scores
    pol = VerdictPolicy(enter, exit_)
    slow = VerdictPolicy(enter, exit_, alpha=0.5, confirm=2, release=2, min_scores=2)
    vs = VerdictScorer(_screen(kind, S), pol)
    alone = Verdicts(S, slow, "cuda")
    seen = np.zeros(S, dtype=np.int64)
    state, state2 = new_state(S), new_state(S)
    want, want2, on_at_reset = [], [], []
    per_slot = [[[]] for _ in range(S)]  # per slot, per session: the (hop index, score) pairs

    def on_tick(t, order):
        if t == _RESET_AT:  # (the reset came before this tick's push)
            on_at_reset.append(int(state[1][1, 2]))
            seen[1] = 0
            alone.reset([1])
            for m, st in (state, state2):
                m[1], st[1] = NAN, (0, 0, 0, -1)
            per_slot[1].append([])
        seen[order] += H
        sc = dry[t][1].cpu().numpy()
        want.extend(pol.step_reference(order, sc, seen[order] // H, *state))
        want2.extend(slow.step_reference(order, sc, seen[order] // H, *state2))
        for s, v in zip(order, sc):
            per_slot[s][-1].append((int(seen[s] // H), v))
        alone.update(dry[t][1], order, hop_index=seen[order] // H)

    got = _run(vs, streams, S, on_tick)
    for t, ((o1, a), (o2, b)) in enumerate(zip(got, dry)):
        assert o1 == o2 and _same_bits(a, b), (kind, t)  # the verdict layer never changes a score
    ev = _events_of(vs)
    print(f"verdict end to end [{kind}]: enter {enter!r} exit {exit_!r}; events {[(e[0], e[1], e[2]) for e in ev]}; "
          f"smoothing policy: {[(e[0], e[1], e[2]) for e in want2]}; slot 1 in alarm at its reset: {on_at_reset}")
    assert ev == want and _events_of(vs) == []
    assert {1, 3} <= {e[1] for e in want}, "the fixture raised and cleared no alarm under the reference"
    # per slot the events are run_reference's over that slot's scores, session by session
    for s in range(S):
        ref = []
        for session in per_slot[s]:
            ref += [(s,) + e[1:] for e in pol.run_reference([v for _, v in session], [k for k, _ in session])[0]]
        assert [e for e in ev if e[0] == s] == ref, (kind, s)
    assert vs.alarm.dtype == torch.bool and vs.alarm.cpu().tolist() == [bool(v) for v in state[1][:, 2]]
    assert _same_bits(vs.smoothed, torch.from_numpy(state[0])) and vs.alarm_since.cpu().tolist() == state[1][:, 3].tolist()
    assert vs.verdicts.st.cpu().numpy().tobytes() == state[1].tobytes() and vs.samples_seen.tolist() == seen.tolist()
    assert _events_of(alone) == want2
    assert alone.st.cpu().numpy().tobytes() == state2[1].tobytes() and _same_bits(alone.m, torch.from_numpy(state2[0]))


def test_update_reads_a_score_column_in_place_and_an_expanded_one_once():
    """A column of a logits matrix is read with its stride; an expanded tensor (stride 0: one value in memory) names A rows
    of one float and is not read past it."""
    from afx.verdict import VerdictPolicy, Verdicts, new_state
    p = VerdictPolicy(0.0, alpha=0.5)
    vd = Verdicts(7, p, "cuda")
    m, st = new_state(7)
    logits = torch.tensor([[9.0, -1.0], [9.0, 2.0], [9.0, -3.0]], device="cuda")
    one = torch.tensor([-4.0], device="cuda")
    assert logits[:, 1].stride(0) == 2 and one.expand(5).stride(0) == 0
    want = p.step_reference([4, 0, 6], [-1.0, 2.0, -3.0], 1, m, st)
    vd.update(logits[:, 1], [4, 0, 6], hop_index=1)
    want += p.step_reference([1, 2, 3, 4, 5], np.full(5, -4.0, np.float32), 2, m, st)
    vd.update(one.expand(5), [1, 2, 3, 4, 5], hop_index=2)
    want += p.step_reference([0], [-8.0], 3, m, st)
    vd.update(one.expand(1) * 2, [0], hop_index=3)
    assert _events_of(vd) == want and [e[:3] for e in want] == [(4, 1, 1), (6, 1, 1), (1, 1, 2), (2, 1, 2), (3, 1, 2), (5, 1, 2), (0, 1, 3)]
    assert vd.st.cpu().numpy().tobytes() == st.tobytes() and _same_bits(vd.m, torch.from_numpy(m))


def test_reset_mid_alarm_starts_a_new_stream():
    from afx.verdict import VerdictPolicy, VerdictScorer
    vs = VerdictScorer(_screen("incremental", 2), VerdictPolicy(INF, INF, alpha=0.5, confirm=2))  # every finite score counts
    hop = lambda t: torch.from_numpy(np.stack([FIX[t * H:(t + 1) * H], FIX[40000 + t * H:40000 + (t + 1) * H]])).cuda()  # noqa: E731
    for t in range(3):
        vs.push(hop(t), [0, 1])
    assert vs.alarm.tolist() == [True, True] and vs.alarm_since.tolist() == [2, 2]
    vs.reset([1])
    assert vs.alarm.tolist() == [True, False] and vs.alarm_since.tolist() == [2, -1] and bool(torch.isnan(vs.smoothed[1]))
    assert vs.verdicts.st.tolist() == [[3, 0, 1, 2], [0, 0, 0, -1]]
    vs.push(hop(3), [0, 1])
    vs.push(hop(4), [0, 1])
    ev = _events_of(vs)  # the log is the scorer's: the reset left the earlier events in it
    assert [e[:3] for e in ev] == [(0, 1, 2), (1, 1, 2), (1, 1, 2)] and vs.alarm_since.tolist() == [2, 2] and vs.samples_seen.tolist() == [5 * H, 2 * H]


def test_around_a_cascade_the_verifier_raises_and_restarts_runs():
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.verdict import VerdictPolicy, VerdictScorer, new_state
    S, ticks = 3, 14
    teacher, tsd = _teacher()
    cpol = CascadePolicy(INF, 1, 2, 2 * H)  # from 2 H on the lowest-scoring slot out of cooldown is verified
    streams = [np.roll(FIX, -o)[:ticks * H].copy() for o in (0, 30000 + 57, 44000)]
    order = [[0, 1, 2], [2, 0, 1]]

    def run(front, cascade):
        out = []
        for t in range(ticks):
            named = order[t % 2]
            chunk = torch.from_numpy(np.stack([streams[s][t * H:(t + 1) * H] for s in named])).cuda()
            sc = front.push(chunk, named).clone()
            v = np.full(S, NAN, np.float32)
            entries = cascade.take_events()  # (the verdict layer peeks: the cascade's log is intact for its caller)
            assert len(entries) <= 1
            for slots, _at, _s, vsc in entries:
                v[[named.index(s) for s in slots.tolist()]] = vsc.cpu().numpy()
            out.append((named, sc, v))
        return out

    dry_c = CascadeScorer(_screen("kv", S), teacher, cpol, state_dict=tsd)
    dry = run(dry_c, dry_c)
    vall = np.concatenate([v[~np.isnan(v)] for _, _, v in dry])
    assert vall.size >= 6
    enter, exit_ = _quartile_and_median(torch.cat([sc for _, sc, _ in dry]).cpu().numpy())
    pol = VerdictPolicy(enter, exit_, alpha=0.5, confirm=2, verifier_enter=float(np.sort(vall)[vall.size // 2]))
    cs = CascadeScorer(_screen("kv", S), teacher, cpol, state_dict=tsd)
    vs = VerdictScorer(cs, pol)
    got = run(vs, cs)
    state, want = new_state(S), []
    for t, ((named, sc, v), (_, sc0, v0)) in enumerate(zip(got, dry)):
        assert _same_bits(sc, sc0) and v.tobytes() == v0.tobytes(), t
        want += pol.step_reference(named, sc.cpu().numpy(), t + 1, *state, v)
    ev = _events_of(vs)
    print(f"verdict around a cascade: verifier_enter {pol.verifier_enter!r}, events {[(e[0], e[1], e[2]) for e in ev]}")
    assert ev == want and 2 in {e[1] for e in want}
    assert vs.verdicts.st.cpu().numpy().tobytes() == state[1].tobytes() and _same_bits(vs.smoothed, torch.from_numpy(state[0]))
    # without verifier_enter the verifier's scores play no part
    none = VerdictPolicy(enter, exit_, alpha=0.5, confirm=2)
    cs2 = CascadeScorer(_screen("kv", S), teacher, cpol, state_dict=tsd)
    vs2 = VerdictScorer(cs2, none)
    run(vs2, cs2)
    state2, want2 = new_state(S), []
    for t, (named, sc, _v) in enumerate(dry):
        want2 += none.step_reference(named, sc.cpu().numpy(), t + 1, *state2)
    assert _events_of(vs2) == want2 and 2 not in {e[1] for e in want2}


def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the reference decodes the same bytes)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def test_behind_the_gate_and_the_packet_front():
    from afx.ingest import PacketScorer
    from afx.vad import GatedScorer, emitted
    from afx.verdict import VerdictPolicy, VerdictScorer
    S, ticks = 3, 24
    streams = [np.roll(FIX, -o)[:ticks * H].copy() for o in (0, 30000 + 57, 44000)]

    def run(front):
        out = [[] for _ in range(S)]
        nans = 0
        for t in range(ticks):
            named = [[0, 1, 2], [2, 0, 1]][t % 2]
            sc = front.push(torch.from_numpy(np.stack([streams[s][t * H:(t + 1) * H] for s in named])).cuda(), named).cpu()
            for s, v, e in zip(named, sc.tolist(), emitted(sc).tolist()):
                nans += not e
                if e:
                    out[s].append(np.float32(v))
        return out, nans

    dry, nans = run(GatedScorer(_screen("kv", S)))
    assert nans >= 3 and min(len(d) for d in dry) >= 4  # pushes that completed no hop of speech sit in between
    _, med = _quartile_and_median(np.concatenate(dry))
    pol = VerdictPolicy(med, med, alpha=0.5)
    vs = VerdictScorer(_screen("kv", S), pol)
    got, _ = run(GatedScorer(vs))
    assert all(np.array(a).tobytes() == np.array(b).tobytes() for a, b in zip(got, dry))
    ev = _events_of(vs)
    for s in range(S):  # the inner session counts the hops of the gated stream
        assert [e for e in ev if e[0] == s] == [(s,) + e[1:] for e in pol.run_reference(dry[s])[0]], s
    assert len(ev) >= 1 and vs.alarm.tolist() == [pol.run_reference(dry[s])[1][-1] for s in range(S)]
    # the packet front around the gate: 20-ms mu-law packets at 8 kHz
    vs = VerdictScorer(_screen("kv", S), pol)
    ps = PacketScorer(GatedScorer(vs), 8000, "mulaw")
    codes = [_mulaw_encode(np.roll(FIX, -o)[:96000:2]) for o in (0, 30000 + 57, 44000)]
    seq = [[] for _ in range(S)]
    for k in range(0, codes[0].size, 160):
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        res = ps.feed([codes[s][k:k + 160].tobytes() for s in named], named)
        for s, part in zip(named, res.split()):
            seq[s] += [np.float32(v) for v in part.cpu().tolist() if v == v]
    ev = _events_of(vs)
    assert sum(len(q) for q in seq) >= 6 and vs.samples_seen.tolist() == [len(q) * H for q in seq]
    for s in range(S):
        assert [e for e in ev if e[0] == s] == [(s,) + e[1:] for e in pol.run_reference(seq[s])[0]], s
    assert vs.alarm.tolist() == [pol.run_reference(seq[s])[1][-1] if seq[s] else False for s in range(S)]


# ---- 3. sessions ---------------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_moved_sessions_continue_bit_for_bit(kind):
    """Session 0 starts at tick 0, session 1 at tick 2; under enter = +inf and confirm = 4 every score counts, so at the move
    (after tick 4) session 0 is in alarm and session 1 is three scores into its confirm run."""
    from afx.verdict import VerdictPolicy, VerdictScorer
    t0, ticks = 5, 9
    pol = VerdictPolicy(INF, INF, alpha=0.5, confirm=4)
    streams = [np.roll(FIX, -2000)[:ticks * H], np.roll(FIX, -50000)[:ticks * H]]
    hopsof = lambda t, rows: torch.from_numpy(np.stack([streams[i][t * H:(t + 1) * H] for i in rows])).cuda()  # noqa: E731

    def step(front, t, s0, s1):
        """Tick t of the two sessions living in slots s0, s1 -> (score of session 0, score of session 1 or None)."""
        if t < 2:
            return front.push(hopsof(t, [0]), [s0]).clone(), None
        sc = front.push(hopsof(t, [1, 0]), [s1, s0]).clone()
        return sc[1:2], sc[0:1]

    never = VerdictScorer(_screen(kind, 3), pol)
    ref = [step(never, t, 0, 2) for t in range(ticks)]
    names = {0: 0, 2: 1}
    ref_events = [(names[e[0]],) + e[1:] for e in _events_of(never)]
    assert [e[:3] for e in ref_events] == [(0, 1, 4), (1, 1, 4)]  # each raised at its fourth score

    a = VerdictScorer(_screen(kind, 3), pol)
    for t in range(t0):
        got = step(a, t, 0, 2)
        assert _same_bits(got[0], ref[t][0]) and (got[1] is None or _same_bits(got[1], ref[t][1]))
    ev = [(names[e[0]],) + e[1:] for e in _events_of(a)]
    st = a.export_slots([0, 2])
    assert st.tensors["verdict_state"].tolist() == [[5, 0, 1, 4], [3, 3, 0, -1]]  # in alarm; mid-run-count
    b = VerdictScorer(_screen(kind, 4), pol)
    b.push(torch.from_numpy(np.stack([FIX[8000:12000], FIX[48000:52000]])).cuda(), [3, 0])  # the destination is in use
    b.take_events()
    # refusals, each with the destination unchanged
    snap = lambda c: (c.verdicts.m.clone(), c.verdicts.st.clone(), c.samples_seen)  # noqa: E731
    before = snap(b)
    for dest, state in ((b, a.scorer.export_slots([0, 2])), (VerdictScorer(_screen(kind, 4), VerdictPolicy(INF, INF, alpha=0.5, confirm=5)), _move(st))):
        with pytest.raises(ValueError):
            dest.import_slots([3, 1], state)
    with pytest.raises(ValueError):
        b.scorer.import_slots([3, 1], _move(st))  # a bare scorer refuses a verdict state
    after = snap(b)
    assert _same_bits(before[0], after[0]) and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])
    b.import_slots([3, 1], _move(st))
    assert b.verdicts.st[[0, 2]].tolist() == before[1][[0, 2]].tolist() and _events_of(b) == []  # the other slots; no event moved
    assert b.alarm.tolist()[3] is True and b.alarm.tolist()[1] is False
    for t in range(t0, ticks):
        got = step(b, t, 3, 1)
        assert _same_bits(got[0], ref[t][0]) and _same_bits(got[1], ref[t][1]), t
    ev += [({3: 0, 1: 1}[e[0]],) + e[1:] for e in _events_of(b)]
    assert ev == ref_events  # kinds, hop indices and the bits of the smoothed scores of sessions that never moved
    assert _same_bits(b.smoothed[[3, 1]], never.smoothed[[0, 2]]) and b.verdicts.st[[3, 1]].tolist() == never.verdicts.st[[0, 2]].tolist()


# ---- 4. the offline counterpart --------------------------------------------------------------------------------------------------
def test_one_slot_stream_logs_what_timeline_alarms_reports():
    from afx.streaming import SlidingWindowScorer
    from afx.timeline import score_timeline
    from afx.verdict import VerdictPolicy, VerdictScorer
    eng, sd = _student("fp16")
    rec = FIX[:_TICKS * H].copy()
    tl = score_timeline(eng, [torch.from_numpy(rec)], window=16000, hop=H, state_dict=sd)[0]
    assert len(tl) == _TICKS
    enter, exit_ = _quartile_and_median(tl.scores.numpy())
    pol = VerdictPolicy(enter, exit_, alpha=0.5)
    want = tl.alarms(pol)
    vs = VerdictScorer(SlidingWindowScorer(eng, 1, window=16000, hop=H, state_dict=sd), pol)
    for t in range(_TICKS):
        sc = vs.push(torch.from_numpy(rec[None, t * H:(t + 1) * H]).cuda())
        assert _same_bits(sc, tl.scores[t:t + 1])
    got = []
    for _slot, kind, k, _bits_ in _events_of(vs):
        if kind == 3:
            got[-1] = (got[-1][0], k * H / 16000, got[-1][2])
        else:
            got.append((k * H / 16000, None, kind))
    print(f"one-slot stream against Timeline.alarms: {want}")
    assert got == want and len(want) >= 1

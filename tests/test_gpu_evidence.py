"""The evidence recorder on the GPU (afx/evidence.py; afx_k_evidence_mark, afx_k_evidence_copy).  Every comparison is exact,
bytes or bits.  The kernels are driven through ``Evidence`` with hand-made verdict state and hops and held against
``EvidencePolicy.step_reference``: after every update the whole device state (the rings, ``rec``, ``left``, the headers, the
counters, and the audio and scores of every pool entry that is not FREE) equals the reference's mirrors, the rows of slots
not named included.  Then ``EvidenceScorer`` end to end for the three scorer kinds, behind the gate and the packet front,
and with sessions moved between scorers.

Tiny engines as in tests/test_gpu_verdict.py: a 1-layer Conformer student, H = 4000; the exact scorers run a 1-s window,
the KV-cached scorer its 4-s window.  ``VerdictPolicy(enter=+inf)``: every slot alarms at its first score."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
INF, NAN = float("inf"), float("nan")
f32 = np.float32
POISON = np.array([0x7FC0DEAD], dtype=np.uint32).view(f32)[0]  # a NaN no hop of these tests holds


def _pcm_edges():
    lsb = f32(1.0) / f32(32768)
    v = [1.0, -1.0, INF, -INF, NAN, 1e-45, -1e-45, 1.1754942e-38, 3e38, -3e38, 32767.5 * lsb, -32768.5 * lsb, 0.0, -0.0]
    for t in (0.5, 1.5, 2.5, -0.5, -1.5, 32766.5, -32767.5):
        v += [t * lsb, np.nextafter(f32(t * lsb), f32(INF)), np.nextafter(f32(t * lsb), f32(-INF))]
    return np.array(v, dtype=f32)


EDGES = _pcm_edges()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Mirror:
    """An ``Evidence`` on the device and the numpy mirrors of its state, both rings poisoned with a NaN pattern first."""

    def __init__(self, S, policy, hop, window=None):
        from afx.evidence import Evidence
        self.S, self.p, self.hop = S, policy, hop
        self.ev = Evidence(S, policy, hop, "cuda", window=window)
        self.st = policy.new_state(S, hop, window)
        self.st["hist"][:] = POISON
        self.st["sring"][:] = POISON
        self.ev.hist.copy_(torch.from_numpy(self.st["hist"]))
        self.ev.sring.copy_(torch.from_numpy(self.st["sring"]))
        self.vst = np.zeros((S, 4), dtype=np.int32)
        self.vst[:, 3] = -1
        self.k = np.zeros(S, dtype=np.int64)  # hops pushed per slot since its reset

    def push(self, slots, hops, scores, raising=(), clearing=()):
        """One update of the named slots (their hop numbers advance by one); the slots in ``raising`` are raised by this push
        as far as the verdict state goes (on = 1, since = k), those in ``clearing`` cleared."""
        slots = list(slots)
        self.k[slots] += 1
        for s in raising:
            self.vst[s, 2:] = (1, self.k[s])
        for s in clearing:
            self.vst[s, 2:] = (0, -1)
        self.vst[slots, 0] += 1
        hops = np.ascontiguousarray(hops, dtype=f32)
        sc = None if scores is None else np.asarray(scores, dtype=f32)
        self.ev.update(torch.from_numpy(hops).cuda(), slots, hop_index=self.k[slots], scores=None if sc is None else torch.from_numpy(sc).cuda(),
                       verdict_state=torch.from_numpy(self.vst).cuda())
        self.p.step_reference(self.st, hops, slots, self.k[slots], sc, self.vst)

    def reset(self, slots):
        self.ev.reset(slots)
        self.p.reset_reference(self.st, slots)
        for s in slots:
            self.k[s], self.vst[s] = 0, (0, 0, 0, -1)

    def take(self):
        got, want = self.ev.take_clips(), self.p.take_reference(self.st)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert (a.slot, a.raised_at, a.first_hop, a.hops, a.complete, a.seq) == (b.slot, b.raised_at, b.first_hop, b.hops, b.complete, b.seq)
            assert a.audio.dtype == b.audio.dtype and a.audio.tobytes() == b.audio.tobytes() and a.scores.tobytes() == b.scores.tobytes()
        return got

    def check(self, what):
        torch.cuda.synchronize()
        ev, st = self.ev, self.st
        for k, t in (("hist", ev.hist), ("sring", ev.sring), ("rec", ev.rec), ("left", ev.left), ("pool", ev.pool), ("counters", ev.counters)):
            assert t.cpu().numpy().tobytes() == st[k].tobytes(), (what, k)
        used = np.flatnonzero(st["pool"][:, 0] != 0)
        assert ev.audio.cpu().numpy()[used].tobytes() == st["audio"][used].tobytes(), (what, "audio")
        assert ev.cscores.cpu().numpy()[used].tobytes() == st["cscores"][used].tobytes(), (what, "cscores")
        assert ev._claim.cpu().tolist() == [(1 << 31) - 1] * self.S, (what, "claim")


def _hops(g, A, hop, edges=False):
    x = (0.3 * g.standard_normal((A, hop))).astype(f32)
    if edges:  # the pcm16 edge values placed in real hops
        at = g.integers(0, A * hop, 2 * EDGES.size)
        x.reshape(-1)[at] = np.tile(EDGES, 2)
    return x


# ---- 1. the kernels against step_reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ["fp32", "pcm16"])
@pytest.mark.parametrize("hop,pre,post,S,clips", [(37, 2, 1, 5, 4), (160, 3, 2, 6, 64), (4000, 1, 1, 3, 3), (36, 0, 1, 5, 4), (160, 2, 0, 4, 3),
                                                  (38, 1, 3, 70, 64)])
def test_kernels_equal_the_reference_update_by_update(hop, pre, post, S, clips, encoding):
    """hop 37: the scalar path, ring columns that are no multiple of 4; 38 and 36: 8-byte rows of pcm16 that are / are not
    16-byte rows of fp32; 160 and 4000: the vector path; pre = 0; post = 0 (a clip complete in the opening update); updates
    of one row, of subsets in permuted order and of every slot; raises at k = 1 and k <= pre over poisoned rings, raises
    while recording, more raises than free entries, resets mid-recording and clips taken mid-run."""
    from afx.evidence import EvidencePolicy
    p = EvidencePolicy(pre=pre, post=post, clips=clips, encoding=encoding)
    g = np.random.default_rng(hop * 100 + pre * 10 + post)
    mir = _Mirror(S, p, hop)
    taken = []
    for t in range(18):
        if t in (7, 13):
            mir.reset([int(s) for s in g.permutation(S)[:2]])
            mir.check((t, "reset"))
        A = 1 if t % 5 == 4 else (S if t % 3 == 0 else int(g.integers(1, S + 1)))
        slots = g.permutation(S)[:A].tolist()
        on = mir.vst[slots, 2] == 1
        draw = g.random(A)
        raising = [s for s, o, d in zip(slots, on, draw) if not o and (d < 0.45 or t == 0)]
        clearing = [s for s, o, d in zip(slots, on, draw) if o and d < 0.5]
        sc = np.where(g.random(A) < 0.2, f32(NAN), g.standard_normal(A).astype(f32))
        mir.push(slots, _hops(g, A, hop, edges=True), None if t == 2 else sc, raising, clearing)
        mir.check(t)
        if t in (5, 11, 17):
            taken += mir.take()
            mir.check((t, "taken"))
    c = mir.st["counters"].tolist()
    print(f"evidence kernels hop {hop} pre {pre} post {post} S {S} clips {clips} {encoding}: counters {c}, {len(taken)} clips taken, "
          f"{sum(not x.complete for x in taken)} truncated")
    # conditions on the fixture, checked on the reference
    assert c[0] >= 4 and c[1] >= 3 and len(taken) >= 3 and any(x.first_hop == 1 and x.raised_at == 1 for x in taken)
    assert (c[3] >= 1 or post < 2) and (c[2] >= 1 or clips == 64)  # (a second raise inside a post-roll of one hop cannot be)
    for x in taken:
        assert not (x.audio.view(np.uint32) == POISON.view(np.uint32)).any() if encoding == "fp32" else True


def test_a_raise_at_the_first_hops_never_reads_the_stale_ring():
    from afx.evidence import EvidencePolicy
    p = EvidencePolicy(pre=3, post=1, clips=8)
    hop, S = 160, 4
    g = np.random.default_rng(7)
    mir = _Mirror(S, p, hop)
    x = [_hops(g, S, hop) for _ in range(6)]
    sc = [g.standard_normal(S).astype(f32) for _ in range(6)]
    for t in range(5):  # slot t raises at k = t + 1: k = 1, k <= pre, k = pre + 1, k = pre + 2
        mir.push(range(S), x[t], sc[t], raising=[t] if t < S else [])
        mir.check(t)
    clips = mir.take()
    assert [(c.slot, c.raised_at, c.first_hop, c.hops) for c in clips] == [(0, 1, 1, 2), (1, 2, 1, 3), (2, 3, 1, 4), (3, 4, 1, 5)]
    for c in clips:
        want = np.concatenate([x[t][c.slot] for t in range(c.first_hop - 1, c.first_hop - 1 + c.hops)])
        assert c.audio.tobytes() == want.tobytes() and c.scores.tobytes() == np.array([sc[t][c.slot] for t in range(c.hops)]).tobytes()
    # a new session in a slot whose ring holds the old one: again nothing from before the reset
    mir.reset([0])
    mir.push([0], x[5][:1], sc[5][:1], raising=[0])
    mir.push([0], x[4][:1], sc[4][:1])
    mir.check("after the reset")
    (c,) = mir.take()
    assert (c.raised_at, c.first_hop, c.hops, c.complete) == (1, 1, 2, True) and c.audio.tobytes() == np.concatenate([x[5][0], x[4][0]]).tobytes()


def test_a_raise_while_recording_is_merged_and_opens_no_second_clip():
    from afx.evidence import EvidencePolicy
    p = EvidencePolicy(pre=1, post=4, clips=4, encoding="pcm16")
    g = np.random.default_rng(8)
    mir = _Mirror(2, p, 40)
    plan = {2: ([0], []), 3: ([], [0]), 4: ([0], []), 5: ([1], [])}  # slot 0: raised at k = 3, cleared, raised again at k = 5
    for t in range(8):
        r, c = plan.get(t, ([], []))
        mir.push([1, 0], _hops(g, 2, 40), g.standard_normal(2), raising=r, clearing=c)
        mir.check(t)
    assert mir.ev.stats() == dict(raised=2, recorded=2, dropped=0, merged=1, free=2, recording=1, finished=1)
    (c,) = mir.take()
    assert (c.slot, c.raised_at, c.first_hop, c.hops, c.complete) == (0, 3, 2, 6, True)


def test_a_full_pool_drops_by_row_position_and_freed_entries_are_reused_in_ascending_index():
    from afx.evidence import COMPLETE, FREE, RECORDING, EvidencePolicy
    p = EvidencePolicy(pre=0, post=1, clips=2)
    g = np.random.default_rng(9)
    S, hop = 6, 37
    mir = _Mirror(S, p, hop)
    mir.push([4, 1, 5, 3], _hops(g, 4, hop), g.standard_normal(4), raising=[5, 3, 4])  # rows 0, 2, 3 raise: slots 4 and 5 win
    mir.check("three raises, two entries")
    assert mir.st["pool"][:, :3].tolist() == [[RECORDING, 4, 1], [RECORDING, 5, 1]] and mir.st["counters"].tolist() == [3, 2, 1, 0]
    assert mir.ev.rec.tolist() == [-1, -1, -1, -1, 0, 1]
    mir.push([5], _hops(g, 1, hop), [0.5])  # entry 1 completes first
    mir.check("entry 1 complete")
    (c,) = mir.take()
    assert c.slot == 5 and mir.st["pool"][:, 0].tolist() == [RECORDING, FREE]
    mir.push([0, 2], _hops(g, 2, hop), None, raising=[2, 0])  # one free entry: row 0 (slot 0) takes it, slot 2 is dropped
    mir.check("one free entry")
    assert mir.st["pool"][1, :3].tolist() == [RECORDING, 0, 1] and mir.st["counters"].tolist() == [5, 3, 2, 0]
    mir.push([0, 4], _hops(g, 2, hop), None)
    assert mir.st["pool"][:, 0].tolist() == [COMPLETE, COMPLETE] and [c.slot for c in mir.take()] == [4, 0]
    mir.push([3, 2, 1], _hops(g, 3, hop), None, raising=[1, 2])  # both free again: ascending index in row order
    mir.check("reused")
    assert mir.st["pool"][:, [1, 5]].tolist() == [[2, 3], [1, 4]]


def test_reset_mid_recording_truncates_with_the_hops_so_far():
    from afx.evidence import TRUNCATED, EvidencePolicy
    p = EvidencePolicy(pre=2, post=5, clips=3)
    g = np.random.default_rng(10)
    mir = _Mirror(3, p, 160)
    x = [_hops(g, 3, 160) for _ in range(6)]
    for t in range(5):
        mir.push(range(3), x[t], g.standard_normal(3), raising=[1] if t == 2 else [])
    mir.reset([1, 2])
    mir.check("reset")
    assert mir.st["pool"][0].tolist() == [TRUNCATED, 1, 3, 1, 5, 0] and mir.ev.rec.tolist() == [-1] * 3
    mir.push(range(3), x[5], g.standard_normal(3))  # the truncated clip takes nothing more
    mir.check("after")
    (c,) = mir.take()
    assert (c.complete, c.hops) == (False, 5) and c.audio.tobytes() == np.concatenate([x[t][1] for t in range(5)]).tobytes()


def test_bad_rows_are_skipped_whole_and_bad_arguments_launch_nothing():
    """The kernels launched directly: ``Evidence.update`` refuses such headers itself."""
    from afx._lib import call_on, lib
    from afx.evidence import EvidencePolicy
    p = EvidencePolicy(pre=1, post=1, clips=4)
    S, hop = 6, 37
    g = np.random.default_rng(11)
    mir = _Mirror(S, p, hop)
    ev, l = mir.ev, lib()
    mir.vst[:, 2:] = (1, 3)  # every slot was raised at k = 3
    slots = np.array([2, -1, 0, S, 2, 1, 1 << 20, 4, 5])
    ks = np.array([3, 3, 0, 3, 3, 3, 3, -5, 3])  # slot 0 with k = 0, slot 4 with k < 0; slot 2 named twice: the first row is taken
    x, sc = _hops(g, slots.size, hop), g.standard_normal(slots.size).astype(f32)
    hdr = torch.from_numpy(np.stack([slots, ks], axis=1).astype(np.int32)).cuda()
    d_x, d_sc, d_vst = torch.from_numpy(x).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(mir.vst).cuda()
    rows_work = torch.full((slots.size, 4), -9, dtype=torch.int32, device="cuda")  # (more rows than slots: not the Evidence's own)
    mark = [hdr, slots.size, d_vst, S, 1, 1, ev.rec, ev.left, ev._claim, ev._pool, 4, ev.counters, rows_work]
    copy = [d_x, d_sc, 1, hdr, rows_work, slots.size, hop, 1, 1, ev.hist, ev.sring, S, ev.audio, ev.cscores, 4, 0]
    conv = lambda args: [_p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]  # noqa: E731
    assert call_on(ev.hist, l.afx_k_evidence_mark, *conv(mark)) == 0, l.afx_last_error()
    assert call_on(ev.hist, l.afx_k_evidence_copy, *conv(copy)) == 0, l.afx_last_error()
    good = [0, 5, 8]
    p.step_reference(mir.st, x[good], slots[good], ks[good], sc[good], mir.vst)
    mir.check("bad rows")
    assert rows_work[:, 0].tolist() == [2, -1, -1, -1, -1, 2, -1, -1, 2] and mir.st["counters"].tolist() == [3, 3, 0, 0]
    # bad arguments: an error, nothing launched, no byte changed
    big = torch.zeros(8193, 2, dtype=torch.int32, device="cuda")
    for i, val in [(0, None), (2, None), (6, None), (7, None), (8, None), (9, None), (11, None), (12, None), (1, 0), (1, -1), (1, 8193), (3, 0), (4, -1),
                   (5, -1), (10, 0), (10, 8193)]:
        args = list(mark)
        args[i] = val
        if (i, val) == (1, 8193):
            args[0] = big
        assert l.afx_k_evidence_mark(*conv(args), None) != 0 and b"evidence_mark" in l.afx_last_error(), (i, val)
    for i, val in [(0, None), (3, None), (4, None), (9, None), (10, None), (12, None), (13, None), (2, 0), (5, 0), (5, 8193), (6, 0), (7, -1), (8, -1),
                   (11, 0), (14, 0), (14, 8193), (15, 2), (15, -1)]:
        args = list(copy)
        args[i] = val
        assert l.afx_k_evidence_copy(*conv(args), None) != 0 and b"evidence_copy" in l.afx_last_error(), (i, val)
    mir.check("bad arguments")
    # a work item that leaves the pool is skipped whole by the copy kernel
    work = torch.tensor([[1, 4, 0, 0], [1, 0, 3, 0], [2, 0, 3, 3], [2, -1, 3, 1], [2, 0, 2, 1], [3, 0, 0, 0]], dtype=torch.int32, device="cuda")
    hdr2 = torch.tensor([[s, 3] for s in range(6)], dtype=torch.int32, device="cuda")
    args = list(copy)
    args[3], args[4], args[5] = hdr2, work, 6
    assert call_on(ev.hist, l.afx_k_evidence_copy, *conv(args)) == 0, l.afx_last_error()
    mir.check("bad work items")


def test_every_row_of_the_largest_update():
    """A = S = 8192 in permuted order: eight chunks of 1024 rows, 5000 entries for 8192 raises, then the post-roll."""
    from afx.evidence import EvidencePolicy
    p = EvidencePolicy(pre=1, post=1, clips=5000, encoding="pcm16")
    S, hop = 8192, 8
    g = np.random.default_rng(12)
    mir = _Mirror(S, p, hop)
    mir.push(g.permutation(S), _hops(g, S, hop), g.standard_normal(S))
    slots = g.permutation(S)
    mir.push(slots, _hops(g, S, hop), g.standard_normal(S), raising=range(S))
    mir.check("raises")
    assert mir.st["counters"].tolist() == [8192, 5000, 3192, 0] and mir.st["pool"][:, 1].tolist() == slots[:5000].tolist()
    mir.push(g.permutation(S), _hops(g, S, hop), g.standard_normal(S))
    mir.check("post-roll")
    assert len(mir.take()) == 5000
    mir.check("taken")


# ---- engines and scorers -----------------------------------------------------------------------------------------------------
_ENGINES = {}


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


def _student():
    if "s" not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES["s"] = (eng, sd)
    return _ENGINES["s"]


def _screen(kind, S):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    eng, sd = _student()
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _recorder(kind, S, epolicy, confirm=1):
    from afx.evidence import EvidenceScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    return EvidenceScorer(VerdictScorer(_screen(kind, S), VerdictPolicy(INF, INF, confirm=confirm)), epolicy)


class _Spy:
    """Records, per slot, the hops the inner (verdict) scorer was pushed and the scores it returned (NaN for a ``None``)."""

    def __init__(self, es):
        self.hops, self.scores = [[] for _ in range(es.S)], [[] for _ in range(es.S)]
        inner_push, S = es.scorer.push, es.S

        def push(chunk, slots=None):
            out = inner_push(chunk, slots)
            idx = list(range(S)) if slots is None else list(slots)
            sc = np.full(len(idx), NAN, f32) if out is None else out.detach().cpu().numpy().copy()
            for i, s in enumerate(idx):
                self.hops[s].append(chunk[i].detach().cpu().numpy().copy())
                self.scores[s].append(sc[i])
            return out

        es.scorer.push = push

    def restart(self, slot):
        self.hops[slot], self.scores[slot] = [], []

    def check(self, clip, hop=H):
        """The clip is the hops first_hop.. of its slot, bit for bit, with the scores ``push`` returned."""
        a, n = clip.first_hop - 1, clip.hops
        assert n >= 1 and a + n <= len(self.hops[clip.slot]), clip
        assert clip.audio.dtype == f32 and clip.audio.tobytes() == np.concatenate(self.hops[clip.slot][a:a + n]).tobytes(), clip
        assert clip.scores.tobytes() == np.array(self.scores[clip.slot][a:a + n], dtype=f32).tobytes(), clip


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_a_clip_is_the_hops_pushed_and_the_scores_returned(kind):
    """pre = None: window // hop - 1.  Subsets and orders of named slots, a reset mid-run; the alarm of a slot is raised by its
    first score that is a number (hops before it, if any, carry NaN scores in the clip)."""
    from afx.evidence import EvidencePolicy
    S, ticks = 3, 12
    es = _recorder(kind, S, EvidencePolicy(post=2, clips=8))
    spy = _Spy(es)
    bare = _screen(kind, S)
    assert es.evidence.pre == (3 if kind != "kv" else 15)
    streams = [np.roll(FIX, -o)[:ticks * H].copy() for o in (0, 30000 + 57, 44000)]
    first_score = lambda sc: next(i + 1 for i, v in enumerate(sc) if v == v)  # noqa: E731
    pos, early, first = [0] * S, [], None
    for t in range(ticks):
        if t == 6:
            es.reset([1])
            bare.reset([1])
            early = es.take_clips()
            first = [first_score(sc) for sc in spy.scores]
            for c in early:
                spy.check(c)
            spy.restart(1)
            pos[1] = 8 * H
        named = [None, [2, 0, 1], [1, 2, 0], [0, 2]][t % 4]
        order = list(range(S)) if named is None else named
        chunk = torch.from_numpy(np.stack([streams[s][pos[s]:pos[s] + H] for s in order])).cuda()
        got, want = es.push(chunk, named), bare.push(chunk.clone(), named)
        assert (got is None) == (want is None) and (got is None or torch.equal(got.view(torch.int32), want.view(torch.int32))), t
        for s in order:
            pos[s] += H
    late = es.take_clips()
    for c in late:
        spy.check(c)
    print(f"evidence end to end [{kind}]: {early + late}; stats {es.stats()}")
    assert sorted(c.slot for c in early) == [0, 1, 2] and [c.seq for c in early] == [0, 1, 2] and [c.slot for c in late] == [1]
    for c in early:
        assert (c.raised_at, c.first_hop, c.hops, c.complete) == (first[c.slot], 1, first[c.slot] + 2, True), c
    k = first_score(spy.scores[1])  # the second session of slot 1
    assert (late[0].raised_at, late[0].first_hop, late[0].hops, late[0].complete, late[0].seq) == (k, 1, k + 2, True, 3)
    assert es.stats()["merged"] == 0 and es.take_clips() == [] and es.alarm.tolist() == [True] * 3


def test_a_push_without_a_score_still_stores_the_audio_with_nan_scores():
    """A KV-cached scorer returns None for a push that completes no frame of its last conv layer (a hop shorter than a
    frame).  Here the KV-cached scorer's first three pushes are made to return None after they ran: the session advances,
    the verdict layer sees no score, and the recorder stores the hops with NaN scores."""
    from afx.evidence import EvidencePolicy
    S = 2
    es = _recorder("kv", S, EvidencePolicy(pre=4, post=2, clips=4))
    kv = es.scorer.scorer
    real, calls = kv.push, []

    def quiet(chunk, slots=None):
        out = real(chunk, slots)
        calls.append(out is not None)
        return None if len(calls) <= 3 else out

    kv.push = quiet
    spy = _Spy(es)
    for t in range(7):
        out = es.push(torch.from_numpy(np.stack([FIX[8000 + t * H:8000 + (t + 1) * H], FIX[50000 + t * H:50000 + (t + 1) * H]])).cuda())
        assert (out is None) == (t < 3) and es.samples_seen.tolist() == [(t + 1) * H] * S
    clips = es.take_clips()
    print(f"evidence around a scorer whose first pushes return None: {clips}")
    assert len(clips) == 2 and all(calls)
    for c in clips:
        spy.check(c)
        k = c.raised_at
        assert k >= 4 and c.first_hop == max(1, k - 4) and np.isnan(c.scores[:4 - c.first_hop]).all() and not np.isnan(c.scores[k - c.first_hop])


def _nth_score(scores, n):
    """The 1-based hop number of the n-th score that is a number."""
    return [i + 1 for i, v in enumerate(scores) if v == v][n - 1]


def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the clip is held against what the front pushed)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def test_behind_the_gate_the_clip_is_the_gated_stream_and_behind_the_packet_front_what_it_pushed():
    from afx.evidence import EvidencePolicy
    from afx.ingest import PacketScorer
    from afx.vad import GatedScorer
    S, ticks = 3, 24
    es = _recorder("kv", S, EvidencePolicy(pre=2, post=3, clips=8, encoding="pcm16"), confirm=4)
    spy = _Spy(es)
    gs = GatedScorer(es)
    streams = [np.roll(FIX, -o)[:ticks * H].copy() for o in (0, 30000 + 57, 44000)]
    for t in range(ticks):
        named = [[0, 1, 2], [2, 0, 1]][t % 2]
        gs.push(torch.from_numpy(np.stack([streams[s][t * H:(t + 1) * H] for s in named])).cuda(), named)
    clips = es.take_clips()
    assert sorted(c.slot for c in clips) == [0, 1, 2]
    from afx.evidence import pcm16_reference
    for c in clips:  # the fourth score of the GATED stream raised the alarm: the clip is cut out of what gate_reference keeps
        kept = gs.gate.gate_reference(streams[c.slot])[1]
        k = _nth_score(spy.scores[c.slot], 4)
        f = max(1, k - 2)
        assert kept.size < streams[c.slot].size and kept.size >= (k + 3) * H
        assert (c.raised_at, c.first_hop, c.hops, c.complete) == (k, f, k - f + 4, True) and c.audio.dtype == np.int16
        assert c.audio.tobytes() == pcm16_reference(kept[(f - 1) * H:(k + 3) * H]).tobytes()
        assert c.scores.tobytes() == np.array(spy.scores[c.slot][f - 1:k + 3], dtype=f32).tobytes()
    # the packet front around the recorder: 20-ms mu-law packets at 8 kHz; the clip is what the front pushed, hop by hop
    es = _recorder("kv", S, EvidencePolicy(pre=2, post=3, clips=8), confirm=3)
    spy = _Spy(es)
    ps = PacketScorer(es, 8000, "mulaw")
    codes = [_mulaw_encode(np.roll(FIX, -o)[:80000:2]) for o in (0, 30000 + 57, 44000)]
    for k in range(0, codes[0].size, 160):
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        ps.feed([codes[s][k:k + 160].tobytes() for s in named], named)
    clips = es.take_clips()
    assert sorted(c.slot for c in clips) == [0, 1, 2]
    for c in clips:
        k = _nth_score(spy.scores[c.slot], 3)
        f = max(1, k - 2)
        assert (c.raised_at, c.first_hop, c.hops, c.complete) == (k, f, k - f + 4, True)
        spy.check(c)


# ---- sessions ----------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_moved_sessions_keep_their_pre_roll_and_the_open_clip_stays_behind(kind):
    """Session 0 starts at tick 0, session 1 at tick 2; confirm = 4: session 0 raises at tick 3 and is recording at the move
    (after tick 4), session 1 raises at tick 5, in the destination, with a pre-roll pushed in the source."""
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    t0, ticks = 5, 9
    streams = [np.roll(FIX, -2000)[:ticks * H], np.roll(FIX, -50000)[:ticks * H]]
    hopsof = lambda t, rows: torch.from_numpy(np.stack([streams[i][t * H:(t + 1) * H] for i in rows])).cuda()  # noqa: E731

    def step(front, t, s0, s1):
        if t < 2:
            return front.push(hopsof(t, [0]), [s0])
        return front.push(hopsof(t, [1, 0]), [s1, s0])

    a = _recorder(kind, 3, EvidencePolicy(pre=3, post=4, clips=4), confirm=4)
    for t in range(t0):
        step(a, t, 0, 2)
    assert a.stats() == dict(raised=1, recorded=1, dropped=0, merged=0, free=3, recording=1, finished=0)
    st = a.export_slots([0, 2])
    assert st.meta["evidence"] == 1 and st.meta["evidence_pre"] == 3 and st.tensors["evidence_hist"].shape == (2, 4 * H)
    b = _recorder(kind, 4, EvidencePolicy(pre=3, post=1, clips=2, encoding="pcm16"), confirm=4)  # post, clips and encoding differ
    b.push(torch.from_numpy(np.stack([FIX[8000:12000], FIX[48000:52000]])).cuda(), [3, 0])  # the destination is in use
    # refusals, each with every byte of the destination as it was
    e = b.evidence
    snap = lambda: [t.clone() for t in (e.hist, e.sring, e.rec, e.left, e._pool, e.audio, e.cscores, e.counters, b.scorer.verdicts.st)] + [b.samples_seen]  # noqa: E731
    before = snap()
    other_pre = _recorder(kind, 3, EvidencePolicy(pre=2, post=4, clips=4), confirm=4).export_slots([0, 2])
    from afx.streaming import StreamState
    moved = _move(st)
    for state in (other_pre, a.scorer.export_slots([0, 2]), StreamState(dict(moved.meta, evidence=2), moved.seen, moved.tensors)):
        with pytest.raises(ValueError):
            b.import_slots([3, 1], state)
    with pytest.raises(ValueError):
        EvidenceScorer(VerdictScorer(_screen(kind, 4), VerdictPolicy(INF, INF, confirm=5)), EvidencePolicy(pre=3)).import_slots([3, 1], moved)
    assert all(u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes() for u, v in zip(before, snap()))
    b.import_slots([3, 1], moved)
    for t in range(t0, ticks):
        step(b, t, 3, 1)
    # the destination: session 1 raised at its fourth hop (tick 5) with hops 1..4, three of them pushed in the source
    from afx.evidence import pcm16_reference
    (c,) = b.take_clips()
    assert (c.slot, c.raised_at, c.first_hop, c.hops, c.complete) == (1, 4, 1, 5, True)
    assert c.audio.tobytes() == pcm16_reference(streams[1][2 * H:7 * H]).tobytes()
    assert b.stats()["raised"] == 1 and b.alarm.tolist() == [False, True, False, True]  # session 0's alarm moved; it raised nothing here
    # the source: the open clip stayed, and comes back truncated when the slot is reset
    assert a.take_clips() == []
    a.reset([0])
    (c,) = a.take_clips()
    assert (c.slot, c.raised_at, c.first_hop, c.hops, c.complete) == (0, 4, 1, 5, False)
    assert c.audio.tobytes() == streams[0][:5 * H].tobytes()

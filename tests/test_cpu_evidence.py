"""The evidence recorder on the host (afx/evidence.py): ``EvidencePolicy`` validation, the pcm16 rule at its edges,
``step_reference`` against hand-worked cases and, chunked at any update boundaries, against ``run_reference``; ``reset`` and
``take_clips`` on host tensors, ``write_wav`` bytes, ``EvidenceScorer``'s surface, session export / import through
``state_dict()`` on a CPU-device scorer with every refusal leaving the scorer unchanged, and the entry points in the header,
the ctypes table and the built library.  No GPU: the kernels are held against ``step_reference`` in
tests/test_gpu_evidence.py.  Every comparison is exact, bytes or bits."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000
INF, NAN = float("inf"), float("nan")
f32 = np.float32


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _verdict_rows(T, S, raises, clears=()):
    """(T, S, 4) verdict state rows after each hop t = 1..T: slot s is raised at the hops raises[s] and cleared at clears[s]."""
    vs = np.zeros((T, S, 4), dtype=np.int32)
    for s in range(S):
        on, since = 0, -1
        for t in range(T):
            k = t + 1
            if k in raises.get(s, ()):
                on, since = 1, k
            elif k in clears.get(s, ()) if clears else False:
                on, since = 0, -1
            vs[t, s] = (k, 0, on, since)
    return vs


def test_policy_arguments_are_validated():
    from afx.evidence import EvidencePolicy
    p = EvidencePolicy()
    assert p.params() == dict(pre=None, post=8, clips=64, encoding="fp32")
    assert p.pre_for(4000, 64000) == 15 and p.pre_for(4000, 4000) == 0 and EvidencePolicy(pre=3).pre_for(160) == 3
    EvidencePolicy(np.int64(0), np.int32(0), np.int64(1), "pcm16")
    EvidencePolicy(65535, 65535, 8192)
    for bad in (dict(pre=-1), dict(pre=1.0), dict(pre=True), dict(pre="2"), dict(pre=65536), dict(post=-1), dict(post=None), dict(post=2.5),
                dict(post=False), dict(post=65536), dict(clips=0), dict(clips=8193), dict(clips=True), dict(clips=1.0), dict(clips=None),
                dict(encoding="wav"), dict(encoding=None), dict(encoding=16), dict(encoding=b"fp32")):
        with pytest.raises(ValueError):
            EvidencePolicy(**bad)
    for args in ((4000, None), (4000, 3999), (0, 4000), (True, 4000), (4000, 4000 * 65538)):
        with pytest.raises(ValueError):
            p.pre_for(*args)
    with pytest.raises(ValueError):
        EvidencePolicy(pre=65535, post=65535).pre_for(1 << 20)  # a clip of 2^31 samples or more


def test_pcm16_rule_at_its_edges():
    from afx.evidence import pcm16_reference
    lsb = f32(1.0) / f32(32768)
    up, down = (lambda v: np.nextafter(f32(v), f32(INF))), (lambda v: np.nextafter(f32(v), f32(-INF)))
    cases = [(1.0, 32767), (-1.0, -32768), (0.0, 0), (-0.0, 0), (INF, 32767), (-INF, -32768), (NAN, 0), (-NAN, 0),
             (0.5 * lsb, 0), (up(0.5 * lsb), 1), (down(0.5 * lsb), 0),            # a tie goes to the even neighbour
             (1.5 * lsb, 2), (up(1.5 * lsb), 2), (down(1.5 * lsb), 1),
             (2.5 * lsb, 2), (up(2.5 * lsb), 3), (down(2.5 * lsb), 2),
             (-0.5 * lsb, 0), (down(-0.5 * lsb), -1), (up(-0.5 * lsb), 0),
             (-1.5 * lsb, -2), (down(-1.5 * lsb), -2), (up(-1.5 * lsb), -1),
             (32766.5 * lsb, 32766), (up(32766.5 * lsb), 32767), (32767.5 * lsb, 32767), (down(1.0), 32767), (2.0, 32767),
             (-32767.5 * lsb, -32768), (up(-32767.5 * lsb), -32767), (-32768.5 * lsb, -32768), (-3e38, -32768), (3e38, 32767),
             (1e-45, 0), (-1e-45, 0), (1.1754942e-38, 0), (-1.1754942e-38, 0), (0.25, 8192), (-0.3, -9830)]
    x = np.array([c[0] for c in cases], dtype=f32)
    got = pcm16_reference(x)
    assert got.dtype == np.int16 and got.tolist() == [c[1] for c in cases]
    # the multiply is ONE fp32 operation: -0.3f * 32768 = -9830.4004 in fp32 (it rounds to -9830 either way); a value whose
    # fp64 product sits on the other side of a tie than its fp32 product pins the precision
    v = f32(0.1) + f32(0.5) * lsb                       # fp32(0.1) * 32768 is exact (a power of two), so this is generic
    assert int(pcm16_reference(v)) == int(np.rint(f32(v * f32(32768))))


def test_step_reference_hand_worked_a_raise_with_pre_roll_and_post_roll():
    from afx.evidence import COMPLETE, FREE, RECORDING, EvidencePolicy
    p = EvidencePolicy(pre=1, post=1, clips=2)
    st = p.new_state(2, 2)
    assert st["hist"].shape == (2, 4) and st["sring"].shape == (2, 2) and st["audio"].shape == (2, 6) and st["cscores"].shape == (2, 3)
    assert st["rec"].tolist() == [-1, -1] and st["pool"].tolist() == [[0] * 6] * 2 and st["audio"].dtype == f32
    hop = lambda k, s: np.array([[10 * k + s, 10 * k + s + 0.5]], dtype=f32)  # noqa: E731
    vs = _verdict_rows(5, 2, {1: [3]})
    for k in range(1, 6):
        p.step_reference(st, hop(k, 1), [1], k, [f32(-k)], vs[k - 1])
        if k == 2:
            assert st["counters"].tolist() == [0, 0, 0, 0] and st["hist"][1].tolist() == [11, 11.5, 21, 21.5]
        if k == 3:  # the raise: hops 2 and 3 out of the ring, which already holds hop 3 where hop 1 was
            assert st["pool"][0].tolist() == [RECORDING, 1, 3, 2, 2, 0] and st["rec"].tolist() == [-1, 0] and st["left"].tolist() == [0, 1]
            assert st["audio"][0].tolist() == [21, 21.5, 31, 31.5, 0, 0] and st["hist"][1].tolist() == [31, 31.5, 21, 21.5]
    assert st["pool"][0].tolist() == [COMPLETE, 1, 3, 2, 3, 0] and st["pool"][1, 0] == FREE
    assert st["audio"][0].tolist() == [21, 21.5, 31, 31.5, 41, 41.5] and st["cscores"][0].tolist() == [-2, -3, -4]
    assert st["rec"].tolist() == [-1, -1] and st["left"].tolist() == [0, 0] and st["counters"].tolist() == [1, 1, 0, 0]
    assert st["hist"][0].tolist() == [0] * 4  # the slot not named was not written
    clips = p.take_reference(st)
    assert len(clips) == 1 and st["pool"][0, 0] == FREE and p.take_reference(st) == []
    c = clips[0]
    assert (c.slot, c.raised_at, c.first_hop, c.hops, c.complete, c.seq) == (1, 3, 2, 3, True, 0)
    assert c.audio.tolist() == [21, 21.5, 31, 31.5, 41, 41.5] and c.scores.tolist() == [-2, -3, -4]


def test_step_reference_first_hop_is_clamped_merges_drops_and_truncates():
    from afx.evidence import COMPLETE, RECORDING, TRUNCATED, EvidencePolicy
    p = EvidencePolicy(pre=2, post=3, clips=2, encoding="pcm16")
    S, hop = 4, 3
    st = p.new_state(S, hop)
    st["hist"][:] = NAN  # a previous session's samples: never read
    x = lambda k: np.full((S, hop), k / 32768, dtype=f32) + np.arange(S, dtype=f32)[:, None] / 256  # noqa: E731
    enc = lambda k, s: [k + 128 * s] * hop  # noqa: E731
    # hop 1: slots 0 and 3 raise at k = 1 (first_hop 1, one hop); hop 2: slot 1 raises (first_hop 1, two hops) but the pool is full
    vs = _verdict_rows(6, S, {0: [1, 3], 3: [1], 1: [2]}, {0: [2]})
    p.step_reference(st, x(1)[[3, 1, 0]], [3, 1, 0], 1, None, vs[0])  # row order decides the entries: slot 3 first
    assert st["pool"].tolist() == [[RECORDING, 3, 1, 1, 1, 0], [RECORDING, 0, 1, 1, 1, 1]] and st["audio"].dtype == np.int16
    assert st["audio"][0, :hop].tolist() == enc(1, 3) and st["audio"][1, :hop].tolist() == enc(1, 0) and np.isnan(st["cscores"][:, 0]).all()
    p.step_reference(st, x(2), None, 2, np.arange(S, dtype=f32), vs[1])
    assert st["counters"].tolist() == [3, 2, 1, 0] and st["rec"].tolist() == [1, -1, -1, 0]  # slot 1's raise was dropped
    p.step_reference(st, x(3), None, 3, np.arange(S, dtype=f32), vs[2])  # slot 0 raises again while recording: merged
    assert st["counters"].tolist() == [3, 2, 1, 1] and st["pool"][:, 4].tolist() == [3, 3] and st["left"].tolist() == [1, 0, 0, 1]
    p.reset_reference(st, [3, 2])  # slot 3 mid-recording; slot 2 was not recording
    assert st["pool"][0].tolist() == [TRUNCATED, 3, 1, 1, 3, 0] and st["rec"].tolist() == [1, -1, -1, -1] and st["left"].tolist() == [1, 0, 0, 0]
    p.step_reference(st, x(4)[:2], [0, 1], 4, [f32(7), f32(8)], vs[3])
    assert st["pool"][1].tolist() == [COMPLETE, 0, 1, 1, 4, 1] and st["rec"].tolist() == [-1] * 4
    a, b = p.take_reference(st)
    assert (a.slot, a.complete, a.hops, a.audio.tolist()) == (3, False, 3, enc(1, 3) + enc(2, 3) + enc(3, 3))
    assert (b.slot, b.complete, b.hops, b.audio.tolist()) == (0, True, 4, enc(1, 0) + enc(2, 0) + enc(3, 0) + enc(4, 0))
    assert b.scores.view(np.int32).tolist() == np.array([NAN, 0, 0, 7], dtype=f32).view(np.int32).tolist()
    # the freed entries are taken again in ascending index, and seq keeps counting
    vs2 = np.zeros((S, 4), dtype=np.int32)
    vs2[:, 2:] = (1, 5)
    p.step_reference(st, x(5)[[2, 1]], [2, 1], 5, None, vs2[None][0])
    assert st["pool"][:, [1, 2, 3, 4, 5]].tolist() == [[2, 5, 3, 3, 2], [1, 5, 3, 3, 3]]
    assert not np.isnan(st["audio"].astype(np.float64)).any()


def test_step_reference_chunked_at_any_update_boundaries_equals_run_reference():
    from afx.evidence import EvidencePolicy
    g = np.random.default_rng(5)
    for enc, pre, post, clips in (("fp32", 2, 2, 3), ("pcm16", 0, 1, 64), ("fp32", 3, 0, 2)):
        p = EvidencePolicy(pre=pre, post=post, clips=clips, encoding=enc)
        T, S, hop = 14, 5, 7
        x = g.standard_normal((T, S, hop)).astype(f32)
        sc = np.where(g.random((T, S)) < 0.2, f32(NAN), g.standard_normal((T, S)).astype(f32))
        raises = {s: sorted(g.choice(np.arange(1, T + 1), 3, replace=False).tolist()) for s in range(S)}
        vs = _verdict_rows(T, S, raises, {s: [k + 1 for k in raises[s]] for s in range(S)})
        want = p.run_reference(x, sc, vs)
        assert want["counters"][0] >= 5 and (want["counters"][2] > 0) == (clips < 10)
        for trial in range(3):
            st = p.new_state(S, hop)
            for t in range(T):  # hop t of every slot, in slot order, cut into updates at random places
                cuts = [0] + sorted(g.choice(np.arange(1, S), g.integers(0, S - 1), replace=False).tolist()) + [S]
                for a, b in zip(cuts[:-1], cuts[1:]):
                    rows = list(range(a, b))
                    p.step_reference(st, x[t, rows], rows, t + 1, sc[t, rows], vs[t])
            assert all(st[k].tobytes() == want[k].tobytes() for k in want), (enc, trial)


def test_write_wav_bytes(tmp_path):
    from afx.evidence import Clip, pcm16_reference
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, NAN, 1.5 / 32768, 3e-5], dtype=f32)
    pcm = pcm16_reference(x)
    assert pcm.tolist() == [0, 16384, -16384, 32767, -32768, 0, 2, 1]
    data = pcm.astype("<i2").tobytes()
    want = (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16)
            + b"data" + struct.pack("<I", len(data)) + data)
    for i, audio in enumerate((x, pcm)):  # an fp32 clip goes through the pcm16 rule; a pcm16 clip is written as it is
        path = str(tmp_path / f"clip{i}.wav")
        Clip(3, 2, 1, audio, np.zeros(2, f32), True, 0).write_wav(path)
        assert open(path, "rb").read() == want


def _bare(S=2, hop=H, window=16000):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=window, hop=hop, device="cpu")


def _scorer(S=2, policy=None, **kw):
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    return EvidenceScorer(VerdictScorer(_bare(S, **kw), VerdictPolicy(0.0)), EvidencePolicy(post=2, clips=4) if policy is None else policy)


class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


def test_evidence_scorer_refuses_what_it_cannot_wrap_and_presents_the_inner_surface(built):
    from afx._lib import AfxError
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import Evidence, EvidencePolicy, EvidenceScorer
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    vp, ep = VerdictPolicy(0.0), EvidencePolicy(post=2, clips=4)
    es = _scorer(S=3)
    for inner in (_bare(), GatedScorer(_bare()), PacketScorer(_bare(), 8000, "mulaw"), es, CascadeScorer(_bare(), _Model(), CascadePolicy(0.0, 2)),
                  object(), None):
        with pytest.raises(ValueError):
            EvidenceScorer(inner, ep)
    with pytest.raises(ValueError):
        EvidenceScorer(VerdictScorer(_bare(), vp), "default")
    with pytest.raises(ValueError):
        EvidenceScorer(VerdictScorer(_bare(hop=16000, window=4000), vp), ep)  # pre=None: window // hop - 1 < 0
    for args in ((0, ep, H), (8193, ep, H), (2.0, ep, H), (2, None, H), (2, ep, 0), (2, ep, H, "cpu", None)):
        with pytest.raises(ValueError):
            Evidence(*args) if len(args) > 3 else Evidence(*args, device="cpu", window=None if args[2] else 16000)
    ev = es.evidence
    assert (es.S, es.hop, es.window, es.device.type) == (3, H, 16000, "cpu") and (ev.pre, ev.post, ev.clips, ev.P, ev.L) == (3, 2, 4, 4, 6)
    assert es._slot_list([2, 0], ordered=True) == [2, 0] and es.samples_seen.tolist() == [0, 0, 0]
    assert es.alarm.tolist() == [False] * 3 and torch.isnan(es.smoothed).all() and es.alarm_since.tolist() == [-1] * 3
    assert [a.tolist() for a in es.take_events()] == [[], [], [], []] and es.take_clips() == []
    assert es.stats() == dict(raised=0, recorded=0, dropped=0, merged=0, free=4, recording=0, finished=0)
    assert ev.hist.shape == (3, 4 * H) and ev.sring.shape == (3, 4) and ev.pool.shape == (4, 6) and ev.audio.shape == (4, 6 * H)
    assert Evidence(2, EvidencePolicy(pre=1, encoding="pcm16"), 160, "cpu").audio.dtype == torch.int16
    # no CPU fallback: push and update raise, and nothing moved
    with pytest.raises(AfxError):
        es.push(torch.zeros(3, H))
    with pytest.raises(AfxError):
        ev.update(torch.zeros(3, H), hop_index=1, verdict_state=es.scorer.verdicts.st)
    st = es.scorer.verdicts.st
    for args, kw in (((torch.zeros(2, H),), dict(hop_index=1, verdict_state=st)), ((torch.zeros(3, H, dtype=torch.float64),), dict(hop_index=1, verdict_state=st)),
                     ((torch.zeros(1, H), [3]), dict(hop_index=1, verdict_state=st)), ((torch.zeros(2, H), [1, 1]), dict(hop_index=1, verdict_state=st)),
                     ((torch.zeros(3, H),), dict(hop_index=[1, 2], verdict_state=st)), ((torch.zeros(3, H),), dict(hop_index=1.5, verdict_state=st)),
                     ((torch.zeros(3, H),), dict(hop_index=0, verdict_state=st)), ((torch.zeros(3, H),), dict(hop_index=1, verdict_state=st.long())),
                     ((torch.zeros(3, H),), dict(hop_index=1, verdict_state=st[:2])), ((torch.zeros(3, H),), dict(hop_index=1, verdict_state=st, scores=torch.zeros(2)))):
        with pytest.raises(ValueError):
            ev.update(*args, **kw)
    assert es.samples_seen.tolist() == [0, 0, 0] and es.stats()["free"] == 4
    # the gate and the fronts accept it in place of a scorer, around a cascade too; the cascade refuses it as a screen
    inner = EvidenceScorer(VerdictScorer(CascadeScorer(_bare(), _Model(), CascadePolicy(0.0, 2)), vp), ep)
    for front in (GatedScorer(es), PacketScorer(GatedScorer(inner), 8000, "mulaw"), JitterScorer(GatedScorer(inner), 8000, "mulaw", 4),
                  PacketScorer(es, 8000, "mulaw")):
        meta = front.state_meta()
        assert meta["evidence"] == 1 and meta["evidence_pre"] == 3 and meta["verdict"] == 1
    assert PacketScorer(GatedScorer(inner), 8000, "mulaw").state_meta()["cascade"] == 1
    with pytest.raises(ValueError):
        CascadeScorer(es, _Model(), CascadePolicy(0.0, 2))
    with pytest.raises(ValueError):
        VerdictScorer(es, vp)
    with pytest.raises(ValueError):
        GatedScorer(GatedScorer(es))


def test_reset_truncates_and_take_clips_frees_on_host_tensors():
    """``reset`` and ``take_clips`` are torch operations: on a CPU-device ``Evidence`` they are held against the numpy
    mirrors, with the pool put into a hand-made state."""
    from afx.evidence import COMPLETE, FREE, RECORDING, TRUNCATED, Evidence, EvidencePolicy
    p = EvidencePolicy(pre=1, post=2, clips=5, encoding="pcm16")
    ev = Evidence(4, p, 3, "cpu")
    st = p.new_state(4, 3)
    g = np.random.default_rng(2)
    st["pool"][:] = [[RECORDING, 2, 4, 3, 3, 7], [FREE, 0, 0, 0, 0, 0], [COMPLETE, 1, 9, 8, 4, 5], [RECORDING, 0, 2, 1, 2, 8], [COMPLETE, 3, 1, 1, 1, 6]]
    st["rec"][:], st["left"][:] = [3, -1, 0, -1], [2, 0, 1, 0]
    st["audio"][:] = g.integers(-3000, 3000, st["audio"].shape)
    st["cscores"][:] = g.standard_normal(st["cscores"].shape)
    st["counters"][:] = [9, 9, 1, 2]
    for k, t in (("pool", ev.pool), ("rec", ev.rec), ("left", ev.left), ("audio", ev.audio), ("cscores", ev.cscores), ("counters", ev.counters)):
        t.copy_(torch.from_numpy(st[k]))
    same = lambda: all(getattr(ev, k).numpy().tobytes() == st[k].tobytes() for k in ("pool", "rec", "left", "audio", "cscores", "counters"))  # noqa: E731
    ev.reset([1, 2])  # slot 2 is recording entry 0; slot 1 records nothing
    p.reset_reference(st, [1, 2])
    assert same() and ev.pool[:, 0].tolist() == [TRUNCATED, FREE, COMPLETE, RECORDING, COMPLETE] and ev.rec.tolist() == [3, -1, -1, -1]
    assert ev.stats() == dict(raised=9, recorded=9, dropped=1, merged=2, free=1, recording=1, finished=3)
    got, want = ev.take_clips(), p.take_reference(st)
    assert same() and ev.pool[:, 0].tolist() == [FREE, FREE, FREE, RECORDING, FREE] and ev.take_clips() == []
    assert [c.seq for c in got] == [5, 6, 7] and [(c.slot, c.raised_at, c.first_hop, c.hops, c.complete) for c in got] == \
        [(1, 9, 8, 4, True), (3, 1, 1, 1, True), (2, 4, 3, 3, False)]
    for a, b in zip(got, want):
        assert a.audio.dtype == np.int16 and a.audio.tobytes() == b.audio.tobytes() and a.scores.tobytes() == b.scores.tobytes()
        assert a.audio.size == a.hops * 3 and (a.seq, a.slot, a.complete) == (b.seq, b.slot, b.complete)
    ev.reset([0, 1, 2, 3])
    assert ev.pool[:, 0].tolist() == [FREE, FREE, FREE, TRUNCATED, FREE] and ev.rec.tolist() == [-1] * 4 and ev.left.tolist() == [0] * 4
    assert ev._pool[5].tolist() == [0] * 6


def test_export_and_import_on_the_host_and_every_refusal_leaves_the_scorer_unchanged(built):
    from afx.evidence import RECORDING, TRUNCATED, EvidencePolicy
    from afx.streaming import StreamState
    from afx.vad import GatedScorer
    a = _scorer(S=3)
    g = torch.Generator().manual_seed(3)
    a.scorer.scorer.ring[:] = torch.randn(3, 16000, generator=g)
    a.scorer.scorer._seen[:] = torch.tensor([8000, 20000, 0])
    a.scorer.verdicts.m[:2] = torch.tensor([-0.75, 0.125])
    a.scorer.verdicts.st[:2] = torch.tensor([[2, 0, 1, 1], [5, 0, 0, -1]], dtype=torch.int32)
    a.evidence.hist[:] = torch.randn(3, 4 * H, generator=g)
    a.evidence.sring[:] = torch.tensor([[1, 2, NAN, 0], [5, 2, 3, 4], [0, 0, 0, 0]])
    a.evidence._pool[1] = torch.tensor([RECORDING, 0, 1, 1, 2, 0], dtype=torch.int32)  # slot 0 is recording entry 1
    a.evidence.rec[0], a.evidence.left[0] = 1, 1
    st = a.export_slots([1, 0])
    assert st.meta["evidence"] == 1 and st.meta["evidence_pre"] == 3 and st.meta["verdict"] == 1 and st.seen.tolist() == [20000, 8000]
    assert torch.equal(st.tensors["evidence_hist"], a.evidence.hist[[1, 0]]) and st.tensors["evidence_hist"].dtype == torch.float32
    assert st.tensors["evidence_scores"].view(torch.int32).tolist() == a.evidence.sring[[1, 0]].view(torch.int32).tolist()
    # post, clips and encoding may differ between source and destination; pre and hop may not
    b = _scorer(S=4, policy=EvidencePolicy(pre=3, post=1, clips=2, encoding="pcm16"))
    b.evidence._pool[0] = torch.tensor([RECORDING, 3, 2, 1, 2, 4], dtype=torch.int32)  # destination slot 3 is recording entry 0
    b.evidence.rec[3], b.evidence.left[3] = 0, 1
    b.evidence.hist[:] = 7.0

    def snap(c):
        e = c.evidence
        return [e.hist.clone(), e.sring.clone(), e.rec.clone(), e.left.clone(), e._pool.clone(), e.audio.clone(), e.cscores.clone(), e.counters.clone(),
                c.scorer.verdicts.st.clone(), c.scorer.scorer.ring.clone(), c.samples_seen]

    before = snap(b)
    t = st.tensors
    foreign = [
        a.scorer.export_slots([1, 0]),                                                     # a verdict state: no evidence part
        GatedScorer(_bare(S=3)).export_slots([1, 0]),
        st.tensors, None,
        StreamState(dict(st.meta, evidence=2), st.seen, t),                                # another format
        StreamState(dict(st.meta, evidence_pre=2), st.seen, t),                            # another pre
        StreamState({k: v for k, v in st.meta.items() if k != "evidence_pre"}, st.seen, t),
        StreamState(st.meta, st.seen, {k: v for k, v in t.items() if k != "evidence_scores"}),
        StreamState(st.meta, st.seen, dict(t, evidence_hist=t["evidence_hist"][:, :-1])),  # not (pre + 1) hops of this hop
        StreamState(st.meta, st.seen, dict(t, evidence_hist=t["evidence_hist"].double())),
        StreamState(st.meta, st.seen, dict(t, evidence_scores=t["evidence_scores"][:, :3])),
        StreamState(st.meta, st.seen, dict(t, evidence_scores=t["evidence_scores"].double())),
        StreamState(dict(st.meta, hop=2000), st.seen, t),                                  # another hop: the inner scorer's refusal
        _scorer(S=3, policy=EvidencePolicy(pre=2, post=2, clips=4)).export_slots([1, 0]),
        _scorer(S=3, hop=2000, policy=EvidencePolicy(pre=3)).export_slots([1, 0]),
    ]
    for i, f in enumerate(foreign):
        with pytest.raises(ValueError):
            b.import_slots([3, 1], f)
        assert all(torch.equal(u.nan_to_num(-7.0), v.nan_to_num(-7.0)) for u, v in zip(before, snap(b))), i
    with pytest.raises(ValueError):
        b.import_slots([3], st)  # two sessions for one slot
    with pytest.raises(ValueError):
        b.scorer.import_slots([3, 1], st)  # a VerdictScorer refuses an evidence state
    b.import_slots([3, 1], StreamState.from_state_dict(st.state_dict()))
    assert torch.equal(b.evidence.hist[[3, 1]], a.evidence.hist[[1, 0]]) and bool((b.evidence.hist[[0, 2]] == 7.0).all())
    assert b.evidence.sring[[3, 1]].view(torch.int32).tolist() == a.evidence.sring[[1, 0]].view(torch.int32).tolist()
    assert b.samples_seen.tolist() == [0, 8000, 0, 20000] and b.alarm.tolist() == [False, True, False, False]
    # what the destination slot was recording is truncated; the source's recording did not move
    assert b.evidence.pool[0].tolist() == [TRUNCATED, 3, 2, 1, 2, 4] and b.evidence.rec.tolist() == [-1] * 4 and b.evidence.left.tolist() == [0] * 4
    assert a.evidence.rec.tolist() == [1, -1, -1] and a.evidence.pool[1, 0] == RECORDING
    back = b.export_slots([3, 1])
    assert all(torch.equal(back.tensors[k].nan_to_num(-7.0), st.tensors[k].nan_to_num(-7.0)) for k in st.tensors) and back.meta == st.meta
    # the source slot is reset: its clip comes back truncated
    a.reset([0])
    assert a.evidence.pool[1].tolist() == [TRUNCATED, 0, 1, 1, 2, 0] and a.samples_seen.tolist() == [0, 20000, 0]
    (clip,) = a.take_clips()
    assert (clip.slot, clip.hops, clip.complete) == (0, 2, False) and clip.audio.shape == (2 * H,)
    # through the gate: every layer peels its own part
    g1, g2 = GatedScorer(_scorer(S=2)), GatedScorer(_scorer(S=2))
    g1.scorer.evidence.sring[1] = torch.tensor([4.0, 3.0, 2.0, 1.0])
    g2.import_slots([0], g1.export_slots([1]))
    assert g2.scorer.evidence.sring.tolist() == [[4.0, 3.0, 2.0, 1.0], [0.0] * 4]
    with pytest.raises(ValueError):
        g2.import_slots([0], GatedScorer(_scorer(S=2).scorer).export_slots([1]))


def test_evidence_entry_points_are_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    lib = ctypes.CDLL(built.LIB_PATH)
    for name, nargs in (("afx_k_evidence_mark", 14), ("afx_k_evidence_copy", 17)):
        assert f"int {name}(" in src and hasattr(lib, name)
        assert name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == nargs
        decl = src[src.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") == nargs - 1
    # bad scalar arguments are refused on the host side of the library: nothing is launched, so no GPU is needed
    l = built.lib()
    one = ctypes.c_void_p(8)  # (never dereferenced: the refusal comes first)
    assert l.afx_k_evidence_mark(None, 1, one, 1, 0, 0, one, one, one, one, 1, one, one, None) != 0 and b"evidence_mark" in l.afx_last_error()
    for A, S, pre, post, clips in ((0, 1, 0, 0, 1), (8193, 1, 0, 0, 1), (1, 0, 0, 0, 1), (1, 1, -1, 0, 1), (1, 1, 0, -1, 1), (1, 1, 0, 0, 0), (1, 1, 0, 0, 8193)):
        assert l.afx_k_evidence_mark(one, A, one, S, pre, post, one, one, one, one, clips, one, one, None) != 0
        assert b"evidence_mark" in l.afx_last_error()
    good = dict(stride=1, A=1, hop=4, pre=0, post=0, S=1, clips=1, enc=0)
    for bad in (dict(A=0), dict(A=8193), dict(hop=0), dict(pre=-1), dict(post=-1), dict(S=0), dict(clips=0), dict(clips=8193), dict(enc=2), dict(enc=-1),
                dict(stride=0), dict(pre=65535, hop=1 << 16), dict(post=1 << 30, hop=4)):
        a = dict(good, **bad)
        rc = l.afx_k_evidence_copy(one, one, a["stride"], one, one, a["A"], a["hop"], a["pre"], a["post"], one, one, a["S"], one, one, a["clips"], a["enc"], None)
        assert rc != 0 and b"evidence_copy" in l.afx_last_error(), bad
    assert l.afx_k_evidence_copy(None, one, 1, one, one, 1, 4, 0, 0, one, one, 1, one, one, 1, 0, None) != 0 and b"evidence_copy" in l.afx_last_error()

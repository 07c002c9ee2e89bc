"""Provenance without a GPU (afx/provenance.py): the policy's numpy statement on hand-made counts, where the new kind nests,
the jitter planner's "spans" ops against oracle/jitter.py's ``RefSlot`` (the byte stream they write is c16 computed from
``RefSlot.kinds`` by the formula, sample for sample), that a chain without the layer plans what it planned, and the session
moves with their refusals.  The numpy device is ``oracle.jitter.NumpyDevice`` with the "spans" verb added here."""
import random
import types

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import NumpyDevice, RefSlot, Schedule, dtx_events
from packet_helpers import bits as _bits, inner as _inner

H, WINDOW = 4000, 16000
QNAN = 0x7fc00000


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


# ---- 1. the policy ---------------------------------------------------------------------------------------------------------
def _policy(**kw):
    from afx.provenance import ProvenancePolicy
    return ProvenancePolicy(**kw)


def test_limit_is_the_floor_of_the_fp32_share_times_the_window():
    p = _policy()
    assert p.limit(4, 4000) == int(np.floor(np.float64(np.float32(0.05)) * 16000)) == 800
    assert _policy(max_share=0.0).limit(4, 4000) == 0 and _policy(max_share=1.0).limit(4, 4000) == 16000
    assert _policy(max_share=0.1).limit(3, 7) == 2  # 2.1000000312924385
    assert p.params() == dict(max_share=float(np.float32(0.05)), abstain=True)


def test_a_young_session_sums_only_its_own_hops_and_the_ring_wraps():
    p = _policy()
    meas, valid = p.run_reference([100, 200, 300, 400, 0, 0, 0, 0, 801], H, WINDOW)
    #                        k:     1    2    3    4   5  6  7  8   9      W = 4, limit = 800
    assert meas[:, 0].tolist() == [100, 200, 300, 400, 0, 0, 0, 0, 801]
    assert meas[:, 1].tolist() == [100, 300, 600, 1000, 900, 700, 400, 0, 801]
    assert valid.tolist() == [True, True, True, False, False, True, True, True, False]
    assert meas[:, 2].tolist() == [int(v) for v in valid]


def test_a_reset_does_not_read_the_previous_sessions_entries():
    from afx.provenance import ProvenanceState
    p, st = _policy(), ProvenanceState(2, 4)
    for k in range(1, 7):
        p.step_reference([0, 1], [H, 0], k, None, st, H)
    assert st.st.tolist() == [[4 * H, 0], [0, 1]] and st.totals.tolist() == [[6, 6 * H, 6], [6, 0, 0]]
    ring = st.ring.copy()
    st.reset([0])
    assert st.st[0].tolist() == [0, 1] and st.totals[0].tolist() == [0, 0, 0] and np.array_equal(st.ring, ring)  # the ring is left alone
    out, meas = p.step_reference([0], [7], 1, np.array([0.25], np.float32), st, H)
    assert meas.tolist() == [[7, 7, 1]] and out.tolist() == [0.25]  # hop 1 of the new session: entries 2..4 are the old one's
    out, meas = p.step_reference([0], [0], 2, np.array([0.25], np.float32), st, H)
    assert meas.tolist() == [[0, 7, 1]]


def test_a_skipped_row_changes_nothing_and_its_score_passes():
    from afx.provenance import ProvenanceState
    p, st = _policy(), ProvenanceState(3, 4)
    p.step_reference([0, 1, 2], [H, H, H], 1, None, st, H)
    before = st.copy()
    s = np.array([0.5, -1.0, 2.0], dtype=np.float32)
    out, meas = p.step_reference([0, 1, 2], [5, -1, H + 1], [0, 2, 2], s, st, H)  # k < 1, c < 0, c > hop
    assert (meas == -1).all() and np.array_equal(_bits(out), _bits(s))
    assert all(np.array_equal(getattr(st, f), getattr(before, f)) for f in ("ring", "st", "totals"))
    out, meas = p.step_reference([2, 0], [0, 0], [2, 0], s[:2], st, H)  # a live row beside a skipped one
    assert meas.tolist() == [[0, H, 0], [-1, -1, -1]] and _bits(out).tolist() == [QNAN, int(_bits(s[1:2])[0])]


def test_counters_saturate_and_abstain_off_passes_every_score():
    from afx.provenance import ProvenanceState
    N = (1 << 31) - 1
    hop = 1 << 24
    p, st = _policy(max_share=1.0), ProvenanceState(1, 1024)
    st.ring[:] = hop
    st.totals[:] = [N - 1, N - 5, N]
    out, meas = p.step_reference([0], [hop], 5000, np.array([1.5], np.float32), st, hop)
    assert meas.tolist() == [[hop, N, 1]] and st.st.tolist() == [[N, 1]]  # 1024 * 2^24 = 2^34: stored saturated, compared exactly
    assert st.totals.tolist() == [[N, N, N]] and out.tolist() == [1.5]
    q, s2 = _policy(max_share=0.0, abstain=False), ProvenanceState(1, 4)
    out, meas = q.step_reference([0], [1], 1, np.array([1.5], np.float32), s2, H)
    assert meas.tolist() == [[1, 1, 0]] and out.tolist() == [1.5] and s2.totals.tolist() == [[1, 1, 1]]
    out, _ = _policy(max_share=0.0).step_reference([0], [1], 2, np.array([1.5], np.float32), s2, H)
    assert out.view(np.int32).tolist() == [QNAN]


def test_argument_refusals():
    from afx.provenance import Provenance, ProvenancePolicy, ProvenanceScorer, ProvenanceState
    for kw in (dict(max_share=-0.1), dict(max_share=1.5), dict(max_share=float("nan")), dict(max_share="0.1"), dict(max_share=True),
               dict(abstain=1), dict(abstain=None)):
        with pytest.raises(ValueError):
            ProvenancePolicy(**kw)
    p, st = ProvenancePolicy(), ProvenanceState(2, 4)
    for args in (([0, 0], [1, 1], 1, None, st, H), ([0, 2], [1, 1], 1, None, st, H), ([0], [1, 1], 1, None, st, H),
                 ([0], [1.5], 1, None, st, H), ([0], [1], [1, 2], None, st, H), ([0], [1], 1, [0.5, 0.5], st, H),
                 ([0], [1], 1, None, object(), H), ([0], [1], 1, None, st, 0), ([0], [1], 1, None, st, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            p.step_reference(*args)
    for args in ((0, p, H, WINDOW), (8193, p, H, WINDOW), (2, object(), H, WINDOW), (2, p, 0, WINDOW), (2, p, H, 1025 * H)):
        with pytest.raises(ValueError):
            Provenance(*args, device="cpu")
    pv = Provenance(2, p, H, WINDOW, device="cpu")
    assert (pv.W, pv.limit) == (4, 800) and pv.valid.tolist() == [True, True] and pv.synthetic.tolist() == [0, 0]
    c = torch.zeros(2, dtype=torch.int32)
    for args, kw in (((c.long(),), dict(hop_index=1)), ((c[:1],), dict(hop_index=1)), ((c,), dict(hop_index=0)),
                     ((c,), dict(hop_index=1, scores=torch.zeros(3))), ((c, [0, 0]), dict(hop_index=1))):
        with pytest.raises(ValueError):
            pv.update(*args, **kw)
    assert pv.update(c[:0], [], hop_index=1)[1].shape == (0, 3)
    layer = ProvenanceScorer(_inner(2))
    for counts, slots in ((c.long(), None), (c[:1], None), (c, [0])):
        with pytest.raises(ValueError):
            layer.note_synthetic(counts, slots)
    assert {k: v.tolist() for k, v in layer.stats().items()} == dict(hops=[0, 0], synthetic=[0, 0], withheld=[0, 0])


# ---- 2. nesting -----------------------------------------------------------------------------------------------------------
class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


def _makers():
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenanceScorer
    from afx.quality import QualityScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    vp = VerdictPolicy(0.0, 0.5, verifier_enter=-0.5)
    return dict(base=lambda s=None: _inner(2), cascade=lambda s: CascadeScorer(s, _Model(), CascadePolicy(0.0, 2)),
                quality=lambda s: QualityScorer(s), provenance=lambda s: ProvenanceScorer(s), verdict=lambda s: VerdictScorer(s, vp),
                evidence=lambda s: EvidenceScorer(s, EvidencePolicy()), gate=lambda s: GatedScorer(s),
                packet=lambda s: PacketScorer(s, 8000, "mulaw"), jitter=lambda s: JitterScorer(s, 8000, "mulaw", 4))


def test_where_the_provenance_layer_nests():
    from afx._layer import ORDER
    m = _makers()
    assert ORDER.index("quality") + 1 == ORDER.index("provenance") == ORDER.index("verdict") - 1
    for below in ((), ("cascade",), ("quality",), ("cascade", "quality")):  # around base, cascade or quality
        s = m["base"]()
        for k in below:
            s = m[k](s)
        p = m["provenance"](s)
        assert p.S == 2 and p.layer == "provenance" and p._cascade == ("cascade" in below)
        assert m["evidence"](m["verdict"](p)).S == 2 and m["gate"](m["verdict"](p)).S == 2  # verdict goes around it
        assert m["jitter"](p).S == 2 and m["packet"](m["gate"](p)).S == 2
    for below in (("verdict",), ("verdict", "evidence"), ("gate",), ("packet",), ("jitter",), ("provenance",)):
        s = m["base"]()
        for k in below:
            s = m[k](s)
        with pytest.raises(ValueError):
            m["provenance"](s)
    for bad in (object(), None):
        with pytest.raises(ValueError):
            m["provenance"](bad)
    for k in ("quality", "cascade"):  # neither goes around it
        with pytest.raises(ValueError):
            m[k](m["provenance"](m["base"]()))
    with pytest.raises(ValueError):
        m["evidence"](m["provenance"](m["base"]()))  # (the evidence layer goes around a verdict layer only)


def test_discovery_attaches_a_plain_or_tone_gate_and_refuses_lookahead_and_turns():
    from afx.jitter import JitterScorer, MixedJitterScorer
    from afx.provenance import ProvenanceScorer
    from afx.turns import TurnScorer
    from afx.vad import GatedScorer, LookaheadGate, ToneGate
    from afx.verdict import VerdictPolicy, VerdictScorer
    from afx.streaming import SlidingWindowScorer
    layer = lambda: ProvenanceScorer(_inner(2))  # noqa: E731
    clip = lambda: SlidingWindowScorer(None, 2, window=WINDOW, hop=WINDOW, device="cpu")  # noqa: E731  (a TurnScorer's inner: hop == window)
    jit = (lambda s: JitterScorer(s, 8000, "mulaw", 4), lambda s: MixedJitterScorer(s, [(8000, "mulaw"), (48000, "pcm_s16le")], 60))
    for front in jit:
        for gate in (None, ToneGate()):
            g = GatedScorer(VerdictScorer(layer(), VerdictPolicy(0.0, 0.5)), gate)
            assert not g._syn and not hasattr(g, "gsyn")
            js = front(g)
            assert g._syn and g.gsyn.shape == (2, 2 * H // 160) and g.gsyn.dtype == torch.int32 and g._syn_below is g.scorer.scorer
            assert js._prov == (g, 160, True) and js.psyn.shape == (2, js.ring_len) and js.psyn.dtype == torch.uint8
        p = layer()
        js = front(p)
        assert js._prov == (p, H, False)
        for g in (GatedScorer(layer(), LookaheadGate()), TurnScorer(ProvenanceScorer(clip()))):
            with pytest.raises(ValueError, match="out of scope"):
                front(g)
        # the same fronts without the layer build as before: no lane, no ring, the gate untouched
        for g in (GatedScorer(_inner(2), LookaheadGate()), TurnScorer(clip()), GatedScorer(_inner(2)), _inner(2)):
            js = front(g)
            assert js._prov is None and not hasattr(js, "psyn") and not getattr(g, "_syn", False) and not hasattr(g, "gsyn")
    with pytest.raises(ValueError, match="not attached"):
        GatedScorer(layer()).note_synthetic(torch.zeros(2, 25, dtype=torch.int32), None)


# ---- 3. the planner against the oracle ----------------------------------------------------------------------------------------
class SpanDevice(NumpyDevice):
    """``NumpyDevice`` with the "spans" verb as include/afx.h states it, on the scorer's own byte ring.  Every release must be
    followed by its spans ops (one, or one per ``SPANS_MAX_ROWS`` rows) whose rows partition each release row's output range; ``marks[s]`` collects, release by release,
    the bytes of that range as the ring then holds them: the slot's 16 kHz mark stream."""

    def __init__(self, js, **kw):
        super().__init__(js, **kw)
        self.psyn = js.psyn.numpy()
        self.marks = [[] for _ in range(js.S)]
        self.span_rows = self.span_ops = 0

    def reset(self, s):
        super().reset(s)
        self.marks[s] = []

    def run(self, plan, pay):
        from afx import jitter
        ops, R = plan.ops, self.js.ring_len
        for i, op in enumerate(ops):
            if op[0] == "spans":
                assert i and ops[i - 1][0] in ("release", "spans")
            if op[0] != "release":
                continue
            mine = []
            while i + 1 + len(mine) < len(ops) and ops[i + 1 + len(mine)][0] == "spans":
                mine.append(ops[i + 1 + len(mine)])
            assert mine, "every release is followed by its spans"
            for sp in mine:
                assert sp[1].dtype == np.int32 and sp[1].ndim == 2 and sp[1].shape[1] == 4 and 1 <= len(sp[1]) <= jitter.SPANS_MAX_ROWS
                assert 0 <= sp[2] <= R and sp[2] == sp[1][:, 2].max()
            assert all(len(sp[1]) == jitter.SPANS_MAX_ROWS for sp in mine[:-1])
            self.span_ops += len(mine)
            rows = np.concatenate([sp[1] for sp in mine])
            self.span_rows += len(rows)
            released = set()
            for rel in op[1].tolist():
                s, n_out, wpos = rel[0], rel[3], rel[6]
                released.add(s)
                mine = sorted(((int(w) - wpos) % R, int(n), int(v)) for q, w, n, v in rows.tolist() if q == s)
                assert mine, "every release row has its spans"
                at = 0
                for off, n, v in mine:  # they tile [0, n_out): no hole, no overlap
                    assert v in (0, 1) and n >= 0 and (off == at or (n == 0 and off == at % R)), (mine, n_out)
                    self.psyn[s, (wpos + at + np.arange(n)) % R] = v
                    at += n
                assert at == n_out
                self.marks[s].extend(self.psyn[s, (wpos + np.arange(n_out)) % R].tolist())
            assert released == set(rows[:, 0].tolist())
        super().run(types.SimpleNamespace(ops=[op for op in ops if op[0] != "spans"]), pay)


def _ref(mode, depth, rate, noise=None):
    if mode == "repeat":
        return RefSlot(depth, mode, rate // 100, 3 * (rate // 100), noise=noise)
    return RefSlot(depth, mode, rate=rate, noise=noise) if mode == "pitch_sync" else RefSlot(depth, mode, noise=noise)


def _c16_equals(dev, s, ref, L, M):
    from afx.provenance import marks16
    want = marks16(ref.kinds, L, M)
    assert len(ref.kinds) == ref.next and len(dev.marks[s]) == len(want) == -(-ref.next * L // M)
    assert np.array_equal(np.array(dev.marks[s], dtype=np.uint8), want)
    return int(want.sum())


def _strip(ops):
    return [op for op in ops if op[0] != "spans"]


def _same_ops(a, b):
    assert [op[0] for op in a] == [op[0] for op in b]
    for x, y in zip(a, b):
        assert np.array_equal(x[1], y[1]) and x[1].dtype == y[1].dtype and x[2] == y[2], x[0]


@pytest.mark.parametrize("rate,encoding,mode,seed", [(8000, "mulaw", "repeat", 11), (8000, "mulaw", "pitch_sync", 12), (8000, "mulaw", "zero", 13),
                                                     (11025, "pcm_s16le", "pitch_sync", 14), (11025, "pcm_s16le", "repeat", 15),
                                                     (16000, "pcm_s16le", "zero", 16), (16000, "pcm_s16le", "repeat", 17),
                                                     (48000, "pcm_s16le", "repeat", 18), (48000, "pcm_s16le", "zero", 19)])
def test_spans_partition_every_release_and_write_c16(rate, encoding, mode, seed):
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenanceScorer
    S, depth = 2, 3 * (rate // 50)
    js = JitterScorer(ProvenanceScorer(_inner(S)), rate, encoding, depth, conceal=mode)
    plain = JitterScorer(_inner(S), rate, encoding, depth, conceal=mode)  # the same scorer without the layer
    assert (js.L, js.M) == {8000: (2, 1), 11025: (640, 441), 16000: (1, 1), 48000: (1, 3)}[rate]
    dev, pdev = SpanDevice(js), NumpyDevice(plain)
    sch = [Schedule(rate, encoding, seed + 100 * s, jump=(rate // 3 if s else 0), short=rate // 200) for s in range(S)]
    refs = [_ref(mode, depth, rate) for _ in range(S)]
    rng = random.Random(seed)
    while not all(x.done() for x in sch):
        rows = []
        for s in range(S):
            if not sch[s].done() and rng.random() < 0.8:
                rows += [(s,) + pk for pk in sch[s].tick()]
        if not rows:
            continue
        args = ([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        plan, pay = js._plan_feed(*args)
        other, _ = plain._plan_feed(*args)
        assert "spans" not in [op[0] for op in other.ops]
        _same_ops(_strip(plan.ops), other.ops)  # without the layer: op for op what the lane's plan is without its spans
        packet_helpers.go(js, dev, plan, pay)
        packet_helpers.go(plain, pdev, other, pay)
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
        for s in sorted({r[0] for r in rows}):
            refs[s].after_feed()
    plan, other = js._plan(list(range(S)), mode="flush"), plain._plan(list(range(S)), mode="flush")
    _same_ops(_strip(plan.ops), other.ops)
    packet_helpers.go(js, dev, plan)
    total = 0
    for s, r in enumerate(refs):
        r.release(r.hi)
        assert np.array_equal(_bits(dev.out[s]), _bits(r.E)) and dev.N[s] == r.next
        total += _c16_equals(dev, s, r, js.L, js.M)
        assert "rl" in "".join(r.kinds) and "lr" in "".join(r.kinds)
    assert total > 1000 and dev.span_rows > dev.launches.count("release")  # some release was cut into several runs


def test_a_rounds_spans_are_split_at_the_launchs_row_limit(monkeypatch):
    """One ``afx_k_prov_spans`` launch takes 65 535 rows and a release may be cut into many runs per slot: with the limit
    lowered to 2 rows, the lossy traffic's rounds come in several spans ops that together still partition every release."""
    from afx import jitter
    from afx.provenance import ProvenanceScorer
    assert jitter.SPANS_MAX_ROWS == 65535
    monkeypatch.setattr(jitter, "SPANS_MAX_ROWS", 2)
    rate, depth = 8000, 480
    js = jitter.JitterScorer(ProvenanceScorer(_inner(2)), rate, "mulaw", depth)
    dev, refs = SpanDevice(js), [_ref("repeat", depth, rate) for _ in range(2)]
    sch = [Schedule(rate, "mulaw", 77 + s, short=40) for s in range(2)]
    while not all(x.done() for x in sch):
        rows = [(s,) + pk for s in range(2) if not sch[s].done() for pk in sch[s].tick()]
        plan, pay = js._plan_feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        packet_helpers.go(js, dev, plan, pay)
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
        for s in sorted({r[0] for r in rows}):
            refs[s].after_feed()
    packet_helpers.go(js, dev, js._plan([0, 1], mode="flush"))
    for s, r in enumerate(refs):
        r.release(r.hi)
        assert _c16_equals(dev, s, r, 2, 1) > 500
    assert dev.span_ops > dev.launches.count("release")  # some round's rows did not fit one op


def test_spans_with_comfort_noise_mark_loss_and_noise_alike():
    from afx.jitter import ComfortNoise, JitterScorer
    from afx.provenance import ProvenanceScorer
    rate, seed = 8000, 7
    depth = 3 * (rate // 50)
    js = JitterScorer(ProvenanceScorer(_inner(1)), rate, "pcm_f32le", depth, comfort_noise=ComfortNoise(seed))
    dev, ref = SpanDevice(js), _ref("repeat", depth, rate, noise=seed)
    ev, at, rng, origin = dtx_events(rate, 1017), 0, random.Random(5), 123456
    while at < len(ev):
        blk = ev[at:at + rng.randint(1, 3)]
        at += len(blk)
        marks = [(0, origin + t, l) for kind, t, l in blk if kind == "cn"]
        audio = [(t, x) for kind, t, x in blk if kind == "pkt"]
        for kind, t, l in blk:
            if kind == "cn":
                ref.mark(t, l)
        mk = tuple(list(c) for c in zip(*marks)) if marks else None
        plan, pay = js._plan_feed([x.tobytes() for t, x in audio], [0] * len(audio), [origin + t for t, x in audio], marks=mk)
        packet_helpers.go(js, dev, plan, pay)
        for t, x in audio:
            ref.packet(t, x)
        if audio:
            ref.after_feed()
        if not audio and ref.started and rng.random() < 0.6:  # clock-driven playout through the silence
            upto = ref.hi + rate // 25
            packet_helpers.go(js, dev, js._plan([0], mode="advance", upto=upto))
            ref.release(max(ref.next, upto))
    packet_helpers.go(js, dev, js._plan([0], mode="flush"))
    ref.release(ref.hi)
    kinds = "".join(ref.kinds)
    assert np.array_equal(_bits(dev.out[0]), _bits(ref.E)) and all(p in kinds for p in ("rl", "ln", "rn", "nr"))
    n = _c16_equals(dev, 0, ref, 2, 1)
    assert n == 2 * (kinds.count("l") + kinds.count("n")) and kinds.count("n") > 1000 and kinds.count("l") > 100


def test_spans_of_a_mixed_scorer_use_each_slots_own_ratio():
    from afx.jitter import MixedJitterScorer
    from afx.provenance import ProvenanceScorer
    formats = [(8000, "mulaw"), (48000, "pcm_s16le")]
    ms = MixedJitterScorer(ProvenanceScorer(_inner(2)), formats, 60)
    plain = MixedJitterScorer(_inner(2), formats, 60)
    for m in (ms, plain):
        m.reset([0, 1], [8000, 48000])
    dev = SpanDevice(ms)
    sch = [Schedule(r, e, 31 + s, short=r // 200) for s, (r, e) in enumerate(formats)]
    refs = [_ref("repeat", 3 * (r // 50), r) for r, _ in formats]
    while not all(x.done() for x in sch):
        rows = [(s,) + pk for s in range(2) if not sch[s].done() for pk in sch[s].tick()]
        args = ([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        plan, pay = ms._plan_feed(*args)
        _same_ops(_strip(plan.ops), plain._plan_feed(*args)[0].ops)
        plain._commit(plain._plan_feed(*args)[0].book)
        packet_helpers.go(ms, dev, plan, pay)
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
        for s in sorted({r[0] for r in rows}):
            refs[s].after_feed()
    packet_helpers.go(ms, dev, ms._plan([0, 1], mode="flush"))
    for s, (L, M) in enumerate(((2, 1), (1, 3))):
        refs[s].release(refs[s].hi)
        assert np.array_equal(_bits(dev.out[s]), _bits(refs[s].E))
        assert _c16_equals(dev, s, refs[s], L, M) > 500


# ---- 4. sessions ----------------------------------------------------------------------------------------------------------------
def _gated_chain(S=3, layer=True, **policy):
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.vad import GatedScorer
    base = _inner(S)
    return JitterScorer(GatedScorer(ProvenanceScorer(base, ProvenancePolicy(**policy)) if layer else base), 16000, "pcm_s16le", 4, conceal="zero")


def _dirty(js, seed):
    """A state in every part that its checks accept: slot s has seen 2 + s hops behind the gate, 1 + s of them kept."""
    S, g = js.S, torch.Generator().manual_seed(seed)
    gate = js.scorer
    layer = gate.scorer
    base = layer.scorer
    for s in range(S):
        base._seen[s] = (1 + s) * H
        gate._seen[s], gate._fill[s], gate._head[s] = (2 + s) * H, 160 * (3 + s), H * (s % 2)
        b = js._b
        b.fill[s], b.head[s] = 100 + s, (7 * H + 3) * s % js.ring_len
        b.next[s] = b.hi[s] = (2 + s) * H + 100 + s  # (16 kHz: made = next = the gate's samples + the pending ones)
        b.started[s], b.received[s], b.concealed[s] = 1, 5 * H, 90
    js.ring[:] = torch.randn(S, js.ring_len, generator=g)
    js.psyn[:] = torch.randint(0, 2, (S, js.ring_len), generator=g).to(torch.uint8)
    gate.ring[:] = torch.randn(S, gate.ring_len, generator=g)
    gate.gsyn[:] = torch.randint(0, 161, gate.gsyn.shape, generator=g).to(torch.int32)
    p = layer.provenance
    p.ring[:] = torch.randint(0, H + 1, (S, 4), generator=g).to(torch.int32)
    for s in range(S):
        k = 1 + s
        tot = int(sum(int(p.ring[s, (k - 1 - i) % 4]) for i in range(min(k, 4))))
        p.st[s] = torch.tensor([tot, int(tot <= p.limit)], dtype=torch.int32)
        p.totals[s] = torch.tensor([k, 17 * k, k - 1], dtype=torch.int32)


def _equal_states(a, b):
    assert a.meta == b.meta and torch.equal(a.seen, b.seen) and sorted(a.tensors) == sorted(b.tensors)
    for k in a.tensors:
        assert a.tensors[k].dtype == b.tensors[k].dtype and torch.equal(a.tensors[k], b.tensors[k]), k


def test_export_and_import_round_trip_with_the_lane_on():
    from afx._layer import StreamState
    A, B = _gated_chain(), _gated_chain(max_share=0.5, abstain=False)  # the policy may differ where a session goes
    _dirty(A, 1)
    st = A.export_slots([2, 0])
    t = st.tensors
    assert {"jitter_syn", "gate_syn", "prov_ring", "prov_state", "prov_totals"} <= set(t)
    assert st.meta["provenance"] == 1 and st.meta["provenance_window"] == dict(W=4, hop=H)
    assert t["jitter_syn"].dtype == torch.uint8 and t["jitter_syn"].shape == t["jitter_pending"].shape
    assert (t["jitter_syn"][0, 102:] == 0).all() and (t["jitter_syn"][1, 100:] == 0).all() and t["jitter_syn"].max() == 1
    assert t["gate_syn"].dtype == torch.int64 and t["gate_syn"].shape == (2, H // 160)
    assert (t["gate_syn"][0, 5:] == -1).all() and (t["gate_syn"][0, :5] >= 0).all() and (t["gate_syn"][1, 3:] == -1).all()
    gate = A.scorer
    assert t["gate_syn"][0, :5].tolist() == gate.gsyn[2, :5].tolist()  # slot 2: head 0
    assert t["prov_ring"].dtype == torch.int32 and t["prov_state"].dtype == t["prov_totals"].dtype == torch.int64
    st = StreamState.from_state_dict(st.state_dict())
    B.import_slots([1, 2], st)
    back = B.export_slots([1, 2])
    want = {k: v.clone() for k, v in st.tensors.items()}
    lim = B.scorer.scorer.provenance.limit
    want["prov_state"][:, 1] = (want["prov_state"][:, 0] <= lim).long()  # valid is set under the importing policy's limit
    _equal_states(back, StreamState(st.meta, st.seen, want))
    assert B.scorer.gsyn[0].abs().sum() == 0 and B.psyn[0].sum() == 0  # a slot that was not named
    # a state without the front's and the gate's parts imports with zeros
    bare = StreamState(st.meta, st.seen, {k: v for k, v in st.tensors.items() if k not in ("jitter_syn", "gate_syn")})
    C = _gated_chain()
    C.psyn[:], C.scorer.gsyn[:] = 1, 9
    C.import_slots([0, 1], bare)
    again = C.export_slots([0, 1]).tensors
    assert again["jitter_syn"].sum() == 0 and again["gate_syn"].max() == 0 and (C.psyn[2] == 1).all() and (C.scorer.gsyn[2] == 9).all()
    assert (C.psyn[:2] == 0).all() and (C.scorer.gsyn[:2] == 0).all()


def test_import_refuses_rows_that_cannot_be_a_sessions():
    from afx._layer import StreamState
    A = _gated_chain()
    _dirty(A, 2)
    st = A.export_slots([0, 1, 2])

    def broken(key, fn):
        t = {k: v.clone() for k, v in st.tensors.items()}
        fn(t[key])
        return StreamState(st.meta, st.seen, t)

    def at(*idx, v):
        def fn(x):
            x[idx] = v
        return fn

    cases = [("jitter_syn", at(0, 5, v=2)), ("jitter_syn", at(0, 100, v=1)),          # a mark that is no mark; a mark beyond the fill
             ("gate_syn", at(0, 0, v=161)), ("gate_syn", at(0, 3, v=0)), ("gate_syn", at(0, 0, v=-1)),  # above frame; -1 after the fill only
             ("prov_ring", at(0, 0, v=H + 1)), ("prov_ring", at(0, 1, v=-1)),       # a count above hop
             ("prov_state", at(1, 0, v=123456)), ("prov_state", at(1, 1, v=2)),     # a total that is not the ring's sum
             ("prov_totals", at(2, 2, v=9)), ("prov_totals", at(2, 1, v=-1))]      # withheld more often than hops
    for key, fn in cases:
        B = _gated_chain()
        before = packet_helpers.snap(B)
        with pytest.raises(ValueError):
            B.import_slots([0, 1, 2], broken(key, fn))
        assert packet_helpers.same(before, packet_helpers.snap(B)), key  # nothing changed, at any depth
    for key, dtype in (("jitter_syn", torch.int32), ("gate_syn", torch.int32), ("prov_ring", torch.int64), ("prov_state", torch.int32)):
        t = dict(st.tensors)
        t[key] = t[key].to(dtype)
        with pytest.raises(ValueError):
            _gated_chain().import_slots([0, 1, 2], StreamState(st.meta, st.seen, t))
    # a chain without the layer refuses the state, and a state without the layer's part is refused by a chain with it
    with pytest.raises(ValueError, match="no provenance layer"):
        _gated_chain(layer=False).import_slots([0, 1, 2], st)
    old = _gated_chain(layer=False).export_slots([0, 1, 2])
    assert not {"jitter_syn", "gate_syn", "prov_ring"} & set(old.tensors) and "provenance" not in old.meta
    with pytest.raises(ValueError, match="provenance part"):
        _gated_chain().import_slots([0, 1, 2], old)
    B = _gated_chain()
    B.import_slots([0, 1, 2], st)  # (the state itself is a good one)


# ---- 5. the entry points --------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_scalars_by_name(built):
    import ctypes
    l = built.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(afx_k_prov_spans=[p, 1, 64, p, 1, 8], afx_k_prov_frames=[p, 1, 64, p, 1, 16, 4, p],
                afx_k_prov_compact=[p, p, p, 1, 4, 16, p, 1, 8], afx_k_prov_take=[p, 1, 8, p, 1, 4, 16, p],
                afx_k_provenance=[p, p, p, 1, 1, 16, 3, 1, p, 2, p, p, 1, p, p])
    bad = dict(afx_k_prov_spans=[(0, None), (3, None), (1, 0), (2, 0), (2, (1 << 30) + 1), (4, 0), (4, 65536), (5, -1), (5, 65)],
               afx_k_prov_frames=[(0, None), (3, None), (7, None), (1, 0), (2, 0), (4, 0), (4, 65536), (5, 0), (5, 65), (6, 0), (6, 3)],
               afx_k_prov_compact=[(0, None), (1, None), (2, None), (6, None), (3, 0), (3, 65536), (4, 0), (4, 513), (5, 0), (7, 0), (8, 3)],
               afx_k_prov_take=[(0, None), (3, None), (7, None), (1, 0), (2, 0), (4, 0), (5, 0), (5, 9), (6, 0)],
               afx_k_provenance=[(0, None), (1, None), (8, None), (10, None), (11, None), (13, None), (14, None), (3, 0), (4, 0), (4, 8193),
                                 (5, 0), (5, (1 << 24) + 1), (6, -1), (6, 33), (7, 2), (9, 0), (9, 1025), (12, 0)])
    for name, args in good.items():
        who = name[len("afx_k_"):].encode()
        for i, v in bad[name]:
            a = list(args)
            a[i] = v
            assert getattr(l, name)(*a, None) != 0, (name, i, v)
            assert l.afx_last_error().startswith(who + b":"), (name, i, v, l.afx_last_error())

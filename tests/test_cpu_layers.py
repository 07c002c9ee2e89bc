"""The streaming stack as a whole on the host (afx/_layer.py): which object may go around which, the layout of the
``StreamState`` a full chain exports, and the contract that a refused ``import_slots`` changes no layer at any depth.  The
tables below are literals: they state what the stack did before the layers shared a base, not what the code's own order
table says.  No GPU: every scorer is built on the CPU, where it can be constructed, given state by hand and moved."""
import io

import numpy as np
import pytest
import torch

H, WINDOW = 4000, 16000


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _bare(S=2):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=WINDOW, hop=H, device="cpu")


class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


# ---- 1. the nesting matrix -------------------------------------------------------------------------------------------------
INNER = "base cascade quality verdict evidence gate packet jitter resampling object none".split()
MATRIX = {
    "cascade":    "ok VE VE VE VE VE VE VE VE VE VE",
    "quality":    "ok ok VE VE VE VE VE VE VE VE VE",
    "verdict":    "ok ok ok VE VE VE VE VE VE VE VE",
    "evidence":   "VE VE VE ok VE VE VE VE VE VE VE",
    "gate":       "ok ok ok ok ok VE VE VE VE VE VE",
    "resampling": "ok ok ok ok ok ok ok ok",  # (the fronts: around what a front around a scorer can be)
    "packet":     "ok ok ok ok ok ok ok ok",
    "jitter":     "ok ok ok ok ok ok ok ok",
}


def _builders():
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.streaming import ResamplingScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    vp = VerdictPolicy(0.0, 0.5, verifier_enter=-0.5)
    outer = {
        "cascade": lambda s: CascadeScorer(s, _Model(), CascadePolicy(0.0, 2)),
        "quality": lambda s: QualityScorer(s, QualityPolicy()),
        "verdict": lambda s: VerdictScorer(s, vp),
        "evidence": lambda s: EvidenceScorer(s, EvidencePolicy()),
        "gate": lambda s: GatedScorer(s),
        "resampling": lambda s: ResamplingScorer(s, 8000),
        "packet": lambda s: PacketScorer(s, 8000, "mulaw"),
        "jitter": lambda s: JitterScorer(s, 8000, "mulaw", 4),
    }
    inner = {k: (lambda k=k: outer[k](_bare())) for k in ("cascade", "quality", "verdict", "gate", "packet", "jitter", "resampling")}
    inner.update(base=_bare, evidence=lambda: outer["evidence"](outer["verdict"](_bare())), object=object, none=lambda: None)
    return outer, inner


def test_the_nesting_matrix(built):
    outer, inner = _builders()
    seen = 0
    for o, row in MATRIX.items():
        for i, want in zip(INNER, row.split()):
            if want == "ok":
                assert outer[o](inner[i]()).S == 2, (o, i)
            else:
                assert want == "VE"
                with pytest.raises(ValueError):
                    outer[o](inner[i]())
            seen += 1
    assert seen == 5 * 11 + 3 * 8


# ---- the full chain, with state given by hand ----------------------------------------------------------------------------------
def _chain(S, front="packet", cooldown=0, confirm=1):
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    quality = QualityScorer(CascadeScorer(_bare(S), _Model(), CascadePolicy(0.0, 2, cooldown=cooldown)), QualityPolicy())
    g = GatedScorer(EvidenceScorer(VerdictScorer(ProvenanceScorer(quality, ProvenancePolicy()),
                                                 VerdictPolicy(0.0, 0.5, confirm=confirm, release=2, verifier_enter=-0.5)), EvidencePolicy()))
    return PacketScorer(g, 8000, "mulaw") if front == "packet" else JitterScorer(g, 8000, "mulaw", 4)


def _layers(front):
    gate = front.scorer
    evidence = gate.scorer
    verdict = evidence.scorer
    provenance = verdict.scorer
    quality = provenance.scorer
    cascade = quality.scorer
    return dict(front=front, gate=gate, evidence=evidence, verdict=verdict, provenance=provenance, quality=quality, cascade=cascade,
                base=cascade.screen)


def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.int32))


COOLDOWN, CONFIRM = 2, 3
NAN, INF = float("nan"), float("inf")


def _dirty(front, seed, roll=0):
    """Non-default state in every layer of a ``_chain(S, "packet", COOLDOWN, CONFIRM)``: every row a state the layer's own
    checks accept, the rings random; ``roll`` shifts which slot gets which row."""
    from afx.evidence import RECORDING
    L, S = _layers(front), front.S
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    pick = lambda rows: [rows[(s + roll) % 4] for s in range(S)]  # noqa: E731
    inner_hops = pick([2, 5, 0, 1])
    b = L["base"]
    b.ring[:] = rnd(S, WINDOW)
    b._seen[:] = torch.tensor(inner_hops) * H
    c = L["cascade"]
    c.wait[:] = torch.tensor(pick([1, 2, 0, 0]), dtype=torch.int32)
    c.verified[:] = torch.tensor(pick([0.5, -1.25, NAN, NAN]))
    c.verified_at[:] = torch.tensor(pick([4000, 20000, -1, -1]))
    q = L["quality"].quality
    q.ring[:] = torch.randint(0, 32, (S, 4), generator=g).to(torch.uint8)
    q.st[:] = torch.tensor(pick([[_bits(0.5), 1, 1], [0, 7000, 2], [0, 0, 0], [5, 3, 0]]), dtype=torch.int32)
    q.totals[:] = torch.tensor(pick([[2, 0, 1, 0, 0, 0], [5, 0, 0, 2, 3, 0], [0] * 6, [1, 0, 0, 0, 0, 1]]), dtype=torch.int32)
    p = L["provenance"].provenance                        # (its own generator: the other layers' rows stay what they were)
    p.ring[:] = torch.randint(0, 401, (S, 4), generator=torch.Generator().manual_seed(100 + seed), dtype=torch.int32)
    hops, slot_of = torch.tensor(inner_hops)[:, None], torch.arange(1, 5)[None, :]  # ring position j holds hop j + 1, j + 5, ...
    total = (p.ring * ((slot_of <= hops) | (hops >= 4))).sum(dim=1)  # the window's hops: all four once four were seen, else 1..k
    p.st[:] = torch.stack([total, total <= p.limit], dim=1).to(torch.int32)
    p.totals[:] = torch.tensor(pick([[2, 30, 1], [5, 900, 2], [0, 0, 0], [1, 0, 0]]), dtype=torch.int32)
    v = L["verdict"].verdicts
    v.m[:] = torch.tensor(pick([0.25, -0.3, NAN, 0.1]))
    v.st[:] = torch.tensor(pick([[5, 2, 0, -1], [7, 1, 1, 4], [0, 0, 0, -1], [1, 0, 0, -1]]), dtype=torch.int32)
    v.log[:5] = torch.tensor([1, 1, 2, 4, _bits(-0.3)], dtype=torch.int32)
    e = L["evidence"].evidence
    e.hist[:] = rnd(S, e.P * H)
    e.sring[:] = rnd(S, e.P)
    e.rec[:] = -1
    e.rec[1] = 0                                          # slot 1 is recording into pool entry 0
    e.left[1] = 3
    e._pool[0] = torch.tensor([RECORDING, 1, 4, 1, 4, 0], dtype=torch.int32)
    gt = L["gate"]
    gt.nf[:] = torch.tensor(pick([1e-3, INF, 2.5e-4, INF]))
    gt.h[:] = torch.tensor(pick([3, 0, 20, 0]), dtype=torch.int32)
    gt.ring[:] = rnd(S, 2 * H)
    gt._fill[:] = pick([480, 0, 160, 0])
    gt._head[:] = pick([100, 0, 7900, 0])                 # (7900: the pending samples wrap)
    gt._seen[:] = (np.array(inner_hops) + 1) * H          # one more hop pushed than the inner session has seen
    f = L["front"]
    f.ring[:] = rnd(S, 5 * H)
    f.hist[:] = rnd(S, f.hist.shape[1])
    f._fill[:] = pick([100, 0, 4100, 2])
    f._head[:] = pick([19990, 0, 5, 0])
    f._in[:] = (gt._seen + f._fill) // 2                  # 8 kHz in, 16 kHz out: two samples made per sample taken


def _snap(front):
    L = _layers(front)
    c, q, v, e, g, f = L["cascade"], L["quality"].quality, L["verdict"].verdicts, L["evidence"].evidence, L["gate"], L["front"]
    p = L["provenance"].provenance
    parts = [L["base"].ring, L["base"]._seen, c.wait, c.verified, c.verified_at, q.ring, q.st, q.totals, p.ring, p.st, p.totals,
             v.m, v.st, v.log,
             e.hist, e.sring, e.rec, e.left, e._pool, g.nf, g.h, g.ring, g._fill, g._head, g._seen, f.ring, f.hist, f._fill, f._head, f._in]
    return [torch.as_tensor(p).clone() for p in parts]


def _same(a, b):
    """Equal dtype, shape and content, NaN equal to NaN (floats by their bits)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _through_a_file(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


# ---- 2. the frozen layout ------------------------------------------------------------------------------------------------------
META = ["arch", "build_id", "cascade", "cascade_policy", "cascade_verifier", "dtype", "evidence", "evidence_pre", "extractor_mode",
        "fingerprint", "format", "gate", "gate_params", "head", "hop", "ingest", "input_rate", "kind", "n_layers", "provenance",
        "provenance_window", "quality", "quality_window", "resampler", "verdict", "verdict_policy", "window"]
f32, i64, i32, u8 = torch.float32, torch.int64, torch.int32, torch.uint8
COMMON = {"cascade_verified": (f32, (2,)), "cascade_verified_at": (i64, (2,)), "cascade_wait": (i64, (2,)),
          "evidence_hist": (f32, (2, 16000)), "evidence_scores": (f32, (2, 4)), "gate_fill": (i64, (2,)), "gate_hang": (i64, (2,)),
          "gate_inner_seen": (i64, (2,)), "gate_nf": (f32, (2,)), "gate_pending": (f32, (2, 4000)), "prov_ring": (i32, (2, 4)),
          "prov_state": (i64, (2, 2)), "prov_totals": (i64, (2, 3)), "quality_ring": (u8, (2, 4)),
          "quality_state": (i64, (2, 3)), "quality_totals": (i64, (2, 6)), "samples": (f32, (2, 16000)), "verdict_m": (f32, (2,)),
          "verdict_state": (i64, (2, 4))}
LAYOUT = {
    "packet": (META, dict(COMMON, ingest_fill=(i64, (2,)), ingest_in=(i64, (2,)), ingest_pending=(f32, (2, 16000)),
                          resample_hist=(f32, (2, 20)))),
    "jitter": (sorted(set(META) - {"ingest"} | {"jitter", "jitter_conceal", "jitter_depth", "jitter_fade", "jitter_period"}),
               dict(COMMON, gate_syn=(i64, (2, 25)), jitter_syn=(u8, (2, 16000)), jitter_book=(i64, (2, 8)), jitter_fill=(i64, (2,)), jitter_intervals=(i64, (2, 1, 2)),
                    jitter_pending=(f32, (2, 16000)), jitter_ring=(f32, (2, 324)), jitter_stats=(i64, (2, 5)))),
}


@pytest.mark.parametrize("front", ["packet", "jitter"])
def test_the_layout_of_a_full_chains_state_is_frozen_and_survives_a_file(built, front):
    st = _chain(3, front).export_slots([2, 0])
    meta, tensors = LAYOUT[front]
    assert sorted(st.meta) == meta
    assert {k: (t.dtype, tuple(t.shape)) for k, t in st.tensors.items()} == tensors
    assert (st.meta["format"], st.meta["cascade"], st.meta["quality"], st.meta["verdict"], st.meta["evidence"], st.meta["gate"]) == (1,) * 6
    assert st.meta["provenance"] == 1
    b = _chain(4, front)
    b.import_slots([1, 3], _through_a_file(st))
    back = b.export_slots([1, 3])
    assert back.meta == st.meta and set(back.tensors) == set(st.tensors) and torch.equal(back.seen, st.seen)
    assert all(_same(back.tensors[k], st.tensors[k]) for k in st.tensors)


# ---- 3. a refusal at any depth leaves every layer unchanged ------------------------------------------------------------------
def test_a_refusal_at_any_depth_leaves_every_layer_unchanged(built):
    from afx.streaming import StreamState
    a, b = _chain(3, "packet", COOLDOWN, CONFIRM), _chain(4, "packet", COOLDOWN, CONFIRM)
    _dirty(a, 1)
    _dirty(b, 2, roll=1)
    good = _through_a_file(a.export_slots([2, 0]))
    m, t = good.meta, good.tensors
    W = m["quality_window"]["W"]
    with_t = lambda **kw: StreamState(m, good.seen, dict(t, **kw))  # noqa: E731
    with_m = lambda **kw: StreamState(dict(m, **kw), good.seen, t)  # noqa: E731
    without = lambda k: StreamState(m, good.seen, {n: v for n, v in t.items() if n != k})  # noqa: E731
    bad_quality, bad_verdict = t["quality_state"].clone(), t["verdict_state"].clone()
    bad_quality[0, 2], bad_verdict[1, 2] = W + 1, 2
    bad_prov = t["prov_state"].clone()
    bad_prov[0, 0] += 1  # a total that is not the ring's sum
    spoiled = {
        "cascade_wait": with_t(cascade_wait=torch.tensor([COOLDOWN + 1, 0])),
        "quality_state": with_t(quality_state=bad_quality),
        "prov_state": with_t(prov_state=bad_prov),
        "verdict_state": with_t(verdict_state=bad_verdict),
        "evidence_hist": with_t(evidence_hist=t["evidence_hist"][:, :-1]),
        "gate_fill": with_t(gate_fill=torch.tensor([H, 0])),
        "ingest_fill": with_t(ingest_fill=torch.tensor([-1, 100])),
        "meta cascade_policy": with_m(cascade_policy=dict(m["cascade_policy"], budget=1)),
        "meta quality_window": with_m(quality_window=dict(W=W + 1, hop=H)),
        "meta provenance_window": with_m(provenance_window=dict(W=W + 1, hop=H)),
        "meta verdict_policy": with_m(verdict_policy=dict(m["verdict_policy"], release=3)),
        "meta evidence_pre": with_m(evidence_pre=m["evidence_pre"] - 1),
        "meta gate_params": with_m(gate_params=dict(m["gate_params"], hang=19)),
        "meta input_rate": with_m(input_rate=16000),
        "no cascade_verified": without("cascade_verified"),
        "no quality_totals": without("quality_totals"),
        "no prov_totals": without("prov_totals"),
        "no verdict_m": without("verdict_m"),
        "no evidence_scores": without("evidence_scores"),
        "no gate_nf": without("gate_nf"),
        "no ingest_in": without("ingest_in"),
        "meta window": with_m(window=2 * WINDOW),
    }
    before, others = _snap(b), b.export_slots([0, 2])
    for name, state in spoiled.items():
        with pytest.raises(ValueError):
            b.import_slots([3, 1], state)
        assert all(_same(u, v) for u, v in zip(before, _snap(b))), name
    for slots in ([3], [3, 1, 0]):  # a session count that does not match
        with pytest.raises(ValueError):
            b.import_slots(slots, good)
        assert all(_same(u, v) for u, v in zip(before, _snap(b))), slots
    b.import_slots([3, 1], good)
    back = b.export_slots([3, 1])
    assert back.meta == m and torch.equal(back.seen, good.seen) and all(_same(back.tensors[k], t[k]) for k in t)
    assert not all(_same(u, v) for u, v in zip(before, _snap(b)))
    # the slots not named keep their sessions
    after = b.export_slots([0, 2])
    assert torch.equal(after.seen, others.seen) and all(_same(after.tensors[k], others.tensors[k]) for k in others.tensors)
    # every layer took its rows: spot checks below the export
    L, A = _layers(b), _layers(a)
    assert L["cascade"].wait[[3, 1]].tolist() == A["cascade"].wait[[2, 0]].tolist()
    assert L["quality"].quality.st[[3, 1]].tolist() == A["quality"].quality.st[[2, 0]].tolist()
    assert L["provenance"].provenance.st[[3, 1]].tolist() == A["provenance"].provenance.st[[2, 0]].tolist()
    assert L["verdict"].verdicts.st[[3, 1]].tolist() == A["verdict"].verdicts.st[[2, 0]].tolist()
    assert L["gate"]._seen[[3, 1]].tolist() == A["gate"]._seen[[2, 0]].tolist() and L["base"]._seen[[3, 1]].tolist() == A["base"]._seen[[2, 0]].tolist()
    assert L["front"]._fill[[3, 1]].tolist() == A["front"]._fill[[2, 0]].tolist() and L["front"]._head[[3, 1]].tolist() == [0, 0]


# ---- 4. every tensor of the per-slot tables is held to its dtype and shape before anything changes ---------------------------
TABLE_FIELDS = ["quality_ring", "quality_state", "quality_totals", "prov_ring", "prov_state", "prov_totals", "verdict_m", "verdict_state",
                "evidence_hist", "evidence_scores"]  # (the cascade's part is checked by the cascade itself)


@pytest.fixture(scope="module")
def a_good_state(built):
    """(a chain of 4 slots in use, its snapshot, a good state of two sessions of another chain): a refusal leaves the chain as
    it was, so every case shares it."""
    a, b = _chain(4, "packet", COOLDOWN, CONFIRM), _chain(4, "packet", COOLDOWN, CONFIRM)
    _dirty(a, 3)
    _dirty(b, 4, roll=1)
    return b, _snap(b), _through_a_file(a.export_slots([2, 0]))


def _spoil(t, how):
    if how == "dtype":
        return t.to({f32: torch.float64, i64: i32, i32: i64, u8: torch.int16}[t.dtype])
    if how == "shape":
        return t[:, :-1] if t.ndim > 1 else t[:, None]
    return t[:1]  # one row for two sessions


@pytest.mark.parametrize("how", ["dtype", "shape", "rows"])
@pytest.mark.parametrize("key", TABLE_FIELDS)
def test_a_table_tensor_of_another_dtype_shape_or_row_count_is_refused_and_changes_nothing(a_good_state, key, how):
    from afx.streaming import StreamState
    b, before, good = a_good_state
    state = StreamState(good.meta, good.seen, good.tensors)
    state.tensors[key] = _spoil(good.tensors[key], how)  # (behind the constructor's back: it counts the rows itself)
    with pytest.raises(ValueError, match="tensor '" + key + "' has 1 rows" if how == "rows" else "import_slots: " + key + " "):
        b.import_slots([3, 1], state)
    assert all(_same(u, v) for u, v in zip(before, _snap(b)))

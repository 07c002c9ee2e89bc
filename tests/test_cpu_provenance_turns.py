"""Provenance through onset pre-roll and through turns, without a GPU (afx/provenance.py, ``ProvenancePolicy(through="all")``):
the policy's new attribute, what a jitter front attaches with it and what it leaves alone without it, ``clip_count`` against
``np.resize``, the session moves of an attached look-ahead gate (``gate_syn_line``) and of an attached ``TurnScorer``
(``turn_syn``) with their refusals, and the three new entry points' refusals by name."""
import ctypes

import numpy as np
import pytest
import torch

import packet_helpers
from packet_helpers import inner as _inner

H, WINDOW, FRAME, PRE = 4000, 16000, 160, 31
MAXF = WINDOW // FRAME


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def _all(**kw):
    from afx.provenance import ProvenancePolicy
    return ProvenancePolicy(through="all", **kw)


def _layer(S=2, policy=None, hop=H):
    from afx.provenance import ProvenanceScorer
    from afx.streaming import SlidingWindowScorer
    return ProvenanceScorer(SlidingWindowScorer(None, S, window=WINDOW, hop=hop, device="cpu"), _all() if policy is None else policy)


def _fronts():
    from afx.jitter import JitterScorer, MixedJitterScorer
    return (lambda s: JitterScorer(s, 8000, "mulaw", 4), lambda s: MixedJitterScorer(s, [(8000, "mulaw"), (48000, "pcm_s16le")], 60))


# ---- 1. the policy ---------------------------------------------------------------------------------------------------------
def test_through_is_plain_or_all_and_no_part_of_params():
    from afx.provenance import ProvenancePolicy
    assert ProvenancePolicy().through == "plain" and ProvenancePolicy(through="plain").through == "plain"
    p = ProvenancePolicy(0.1, False, through="all")
    assert p.through == "all" and p.params() == dict(max_share=float(np.float32(0.1)), abstain=False)
    assert ProvenancePolicy(0.1, False).params() == p.params() and p.limit(1, WINDOW) == ProvenancePolicy(0.1).limit(1, WINDOW)
    for bad in ("ALL", "", "turns", None, True, 1, b"all", ("all",)):
        with pytest.raises(ValueError, match="through"):
            ProvenancePolicy(through=bad)


@pytest.mark.parametrize("m", range(1, 13))
def test_clip_count_is_the_sum_of_the_tiled_turn(m):
    from afx.provenance import clip_count
    g = np.random.default_rng(m)
    for _ in range(5):
        n = g.integers(0, FRAME + 1, m)
        assert clip_count(n, 12) == int(np.resize(n, 12).sum())
    assert clip_count(np.full(m, FRAME), 12) == 12 * FRAME
    for bad in (([], 12), (np.zeros(13, dtype=np.int64), 12), ([0.5], 12), ([True], 12), ([1], 0)):
        with pytest.raises(ValueError):
            clip_count(*bad)


# ---- 2. discovery ----------------------------------------------------------------------------------------------------------
def test_discovery_with_all_attaches_a_lookahead_gate_and_a_turn_scorer():
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import GatedScorer, LookaheadGate
    from afx.verdict import VerdictPolicy, VerdictScorer
    for front in _fronts():
        g = GatedScorer(VerdictScorer(_layer(), VerdictPolicy(0.0, 0.5)), LookaheadGate(pre=7))
        assert not g._syn and not hasattr(g, "gline") and not hasattr(g, "gsyn")
        js = front(g)
        assert js._prov == (g, FRAME, True) and g._syn and g._syn_below is g.scorer.scorer
        assert g.gline.shape == (2, 7) and g.gline.dtype == torch.int32 and g.gsyn.shape == (2, 2 * H // FRAME) and g.gsyn.dtype == torch.int32
        assert js.psyn.shape == (2, js.ring_len)
        t = TurnScorer(_layer(hop=WINDOW), None, TurnPolicy(25), hop=H)
        assert not t._syn and not hasattr(t, "bsyn")
        js = front(t)
        assert js._prov == (t, FRAME, True) and t._syn and t._syn_below is t.scorer
        assert t.bsyn.shape == (2, 2, MAXF) and t.bsyn.dtype == torch.int32
        with pytest.raises(ValueError, match="at most 512"):  # the limit of 512 frames a push holds for both
            front(GatedScorer(_layer(hop=513 * 16), LookaheadGate(frame=16)))
    with pytest.raises(ValueError, match="not attached"):
        TurnScorer(_layer(hop=WINDOW), None, TurnPolicy(25), hop=H).note_synthetic(torch.zeros(2, 25, dtype=torch.int32), None)


def test_without_the_layer_or_with_a_plain_policy_nothing_new_appears():
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.streaming import SlidingWindowScorer
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import GatedScorer, LookaheadGate
    clip = lambda: SlidingWindowScorer(None, 2, window=WINDOW, hop=WINDOW, device="cpu")  # noqa: E731
    new = {"gate_syn_line", "turn_syn"}
    for front in _fronts():
        for g in (GatedScorer(_inner(2), LookaheadGate()), TurnScorer(clip(), None, TurnPolicy(25), hop=H), GatedScorer(_inner(2))):
            js = front(g)
            assert js._prov is None and not g._syn and not any(hasattr(g, a) for a in ("gline", "bsyn", "gsyn"))
            assert not ({"gate_syn", "jitter_syn"} | new) & set(js.export_slots([0, 1]).tensors)
        for policy in (ProvenancePolicy(), _all()):  # a plain gate over the layer: attached as ever, under either value
            g = GatedScorer(ProvenanceScorer(_inner(2), policy))
            js = front(g)
            assert g._syn and hasattr(g, "gsyn") and not hasattr(g, "gline") and not hasattr(g, "bsyn")
            assert "gate_syn" in js.export_slots([0, 1]).tensors and not new & set(js.export_slots([0, 1]).tensors)
        for g in (GatedScorer(ProvenanceScorer(_inner(2)), LookaheadGate()), TurnScorer(ProvenanceScorer(clip()), None, TurnPolicy(25), hop=H)):
            with pytest.raises(ValueError, match="out of scope"):  # the default policy: today's refusals
                front(g)
            assert not g._syn


# ---- 3. sessions -----------------------------------------------------------------------------------------------------------
def _la_gate(S=3, attach=True, layer=True):
    from afx.jitter import JitterScorer
    from afx.vad import GatedScorer, LookaheadGate
    g = GatedScorer(_layer(S) if layer else _inner(S), LookaheadGate(pre=PRE))
    if attach:
        JitterScorer(g, 16000, "pcm_s16le", 4, conceal="zero")
    return g


def _dirty_gate(g, seed):
    """Slot s has seen 1 + s hops: slot 0 holds 25 < pre delayed frames and nothing pending, the others a full line."""
    gen = torch.Generator().manual_seed(seed)
    per = H // FRAME
    for s in range(g.S):
        g.scorer.scorer._seen[s] = s * H
        g._seen[s], g._fill[s], g._head[s] = (1 + s) * H, FRAME * (2 + s) * (s > 0), H * (s % 2)
        for j in range(int(g._fill[s]) // FRAME):
            g.src[s, (int(g._head[s]) // FRAME + j) % (2 * per)] = 3 * j + s
    g.ring[:] = torch.randn(g.S, g.ring_len, generator=gen)
    g.line[:] = torch.randn(g.S, PRE * FRAME, generator=gen)
    g.flags[:] = torch.tensor([0b101] + [0x5a5a5a5a & ((1 << PRE) - 1)] * (g.S - 1), dtype=torch.int32)
    g.gsyn[:] = torch.randint(0, FRAME + 1, g.gsyn.shape, generator=gen).to(torch.int32)
    g.gline[:] = torch.randint(1, FRAME + 1, g.gline.shape, generator=gen).to(torch.int32)
    p = g.scorer.provenance
    for s in range(g.S):
        p.totals[s] = torch.tensor([s, 0, 0], dtype=torch.int32)


def _equal_states(a, b):
    assert a.meta == b.meta and torch.equal(a.seen, b.seen) and sorted(a.tensors) == sorted(b.tensors)
    for k in a.tensors:
        assert a.tensors[k].dtype == b.tensors[k].dtype and torch.equal(a.tensors[k], b.tensors[k]), k


def _broken(st, key, fn):
    from afx._layer import StreamState
    t = {k: v.clone() for k, v in st.tensors.items()}
    fn(t[key])
    return StreamState(st.meta, st.seen, t)


def _without(st, *keys):
    from afx._layer import StreamState
    return StreamState(st.meta, st.seen, {k: v for k, v in st.tensors.items() if k not in keys})


def _at(*idx, v):
    def fn(x):
        x[idx] = v
    return fn


def test_a_lookahead_gates_session_round_trip_and_refusals():
    from afx._layer import StreamState
    A, B = _la_gate(), _la_gate()
    _dirty_gate(A, 1)
    st = A.export_slots([2, 0, 1])
    ln = st.tensors["gate_syn_line"]
    assert ln.dtype == torch.int64 and ln.shape == (3, PRE) and "gate_syn" in st.tensors
    # slot 0 (row 1): F = 25 frames seen, all delayed, at the blocks 0..24; six zeros in front
    assert ln[1, :PRE - 25].tolist() == [0] * (PRE - 25) and ln[1, PRE - 25:].tolist() == A.gline[0, :25].tolist()
    F2 = 3 * H // FRAME  # slot 2 (row 0): exported block c is frame F - pre + c, at block (F + c) mod pre
    assert ln[0].tolist() == [int(A.gline[2, (F2 + c) % PRE]) for c in range(PRE)] and int(ln.min()) == 0 < int(ln[0].min())
    st = StreamState.from_state_dict(st.state_dict())
    B.gline[:] = 77
    B.import_slots([1, 2, 0], st)
    _equal_states(B.export_slots([1, 2, 0]), st)
    assert B.gline[2, 25:].tolist() == [0] * (PRE - 25)  # (slot 0's session: the blocks it has not reached are cleared)
    C = _la_gate()  # a state without the counts imports with zeros; a slot that is not named keeps what it has
    C.gline[:], C.gsyn[:] = 9, 9
    C.import_slots([0, 1], _without(A.export_slots([1, 2]), "gate_syn", "gate_syn_line"))
    again = C.export_slots([0, 1]).tensors
    assert int(again["gate_syn_line"].abs().sum()) == 0 and int(again["gate_syn"].max()) == 0
    assert (C.gline[:2] == 0).all() and (C.gline[2] == 9).all()
    for key, fn in (("gate_syn_line", _at(0, 3, v=FRAME + 1)), ("gate_syn_line", _at(0, 30, v=-1)),  # outside 0..frame
                    ("gate_syn_line", _at(1, 0, v=1)), ("gate_syn_line", _at(1, 5, v=FRAME))):       # in front of the delayed frames
        D = _la_gate()
        before = [t.clone() for t in (D.gline, D.gsyn, D.line, D.flags, D.src, D.ring)]
        with pytest.raises(ValueError, match="gate_syn_line"):
            D.import_slots([0, 1, 2], _broken(st, key, fn))
        assert all(torch.equal(a, b) for a, b in zip(before, (D.gline, D.gsyn, D.line, D.flags, D.src, D.ring))) and not D._seen.any()
    for bad in (st.tensors["gate_syn_line"].to(torch.int32), st.tensors["gate_syn_line"][:, :PRE - 1]):
        with pytest.raises(ValueError, match="gate_syn_line"):
            _la_gate().import_slots([0, 1, 2], StreamState(st.meta, st.seen, dict(st.tensors, gate_syn_line=bad)))
    # a gate that is not attached refuses the new key (and the old one), with the layer below it or without
    with pytest.raises(ValueError, match=r"gate_syn_line\) and this chain has no provenance layer"):
        _la_gate(attach=False).import_slots([0, 1, 2], _without(st, "gate_syn"))
    with pytest.raises(ValueError, match="no provenance layer"):
        _la_gate(attach=False, layer=False).import_slots([0, 1, 2], st)
    old = _la_gate(attach=False).export_slots([0, 1, 2])
    assert not {"gate_syn", "gate_syn_line"} & set(old.tensors)
    E = _la_gate()
    E.import_slots([0, 1, 2], old)  # the old format imports into an attached gate
    assert int(E.export_slots([0, 1, 2]).tensors["gate_syn_line"].abs().sum()) == 0


def _turns(S=3, attach=True):
    from afx.jitter import JitterScorer
    from afx.turns import TurnPolicy, TurnScorer
    t = TurnScorer(_layer(S, hop=WINDOW), None, TurnPolicy(25), hop=H)
    if attach:
        JitterScorer(t, 16000, "pcm_s16le", 4, conceal="zero")
    return t


def _dirty_turns(t, seed):
    """Slot s has seen 3 + s hops and scored s turns; its open turn has 4 s frames (slot 0: none) in buffer s mod 2."""
    gen = torch.Generator().manual_seed(seed)
    t.bufs[:] = torch.randn(t.bufs.shape, generator=gen)
    t.bsyn[:] = torch.randint(1, FRAME + 1, t.bsyn.shape, generator=gen).to(torch.int32)
    for s in range(t.S):
        t.scorer.scorer._seen[s] = s * WINDOW
        t._seen[s] = (3 + s) * H
        n = 4 * s
        t.turn_state[s] = torch.tensor([s % 2, n, (3 + s) * 25 - n - 1 if n else 0], dtype=torch.int32)
        t._totals[s] = torch.tensor([s, 1, 0, 30 + s], dtype=torch.int32)
        t.scorer.provenance.totals[s] = torch.tensor([s, 0, 0], dtype=torch.int32)


def test_a_turn_scorers_session_round_trip_and_refusals():
    from afx._layer import StreamState
    A, B = _turns(), _turns()
    _dirty_turns(A, 2)
    st = A.export_slots([2, 0, 1])
    syn = st.tensors["turn_syn"]
    assert syn.dtype == torch.int64 and syn.shape == (3, MAXF)
    assert syn[0, :8].tolist() == A.bsyn[2, 0, :8].tolist() and (syn[0, 8:] == -1).all()   # slot 2: 8 frames, open = 0
    assert syn[2, :4].tolist() == A.bsyn[1, 1, :4].tolist() and (syn[2, 4:] == -1).all()   # slot 1: 4 frames, open = 1
    assert (syn[1] == -1).all() and int(syn[0, :8].min()) > 0
    st = StreamState.from_state_dict(st.state_dict())
    B.bsyn[:] = 77
    B.import_slots([1, 2, 0], st)
    _equal_states(B.export_slots([1, 2, 0]), st)
    assert B.turn_state[:, 0].tolist() == [0, 0, 0] and B.bsyn[1, 0, :8].tolist() == A.bsyn[2, 0, :8].tolist()  # it lands in buffer 0
    assert B.bsyn[0, 0, :4].tolist() == A.bsyn[1, 1, :4].tolist()
    C = _turns()  # a state without the counts imports with zeros; a slot that is not named keeps what it has
    C.bsyn[:] = 9
    C.import_slots([0, 1], _without(A.export_slots([1, 2]), "turn_syn"))
    again = C.export_slots([0, 1]).tensors["turn_syn"]
    assert again[0, :4].tolist() == [0] * 4 and again[1, :8].tolist() == [0] * 8 and (C.bsyn[:2] == 0).all() and (C.bsyn[2] == 9).all()
    for key, fn in (("turn_syn", _at(0, 3, v=FRAME + 1)), ("turn_syn", _at(0, 0, v=-1)),      # outside 0..frame
                    ("turn_syn", _at(0, 8, v=0)), ("turn_syn", _at(1, 0, v=5)), ("turn_syn", _at(2, MAXF - 1, v=-2))):  # after the turn: -1
        D = _turns()
        before = [x.clone() for x in (D.bsyn, D.bufs, D.turn_state, D._totals)]
        with pytest.raises(ValueError, match="turn_syn"):
            D.import_slots([0, 1, 2], _broken(st, key, fn))
        assert all(torch.equal(a, b) for a, b in zip(before, (D.bsyn, D.bufs, D.turn_state, D._totals))) and not D._seen.any()
    for bad in (st.tensors["turn_syn"].to(torch.int32), st.tensors["turn_syn"][:, :MAXF - 1]):
        with pytest.raises(ValueError, match="turn_syn"):
            _turns().import_slots([0, 1, 2], StreamState(st.meta, st.seen, dict(st.tensors, turn_syn=bad)))
    with pytest.raises(ValueError, match=r"turn_syn\) and this chain has no provenance layer"):
        _turns(attach=False).import_slots([0, 1, 2], st)
    old = _turns(attach=False).export_slots([0, 1, 2])
    assert "turn_syn" not in old.tensors
    E = _turns()
    E.import_slots([0, 1, 2], old)  # the old format imports into an attached layer
    assert (E.export_slots([0, 1, 2]).tensors["turn_syn"] == -1).all()


def test_a_session_moves_between_layers_that_differ_in_through():
    """``through`` is no part of a session: a plain-gate chain's state moves between a "plain" and an "all" layer."""
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.vad import GatedScorer
    chain = lambda p: JitterScorer(GatedScorer(ProvenanceScorer(_inner(2), p)), 16000, "pcm_s16le", 4, conceal="zero")  # noqa: E731
    A, B = chain(ProvenancePolicy()), chain(_all())
    assert A.state_meta() == B.state_meta()
    st = A.export_slots([0, 1])
    B.import_slots([1, 0], st)
    _equal_states(B.export_slots([1, 0]), st)
    A.import_slots([0, 1], B.export_slots([0, 1]))


# ---- 4. the entry points ---------------------------------------------------------------------------------------------------
def test_the_new_entry_points_refuse_bad_scalars_by_name(built):
    l = built.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(afx_k_prov_compact_la=[p, p, p, 1, 4, 16, 3, p, p, 1, 8], afx_k_prov_turn=[p, p, p, 1, 4, 16, 4, 8, p, p, 1],
                afx_k_prov_turn_sum=[p, 1, 8, p, 1, p])
    bad = dict(afx_k_prov_compact_la=[(0, None), (1, None), (2, None), (7, None), (8, None), (3, 0), (3, 65536), (4, 0), (4, 513), (4, 9),
                                      (5, 0), (6, 0), (6, 32), (9, 0), (10, 3), (10, (1 << 30) + 1)],
               afx_k_prov_turn=[(0, None), (1, None), (2, None), (8, None), (9, None), (3, 0), (3, 65536), (4, 0), (4, 513), (5, 0),
                                (6, 3), (6, 9), (7, 1 << 27), (10, 0)],
               afx_k_prov_turn_sum=[(0, None), (3, None), (5, None), (1, 0), (2, 0), (4, 0), (4, 65535 * 4 + 1)])
    for name, args in good.items():
        who = name[len("afx_k_"):].encode()
        for i, v in bad[name]:
            a = list(args)
            a[i] = v
            assert getattr(l, name)(*a, None) != 0, (name, i, v)
            assert l.afx_last_error().startswith(who + b":"), (name, i, v, l.afx_last_error())

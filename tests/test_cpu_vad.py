"""The speech gate (afx/vad.py) without a GPU: parameter validation, the numpy restatement of the function (energy order,
chunking with carried state, hangover, non-finite frames, the floor's minimum, the keep runs of the 8-s fixture stream),
``GatedScorer``'s refusals on host-only scorers and every inconsistency ``import_slots`` refuses on hand-built states,
each leaving the scorer unchanged."""
import math

import numpy as np
import pytest
import torch

H = 4000


def fixture_stream():
    """8 s: noise at -54 dBFS, four talk spurts (0.8 s, 0.15 s, 2 s, 20 ms) of a 180 Hz tone with a 4 Hz tremolo, 0.5 s of zeros."""
    g = np.random.default_rng(0)
    x = (0.002 * g.standard_normal(128000)).astype(np.float32)
    t = np.arange(128000) / 16000
    for a, b in [(0.5, 1.3), (2.0, 2.15), (3.0, 5.0), (6.5, 6.52)]:
        m = (t >= a) & (t < b)
        x[m] += (0.2 * np.sin(2 * np.pi * 180 * t[m]) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t[m]))).astype(np.float32)
    x[112000:120000] = 0
    return x


def _runs(mask):
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def test_parameters_are_validated_and_identify_the_gate():
    from afx.vad import SpeechGate
    g = SpeechGate()
    assert g.params() == dict(floor=1e-6, ratio=8.0, rise=1.01, hang=20, frame=160)
    assert all(type(v) in (int, float) for v in g.params().values())
    assert g.E_floor.dtype == np.float32 and g.E_floor == np.float32(1e-6 * 160) and g.nf_min == np.float32(g.E_floor / np.float32(8.0))
    assert SpeechGate(**g.params()).params() == g.params() and SpeechGate(hang=0, rise=1, frame=1).params()["hang"] == 0
    for kw in (dict(floor=0.0), dict(floor=-1e-6), dict(floor=math.inf), dict(floor=math.nan), dict(floor="1e-6"),
               dict(ratio=1.0), dict(ratio=0.5), dict(ratio=math.inf), dict(ratio=math.nan),
               dict(rise=0.99), dict(rise=math.inf), dict(rise=math.nan), dict(rise=None),
               dict(hang=-1), dict(hang=2.5), dict(hang=True), dict(frame=0), dict(frame=-160), dict(frame=160.0)):
        with pytest.raises(ValueError):
            SpeechGate(**kw)


def _energy_scalar(x):
    """The stated order, one np.float32 operation at a time."""
    sq = [np.float32(v) * np.float32(v) for v in x]
    p = [None] * 64
    for l in range(64):
        for i in range(l, len(x), 64):
            p[l] = sq[i] if p[l] is None else np.float32(p[l] + sq[i])
    p = [np.float32(0) if v is None else v for v in p]
    w = 32
    while w:
        for l in range(w):
            p[l] = np.float32(p[l] + p[l + w])
        w //= 2
    return p[0]


@pytest.mark.parametrize("frame", [160, 200, 50, 64, 1])
def test_frame_energies_follow_the_stated_order(frame):
    from afx.vad import frame_energies
    x = np.random.default_rng(frame).standard_normal(6 * frame).astype(np.float32)
    got = frame_energies(x, frame)
    assert got.dtype == np.float32 and got.shape == (6,)
    for f in range(6):
        assert got[f].tobytes() == _energy_scalar(x[f * frame:(f + 1) * frame]).tobytes()
    exact = (x.astype(np.float64).reshape(6, frame) ** 2).sum(1)
    assert np.abs(got - exact).max() <= 8 * 2.0 ** -24 * exact.max()  # (at most 2 + 6 roundings deep, each half an ulp of a partial sum)


def test_chunked_at_random_frame_boundaries_equals_the_whole_stream():
    from afx.vad import SpeechGate
    x = fixture_stream()
    for gate in (SpeechGate(), SpeechGate(frame=200, hang=3, ratio=4.0)):
        mask, kept, st = gate.gate_reference(x)
        rng = np.random.default_rng(7)
        for trial in range(3):
            cuts = np.sort(rng.choice(np.arange(1, x.size // gate.frame), size=17, replace=False)) * gate.frame
            state, masks, parts = None, [], []
            for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [x.size]])):
                before = None if state is None else dict(state)
                m, k, state2 = gate.gate_reference(x[a:b], state)
                assert before is None or before == state  # (the state passed in is not modified)
                state = state2
                masks.append(m)
                parts.append(k)
            assert np.array_equal(np.concatenate(masks), mask)
            assert np.concatenate(parts).tobytes() == kept.tobytes()
            assert state["nf"].tobytes() == st["nf"].tobytes() and state["h"] == st["h"]
    with pytest.raises(ValueError):
        SpeechGate().gate_reference(x[:161])


@pytest.mark.parametrize("hang", [0, 1, 7, 20])
def test_hangover_keeps_exactly_hang_frames_and_no_pre_roll(hang):
    from afx.vad import SpeechGate
    gate = SpeechGate(hang=hang)
    g = np.random.default_rng(3)
    x = (0.002 * g.standard_normal(100 * 160)).astype(np.float32)
    x[30 * 160:42 * 160] += (0.2 * np.sin(2 * np.pi * 180 * np.arange(12 * 160) / 16000)).astype(np.float32)
    mask, kept, st = gate.gate_reference(x)
    assert _runs(mask) == [(30, 42 + hang)]
    assert kept.tobytes() == x[30 * 160:(42 + hang) * 160].tobytes()
    assert st["h"] == 0
    # cut inside the hangover: the state carries what is left of it
    cut = 42 + hang // 2
    _, _, mid = gate.gate_reference(x[:cut * 160])
    assert mid["h"] == hang - hang // 2


def test_a_non_finite_frame_is_not_speech_and_leaves_the_floor_alone():
    from afx.vad import SpeechGate
    gate = SpeechGate(hang=2)
    g = np.random.default_rng(4)
    quiet = (0.002 * g.standard_normal(10 * 160)).astype(np.float32)
    _, _, st = gate.gate_reference(quiet)
    for bad in (np.inf, -np.inf, np.nan, 1e30):  # (1e30 squared overflows fp32: the energy is inf)
        fr = quiet[:160].copy()
        fr[17] = bad
        mask, kept, after = gate.gate_reference(fr, st)
        assert mask.tolist() == [False] and kept.size == 0
        assert after["nf"].tobytes() == st["nf"].tobytes() and after["h"] == st["h"] == 0
    # inside a hangover it is kept like any frame, and counts against the hangover
    loud = (0.2 * np.sin(2 * np.pi * 180 * np.arange(160) / 16000)).astype(np.float32)
    _, _, sp = gate.gate_reference(loud, st)
    assert sp["h"] == 2
    fr = quiet[:160].copy()
    fr[0] = np.inf
    mask, kept, after = gate.gate_reference(fr, sp)
    assert mask.tolist() == [True] and after["h"] == 1 and after["nf"].tobytes() == sp["nf"].tobytes()
    assert kept.tobytes() == fr.tobytes()
    # a new stream that begins with one: the floor stays +inf
    _, _, first = gate.gate_reference(fr)
    assert np.isposinf(first["nf"]) and first["h"] == 0


def test_zeros_drive_the_floor_to_its_minimum_and_not_below():
    from afx.vad import SpeechGate
    gate = SpeechGate()
    _, _, st = gate.gate_reference(np.zeros(160, dtype=np.float32))
    assert st["nf"].tobytes() == gate.nf_min.tobytes()  # the first frame sets the floor
    g = np.random.default_rng(5)
    noise = (0.01 * g.standard_normal(20 * 160)).astype(np.float32)
    _, _, st = gate.gate_reference(noise)
    assert st["nf"] > gate.nf_min
    mask, _, st = gate.gate_reference(np.zeros(50 * 160, dtype=np.float32), st)
    assert not mask.any() and st["nf"].tobytes() == gate.nf_min.tobytes()
    # from the minimum the threshold is E_floor (ratio * nf_min <= E_floor up to one rounding): a frame just above it is speech
    amp = np.float32(math.sqrt(1.5e-6))
    mask, _, _ = gate.gate_reference(np.full(160, amp, dtype=np.float32), st)
    assert mask.tolist() == [True]
    mask, _, _ = gate.gate_reference(np.full(160, np.float32(math.sqrt(0.5e-6)), dtype=np.float32), st)
    assert mask.tolist() == [False]


def test_the_fixture_stream_gives_the_stated_keep_runs():
    from afx.vad import SpeechGate, frame_energies
    x = fixture_stream()
    mask, kept, st = SpeechGate().gate_reference(x)
    assert _runs(mask) == [(50, 150), (200, 235), (300, 520), (650, 672), (750, 800)]
    assert int(mask.sum()) == 427 and kept.size == 427 * 160 and kept.size // H == 17
    assert kept.tobytes() == x.reshape(800, 160)[mask].tobytes()
    nz = x[x != 0].astype(np.float64) ** 2
    assert nz.min() > np.finfo(np.float32).tiny  # no square is subnormal: a device that flushes them cannot differ
    # a stream that begins in the middle of speech is kept only from its first energy dip of `ratio` on
    start = 60 * 160
    m2, _, _ = SpeechGate().gate_reference(x[start:])
    e = frame_energies(x[start:], 160)
    first = int(np.flatnonzero(m2)[0])
    assert first > 0 and not m2[:first].any() and e[first] > 8 * e[:first].min() and (e[:first] > 100 * 160e-6).all()


# ---- GatedScorer on host-only scorers --------------------------------------------------------------------------------------
def _bare(S=2, hop=H, window=16000):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=window, hop=hop, device="cpu")


def test_gated_scorer_refuses_a_front_a_hop_off_the_grid_and_a_cpu_push(built):
    from afx._lib import AfxError
    from afx.ingest import PacketScorer
    from afx.streaming import ResamplingScorer
    from afx.vad import GatedScorer, SpeechGate
    for front in (ResamplingScorer(_bare(), 8000), PacketScorer(_bare(), 8000, "mulaw"), GatedScorer(_bare())):
        with pytest.raises(ValueError):
            GatedScorer(front)
    with pytest.raises(ValueError):
        GatedScorer(object())
    with pytest.raises(ValueError):
        GatedScorer(_bare(hop=4040))
    with pytest.raises(ValueError):
        GatedScorer(_bare(), SpeechGate(frame=300))
    with pytest.raises(ValueError):
        GatedScorer(_bare(), gate="default")
    GatedScorer(_bare(hop=4200), SpeechGate(frame=300))
    gs = GatedScorer(_bare(S=3))
    assert (gs.S, gs.hop, gs.window, gs.device.type) == (3, H, 16000, "cpu")
    assert gs._slot_list([2, 0], ordered=True) == [2, 0]
    with pytest.raises(AfxError):
        gs.push(torch.zeros(3, H))
    with pytest.raises(AfxError):
        gs.push(torch.zeros(1, H), [1])
    with pytest.raises(ValueError):
        gs.push(torch.zeros(1, H), [3])
    with pytest.raises(AfxError):
        SpeechGate().gate([torch.zeros(320)])
    for t in (gs.samples_seen, gs.samples_kept, gs.pending):
        assert t.dtype == torch.int64 and t.tolist() == [0, 0, 0]
    assert gs.emitted(torch.tensor([1.0, float("nan"), -2.0])).tolist() == [True, False, True]
    # the fronts accept it in place of a scorer
    ps = PacketScorer(gs, 8000, "mulaw")
    assert ps.state_meta()["gate"] == 1 and ps.state_meta()["gate_params"] == SpeechGate().params()


def _snapshot(gs):
    return [gs.ring.clone(), gs.nf.clone(), gs.h.clone(), gs._head.copy(), gs._fill.copy(), gs._seen.copy(),
            gs.scorer.ring.clone(), gs.scorer.samples_seen]


def _same(a, b):
    return all(torch.equal(torch.as_tensor(u), torch.as_tensor(v)) for u, v in zip(a, b))


def _valid_state(gs):
    """Two sessions as a GatedScorer would export them, hand-built: one mid-hangover with pending samples, one in silence."""
    from afx.streaming import StreamState
    st = gs.export_slots([0, 1])
    t = dict(st.tensors)
    g = torch.Generator().manual_seed(1)
    t["samples"] = torch.randn(2, gs.window, generator=g)
    t["gate_pending"] = torch.zeros(2, H)
    t["gate_pending"][0, :480] = torch.randn(480, generator=g)
    t["gate_fill"] = torch.tensor([480, 0])
    t["gate_hang"] = torch.tensor([5, 0])
    t["gate_inner_seen"] = torch.tensor([2 * H, 0])
    t["gate_nf"] = torch.tensor([3e-3, float("inf")])
    return StreamState(st.meta, torch.tensor([5 * H, 3 * H]), t)


def test_export_adds_the_gate_part_and_import_restores_it(built):
    from afx.streaming import StreamState
    from afx.vad import GATE_FORMAT, GatedScorer, SpeechGate
    gs = GatedScorer(_bare())
    st = gs.export_slots([1, 0])
    assert set(st.tensors) == {"samples", "gate_pending", "gate_fill", "gate_hang", "gate_inner_seen", "gate_nf"}
    assert tuple(st.tensors["gate_pending"].shape) == (2, H) and st.tensors["gate_pending"].dtype == torch.float32
    assert all(st.tensors[k].dtype == torch.int64 and st.tensors[k].tolist() == [0, 0] for k in ("gate_fill", "gate_hang", "gate_inner_seen"))
    assert st.tensors["gate_nf"].dtype == torch.float32 and torch.isposinf(st.tensors["gate_nf"]).all()
    assert st.meta["gate"] == GATE_FORMAT and st.meta["gate_params"] == SpeechGate().params() and gs.state_meta() == st.meta
    good = _valid_state(gs)
    dst = GatedScorer(_bare(S=4))
    dst.import_slots([3, 1], StreamState.from_state_dict(good.state_dict()))
    assert dst.samples_seen.tolist() == [0, 3 * H, 0, 5 * H] and dst.pending.tolist() == [0, 0, 0, 480]
    assert dst.samples_kept.tolist() == [0, 0, 0, 2 * H + 480] and dst.scorer.samples_seen.tolist() == [0, 0, 0, 2 * H]
    back = dst.export_slots([3, 1])
    assert torch.equal(back.seen, good.seen) and set(back.tensors) == set(good.tensors)
    for k in good.tensors:
        if k == "samples":  # (the inner scorer exports a session's own samples only: zeros past them)
            assert torch.equal(back.tensors[k][0, :2 * H], good.tensors[k][0, :2 * H]) and not back.tensors[k][1].any()
        else:
            assert torch.equal(back.tensors[k], good.tensors[k]), k
    dst.reset([3])
    assert dst.samples_seen.tolist() == [0, 3 * H, 0, 0] and dst.pending.tolist() == [0] * 4
    assert torch.isposinf(dst.nf[3]) and int(dst.h[3]) == 0 and dst.scorer.samples_seen.tolist() == [0] * 4


def test_import_refuses_every_inconsistency_with_nothing_changed(built):
    from afx.ingest import PacketScorer
    from afx.streaming import StreamState
    from afx.vad import GatedScorer, SpeechGate
    src = GatedScorer(_bare())
    good = _valid_state(src)
    dst = GatedScorer(_bare(S=3))
    dst.import_slots([2, 0], good)  # something to lose
    before = _snapshot(dst)

    def variant(seen=None, meta=None, drop=(), **tensors):
        t = {k: v for k, v in dict(good.tensors, **tensors).items() if k not in drop}
        return StreamState(dict(good.meta, **(meta or {})) if meta is not None else good.meta, good.seen if seen is None else seen, t)

    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)  # noqa: E731
    bad = {
        "no gate tensors": src.scorer.export_slots([0, 1]),
        "a gate tensor missing": variant(drop=("gate_nf",)),
        "no gate meta": StreamState({k: v for k, v in good.meta.items() if k != "gate"}, good.seen, good.tensors),
        "other params": variant(meta=dict(gate_params=SpeechGate(hang=19).params())),
        "another format": variant(meta=dict(gate=2)),
        "fill negative": variant(gate_fill=i64(-160, 0)),
        "fill a whole hop": variant(gate_fill=i64(H, 0)),
        "fill off the frame grid": variant(gate_fill=i64(481, 0)),
        "fill not int64": variant(gate_fill=torch.tensor([480, 0], dtype=torch.int32)),
        "kept more than pushed": variant(gate_inner_seen=i64(5 * H, 0)),
        "inner count off the hop grid": variant(gate_inner_seen=i64(2 * H + 160, 0)),
        "inner count negative": variant(gate_inner_seen=i64(-H, 0)),
        "seen off the hop grid": variant(seen=i64(5 * H + 160, 3 * H)),
        "hang negative": variant(gate_hang=i64(-1, 0)),
        "hang above the gate's": variant(gate_hang=i64(21, 0)),
        "nf NaN": variant(gate_nf=torch.tensor([float("nan"), float("inf")])),
        "nf below the minimum": variant(gate_nf=torch.tensor([1e-6, float("inf")])),
        "nf of another type": variant(gate_nf=torch.tensor([3e-3, 1.0], dtype=torch.float64)),
        "pending of another shape": variant(gate_pending=torch.zeros(2, 2 * H)),
        "not a state": good.tensors,
    }
    for what, st in bad.items():
        with pytest.raises(ValueError):
            dst.import_slots([2, 0], st)
        assert _same(before, _snapshot(dst)), what
    with pytest.raises(ValueError):
        dst.import_slots([1], good)  # two sessions for one slot
    with pytest.raises(ValueError):
        GatedScorer(_bare(S=3), SpeechGate(ratio=4.0)).import_slots([2, 0], good)
    assert _same(before, _snapshot(dst))
    # a bare scorer refuses a gated state (its tensor-key check), a front around a bare scorer too
    bare = _bare()
    seen0, ring0 = bare.samples_seen, bare.ring.clone()
    with pytest.raises(ValueError):
        bare.import_slots([0, 1], good)
    assert torch.equal(bare.samples_seen, seen0) and torch.equal(bare.ring, ring0)
    # through a front: the packet scorer's export / import carry the gate's part and its sample count
    ps = PacketScorer(GatedScorer(_bare()), 8000, "mulaw")
    ps.scorer.import_slots([0, 1], good)
    ps._in[:] = [5 * H // 2, 3 * H // 2]  # (hand-built like the rest: the 8 kHz samples that make the gate's 16 kHz counts)
    wrapped = ps.export_slots([0, 1])
    assert torch.equal(wrapped.seen, good.seen) and "gate_nf" in wrapped.tensors and "ingest_fill" in wrapped.tensors
    ps2 = PacketScorer(GatedScorer(_bare(S=3)), 8000, "alaw")
    ps2.import_slots([2, 1], wrapped)
    assert ps2.scorer.samples_seen.tolist() == [0, 3 * H, 5 * H] and ps2.scorer.pending.tolist() == [0, 0, 480]
    with pytest.raises(ValueError):
        PacketScorer(_bare(), 8000, "mulaw").import_slots([0, 1], wrapped)
    with pytest.raises(ValueError):
        ps2.import_slots([0, 1], PacketScorer(_bare(), 8000, "mulaw").export_slots([0, 1]))

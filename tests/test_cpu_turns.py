"""Talk spurts on the host (afx/turns.py, afx_k_turn / afx_k_turn_collect): the two numpy restatements against each other,
the at-most-one-turn-per-push property by exhaustion, the argument and stack-order refusals, the ABI, and the session part
of a ``TurnScorer`` built on the CPU.  Every comparison is exact.  No GPU."""
import ctypes
import io
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _stream(offset=0, n=128000):
    """The talk-spurt fixture of the gate tests: 0.8 s, 0.15 s, 2 s and 20 ms of "voice" over noise, then zeros."""
    g = np.random.default_rng(0)
    x = (0.002 * g.standard_normal(128000)).astype(f32)
    t = np.arange(128000) / 16000
    for a, b in [(0.5, 1.3), (2.0, 2.15), (3.0, 5.0), (6.5, 6.52)]:
        m = (t >= a) & (t < b)
        x[m] += (0.2 * np.sin(2 * np.pi * 180 * t[m]) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t[m]))).astype(f32)
    x[112000:120000] = 0
    return np.roll(x, -offset)[:n]


def _bare(S, window=16000, hop=None):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=window, hop=window if hop is None else hop, device="cpu")


# ---- 1. the two restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5, 25])
@pytest.mark.parametrize("gate_name", ["SpeechGate", "ToneGate"])
def test_step_reference_push_by_push_equals_turns_reference(built, F, gate_name):
    from afx import turns, vad
    gate, policy, top, frame = getattr(vad, gate_name)(), turns.TurnPolicy(25), 100, 160
    for offset in (0, 30057, 44000):
        x = _stream(offset)
        x = x[:x.size // (F * frame) * (F * frame)]
        want, totals, still_open = policy.turns_reference(x, gate, top)
        assert sum(t["scored"] and not t["cut"] for t in want) >= 1 and sum(t["cut"] for t in want) >= 1
        assert sum(not t["scored"] for t in want) >= 1
        keep, kept, _ = gate.gate_reference(x)
        kept = kept.reshape(-1, frame)
        state, bufs, got, r = policy.new_state(top), np.zeros((2, top, frame), dtype=f32), [], 0
        for p in range(keep.size // F):
            row = keep[p * F:(p + 1) * F]
            k = int(row.sum())
            state, done = policy.step_reference(state, row.astype(np.uint8), p * F, kept[r:r + k], bufs)
            r += k
            if done[1]:
                got.append((done[2], done[3], p, bufs[done[0], :done[1]].reshape(-1).copy()))
            assert 0 <= state["n"] < top and state["open"] in (0, 1)
        scored = [t for t in want if t["scored"]]
        assert [(a, b, p) for a, b, p, _ in got] == [(t["first"], t["end"], t["close"] // F) for t in scored]
        assert all(a[3].tobytes() == t["audio"].tobytes() for a, t in zip(got, scored))
        assert state["totals"] == totals
        assert (None if state["n"] == 0 else (state["g"], state["n"])) == still_open
        if still_open:
            assert bufs[state["open"], :state["n"]].tobytes() == x.reshape(-1, frame)[state["g"]:state["g"] + state["n"]].tobytes()
    clip = policy.clip_reference(np.arange(7, dtype=f32), 17)
    assert clip.tolist() == [float(k % 7) for k in range(17)]


def _closed_runs(bits, top):
    """(closed runs, open frames at the end) of a mask sequence, runs cut at ``top``, by a direct count."""
    closed, n = 0, 0
    for b in bits:
        if b:
            n += 1
            if n == top:
                closed, n = closed + 1, 0
        elif n:
            closed, n = closed + 1, 0
    return closed, n


@pytest.mark.parametrize("F,least,top", [(3, 3, 3), (3, 3, 5), (4, 4, 6), (4, 5, 9)])
def test_no_push_completes_two_turns_by_exhaustion(built, F, least, top):
    from afx.turns import TurnPolicy
    policy = TurnPolicy(least)
    for bits in itertools.product((0, 1), repeat=3 * F):
        state, closes = policy.new_state(top), 0
        for p in range(3):
            row = bits[p * F:(p + 1) * F]
            before = state["totals"][0]
            state, done = policy.step_reference(state, row, p * F)
            assert state["totals"][0] - before == (1 if done[1] else 0) <= 1, bits  # never two done in a push
            closes += bool(done[1])
        closed, n = _closed_runs(bits, top)
        scored, short, cut, kept = state["totals"]
        assert scored + short == closed and scored == closes and state["n"] == n and kept == sum(bits), bits
    # with min_frames < F two can occur: 1 1 0 1 1 closes two turns of two frames in one push of five
    state, _ = TurnPolicy(2).step_reference(TurnPolicy.new_state(4), (1, 1, 0, 1, 1, 0), 0)
    assert state["totals"][0] == 2


def test_a_skipped_row_and_saturating_totals(built):
    from afx.turns import TurnPolicy
    policy, top = TurnPolicy(2), (1 << 31) - 1
    state = dict(policy.new_state(4), totals=(top, top - 1, top, top - 1), n=1, g=3)
    for g0 in (-1, (1 << 31) - 2):
        after, done = policy.step_reference(state, (1, 0), g0)
        assert after == state and done == (-1, -1, -1, -1)
    after, done = policy.step_reference(state, (1, 0), 4)
    assert done == (0, 2, 3, 5) and after["totals"] == (top, top - 1, top, top) and after["open"] == 1
    after, _ = policy.step_reference(after, (1, 0), 6)
    assert after["totals"] == (top, top, top, top)


# ---- 2. arguments and the stack order --------------------------------------------------------------------------------------
def test_the_arguments_are_checked(built):
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import LookaheadGate, SpeechGate, ToneGate
    ts = TurnScorer(_bare(2, 64000))
    assert (ts.layer, ts.hop, ts.window, ts.F, ts.min_frames, ts.max_frames) == ("gate", 4000, 64000, 25, 50, 400)
    assert ts.bufs.shape == (2, 2, 64000) and ts.staging.shape == (2, 4000) and ts.samples_seen.tolist() == [0, 0]
    assert TurnScorer(_bare(1), ToneGate(), TurnPolicy(25)).tone_frames.tolist() == [0] and ts.tone_frames is None
    for bad in (0, -1, 2.0, True, None, "50"):
        with pytest.raises(ValueError):
            TurnPolicy(bad)
    with pytest.raises(ValueError, match="min_frames"):
        TurnScorer(_bare(2), policy=TurnPolicy(24))  # min_frames < F: a push could complete two turns
    with pytest.raises(ValueError, match="min_frames"):
        TurnScorer(_bare(2), policy=TurnPolicy(101))  # min_frames > max_frames
    TurnScorer(_bare(2), policy=TurnPolicy(100))
    with pytest.raises(ValueError, match="hop == window"):
        TurnScorer(_bare(2, 16000, 4000), policy=TurnPolicy(25))
    with pytest.raises(ValueError, match="LookaheadGate"):
        TurnScorer(_bare(2), LookaheadGate(), TurnPolicy(25))
    with pytest.raises(ValueError):
        TurnScorer(_bare(2), "speech", TurnPolicy(25))
    with pytest.raises(ValueError):
        TurnScorer(_bare(2), None, 25)
    for hop in (4001, 0, 160 * 513, 4000.0):  # off the frame grid, no frame, more than 512 frames, not an integer
        with pytest.raises(ValueError):
            TurnScorer(_bare(2, 160 * 600), policy=TurnPolicy(513), hop=hop)
    with pytest.raises(ValueError):
        TurnScorer(_bare(2, 16100), policy=TurnPolicy(25))  # a window that is not whole frames
    with pytest.raises(ValueError):
        TurnScorer(_bare(2, 16000), SpeechGate(frame=200), TurnPolicy(25), hop=4100)
    with pytest.raises(ValueError):
        TurnPolicy(25).turns_reference(np.zeros(1600, dtype=f32), LookaheadGate(), 100)


def test_the_stack_order(built):
    from afx.ingest import PacketScorer
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    policy = TurnPolicy(25)
    ts = TurnScorer(_bare(2), policy=policy)
    with pytest.raises(ValueError, match="stack order"):
        GatedScorer(ts)
    with pytest.raises(ValueError, match="stack order"):
        TurnScorer(ts, policy=policy)
    with pytest.raises(ValueError, match="stack order"):
        TurnScorer(GatedScorer(_bare(2)), policy=policy)
    with pytest.raises(ValueError, match="stack order"):
        TurnScorer(PacketScorer(_bare(2), 8000, "mulaw"), policy=policy)
    inside = TurnScorer(VerdictScorer(_bare(2), VerdictPolicy(0.0)), policy=policy)  # around anything before "gate"
    front = PacketScorer(inside, 8000, "mulaw")  # and inside the fronts, which drive it by its own hop
    assert inside.hop == 4000 and inside.window == 16000 and front.scorer is inside


# ---- 3. the ABI -------------------------------------------------------------------------------------------------------------------
def test_the_abi_has_both_kernels(built):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afx.h")).read(), flags=re.S)
    so = ctypes.CDLL(built.LIB_PATH)
    for name, args in (("afx_k_turn", 15), ("afx_k_turn_collect", 8)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(so, name) and name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == args


# ---- 4. sessions, on the CPU ---------------------------------------------------------------------------------------------------
def _scorer(S, gate=None, seed=None):
    """A TurnScorer on the CPU; seed: slots in the middle of a call, set by hand (no kernel runs without a GPU)."""
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import ToneGate
    ts = TurnScorer(_bare(S), gate, TurnPolicy(25))
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        ts.bufs.copy_(torch.randn(ts.bufs.shape, generator=g))
        ts.scorer.ring.copy_(torch.randn(ts.scorer.ring.shape, generator=g))
        for s in range(S):
            ts._seen[s] = 4000 * (7 + s)
            ts.scorer._seen[s] = 16000 * (s % 2)
            ts.nf[s], ts.h[s] = 0.01 * (s + 1), s % 3
            n = [0, 37, 99][s % 3]
            ts.turn_state[s] = torch.tensor([s % 2, n, 25 * (7 + s) - n - (s % 2)], dtype=torch.int32)
            ts._totals[s] = torch.tensor([s % 2, s, 0, 50 + s], dtype=torch.int32)
            if isinstance(gate, ToneGate):
                ts.tone_state[s] = torch.tensor([s, gate.hold if s >= gate.confirm else 1, 5 + s], dtype=torch.int32)
    return ts


def _snap(ts):
    parts = [ts.scorer.ring, ts.scorer._seen, ts.nf, ts.h, ts.bufs, ts.turn_state, ts._totals, ts._seen, ts.staging]
    return [torch.as_tensor(p).clone() for p in parts + ([ts.tone_state] if ts._tone else [])]


def _same(a, b):
    return len(a) == len(b) and all(u.dtype == v.dtype and u.shape == v.shape and (
        torch.equal(u.view(torch.int32), v.view(torch.int32)) if u.dtype == torch.float32 else torch.equal(u, v)) for u, v in zip(a, b))


def _through_a_file(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


@pytest.mark.parametrize("gate_name", ["SpeechGate", "ToneGate"])
def test_a_turn_state_round_trips_and_every_bad_one_is_refused(built, gate_name):
    from afx import vad
    from afx.streaming import StreamState
    from afx.turns import TurnPolicy, TurnScorer
    gate = getattr(vad, gate_name)()
    a = _scorer(3, gate, seed=1)
    before = _snap(a)
    st = a.export_slots([2, 1])
    assert _same(before, _snap(a))  # no byte of the scorer changes
    assert st.seen.tolist() == [36000, 32000] and st.meta["turn"] == 1 and st.meta["turn_params"] == [4000, 25, 100]
    assert set(st.tensors) == {"samples", "gate_nf", "gate_hang", "gate_inner_seen", "turn_open", "turn_frames", "turn_first",
                               "turn_totals"} | ({"gate_tone"} if gate_name == "ToneGate" else set())
    assert st.tensors["turn_frames"].tolist() == [99, 37] and st.tensors["turn_first"].tolist() == [25 * 9 - 99, 25 * 8 - 38]
    assert st.tensors["turn_totals"].tolist() == [[0, 2, 0, 52], [1, 1, 0, 51]] and st.tensors["gate_inner_seen"].tolist() == [0, 16000]
    for i, (s, n) in enumerate(((2, 99), (1, 37))):
        row, src = st.tensors["turn_open"][i], a.bufs[s, int(a.turn_state[s, 0])]
        assert torch.equal(row[:n * 160].view(torch.int32), src[:n * 160].view(torch.int32)) and not row[n * 160:].any()
    idle = a.export_slots([0])
    assert idle.tensors["turn_frames"].tolist() == [0] and idle.tensors["turn_first"].tolist() == [-1] and not idle.tensors["turn_open"].any()

    b = _scorer(4, gate, seed=2)
    b.import_slots([0, 3], _through_a_file(st))
    again = b.export_slots([0, 3])
    assert again.meta == st.meta and again.seen.tolist() == st.seen.tolist()
    assert _same([again.tensors[k] for k in sorted(again.tensors)], [st.tensors[k] for k in sorted(st.tensors)])
    assert b.turn_state[[0, 3], 0].tolist() == [0, 0]  # an imported open turn lands in buffer 0
    untouched = _snap(_scorer(4, gate, seed=2))
    assert all(torch.equal(x[[1, 2]], y[[1, 2]]) for x, y in zip(_snap(b), untouched) if x.ndim and x.shape[0] == 4)

    def edited(**kw):
        t = {k: v.clone() for k, v in st.tensors.items()}
        seen = kw.pop("seen", st.seen.clone())
        for k, (i, v) in kw.items():
            t[k][i] = v
        return StreamState(st.meta, seen, t)

    loud = st.tensors["turn_open"].clone()
    loud[1, 37 * 160] = 1e-3
    bad = [edited(turn_frames=(0, 100)), edited(turn_frames=(0, -1)), edited(turn_first=(0, -1)), edited(turn_first=(1, 200)),
           edited(turn_frames=(1, 0)),  # (turn_first is then not -1, and samples stand after the open turn)
           StreamState(st.meta, st.seen, dict(st.tensors, turn_open=loud)),
           edited(turn_totals=((0, 2), -1)), edited(turn_totals=((1, 0), 1 << 31)), edited(gate_hang=(0, 21)),
           edited(gate_nf=(1, float("nan"))), edited(gate_nf=(0, 0.0)), edited(gate_inner_seen=(0, 4000)),
           edited(seen=torch.tensor([36000, 32001])), edited(seen=torch.tensor([-4000, 32000])),
           StreamState(st.meta, st.seen, dict(st.tensors, turn_open=st.tensors["turn_open"][:, :4000].contiguous())),
           StreamState(st.meta, st.seen, dict(st.tensors, turn_totals=st.tensors["turn_totals"].to(torch.int32))),
           StreamState(st.meta, st.seen, dict(st.tensors, turn_frames=st.tensors["turn_frames"].to(torch.int32))),
           StreamState(st.meta, st.seen, {k: v for k, v in st.tensors.items() if k != "turn_first"}),
           StreamState(dict(st.meta, turn=2), st.seen, st.tensors),
           StreamState(dict(st.meta, turn_params=[4000, 50, 100]), st.seen, st.tensors),
           StreamState(dict(st.meta, gate_params=dict(st.meta["gate_params"], hang=10)), st.seen, st.tensors)]
    if gate_name == "ToneGate":
        bad += [edited(gate_tone=((0, 1), 9)), edited(gate_tone=((1, 2), 10 ** 6))]
    fresh = _snap(b)
    for i, state in enumerate(bad):
        with pytest.raises(ValueError):
            b.import_slots([1, 2], state)
        assert _same(fresh, _snap(b)), i  # refused before anything changed, here or below
    with pytest.raises(ValueError):
        b.import_slots([1], st)  # two sessions for one slot
    # other parameters, the other gate, a gated state and a bare one: each refuses the other
    others = [TurnScorer(_bare(4), gate, TurnPolicy(50)), TurnScorer(_bare(4), gate, TurnPolicy(25), hop=1600),
              TurnScorer(_bare(4), vad.SpeechGate(hang=10), TurnPolicy(25)),
              TurnScorer(_bare(4), vad.ToneGate() if gate_name == "SpeechGate" else vad.SpeechGate(), TurnPolicy(25)),
              vad.GatedScorer(_bare(4, 16000, 4000), gate), vad.GatedScorer(_bare(4), gate), _bare(4)]
    for other in others:
        with pytest.raises(ValueError):
            other.import_slots([0, 1], st)
    gated = vad.GatedScorer(_bare(4), gate)
    for foreign in (gated.export_slots([0, 1]), _bare(4).export_slots([0, 1])):
        with pytest.raises(ValueError):
            b.import_slots([1, 2], foreign)
    assert _same(fresh, _snap(b))
    # the gated scorer's own part is what it was: no turn key, no turn meta
    assert not any(k.startswith("turn") for k in list(gated.export_slots([0]).tensors) + list(gated.export_slots([0]).meta))


def test_reset_drops_the_turn_and_the_totals(built):
    from afx.vad import ToneGate
    ts = _scorer(3, ToneGate(), seed=4)
    keep = _snap(ts)
    ts.reset([1])
    now = _snap(ts)
    assert ts.turn_state[1].tolist() == [0, 0, 0] and ts.turn_totals[1].tolist() == [0, 0, 0, 0] and ts.samples_seen.tolist()[1] == 0
    assert float(ts.nf[1]) == float("inf") and int(ts.h[1]) == 0 and ts.tone_state[1].tolist() == [0, 0, 0]
    assert int(ts.scorer.samples_seen[1]) == 0 and ts.turns_scored.tolist() == [0, 0, 0]
    assert all(torch.equal(x[[0, 2]], y[[0, 2]]) for x, y in zip(keep, now) if x.ndim and x.shape[0] == 3)
    with pytest.raises(Exception):
        ts.push(torch.zeros(3, 4000))  # on the GPU only: there is no CPU fallback

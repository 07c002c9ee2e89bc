"""The look-ahead gate (afx/vad.py LookaheadGate) without a GPU: the numpy restatement against the dilated mask
``keep'[g] = keep[g] or any(speech[g+1 .. g+pre])``, chunking with carried state (single frames, chunks shorter than ``pre``),
non-finite frames, the argument checks, and every malformed look-ahead row ``import_slots`` refuses on hand-built states.

The input: 6 s of noise at -60 dBFS with six 0.3-s bursts at -20 dBFS under a 40-ms linear onset ramp.  The plain gate
gives 600 frames, 180 speech, 300 kept, 6 onsets; look-ahead adds 6, 30 and 186 frames for pre = 1, 5 and 31."""
import numpy as np
import pytest
import torch

H = 4000
ADDED = {1: 6, 5: 30, 31: 186}


def burst_stream():
    g = np.random.default_rng(0)
    x = (1e-3 * g.standard_normal(96000)).astype(np.float32)
    ramp = np.minimum(np.arange(4800) / 640.0, 1.0)
    for k in range(6):
        a = 8000 + k * 14400
        x[a:a + 4800] += (0.1 * g.standard_normal(4800) * ramp).astype(np.float32)
    return x


X = burst_stream()


def dilated(gate, x):
    """(keep, keep') over the whole of x, from the plain decision: the definition, not the delay line."""
    _, speech, keep, _, _ = gate._decide(x, {"nf": np.float32(np.inf), "h": 0})
    out = keep.copy()
    for g in np.flatnonzero(speech):
        out[max(0, g - gate.pre):g] = True
    return keep, out


def test_the_input_is_what_the_tests_assume():
    from afx.vad import LookaheadGate, SpeechGate
    _, speech, keep, _, _ = SpeechGate()._decide(X, SpeechGate.new_state())
    assert (keep.size, int(speech.sum()), int(keep.sum())) == (600, 180, 300)
    assert int(np.sum(keep[1:] & ~keep[:-1])) == 6 and not keep[0]
    for pre, added in ADDED.items():
        k, kd = dilated(LookaheadGate(pre=pre), X)
        assert int(kd.sum()) - int(k.sum()) == added and not (k & ~kd).any()


@pytest.mark.parametrize("pre", [1, 5, 31])
def test_reference_over_the_whole_stream_equals_the_dilated_mask(pre):
    from afx.vad import LookaheadGate, SpeechGate
    gate = LookaheadGate(pre=pre)
    keep, kd = dilated(gate, X)
    assert (kd != keep).any()
    mask, out, src, st = gate.gate_reference(X)
    assert mask.dtype == bool and np.array_equal(mask, kd[:600 - pre])
    assert src.dtype == np.int64 and np.array_equal(src, np.flatnonzero(kd[:600 - pre]))
    assert out.dtype == np.float32 and out.tobytes() == X.reshape(600, 160)[src].tobytes()
    plain = SpeechGate().gate_reference(X)[2]
    assert st["F"] == 600 and st["nf"].tobytes() == plain["nf"].tobytes() and st["h"] == plain["h"]
    assert st["line"].tobytes() == X[(600 - pre) * 160:].tobytes() and np.array_equal(st["flags"], kd[600 - pre:])
    # the tail of a finished call: one hop of zeros decides every real frame and emits none of its own
    m2, out2, src2, _ = gate.gate_reference(np.zeros(40 * 160, dtype=np.float32), st)
    assert np.array_equal(np.concatenate([mask, m2])[:600], kd) and (src2 < 600).all()
    with pytest.raises(ValueError):
        gate.gate_reference(X[:161])


@pytest.mark.parametrize("pre", [1, 5, 31])
def test_chunked_at_random_frame_boundaries_equals_the_whole_stream(pre):
    from afx.vad import LookaheadGate
    gate = LookaheadGate(pre=pre)
    keep, kd = dilated(gate, X)
    assert (kd != keep).any()
    mask, out, src, st = gate.gate_reference(X)
    rng = np.random.default_rng(pre)
    plans = [np.arange(1, 600)]  # single frames
    plans.append(np.arange(max(pre - 1, 1), 600, max(pre - 1, 1)))  # every chunk shorter than pre (pre = 1: single frames)
    plans += [np.sort(rng.choice(np.arange(1, 600), size=k, replace=False)) for k in (17, 200)]
    for cuts in plans:
        state, masks, outs, srcs = None, [], [], []
        for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [600]])):
            before = None if state is None else {k: np.copy(v) for k, v in state.items()}
            m, o, s, state2 = gate.gate_reference(X[a * 160:b * 160], state)
            assert before is None or all(np.array_equal(before[k], state[k]) for k in before)  # (not modified)
            assert len(state2["flags"]) == min(b, pre) == state2["line"].shape[0]
            state = state2
            masks.append(m), outs.append(o), srcs.append(s)
        assert np.array_equal(np.concatenate(masks), mask)
        assert np.concatenate(outs).tobytes() == out.tobytes() and np.array_equal(np.concatenate(srcs), src)
        assert state["nf"].tobytes() == st["nf"].tobytes() and (state["h"], state["F"]) == (st["h"], 600)
        assert state["line"].tobytes() == st["line"].tobytes() and np.array_equal(state["flags"], st["flags"])


def test_non_finite_frames_behave_as_in_the_plain_gate():
    from afx.vad import LookaheadGate, SpeechGate
    gate, plain = LookaheadGate(hang=2, pre=3), SpeechGate(hang=2)
    x = X[40 * 160:70 * 160].copy()  # ten quiet frames, then an onset
    x[3 * 160 + 17] = np.nan  # a quiet frame: not speech, flags nothing, leaves the floor alone
    x[8 * 160 + 5] = np.inf   # within pre of the onset: flagged by it like any frame, and copied bit for bit
    x[12 * 160] = 1e30        # inside the burst: its energy is inf, not speech, kept by the hangover
    keep, _, pst = plain.gate_reference(x)
    _, speech, _, _, _ = plain._decide(x, SpeechGate.new_state())
    assert not speech[[3, 8, 12]].any() and keep[12] and not keep[3] and not keep[8] and speech[10]
    mask, out, src, st = gate.gate_reference(np.concatenate([x, np.zeros(3 * 160, dtype=np.float32)]))
    want = keep.copy()
    for g in np.flatnonzero(speech):
        want[max(0, g - 3):g] = True
    assert np.array_equal(mask, want) and want[8] and not want[3] and (want != keep).any()
    assert out.tobytes() == x.reshape(-1, 160)[want].tobytes() and np.array_equal(src, np.flatnonzero(want))
    assert st["nf"].tobytes() == plain.gate_reference(np.zeros(480, dtype=np.float32), pst)[2]["nf"].tobytes()


def test_arguments_are_checked_and_the_plain_gate_is_unchanged():
    from afx.vad import LookaheadGate, SpeechGate
    assert SpeechGate().params() == dict(floor=1e-6, ratio=8.0, rise=1.01, hang=20, frame=160)
    g = LookaheadGate()
    assert g.params() == dict(floor=1e-6, ratio=8.0, rise=1.01, hang=20, frame=160, pre=5)
    assert all(type(v) in (int, float) for v in g.params().values()) and isinstance(g, SpeechGate)
    assert LookaheadGate(**LookaheadGate(pre=31, frame=200).params()).params()["pre"] == 31 and LookaheadGate(pre=1).pre == 1
    for bad in (0, 32, -1, True, 5.0, None, "5"):
        with pytest.raises(ValueError):
            LookaheadGate(pre=bad)
    with pytest.raises(ValueError):
        LookaheadGate(ratio=1.0)  # (the plain gate's checks hold)


# ---- sessions on host-only scorers -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _bare(S=2):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=16000, hop=H, device="cpu")


def _snapshot(gs):
    return [gs.ring.clone(), gs.nf.clone(), gs.h.clone(), gs.flags.clone(), gs.line.clone(), gs.src.clone(), gs._head.copy(),
            gs._fill.copy(), gs._seen.copy(), gs.scorer.ring.clone(), gs.scorer.samples_seen]


def _same(a, b):
    return all(torch.equal(torch.as_tensor(u), torch.as_tensor(v)) for u, v in zip(a, b))


def _valid_state(gs):
    """Two sessions as a look-ahead GatedScorer would export them, hand-built: one 5 hops (125 frames) in, three frames
    pending, flags on its two newest delayed frames; one a new stream."""
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
    t["gate_line"] = torch.zeros(2, 5 * 160)
    t["gate_line"][0] = torch.randn(5 * 160, generator=g)
    t["gate_flags"] = torch.tensor([0b11000, 0])
    t["gate_sources"] = torch.full((2, 25), -1, dtype=torch.int64)
    t["gate_sources"][0, :3] = torch.tensor([100, 101, 119])
    return StreamState(st.meta, torch.tensor([5 * H, 0]), t)


def test_export_adds_the_line_and_import_lays_it_out_for_the_slots_own_count(built):
    from afx.streaming import StreamState
    from afx.vad import GatedScorer, LookaheadGate
    gs = GatedScorer(_bare(), LookaheadGate())
    assert gs.last_span is None and gs.state_meta()["gate_params"]["pre"] == 5
    st = gs.export_slots([1, 0])
    assert set(st.tensors) == {"samples", "gate_pending", "gate_fill", "gate_hang", "gate_inner_seen", "gate_nf", "gate_line",
                               "gate_flags", "gate_sources"}
    assert tuple(st.tensors["gate_line"].shape) == (2, 800) and not st.tensors["gate_line"].any()
    assert st.tensors["gate_flags"].dtype == torch.int64 and st.tensors["gate_flags"].tolist() == [0, 0]
    assert st.tensors["gate_sources"].dtype == torch.int64 and (st.tensors["gate_sources"] == -1).all()
    good = _valid_state(gs)
    dst = GatedScorer(_bare(S=4), LookaheadGate())
    dst.import_slots([3, 1], StreamState.from_state_dict(good.state_dict()))
    # F = 125: delayed frames 120 .. 124 sit at blocks 0 .. 4, so the flags of the two newest are bits 3 and 4
    assert int(dst.flags[3]) == 0b11000 and torch.equal(dst.line[3], good.tensors["gate_line"][0])
    assert dst.src[3, :4].tolist() == [100, 101, 119, -1] and int(dst.flags[1]) == 0
    back = dst.export_slots([3, 1])
    for k in ("gate_line", "gate_flags", "gate_sources", "gate_pending", "gate_fill"):
        assert torch.equal(back.tensors[k], good.tensors[k]), k
    # a count that is no multiple of pre rotates the line: F = 127 puts frames 122 .. 126 at blocks 2, 3, 4, 0, 1
    H2 = 127 * 160
    from afx.streaming import SlidingWindowScorer
    odd = GatedScorer(SlidingWindowScorer(None, 1, window=4 * H2, hop=H2, device="cpu"), LookaheadGate())
    one = odd.export_slots([0])
    t = dict(one.tensors)
    t["gate_line"] = torch.arange(800, dtype=torch.float32)[None]
    t["gate_flags"] = torch.tensor([0b00110])
    odd.import_slots([0], StreamState(one.meta, torch.tensor([H2]), t))
    assert torch.equal(odd.line[0].view(5, 160)[[2, 3, 4, 0, 1]].reshape(-1), t["gate_line"][0])
    assert int(odd.flags[0]) == (1 << 3) | (1 << 4)  # the 2nd and 3rd oldest: frames 123 and 124
    again = odd.export_slots([0])
    assert torch.equal(again.tensors["gate_line"], t["gate_line"]) and again.tensors["gate_flags"].tolist() == [0b00110]
    odd.reset([0])
    assert int(odd.flags[0]) == 0 and (odd.src[0] == -1).all() and not odd.export_slots([0]).tensors["gate_line"].any()


def test_import_refuses_every_malformed_row_with_nothing_changed(built):
    from afx.streaming import StreamState
    from afx.vad import GatedScorer, LookaheadGate, SpeechGate
    src = GatedScorer(_bare(), LookaheadGate())
    good = _valid_state(src)
    dst = GatedScorer(_bare(S=3), LookaheadGate())
    dst.import_slots([2, 0], good)  # something to lose
    before = _snapshot(dst)

    def variant(seen=None, drop=(), **tensors):
        t = {k: v for k, v in dict(good.tensors, **tensors).items() if k not in drop}
        return StreamState(good.meta, good.seen if seen is None else seen, t)

    def sources(*v):
        s = torch.full((2, 25), -1, dtype=torch.int64)
        s[0, :len(v)] = torch.tensor(v)
        return s

    young = dict(seen=torch.tensor([H, 0]), gate_inner_seen=torch.tensor([0, 0]), gate_sources=sources(2, 3, 19))
    bad = {
        "a flag bit beyond the delayed count": variant(gate_flags=torch.tensor([0b100000, 0])),
        "a flag on a new stream": variant(gate_flags=torch.tensor([0b11000, 1])),
        "flags negative": variant(gate_flags=torch.tensor([-1, 0])),
        "flags not int64": variant(gate_flags=torch.tensor([0b11000, 0], dtype=torch.int32)),
        "sources not increasing": variant(gate_sources=sources(100, 100, 119)),
        "sources decreasing": variant(gate_sources=sources(101, 100, 119)),
        "a source at the oldest delayed frame": variant(gate_sources=sources(100, 101, 120)),
        "a source negative": variant(gate_sources=sources(-1, 101, 119)),
        "a source after the fill": variant(gate_sources=sources(100, 101, 119, 119)),
        "a source missing": variant(gate_sources=sources(100, 101)),
        "sources of another shape": variant(gate_sources=torch.full((2, 50), -1, dtype=torch.int64)),
        "sources not int64": variant(gate_sources=sources(100, 101, 119).to(torch.int32)),
        "line of another shape": variant(gate_line=torch.zeros(2, 6 * 160)),
        "line of another type": variant(gate_line=torch.zeros(2, 800, dtype=torch.float64)),
        "a line tensor missing": variant(drop=("gate_flags",)),
        "the plain gate's checks hold": variant(gate_hang=torch.tensor([21, 0])),
        # one hop = 25 frames in: frames 20 .. 24 are delayed, so a source of 20 is beyond what has left the line
        "a source beyond a young session's decided frames": variant(**dict(young, gate_sources=sources(2, 3, 20))),
        "a plain gate's state": GatedScorer(_bare(), SpeechGate()).export_slots([0, 1]),
    }
    for what, st in bad.items():
        with pytest.raises(ValueError):
            dst.import_slots([2, 0], st)
        assert _same(before, _snapshot(dst)), what
    dst.import_slots([2, 0], variant(**young))  # (the young session itself is fine)
    # the two kinds of gate refuse each other's states, and another pre is another gate
    plain = GatedScorer(_bare(), SpeechGate())
    ring0 = plain.ring.clone()
    for other in (plain, GatedScorer(_bare(), LookaheadGate(pre=4))):
        with pytest.raises(ValueError):
            other.import_slots([0, 1], good)
    assert torch.equal(plain.ring, ring0) and plain.pending.tolist() == [0, 0]
    assert plain._keys == ("gate_pending", "gate_fill", "gate_hang", "gate_inner_seen", "gate_nf") == GatedScorer._keys
    assert "pre" not in plain.state_meta()["gate_params"] and not hasattr(plain, "line")

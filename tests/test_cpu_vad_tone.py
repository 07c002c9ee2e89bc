"""The tone gate on the host (afx/vad.py ToneGate, afx_k_gate_tone): the argument checks, the numpy restatement against a
scalar loop over the stated operations, a hand-worked decision table, equality with ``SpeechGate`` where no frame is tonal,
chunking, and the session part of a tone-gated ``GatedScorer`` built on the CPU.  Every comparison is exact: bits of fp32,
and integers.  No GPU."""
import ctypes
import io

import numpy as np
import pytest
import torch

H, WINDOW = 4000, 16000
f32 = np.float32


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _sin(n, *freqs, amp=0.3, start=0):
    t = (start + np.arange(n)) / 16000
    return sum((amp * np.sin(2 * np.pi * f * t)).astype(f32) for f in freqs)


def _voice(n, seed=0):
    """The 180 Hz tremolo "voice" of tools/gate_bench.py over background noise."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000
    return (0.2 * np.sin(2 * np.pi * 180 * t) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t))).astype(f32) + \
        (0.002 * g.standard_normal(n)).astype(f32)


# ---- 1. arguments ------------------------------------------------------------------------------------------------------------------
def test_the_arguments_are_checked(built):
    from afx.vad import TELEPHONY_TONES, LookaheadGate, SpeechGate, ToneGate
    assert TELEPHONY_TONES == (697, 770, 852, 941, 1209, 1336, 1477, 1633, 350, 440, 480, 620, 425, 1004, 1100, 2100)
    g = ToneGate()
    assert isinstance(g, SpeechGate) and not isinstance(g, LookaheadGate)
    p = g.params()
    assert p == dict(SpeechGate().params(), freqs=[float(f) for f in TELEPHONY_TONES], frac=0.85, confirm=4, hold=3)
    assert (g.E_floor, g.ratio32, g.rise32, g.nf_min) == (SpeechGate().E_floor, SpeechGate().ratio32, SpeechGate().rise32, SpeechGate().nf_min)
    assert g.coef.dtype == np.float32 and g.coef.shape == (16,) and g.thr.dtype == np.float32
    assert g.coef.tolist() == [float(f32(2 * np.cos(2 * np.pi * np.float64(f) / 16000))) for f in TELEPHONY_TONES]
    assert float(g.thr) == float(f32(0.85 * 160 / 2))
    assert g.new_state() == {"nf": f32(np.inf), "h": 0, "r": 0, "q": 0, "tones": 0}
    assert ToneGate(freqs=[1000.5], frac=2.0, confirm=1, hold=0).params()["freqs"] == [1000.5]
    bad = [dict(freqs=()), dict(freqs=list(range(100, 1800, 100))), dict(freqs=(440, 440)), dict(freqs=(0,)), dict(freqs=(8000,)),
           dict(freqs=(-5,)), dict(freqs=(float("nan"),)), dict(freqs=(float("inf"),)), dict(freqs=("440",)), dict(freqs=440),
           dict(freqs="440"), dict(freqs=(True,)), dict(freqs=None), dict(frac=0), dict(frac=-0.5), dict(frac=2.0001),
           dict(frac=float("nan")), dict(frac=float("inf")), dict(frac=1e-60), dict(frac="1"), dict(confirm=0), dict(confirm=-1),
           dict(confirm=1.0), dict(confirm=True), dict(confirm=1 << 31), dict(hold=-1), dict(hold=2.0), dict(hold=None),
           dict(hold=1 << 31), dict(floor=0), dict(ratio=1.0), dict(rise=0.5), dict(hang=-1), dict(frame=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            ToneGate(**kw)
    with pytest.raises(ValueError):
        g.tone_powers(np.zeros(161, dtype=f32))
    with pytest.raises(ValueError):
        g.gate_reference(np.zeros(100, dtype=f32))
    # the C ABI has the symbol, and the ctypes table binds it
    assert "afx_k_gate_tone" in built.SIGNATURES and hasattr(ctypes.CDLL(built.LIB_PATH), "afx_k_gate_tone")
    assert len(built.SIGNATURES["afx_k_gate_tone"][1]) == 25


# ---- 2. the powers against a scalar loop over the stated operations -----------------------------------------------------------------
def _scalar_powers(x, frame, coef):
    out = np.zeros((x.size // frame, len(coef)), dtype=f32)
    with np.errstate(all="ignore"):
        for f in range(out.shape[0]):
            for k, c in enumerate(coef):
                s1 = s2 = f32(0.0)
                for i in range(frame):
                    t = f32(c * s1)
                    t = f32(t - s2)
                    s0 = f32(x[f * frame + i] + t)
                    s2 = s1
                    s1 = s0
                a, b = f32(s1 * s1), f32(s2 * s2)
                m = f32(c * s1)
                m = f32(m * s2)
                out[f, k] = f32(f32(a + b) - m)
    return out


@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("frame", [1, 2, 63, 160, 161])
def test_tone_powers_equal_a_scalar_loop(built, frame, K):
    from afx.vad import TELEPHONY_TONES, ToneGate
    gate = ToneGate(frame=frame, freqs=TELEPHONY_TONES[:K])
    g = np.random.default_rng(100 * frame + K)
    frames = 5
    x = (0.1 * g.standard_normal(frames * frame)).astype(f32) + _sin(frames * frame, 697, 1209)
    x[frame:2 * frame] *= f32(1e-20)              # squares and products underflow
    if frame > 2:
        x[2 * frame + 1], x[3 * frame + frame // 2] = np.inf, np.nan
    got = gate.tone_powers(x)
    want = _scalar_powers(x, frame, gate.coef)
    assert got.dtype == np.float32 and got.shape == (frames, K)
    assert got.tobytes() == want.tobytes()
    assert np.isfinite(got[0]).all() and (got[0] > 0).any()
    # T: the two largest positive powers, anything else counts as +0.0
    T = gate.decide_reference(x)[0]
    for f in range(frames):
        v = sorted((float(p) for p in want[f] if p > 0), reverse=True) + [0.0, 0.0]
        assert T[f].tobytes() == f32(f32(v[0]) + f32(v[1])).tobytes(), f
    assert not np.isnan(T).any()


# ---- 3. a hand-worked decision table -------------------------------------------------------------------------------------------------
# gate: confirm 3, hold 3, hang 4.  Frames: T an exact bank sinusoid (1004 Hz, amplitude 0.3: loud, so "speech" to the plain
# gate), S loud white noise (speech, not tonal), Q noise below the floor (neither).  Columns: kind, tonal, tone, keep.
TABLE = [
    ("Q", 0, 0, 0), ("Q", 0, 0, 0),
    # a burst of confirm - 1 frames never becomes tone: kept as speech, then the hangover of 4
    ("T", 1, 0, 1), ("T", 1, 0, 1), ("Q", 0, 0, 1), ("Q", 0, 0, 1), ("Q", 0, 0, 1), ("Q", 0, 0, 1), ("Q", 0, 0, 0),
    # a burst of exactly confirm: its third frame is tone, ends the hangover; hold 3, then it expires
    ("T", 1, 0, 1), ("T", 1, 0, 1), ("T", 1, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 0, 0),
    # a hold bridged by a new run: one loud non-tonal frame, then the run is confirmed again before the hold is out
    ("T", 1, 0, 1), ("T", 1, 0, 1), ("T", 1, 1, 0), ("S", 0, 1, 0), ("T", 1, 1, 0), ("T", 1, 1, 0), ("T", 1, 1, 0),
    ("Q", 0, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 0, 0),
    # a tone inside a hangover: h becomes 0 and the following silence is dropped
    ("S", 0, 0, 1), ("S", 0, 0, 1), ("Q", 0, 0, 1), ("T", 1, 0, 1), ("T", 1, 0, 1), ("T", 1, 1, 0),
    ("Q", 0, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 1, 0), ("Q", 0, 0, 0), ("Q", 0, 0, 0),
]


def _table_stream():
    g = np.random.default_rng(5)
    n = len(TABLE) * 160
    tone, loud, quiet = _sin(n, 1004), (0.1 * g.standard_normal(n)).astype(f32), (0.0003 * g.standard_normal(n)).astype(f32)
    x = np.concatenate([{"T": tone, "S": loud, "Q": quiet}[k][i * 160:(i + 1) * 160] for i, (k, *_) in enumerate(TABLE)])
    return x


def test_the_decision_table_by_hand(built):
    from afx.vad import SpeechGate, ToneGate
    gate = ToneGate(hang=4, confirm=3, hold=3)
    x = _table_stream()
    T, tonal, tone, keep = gate.decide_reference(x)
    assert T.dtype == np.float32 and T.shape == (len(TABLE),)
    assert tonal.astype(int).tolist() == [r[1] for r in TABLE]
    assert tone.astype(int).tolist() == [r[2] for r in TABLE]
    assert keep.astype(int).tolist() == [r[3] for r in TABLE]
    mask, kept, st = gate.gate_reference(x)
    assert mask.tolist() == keep.tolist() and kept.tobytes() == x.reshape(-1, 160)[keep].tobytes()
    assert (st["r"], st["q"], st["h"], st["tones"]) == (0, 0, 0, sum(r[2] for r in TABLE))
    # the plain gate keeps the tones and the silence after them: the last block's hangover is what the tone ended
    plain = SpeechGate(hang=4).gate_reference(x)[0]
    assert plain[30:37].all() and not keep[32:37].any()
    # where nothing was tone yet, the two gates agree (the first confirm - 1 frames of a burst are the plain gate's)
    assert plain[:11].tolist() == keep[:11].tolist()
    # the state in the middle: inside a confirmed tone r >= confirm and q == hold; inside a hold r == 0 and 0 < q < hold
    assert [gate.gate_reference(x[:n * 160])[2][k] for n in (12, 13, 23) for k in ("r", "q")] == [3, 3, 0, 2, 3, 3]


# ---- 4. no tonal frame: the plain gate, bit for bit -------------------------------------------------------------------------------
def _noise_bursts(n, seed):
    g = np.random.default_rng(seed)
    x = (0.002 * g.standard_normal(n)).astype(f32)
    pos = 0
    while pos < n:
        m = int(g.integers(800, 8000))
        if g.random() < 0.5:
            x[pos:pos + m] += (0.1 * g.standard_normal(min(m, n - pos))).astype(f32)
        pos += m
    return x


@pytest.mark.parametrize("name", ["noise bursts", "tremolo voice"])
def test_without_a_tonal_frame_it_is_the_plain_gate(built, name):
    from afx.vad import SpeechGate, ToneGate
    n = 64000
    x = _noise_bursts(n, 3) if name == "noise bursts" else _voice(n, 4) * np.repeat((np.arange(n // 8000) % 2).astype(f32), 8000)
    x = x + (0.002 * np.random.default_rng(9).standard_normal(n)).astype(f32)
    tone, plain = ToneGate(), SpeechGate()
    _, tonal, is_tone, keep = tone.decide_reference(x)
    assert not tonal.any() and not is_tone.any() and keep.any() and not keep.all()
    st_t, st_p = None, None
    for a, b in [(0, 16000), (16000, 16160), (16160, 64000)]:
        mt, kt, st_t = tone.gate_reference(x[a:b], st_t)
        mp, kp, st_p = plain.gate_reference(x[a:b], st_p)
        assert mt.tolist() == mp.tolist() and kt.tobytes() == kp.tobytes()
        assert f32(st_t["nf"]).tobytes() == f32(st_p["nf"]).tobytes() and st_t["h"] == st_p["h"]
        assert (st_t["r"], st_t["q"], st_t["tones"]) == (0, 0, 0)


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------------
def call_stream(seed=0, n=96000):
    """Ringback cadence (440 + 480 Hz, 1 s on, 1 s off here), then talk with a DTMF digit string inside it, over line noise."""
    g = np.random.default_rng(seed)
    x = (0.002 * g.standard_normal(n)).astype(f32)
    x[:16000] += _sin(16000, 440, 480, amp=0.15)
    x[32000:] += _voice(n - 32000, seed + 1)
    for d, (lo, hi) in enumerate([(697, 1209), (770, 1336), (852, 1477), (941, 1633)]):
        a = 48000 + d * 2400 + 37 * d
        x[a:a + 1600] = _sin(1600, lo, hi, amp=0.25) + (0.002 * g.standard_normal(1600)).astype(f32)
    return x


def test_a_stream_cut_at_random_frame_boundaries_equals_the_whole(built):
    from afx.vad import ToneGate
    gate = ToneGate()
    x = call_stream()
    T, tonal, tone, keep = gate.decide_reference(x)
    mask, kept, st = gate.gate_reference(x)
    # the input exercised the gate: both values of each flag, a confirmed run, a hold that expired, a burst that stayed short
    for flag in (tonal, tone, keep):
        assert flag.any() and not flag.all()
    assert (tone & ~tonal).any() and (tonal & ~tone).any() and st["tones"] == int(tone.sum()) and st["q"] == 0
    g = np.random.default_rng(1)
    for trial in range(3):
        cuts = [0] + sorted(g.choice(np.arange(1, x.size // 160), size=12, replace=False).tolist()) + [x.size // 160]
        s, parts, masks, rows = None, [], [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            rows.append(gate.decide_reference(x[a * 160:b * 160], s))
            m, k, s = gate.gate_reference(x[a * 160:b * 160], s)
            masks.append(m)
            parts.append(k)
        assert np.concatenate(masks).tolist() == mask.tolist() and np.concatenate(parts).tobytes() == kept.tobytes()
        assert np.concatenate([r[0] for r in rows]).tobytes() == T.tobytes()
        assert np.concatenate([r[1] for r in rows]).tolist() == tonal.tolist()
        assert np.concatenate([r[2] for r in rows]).tolist() == tone.tolist()
        assert np.concatenate([r[3] for r in rows]).tolist() == keep.tolist()
        assert f32(s["nf"]).tobytes() == f32(st["nf"]).tobytes() and {k: s[k] for k in "hrq"} == {k: st[k] for k in "hrq"}
        assert s["tones"] == st["tones"]


# ---- 6. sessions, with the scorer built on the CPU ------------------------------------------------------------------------------------
def _bare(S):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=WINDOW, hop=H, device="cpu")


def _tone_scorer(S, gate=None, seed=0, dirty=True):
    from afx.vad import GatedScorer, ToneGate
    gs = GatedScorer(_bare(S), ToneGate() if gate is None else gate)
    if dirty:
        g = torch.Generator().manual_seed(seed)
        rows = [[5, 3, 40], [0, 2, 7], [0, 0, 0], [2, 0, 9]]  # confirmed; in a hold; fresh; a short run after tones
        gs.tone_state[:] = torch.tensor([rows[(s + seed) % 4] for s in range(S)], dtype=torch.int32)
        gs.nf[:] = torch.tensor([[1e-3, float("inf"), 2.5e-4, 5e-5][(s + seed) % 4] for s in range(S)])
        gs.h[:] = torch.tensor([[0, 0, 20, 3][(s + seed) % 4] for s in range(S)], dtype=torch.int32)
        gs.ring[:] = torch.randn(S, 2 * H, generator=g)
        gs._fill[:] = [[480, 0, 160, 0][(s + seed) % 4] for s in range(S)]
        gs._head[:] = [[100, 0, 7900, 0][(s + seed) % 4] for s in range(S)]
        gs._seen[:] = 3 * H
        gs.scorer._seen[:] = 2 * H
        gs.scorer.ring[:] = torch.randn(S, WINDOW, generator=g)
    return gs


def _snap(gs):
    parts = [gs.scorer.ring, gs.scorer._seen, gs.nf, gs.h, gs.ring, gs._fill, gs._head, gs._seen]
    return [torch.as_tensor(p).clone() for p in parts + ([gs.tone_state] if hasattr(gs, "tone_state") else [])]


def _same(a, b):
    return len(a) == len(b) and all(u.dtype == v.dtype and u.shape == v.shape and (
        torch.equal(u.view(torch.int32), v.view(torch.int32)) if u.dtype == torch.float32 else torch.equal(u, v)) for u, v in zip(a, b))


def _through_a_file(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def test_a_tone_state_round_trips_and_every_bad_one_is_refused(built):
    from afx.streaming import StreamState
    from afx.vad import GatedScorer, LookaheadGate, SpeechGate, ToneGate
    a, b = _tone_scorer(3, seed=0), _tone_scorer(4, seed=1)
    assert a.last_tone_frames is None and a.tone_frames.tolist() == [40, 7, 0] and a.tone_frames.dtype == torch.int32
    assert GatedScorer(_bare(2)).tone_frames is None and GatedScorer(_bare(2)).last_tone_frames is None
    st = a.export_slots([1, 0])
    assert st.tensors["gate_tone"].dtype == torch.int64 and st.tensors["gate_tone"].tolist() == [[0, 2, 7], [5, 3, 40]]
    assert st.meta["gate_params"] == ToneGate().params() and st.seen.tolist() == [3 * H, 3 * H]
    good = _through_a_file(st)
    m, t = good.meta, good.tensors
    tone = lambda rows: StreamState(m, good.seen, dict(t, gate_tone=torch.tensor(rows)))  # noqa: E731
    frames = 3 * H // 160
    spoiled = {
        "r negative": tone([[-1, 2, 7], [5, 3, 40]]),
        "q negative": tone([[0, -1, 7], [5, 3, 40]]),
        "q above hold": tone([[0, 4, 7], [5, 3, 40]]),
        "confirmed without the full hold": tone([[0, 2, 7], [4, 2, 40]]),
        "tones negative": tone([[0, 2, -1], [5, 3, 40]]),
        "tones above the frames seen": tone([[0, 2, 7], [5, 3, frames + 1]]),
        "int32": StreamState(m, good.seen, dict(t, gate_tone=t["gate_tone"].to(torch.int32))),
        "two columns": StreamState(m, good.seen, dict(t, gate_tone=t["gate_tone"][:, :2])),
        "no gate_tone": StreamState(m, good.seen, {k: v for k, v in t.items() if k != "gate_tone"}),
        "another hold": StreamState(dict(m, gate_params=dict(m["gate_params"], hold=4)), good.seen, t),
        "another bank": StreamState(dict(m, gate_params=dict(m["gate_params"], freqs=[440.0])), good.seen, t),
        "a plain gate's params": StreamState(dict(m, gate_params=SpeechGate().params()), good.seen, t),
    }
    before = _snap(b)
    for name, state in spoiled.items():
        with pytest.raises(ValueError):
            b.import_slots([3, 1], state)
        assert _same(before, _snap(b)), name
    # a plain, a look-ahead and a tone state do not import into each other, in any direction, and nothing changes
    plain, look = GatedScorer(_bare(4)), GatedScorer(_bare(4), LookaheadGate())
    states = {"plain": plain.export_slots([0, 1]), "look": look.export_slots([0, 1]), "tone": _tone_scorer(4, dirty=False).export_slots([0, 1])}
    for dst_name, dst in (("plain", plain), ("look", look), ("tone", b)):
        snap = _snap(dst)
        for src_name, state in states.items():
            if src_name != dst_name:
                with pytest.raises(ValueError):
                    dst.import_slots([3, 1], _through_a_file(state))
                assert _same(snap, _snap(dst)), (src_name, dst_name)
    # the good state: the rows arrive, the other slots keep theirs, and it exports again as it was
    others = b.export_slots([0, 2])
    b.import_slots([3, 1], good)
    back = b.export_slots([3, 1])
    assert back.meta == m and torch.equal(back.seen, good.seen) and set(back.tensors) == set(t)
    assert _same([back.tensors[k] for k in sorted(t)], [t[k] for k in sorted(t)])
    assert b.tone_state[[3, 1]].tolist() == [[0, 2, 7], [5, 3, 40]] and b.tone_frames[[3, 1]].tolist() == [7, 40]
    after = b.export_slots([0, 2])
    assert _same([after.tensors[k] for k in sorted(t)], [others.tensors[k] for k in sorted(t)])
    # at the edge: tones == the frames seen, q == hold with r below confirm
    b.import_slots([0], StreamState(m, good.seen[:1], dict({k: v[:1] for k, v in t.items()}, gate_tone=torch.tensor([[1, 3, frames]]))))
    assert b.tone_state[0].tolist() == [1, 3, frames]
    b.reset([0, 3])
    assert b.tone_state.tolist() == [[0, 0, 0], [5, 3, 40], b.tone_state[2].tolist(), [0, 0, 0]]
    assert float(b.nf[3]) == float("inf") and int(b.h[3]) == 0


def test_a_plain_chains_layout_does_not_gain_a_tone_part(built):
    from afx.vad import GatedScorer
    st = GatedScorer(_bare(2)).export_slots([0, 1])
    assert "gate_tone" not in st.tensors and set(k for k in st.tensors if k.startswith("gate_")) == {
        "gate_pending", "gate_fill", "gate_hang", "gate_inner_seen", "gate_nf"}
    assert sorted(st.meta["gate_params"]) == ["floor", "frame", "hang", "ratio", "rise"]

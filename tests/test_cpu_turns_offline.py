"""Turns offline and the end of a call, on the host (afx/turns.py: ``close_reference``, ``cut_reference``, ``Turns``,
``score_turns`` and ``TurnScorer.flush``; afx_k_turn_scan / afx_k_turn_clips / afx_k_turn_close): the whole-array restatement
of the cut against the push-by-push one chained and closed, and against ``turns_reference`` on the fixture; the methods of
``Turns`` on hand-made values; the refusals; the ABI.  Every comparison is exact.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_cpu_turns import _bare, _stream
from test_gpu_turns import _programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _chained(policy, keep, top, F, close):
    """``step_reference`` over pushes of F frames (the last one shorter), then ``close_reference`` -> what ``cut_reference``
    returns."""
    state, turns = policy.new_state(top), []
    for g0 in range(0, len(keep), F):
        state, done = policy.step_reference(state, keep[g0:g0 + F], g0)
        if done[1]:
            turns.append(dict(first=done[2], end=done[3], cut=done[1] == top, at_end=False))
    still = (state["g"], state["n"]) if state["n"] else (-1, 0)
    if close:
        state, done = policy.close_reference(state)
        if done[1]:
            turns.append(dict(first=done[2], end=done[3], cut=False, at_end=True))
        still = (-1, 0)
        assert state["n"] == 0 and policy.close_reference(state) == (state, (0, 0, 0, 0))  # a second close finds nothing
    return turns, state["totals"], still


def _masks(least, top):
    """Seeded random masks of several densities and lengths (0 and 1 frames among them), with bytes whose other bits are
    set, and the constructed streams of the kernel tests."""
    g = np.random.default_rng(least * 131 + top)
    out = [np.zeros(0, dtype=np.uint8), np.ones(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8), np.ones(3 * top + 1, dtype=np.uint8)]
    for n in (7, 64, 257, 1000):
        for density in (0.3, 0.8, 0.97):
            m = (g.random(n) < density).astype(np.uint8)
            out.append(m | (g.integers(0, 128, n).astype(np.uint8) << 1))  # only bit 0 counts
    out += [np.array(p, dtype=np.uint8) for p in _programs(max(1, min(4, least)), least, top)]
    out += [np.array(p + [1] * k, dtype=np.uint8) for p in _programs(1, least, top)[:2] for k in (1, least - 1, least, top)]
    return out


@pytest.mark.parametrize("least,top", [(4, 8), (5, 7), (25, 100), (1, 1), (3, 3)])
def test_cut_reference_equals_the_chained_steps_and_the_close(built, least, top):
    from afx.turns import TurnPolicy
    policy = TurnPolicy(least)
    seen = dict(at_end=0, short_end=0, cut=0, cut_on_last=0, open=0)
    for keep in _masks(least, top):
        for close in (True, False):
            got = policy.cut_reference(keep, top, close_end=close)
            turns, totals, still = got
            for F in sorted({1, 4, least, top}):
                chained = _chained(policy, keep, top, F, close)
                if F <= least:  # a push completes at most one scored turn: ``done`` names every one
                    assert got == chained, (keep.tolist(), close, F)
                else:  # a push may complete two and ``done`` names the later one: the totals and the open turn still agree
                    assert got[1:] == chained[1:] and all(t in turns for t in chained[0]), (keep.tolist(), close, F)
            assert totals[0] == len(turns) and totals[2] == sum(t["cut"] for t in turns) and totals[3] == int((keep & 1).sum())
            assert all(t["end"] - t["first"] == top if t["cut"] else least <= t["end"] - t["first"] < top for t in turns)
            assert all(a["end"] <= b["first"] for a, b in zip(turns, turns[1:]))
            seen["at_end"] += sum(t["at_end"] for t in turns)
            seen["cut"] += totals[2]
            seen["cut_on_last"] += bool(turns and turns[-1]["cut"] and turns[-1]["end"] == keep.size)
            seen["open"] += still != (-1, 0)
        a, b = policy.cut_reference(keep, top, True), policy.cut_reference(keep, top, False)
        seen["short_end"] += a[1][1] > b[1][1]
        assert [t for t in a[0] if not t["at_end"]] == b[0]  # close_end=False drops exactly the at_end turns
    # the masks show every case the parameters allow: a scored turn closed by the end needs min < max, a short one min > 1
    need = {"cut", "cut_on_last"} | ({"at_end"} if least < top else set()) | ({"short_end"} if least > 1 else set()) | (
        {"open"} if top > 1 else set())
    assert all(seen[k] for k in need), seen


@pytest.mark.parametrize("gate_name", ["SpeechGate", "ToneGate"])
def test_cut_reference_equals_turns_reference_on_the_fixture(built, gate_name):
    from afx import turns, vad
    gate, policy, top = getattr(vad, gate_name)(), turns.TurnPolicy(25), 100
    for offset, n in ((0, 128000), (30057, 128000), (0, 72000), (0, 68000)):
        x = _stream(offset, n)
        want, totals, still = policy.turns_reference(x, gate, top)
        keep = gate.gate_reference(x)[0]
        got = policy.cut_reference(keep, top, close_end=False)
        assert [(t["first"], t["end"], t["cut"]) for t in got[0]] == [(t["first"], t["end"], t["cut"]) for t in want if t["scored"]]
        assert got[1] == totals and got[2] == ((-1, 0) if still is None else still)
        closed = policy.cut_reference(keep, top)
        assert closed[2] == (-1, 0) and closed[1][3] == totals[3] and closed[1][2] == totals[2]
        if still is not None:
            scored = still[1] >= 25
            assert closed[1][:2] == (totals[0] + scored, totals[1] + (not scored))
            assert not scored or closed[0][-1] == dict(first=still[0], end=still[0] + still[1], cut=False, at_end=True)


def test_close_reference_by_hand(built):
    from afx.turns import TurnPolicy
    policy, top = TurnPolicy(3), (1 << 31) - 1
    base = dict(policy.new_state(8), g=40, totals=(5, 6, 7, 8))
    assert policy.close_reference(dict(base, n=3, open=1)) == (dict(base, n=0, open=0, totals=(6, 6, 7, 8)), (1, 3, 40, 43))
    assert policy.close_reference(dict(base, n=7, open=0)) == (dict(base, n=0, open=1, totals=(6, 6, 7, 8)), (0, 7, 40, 47))
    assert policy.close_reference(dict(base, n=2, open=1)) == (dict(base, n=0, open=1, totals=(5, 7, 7, 8)), (0, 0, 0, 0))
    assert policy.close_reference(dict(base, n=0, open=1)) == (dict(base, n=0, open=1), (0, 0, 0, 0))
    full = dict(base, totals=(top, top, 1, 2))
    assert policy.close_reference(dict(full, n=3))[0]["totals"] == (top, top, 1, 2)  # the counters saturate
    assert policy.close_reference(dict(full, n=1))[0]["totals"] == (top, top, 1, 2)
    state = dict(base, n=3)
    policy.close_reference(state)
    assert state == dict(base, n=3)  # the argument is not modified


def test_turns_methods_on_hand_made_values(built):
    from afx.turns import Turns
    from afx.verdict import VerdictPolicy
    t = Turns([0.5, -1.0, -2.0, 3.0, -4.0], [8000, 16000, 32000, 48000, 80000], [12000, 32000, 40000, 64000, 96000],
              [False, True, False, False, False], [False, False, False, False, True],
              dict(scored=5, short=2, cut=1, kept_frames=500, open_frames=0))
    assert len(t) == 5 and t.sample_rate == 16000 and t.scores.dtype == torch.float32 and t.starts.dtype == torch.float64
    assert t.cut.dtype == torch.bool and t.at_end.tolist() == [False] * 4 + [True] and t.totals["short"] == 2
    assert t.times().tolist() == [[0.5, 0.75], [1.0, 2.0], [2.0, 2.5], [3.0, 4.0], [5.0, 6.0]]
    # turns 1 and 2 are the pieces of one cut run (the second begins where the first ends): merged; turn 4 stands alone
    assert t.segments(0.0) == [(1.0, 2.5), (5.0, 6.0)]
    assert t.segments(-1.5) == [(2.0, 2.5), (5.0, 6.0)] and t.segments(-10.0) == [] and t.segments(10.0)[0] == (0.5, 0.75)
    assert t.summary(0.0) == {"turns": 5, "min": -4.0, "mean": -0.7, "flagged": 0.6}
    empty = Turns([], [], [], [], [])
    assert len(empty) == 0 and empty.segments(0.0) == [] and empty.summary(0.0)["turns"] == 0 and empty.times().shape == (0, 2)
    assert empty.totals == dict(scored=0, short=0, cut=0, kept_frames=0, open_frames=0) and empty.alarms(VerdictPolicy(0.0)) == []
    half = Turns([1.0], [4000.0], [8000.0], [False], [True], sample_rate=8000)
    assert half.times().tolist() == [[0.5, 1.0]]
    with pytest.raises(ValueError):
        Turns([0.1], [0, 1], [1], [False], [False])
    # alarms: run_reference over the scores, the hop index counting utterances from 1
    policy = VerdictPolicy(0.0)
    events, _ = policy.run_reference(t.scores.numpy())
    assert events and [e[2] for e in events] == sorted(e[2] for e in events) and all(1 <= e[2] <= 5 for e in events)
    ends = [0.75, 2.0, 2.5, 4.0, 6.0]
    want = []
    for _slot, kind, j, _bits in events:
        if kind == 3:
            want[-1] = (want[-1][0], ends[j - 1], want[-1][2])
        else:
            want.append((ends[j - 1], None, kind))
    assert t.alarms(policy) == want and want[0][0] == ends[events[0][2] - 1]


def test_turns_file_format(built, tmp_path):
    from afx import harness
    from afx.turns import Turns
    turns = [Turns([0.5, -1.25], [0, 4000], [4000, 8000], [True, False], [False, True]), Turns([], [], [], [], []),
             Turns([2.0], [22050.0], [44100.0], [False], [False], sample_rate=44100)]
    path = tmp_path / "sub" / "turns.txt"
    harness.write_turns_file(str(path), ["a", "b", "c"], turns)
    assert path.read_text().splitlines() == ["a 0.000 0.250 0.5", "a 0.250 0.500 -1.25", "c 0.500 1.000 2.0"]


def test_score_turns_and_flush_refusals(built):
    from afx import turns
    from afx._lib import AfxError
    from afx.engine import Engine
    from afx.vad import LookaheadGate, SpeechGate
    eng, rec = Engine.__new__(Engine), [torch.zeros(16000)]
    with pytest.raises(ValueError, match="LookaheadGate"):
        turns.score_turns(eng, rec, gate=LookaheadGate())
    with pytest.raises(ValueError):
        turns.score_turns(eng, rec, gate="speech")
    with pytest.raises(ValueError):
        turns.score_turns(eng, rec, policy=25)
    with pytest.raises(ValueError, match="whole number"):
        turns.score_turns(eng, rec, window=16100)
    with pytest.raises(ValueError, match="whole number"):
        turns.score_turns(eng, rec, gate=SpeechGate(frame=200), window=16100)
    with pytest.raises(ValueError, match="min_frames"):
        turns.score_turns(eng, rec, policy=turns.TurnPolicy(101), window=16000)
    with pytest.raises(ValueError):
        turns.score_turns(object(), rec)  # neither an Engine nor a drop-in module
    for bad in (0, -1, 2.5, 65536):
        with pytest.raises(ValueError):
            turns.score_turns(eng, rec, batch=bad)
    if not torch.cuda.is_available():
        with pytest.raises(AfxError):
            turns.score_turns(eng, rec, policy=turns.TurnPolicy(100), window=16000)  # no CPU fallback
    ts = turns.TurnScorer(_bare(3), policy=turns.TurnPolicy(25))
    with pytest.raises(AfxError):
        ts.flush()  # on the GPU only
    with pytest.raises(AfxError):
        ts.flush([1])
    for bad in ([3], [0, 0], [-1]):
        with pytest.raises((ValueError, IndexError)):
            ts.flush(bad)
    with pytest.raises(ValueError):
        turns.TurnPolicy(25).cut_reference(np.ones(30, dtype=np.uint8), 24)  # max_frames below min_frames


def test_the_abi_has_the_three_entry_points(built):
    from afx import turns
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afx.h")).read(), flags=re.S)
    so = ctypes.CDLL(built.LIB_PATH)
    for name, args in (("afx_k_turn_scan", 12), ("afx_k_turn_clips", 10), ("afx_k_turn_close", 9)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(so, name) and name in built.SIGNATURES and len(built.SIGNATURES[name][1]) == args
    assert turns.SCAN_STEP == 4096
    src = open(os.path.join(ROOT, "real-time-deepfake-speech-detection_amd", "csrc", "afx_gate.hip")).read()
    assert re.search(r"TURN_SCAN_STEP\s*=\s*256\s*\*\s*TURN_SCAN_LANE", src) and re.search(r"TURN_SCAN_LANE\s*=\s*16\b", src)

"""Turns offline and the end of a call on the GPU (afx/turns.py ``score_turns`` and ``TurnScorer.flush``; afx_k_turn_scan,
afx_k_turn_clips, afx_k_turn_close).  Every comparison is exact, on bits or integers: the scan against ``cut_reference`` over
constructed masks, the clips against ``np.resize``, the close step against ``close_reference``, ``score_turns`` against the
references and the engine's own forward of each clip, and against a ``TurnScorer`` pushed hop by hop and then flushed."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_turns import _tap
from test_gpu_vad import _engine, _same_bits, fixture_stream
from test_gpu_vad_tone import call_stream

pytestmark = pytest.mark.gpu

H, W, LEAST, TOP, FRAME = 4000, 16000, 25, 100, 160
FIX = fixture_stream()
RECS = [FIX, FIX[:72000], FIX[:68000], np.zeros(8000, dtype=np.float32)]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- 1. afx_k_turn_scan against cut_reference ------------------------------------------------------------------------------------
def _scan_rows(least, top):
    """Seven rows of mask bytes that together hold every case the test names (checked on the reference by the test)."""
    from afx.turns import SCAN_STEP as STEP
    g = np.random.default_rng(7 * least + top)
    long = (g.random(2 * STEP + 38) < 0.2).astype(np.uint8)
    long[STEP - top - 1:STEP + 5] = [0] + [1] * (top + 4) + [0]                     # a cut that ends on the step boundary; the run goes on
    long[2 * STEP - 4:2 * STEP + least + 1] = [0] + [1] * (least + 3) + [0]       # a run across the second boundary
    long[-least - 1:] = [0] + [1] * least                                           # a scored run that ends on the last frame
    short_end = np.array([0, 1, 0] + [1] * max(least - 1, 0), dtype=np.uint8)      # a short run that ends on the last frame
    empty = np.zeros(0, dtype=np.uint8)
    zeros = np.array([0, 2, 0xFE, 0] * 12 + [2, 0xFE], dtype=np.uint8)              # not kept: bit 0 is clear
    full = np.array([1, 3] * (3 * top + 1), dtype=np.uint8)[:3 * top + 1]          # all kept
    cuts = np.array([0] * 3 + [1] * (top + least - 1) + [0] + [1] * top + [0, 0] + [3] * (top + least) + [0xFE], dtype=np.uint8)
    noisy = (g.random(1000) < 0.9).astype(np.uint8) | (g.integers(0, 128, 1000).astype(np.uint8) << 1)
    return [long, short_end, empty, zeros, full, cuts, noisy]


def _scan(mask, offs, A, least, top, close_end, table, cap, row_base, totals, still):
    from afx._lib import lib
    rc = lib().afx_k_turn_scan(_p(mask), _p(offs), A, least, top, close_end, _p(table), cap, _p(row_base), _p(totals), _p(still), None)
    torch.cuda.synchronize()
    return rc


def _scan_want(policy, rows, top, close_end):
    table, base, totals, still = [], [0], [], []
    for i, m in enumerate(rows):
        turns, tot, op = policy.cut_reference(m, top, close_end=bool(close_end))
        table += [[i, t["first"], t["end"], int(t["cut"]) | 2 * int(t["at_end"])] for t in turns]
        base.append(len(table))
        totals.append(list(tot))
        still.append(list(op))
    return table, base, totals, still


def _case_set(least, top, lead):
    """The rows of ``_scan_rows``, after asserting on the reference that they hold every case the test names (a row alone
    or first in the buffer begins on a 16-byte boundary, or ``lead`` bytes behind one)."""
    from afx.turns import SCAN_STEP as STEP
    from afx.turns import TurnPolicy
    policy, rows = TurnPolicy(least), _scan_rows(least, top)
    long, short_end, empty, zeros, full, cuts, noisy = rows
    ref = [policy.cut_reference(m, top) for m in rows]
    opened = [policy.cut_reference(m, top, close_end=False) for m in rows]
    assert long[STEP - 1] & long[STEP] & 1 and long[2 * STEP - 1] & long[2 * STEP] & 1            # runs across step boundaries
    assert any(t["cut"] and t["end"] == STEP for t in ref[0][0])                                  # a cut exactly on the boundary
    assert long.size > 2 * STEP + 1
    assert ref[0][0][-1]["end"] == long.size and (ref[0][0][-1]["at_end"] or least == top)       # a scored run ends the row
    assert opened[0][2] == ((long.size - least, least) if least < top else (-1, 0)) and len(opened[0][0]) == len(ref[0][0]) - (least < top)
    if least > 1:  # (with min_frames 1 no turn is short)
        assert ref[1][1][1] == opened[1][1][1] + 1 == 2 and opened[1][2] == (3, least - 1)      # a short run ends the row
        c = [t for t in ref[5][0]]
        assert c[0]["cut"] and c[1]["first"] != c[0]["end"] and ref[5][1][1] >= 1                # a cut whose remainder is short
    assert any(a["cut"] and cuts[a["end"]] & 1 == 0 for a in ref[5][0])                           # a cut followed by a gap
    assert empty.size == 0 and rows[1].size and rows[3].size                                      # an empty row between non-empty rows
    assert zeros.any() and ref[3][1] == (0, 0, 0, 0) and {2, 0xFE} <= set(zeros.tolist())          # an all-zero row of bytes 2 and 0xFE
    assert full.size == 3 * top + 1 and ref[4][1][3] == full.size and 3 in full.tolist()         # an all-kept row of 3 max + 1 frames
    assert ref[4][1][:3] == ((4, 0, 4) if top == 1 else (4, 0, 3) if least == 1 else (3, 1, 3))
    starts = np.concatenate([[0], np.cumsum([m.size for m in rows])])
    assert starts[1] % 16 and lead % 16 and (lead + starts[1]) % 16                              # rows whose offset is no multiple of 16
    return policy, rows


@pytest.mark.parametrize("A", [1, 7])
@pytest.mark.parametrize("least,top", [(4, 8), (5, 7), (25, 100), (1, 1)])
def test_scan_kernel_equals_cut_reference(least, top, A):
    lead = 5
    policy, rows = _case_set(least, top, lead)  # (asserted on the reference, before anything is compared)
    for close_end in (1, 0):
        groups = [rows] if A == 7 else [[m] for m in rows]
        for gi, group in enumerate(groups):
            for shift in (0, lead):  # the first row begins on a 16-byte boundary (its steps are the reference's) and off one
                n = [m.size for m in group]
                buf = torch.full((shift + sum(n) + 16,), 1, dtype=torch.uint8)  # (kept bytes around the rows: they are not read as frames)
                buf[shift:shift + sum(n)] = torch.from_numpy(np.concatenate(group))
                mask = buf.cuda()
                offs = torch.tensor(shift + np.concatenate([[0], np.cumsum(n)]), dtype=torch.int64).cuda()
                assert mask.data_ptr() % 16 == 0
                want_table, want_base, want_totals, want_open = _scan_want(policy, group, top, close_end)
                R = len(want_table)
                outs = lambda cap: (torch.full((max(cap, 1), 4), -7, dtype=torch.int32, device="cuda"),  # noqa: E731
                                    torch.full((A + 1,), -7, dtype=torch.int32, device="cuda"),
                                    torch.full((A, 4), -7, dtype=torch.int32, device="cuda"),
                                    torch.full((A, 2), -7, dtype=torch.int32, device="cuda"))
                cap = R + 3
                table, row_base, totals, still = outs(cap)
                assert _scan(mask, offs, A, least, top, close_end, table, cap, row_base, totals, still) == 0
                where = (close_end, gi, shift)
                assert row_base.tolist() == want_base, where
                assert totals.tolist() == want_totals, where
                assert still.tolist() == want_open, where
                assert table[:R].tolist() == want_table, where
                assert (table[R:] == -7).all(), where  # the rows beyond R are untouched
                if R:  # a table one row too small: true counts, a right prefix, nothing beyond it written
                    table, row_base, totals, still = outs(R + 2)
                    assert _scan(mask, offs, A, least, top, close_end, table, R - 1, row_base, totals, still) == 0
                    assert row_base.tolist() == want_base and totals.tolist() == want_totals and still.tolist() == want_open, where
                    assert table[:R - 1].tolist() == want_table[:R - 1] and (table[R - 1:] == -7).all(), where


def test_scan_kernel_refuses_bad_arguments_with_nothing_launched():
    from afx._lib import lib
    mask = torch.ones(64, dtype=torch.uint8, device="cuda")
    offs = torch.tensor([0, 40, 64], dtype=torch.int64).cuda()
    table, row_base = torch.full((8, 4), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int32, device="cuda")
    totals, still = torch.full((2, 4), -7, dtype=torch.int32, device="cuda"), torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    ok = dict(mask=mask, offs=offs, A=2, least=4, top=8, close_end=1, table=table, cap=8, row_base=row_base, totals=totals, still=still)
    for bad in (dict(A=0), dict(A=65536), dict(least=0), dict(least=9), dict(cap=-1), dict(mask=None), dict(offs=None), dict(table=None),
                dict(row_base=None), dict(totals=None), dict(still=None)):
        assert _scan(**dict(ok, **bad)) != 0 and b"turn_scan:" in lib().afx_last_error(), bad
        assert all((t == -7).all() for t in (table, row_base, totals, still)), bad
    assert _scan(**dict(ok, cap=0)) == 0  # a table of no rows: the counts alone
    assert row_base.tolist() == [0, 5, 8] and totals.tolist() == [[5, 0, 5, 40], [3, 0, 3, 24]] and (table == -7).all()
    # offsets that decrease: the row is taken as one of no frames
    assert _scan(**dict(ok, offs=torch.tensor([40, 0, 64], dtype=torch.int64).cuda())) == 0
    assert row_base.tolist() == [0, 0, 8] and totals.tolist() == [[0, 0, 0, 0], [8, 0, 8, 64]] and still.tolist() == [[-1, 0], [-1, 0]]


# ---- 2. afx_k_turn_clips against np.resize ----------------------------------------------------------------------------------------
def _clips(x, xoffs, A, frame, top, table, r0, R, out):
    from afx._lib import lib
    rc = lib().afx_k_turn_clips(_p(x), _p(xoffs), A, frame, top, _p(table), r0, R, _p(out), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("frame,top,odd,shift", [(160, 100, False, 0), (6, 7, False, 0), (160, 100, True, 0), (160, 100, False, 1)])
def test_clips_kernel_equals_numpy_resize(frame, top, odd, shift):
    """odd: the second recording begins at an odd sample offset, which takes its turns through the one-sample-per-lane path
    at a frame of 160; shift: the output begins that many floats off a 16-byte boundary, which does the same for every row."""
    from afx._lib import lib
    A, Wn = 3, top * frame
    lens = [(2 * top + 3) * frame + (1 if odd else 0), (top + 5) * frame, 4 * frame]
    g = torch.Generator().manual_seed(frame + top)
    x = torch.randn(sum(lens), generator=g)
    xo = np.concatenate([[0], np.cumsum(lens)])
    assert (xo[1] % 2 == 1) == odd
    host, xd, xoffs = x.numpy(), x.cuda(), torch.tensor(xo, dtype=torch.int64).cuda()
    # one frame, the window, a length that does not divide it, a turn that ends with its recording
    rows = [(0, 5, 6, 0), (0, 7, 7 + top, 1), (1, 2, 5, 0), (1, 5, top + 5, 3), (2, 0, 4, 2), (0, top + 3, 2 * top + 3, 1), (1, 0, 3, 0)]
    assert Wn % (3 * frame) and rows[3][2] * frame == lens[1] and rows[4][2] * frame == lens[2]
    table = torch.tensor(rows, dtype=torch.int32).cuda()
    for r0, R in ((0, 7), (0, 1), (2, 5), (3, 2), (6, 1)):
        flat = torch.full((R * Wn + 4,), -3.0, device="cuda")
        out = flat[shift:shift + R * Wn].view(R, Wn)
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        assert _clips(xd, xoffs, A, frame, top, table, r0, R, out) == 0
        want = np.stack([np.resize(host[xo[i] + a * frame:xo[i] + b * frame], Wn) for i, a, b, _ in rows[r0:r0 + R]])
        assert out.cpu().numpy().tobytes() == want.tobytes(), (r0, R)
        assert flat[:shift].tolist() == [-3.0] * shift and flat[shift + R * Wn:].tolist() == [-3.0] * (4 - shift)
    # each kind of bad row leaves its output row as it was: the recording outside [0, A), first < 0, end <= first, a turn
    # longer than the window, a turn that runs past its recording
    past = lens[2] // frame + 1
    bad = [(0, 1, 3, 0), (-1, 1, 3, 0), (A, 1, 3, 0), (0, -1, 2, 0), (0, 3, 3, 0), (0, 4, 3, 0), (0, 0, top + 1, 0), (2, past - 2, past, 0),
           (2, 1, 4, 0)]
    out = torch.full((len(bad), Wn), -3.0, device="cuda")
    assert _clips(xd, xoffs, A, frame, top, torch.tensor(bad, dtype=torch.int32).cuda(), 0, len(bad), out) == 0
    got = out.cpu().numpy()
    assert got[0].tobytes() == np.resize(host[frame:3 * frame], Wn).tobytes()
    assert got[8].tobytes() == np.resize(host[xo[2] + frame:xo[2] + 4 * frame], Wn).tobytes()
    assert (got[1:8] == -3.0).all()
    # bad scalar arguments launch nothing
    ok = dict(x=xd, xoffs=xoffs, A=A, frame=frame, top=top, table=table, r0=0, R=1, out=out)
    for change in (dict(A=0), dict(frame=0), dict(top=0), dict(r0=-1), dict(R=0), dict(R=65536), dict(x=None), dict(xoffs=None),
                   dict(table=None), dict(out=None), dict(top=(1 << 30) // frame + 1)):
        assert _clips(**dict(ok, **change)) != 0 and b"turn_clips:" in lib().afx_last_error(), change
    assert out.cpu().numpy().tobytes() == got.tobytes()


# ---- 3. afx_k_turn_close against close_reference ----------------------------------------------------------------------------------
def test_close_kernel_equals_close_reference():
    from afx._lib import lib
    from afx.turns import TurnPolicy
    least, top, S, big = 4, 8, 8, (1 << 31) - 1
    policy = TurnPolicy(least)
    #        n >= min (both buffers)   0 < n < min       n = 0        saturated counters                       not a turn state
    state = [[0, 4, 10], [1, 7, 20], [0, 3, 30], [1, 1, 40], [1, 0, 50], [0, 5, 60], [1, 2, 70], [2, 3, 80]]
    totals = [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [0, 0, 0, 1], [3, 3, 3, 3], [big, 1, 2, 3], [1, big, 2, 3], [4, 4, 4, 4]]
    st, tot = torch.tensor(state, dtype=torch.int32).cuda(), torch.tensor(totals, dtype=torch.int32).cuda()

    def close(slots, st, tot, A=None, S=S, least=least, top=top, done=None):
        sl = None if slots is None else torch.tensor(slots, dtype=torch.int32).cuda()
        rows = 1 if slots is None else len(slots)
        done = torch.full((rows, 4), -9, dtype=torch.int32, device="cuda") if done is None else done
        rc = lib().afx_k_turn_close(_p(sl), rows if A is None else A, S, least, top, _p(st), _p(tot), _p(done), None)
        torch.cuda.synchronize()
        return rc, done

    named = [6, 0, 8, 5, 2, -1, 4, 1, 7]  # slot 3 is not named; 8 and -1 are out of range; slot 7's state is no turn state
    rc, done = close(named, st, tot)
    assert rc == 0
    want_state, want_totals, want_done = [list(r) for r in state], [list(r) for r in totals], []
    for s in named:
        if not 0 <= s < S or s == 7:
            want_done.append([-1] * 4)
            continue
        after, d = policy.close_reference(dict(open=state[s][0], n=state[s][1], g=state[s][2], totals=tuple(totals[s]), max_frames=top))
        want_state[s], want_totals[s] = [after["open"], after["n"], after["g"]], list(after["totals"])
        want_done.append(list(d))
    assert want_done[1] == [0, 4, 10, 14] and want_done[7] == [1, 7, 20, 27] and want_done[4] == [0] * 4 and want_done[3] == [0, 5, 60, 65]
    assert want_totals[5] == [big, 1, 2, 3] and want_totals[6] == [1, big, 2, 3] and want_totals[2] == [9, 11, 11, 12]
    assert done.tolist() == want_done and st.tolist() == want_state and tot.tolist() == want_totals
    # closed slots have nothing open: a second close changes nothing and completes nothing
    rc, done = close([0, 1, 2, 4], st, tot)
    assert rc == 0 and done.tolist() == [[0] * 4] * 4 and st.tolist() == want_state and tot.tolist() == want_totals
    marks = torch.full((1, 4), -9, dtype=torch.int32, device="cuda")
    for bad in (dict(A=0), dict(A=65536), dict(S=0), dict(least=0), dict(least=top + 1), dict(slots=None), dict(st=None), dict(tot=None)):
        a = dict(dict(slots=[3], st=st, tot=tot, done=marks), **bad)
        assert close(**a)[0] != 0 and b"turn_close:" in lib().afx_last_error(), bad
    assert lib().afx_k_turn_close(_p(st), 1, S, least, top, _p(st), _p(tot), None, None) != 0
    assert (marks == -9).all() and st.tolist() == want_state and tot.tolist() == want_totals


# ---- 4. score_turns on the fixture -----------------------------------------------------------------------------------------------
_CACHE = {}


def _gate(name="SpeechGate"):
    from afx import vad
    if name not in _CACHE:
        _CACHE[name] = getattr(vad, name)()
    return _CACHE[name]


def _fixture_reference():
    """Per recording of RECS: (the scored turns of ``cut_reference`` on the reference gate's mask, totals), computed once."""
    from afx.turns import TurnPolicy
    if "ref" not in _CACHE:
        _CACHE["ref"] = [TurnPolicy(LEAST).cut_reference(_gate().gate_reference(x[:x.size // FRAME * FRAME])[0], TOP)[:2] for x in RECS]
    return _CACHE["ref"]


def _scored(**kw):
    """``score_turns`` of RECS with the test's engine, computed once per argument set."""
    from afx.turns import TurnPolicy, score_turns
    key = ("scored",) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        recs = [torch.from_numpy(x).cuda() if i % 2 else torch.from_numpy(x) for i, x in enumerate(RECS)]  # on the GPU and on the host
        _CACHE[key] = score_turns(_engine("fp16")[0], recs, _gate(), TurnPolicy(LEAST), window=W, **kw)
    return _CACHE[key]


def _spans(turns):
    return [(int(s), int(e), bool(c), bool(a)) for s, e, c, a in zip(turns.starts.tolist(), turns.ends.tolist(), turns.cut.tolist(),
                                                                     turns.at_end.tolist())]


def test_score_turns_on_the_fixture():
    from afx.turns import TurnPolicy, Turns
    ref = _fixture_reference()
    # what the fixture holds (asserted on the reference, before anything is compared)
    full, tot = ref[0]
    assert [(t["first"], t["end"]) for t in full if t["cut"]] == [(50, 150), (300, 400), (400, 500)]
    assert [(t["first"], t["end"]) for t in full if not t["cut"]] == [(200, 235), (750, 800)] and full[-1]["at_end"] and tot[1] == 2
    assert ref[1][0][-1] == dict(first=400, end=450, cut=False, at_end=True) and ref[2][0][-1] == dict(first=400, end=425, cut=False, at_end=True)
    assert ref[3] == ([], (0, 0, 0, 0))
    got = _scored()
    assert len(got) == 4 and all(isinstance(t, Turns) and t.sample_rate == 16000 for t in got) and len(got[3]) == 0
    eng = _engine("fp16")[0]
    for i, (turns, (want, totals)) in enumerate(zip(got, ref)):
        assert _spans(turns) == [(t["first"] * FRAME, t["end"] * FRAME, t["cut"], t["at_end"]) for t in want], i
        assert turns.totals == dict(scored=totals[0], short=totals[1], cut=totals[2], kept_frames=totals[3], open_frames=0), i
        assert turns.scores.dtype == torch.float32 and not turns.scores.is_cuda and turns.starts.dtype == torch.float64
        for j, t in enumerate(want):  # the score: the engine's own forward of the clip alone
            clip = torch.from_numpy(TurnPolicy.clip_reference(RECS[i][t["first"] * FRAME:t["end"] * FRAME], W)).cuda()
            assert torch.equal(turns.scores[j], eng.forward(clip[None].contiguous())[0, 1].float().cpu()), (i, j)
    for kw in (dict(batch=2), dict(batch=64)):  # the batch changes no bit
        again = _scored(**kw)
        assert all(_spans(a) == _spans(b) and _same_bits(a.scores, b.scores) for a, b in zip(again, got)), kw
    still_open = _scored(close_end=False)  # exactly the at_end turns go, and are reported as open
    for i, (a, b) in enumerate(zip(still_open, got)):
        keep = ~b.at_end
        assert _spans(a) == [s for s in _spans(b) if not s[3]] and _same_bits(a.scores, b.scores[keep]), i
        assert a.totals["open_frames"] == [50, 50, 25, 0][i] and a.totals["scored"] == b.totals["scored"] - int(b.at_end.sum())


# ---- 5. streamed, then flushed -----------------------------------------------------------------------------------------------------
def _sliding(S):
    from afx.streaming import SlidingWindowScorer
    eng, sd = _engine("fp16")
    return SlidingWindowScorer(eng, S, window=W, hop=W, state_dict=sd)


def test_a_stream_pushed_hop_by_hop_and_flushed_equals_score_turns():
    from afx.turns import TurnPolicy, TurnScorer
    S = 3
    ts = TurnScorer(_sliding(S), _gate(), TurnPolicy(LEAST), hop=H)
    streams = [torch.from_numpy(x).cuda() for x in RECS[:S]]
    assert all(x.numel() % H == 0 for x in streams)
    scores, spans = [[] for _ in range(S)], [[] for _ in range(S)]

    def collect(named, out):
        for s, v, e, span in zip(named, out, ts.emitted(out).tolist(), ts.last_turn.tolist()):
            assert (span != [-1, -1]) == e
            if e:
                scores[s].append(v.clone().cpu())
                spans[s].append(tuple(span))

    for t in range(max(x.numel() for x in streams) // H):
        named = [s for s in ([0, 1, 2] if t % 2 else [2, 1, 0]) if (t + 1) * H <= streams[s].numel()]  # finished slots are no longer named
        collect(named, ts.push(torch.stack([streams[s][t * H:(t + 1) * H] for s in named]), named))
    seen = ts.samples_seen.tolist()
    gate_state = [ts.nf.clone(), ts.h.clone()]
    before = ts.stats()
    assert before["open_frames"].tolist() == [50, 50, 25]
    out = ts.flush([1, 0, 2])
    assert out.shape == (3,) and out.dtype == torch.float32 and out.is_cuda and ts.emitted(out).all()
    collect([1, 0, 2], out)
    want = _scored()
    for s in range(S):
        assert spans[s] == [(a, b) for a, b, _, _ in _spans(want[s])], s
        assert _same_bits(torch.stack(scores[s]), want[s].scores), s
        assert ts.turn_totals[s].tolist() == [want[s].totals[k] for k in ("scored", "short", "cut", "kept_frames")], s
    # the gate and the sample counts did not move; nothing is open, in the state and in an export
    assert ts.samples_seen.tolist() == seen and _same_bits(ts.nf, gate_state[0]) and torch.equal(ts.h, gate_state[1])
    assert ts.stats()["open_frames"].tolist() == [0, 0, 0]
    assert ts.export_slots([0, 1, 2]).tensors["turn_frames"].tolist() == [0, 0, 0]
    # a second flush returns NaN and moves nothing
    snap = [ts.turn_state.clone(), ts.turn_totals.clone(), ts.scorer.samples_seen.clone(), ts.bufs.clone()]
    again = ts.flush()
    assert again.shape == (3,) and torch.isnan(again).all() and ts.last_turn.tolist() == [[-1, -1]] * 3
    assert torch.equal(ts.turn_state, snap[0]) and torch.equal(ts.turn_totals, snap[1]) and torch.equal(ts.scorer.samples_seen, snap[2])
    assert _same_bits(ts.bufs, snap[3]) and ts.samples_seen.tolist() == seen
    assert ts.flush([]).shape == (0,) and ts.last_turn.shape == (0, 2)


def test_a_slot_flushed_mid_run_and_pushed_on_equals_the_mirror():
    from afx.turns import TurnPolicy, TurnScorer
    S, policy, gate = 3, TurnPolicy(LEAST), _gate()
    tap = _tap(S)
    ts = TurnScorer(tap, gate, policy, hop=H)
    host = [np.roll(FIX, -o) for o in (0, 1600, 30057)]
    x = [torch.from_numpy(h.copy()).cuda() for h in host]
    keep = [gate.gate_reference(h)[0].astype(np.uint8) for h in host]
    F = H // FRAME
    mirror, want = [policy.new_state(TOP) for _ in range(S)], [[] for _ in range(S)]
    # slot 1 with a short turn open; slot 2 with none and slot 1 inside a turn that is scored; every slot, two with nothing open
    flush_at = {11: [1], 13: [2, 1], 19: [0, 1, 2]}
    flushed_open = []
    for t in range(FIX.size // H):
        named = [0, 1, 2] if t % 2 else [1, 2, 0]
        out = ts.push(torch.stack([x[s][t * H:(t + 1) * H] for s in named]), named)
        for i, s in enumerate(named):
            mirror[s], done = policy.step_reference(mirror[s], keep[s][t * F:(t + 1) * F], t * F)
            assert bool(done[1]) == bool(ts.emitted(out)[i])
            if done[1]:
                want[s].append((done[2], done[3]))
        if t in flush_at:
            named = flush_at[t]
            flushed_open.append([mirror[s]["n"] for s in named])
            out = ts.flush(named)
            for i, s in enumerate(named):
                mirror[s], done = policy.close_reference(mirror[s])
                assert bool(done[1]) == bool(ts.emitted(out)[i]), (t, s)
                assert ts.last_turn[i].tolist() == ([done[2] * FRAME, done[3] * FRAME] if done[1] else [-1, -1]), (t, s)
                if done[1]:
                    want[s].append((done[2], done[3]))
        assert ts.turn_state.tolist() == [[m["open"], m["n"], m["g"]] for m in mirror], t
        assert ts.turn_totals.tolist() == [list(m["totals"]) for m in mirror], t
    assert flushed_open == [[10], [0, 50], [0, 50, 0]]  # (the mirror's open frames at each flush: the cases named above)
    assert (300, 350) in want[1] and (350, 450) in want[1] and mirror[1]["totals"][1] > policy.cut_reference(keep[1], TOP)[1][1]
    for s in range(S):  # every clip the inner scorer was pushed: the turn's samples from the source, tiled
        assert len(tap.got[s]) == len(want[s]) >= 4
        for clip, (a, b) in zip(tap.got[s], want[s]):
            assert clip.cpu().numpy().tobytes() == np.resize(host[s][a * FRAME:b * FRAME], W).tobytes(), (s, a, b)


# ---- 6. the tone gate, another sample rate, the file ------------------------------------------------------------------------------
def test_score_turns_with_a_tone_gate_equals_turns_reference():
    from afx.turns import TurnPolicy, score_turns
    from afx.vad import ToneGate
    gate, policy = ToneGate(), TurnPolicy(LEAST)
    x = np.concatenate([call_stream(3), np.zeros(4000, dtype=np.float32), call_stream(5)[8000:]])
    want, totals, still = policy.turns_reference(x, gate, TOP)
    plain = policy.turns_reference(x, _gate(), TOP)
    assert [(t["first"], t["end"]) for t in want] != [(t["first"], t["end"]) for t in plain[0]]  # the tones change the turns
    scored = [t for t in want if t["scored"]]
    assert len(scored) >= 2 and any(t["cut"] for t in scored)
    eng = _engine("fp16")[0]
    got = score_turns(eng, [torch.from_numpy(x).cuda()], gate, policy, window=W, close_end=False)[0]
    assert _spans(got) == [(t["first"] * FRAME, t["end"] * FRAME, t["cut"], False) for t in scored]
    assert got.totals == dict(scored=totals[0], short=totals[1], cut=totals[2], kept_frames=totals[3], open_frames=still[1] if still else 0)
    for j, t in enumerate(scored):
        clip = torch.from_numpy(policy.clip_reference(t["audio"], W)).cuda()
        assert torch.equal(got.scores[j], eng.forward(clip[None].contiguous())[0, 1].float().cpu()), j
    closed = score_turns(eng, [torch.from_numpy(x).cuda()], gate, policy, window=W)[0]
    ref = policy.cut_reference(gate.gate_reference(x)[0], TOP)
    assert _spans(closed) == [(t["first"] * FRAME, t["end"] * FRAME, t["cut"], t["at_end"]) for t in ref[0]]


def test_score_turns_at_another_sample_rate():
    from afx.resample import Resampler
    from afx.turns import TurnPolicy, score_turns
    eng, policy = _engine("fp16")[0], TurnPolicy(LEAST)
    recs = [torch.from_numpy(FIX[::2][:36000].copy()), torch.from_numpy(FIX[40000:104001:2].copy()).cuda()]  # "8 kHz" by plain slicing
    rs = Resampler(8000)
    want = score_turns(eng, rs.clips([r.cuda() for r in recs]), _gate(), policy, window=W)
    got = score_turns(eng, recs, _gate(), policy, window=W, sample_rate=8000)
    assert sum(len(t) for t in want) >= 3 and rs.delay > 0
    for a, b in zip(got, want):
        assert a.sample_rate == 8000 and b.sample_rate == 16000 and _same_bits(a.scores, b.scores)
        assert torch.equal(a.cut, b.cut) and torch.equal(a.at_end, b.at_end) and a.totals == b.totals
        assert torch.equal(a.starts, (b.starts - rs.delay).clamp(min=0) * 0.5) and torch.equal(a.ends, (b.ends - rs.delay).clamp(min=0) * 0.5)


def test_turns_file_from_dataset(tmp_path):
    from afx import harness
    from afx.turns import TurnPolicy
    eng = _engine("fp16")[0]
    recs = [torch.from_numpy(x) for x in (RECS[1], RECS[3], RECS[2])]

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(recs)

        def __getitem__(self, i):
            return f"utt{i}", recs[i], 0

    path = tmp_path / "turns.txt"
    names, turns = harness.produce_turns_file(DS(), eng, "cuda", str(path), gate=_gate(), policy=TurnPolicy(LEAST), window=W,
                                              batch_size=2, num_workers=0)
    ref = _scored()
    assert names == ["utt0", "utt1", "utt2"] and [len(t) for t in turns] == [4, 0, 4]
    want = []
    for name, t in (("utt0", ref[1]), ("utt2", ref[2])):
        want += ["{} {:.3f} {:.3f} {}".format(name, s / 16000, e / 16000, v) for s, e, v in zip(t.starts.tolist(), t.ends.tolist(), t.scores.tolist())]
    assert path.read_text().splitlines() == want and want[0].startswith("utt0 0.500 1.500 ") and want[-1].startswith("utt2 4.000 4.250 ")

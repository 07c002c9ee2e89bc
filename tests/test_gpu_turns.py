"""Talk spurts on the GPU (afx/turns.py, afx_k_turn / afx_k_turn_collect).  Every comparison is exact, on bits or integers:
``afx_k_turn`` against ``TurnPolicy.step_reference`` launch by launch over constructed masks, ``afx_k_turn_collect`` against
``np.resize``, ``TurnScorer`` streamed against ``turns_reference`` with a tap for the inner scorer, its scores against a
fresh scorer and the engine's own forward of the reference clips, the composition with the verdict layer and the packet
front, and sessions moved between scorers."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from test_gpu_vad import _engine, _mulaw_encode, _same_bits, fixture_stream

pytestmark = pytest.mark.gpu

H, W, LEAST, TOP, FRAME = 4000, 16000, 25, 100, 160
OFFSETS = (0, 30057, 44000)
FIX = fixture_stream()


# ---- 1. afx_k_turn against step_reference ------------------------------------------------------------------------------------
def _programs(F, least, top):
    """Five mask streams (0 / 1 per frame) that together hold every case the test names; L = least is a natural length."""
    L = least

    class Stream(list):
        def gap_to(self, m):  # at least one non-kept frame, up to position m of a push
            self.append(0)
            while len(self) % F != m % F:
                self.append(0)
            return self

        def run(self, k):
            self.extend([1] * k)
            return self

        def gap(self):
            self.append(0)
            return self

    s0 = Stream().gap_to(-L).run(L).gap()         # closed by the first frame of a push
    s0.gap_to(F - 1 - L).run(L).gap()             # closed by the last frame of a push
    s1 = Stream().gap_to(F - top).run(top).gap()  # a cut on the last frame of a push, and the next frame is not kept
    s1.gap_to(1).run(top + least).gap()           # a cut whose remainder is scored
    s2 = Stream().gap().run(least - 1).gap()      # a short turn dropped
    s2.run(top + 1).gap().run(L).gap()            # a cut whose remainder is dropped as short
    s3 = Stream().gap_to(1 - L).run(L).gap().run(L).gap()      # a close at frame 1 of a push, a new turn open behind it
    s4 = Stream().gap_to(1 - L).run(L).gap().run(1).gap()      # two closes in one push, the second short
    s4.run(L).gap()
    return [list(s) for s in (s0, s1, s2, s3, s4)]


def _turn_cases(frame, F, least, top, seed):
    """-> (launches, seen): per launch (slots, wpos, g0, masks (A, F)); ``seen`` says which cases the reference shows."""
    from afx.turns import TurnPolicy
    S, policy = 5, TurnPolicy(least)
    ring_len = (F + 2) * frame
    rng = np.random.default_rng(seed)
    prog = [np.array(p + [0] * (-len(p) % F + F), dtype=np.uint8).reshape(-1, F) for p in _programs(F, least, top)]
    prog = [np.concatenate([p, np.zeros((max(0, 12 - len(p)), F), dtype=np.uint8)]) for p in prog]
    at, launches, it = [0] * S, [], 0
    state = [policy.new_state(top) for _ in range(S)]
    seen = dict(first=False, last=False, cut_last=False, cut_then_gap=False, short=False, reopened=False, two=False,
                wrap_vec=False, wrap_scalar=False, open=[set() for _ in range(S)], sizes=set())
    while any(a < len(p) for a, p in zip(at, prog)):
        size = (5, 1, 2, 3, 4)[it % 5]
        slots = rng.permutation(S)[:size].tolist()
        masks, wpos, g0 = [], [], []
        for i, s in enumerate(slots):
            m = prog[s][at[s]] if at[s] < len(prog[s]) else np.zeros(F, dtype=np.uint8)
            kind = (it + i) % 4
            w = [0, 4 * int(rng.integers(0, ring_len // 4)), int(rng.integers(0, ring_len)), ring_len - 4 * (frame // 4)][kind]
            w = ring_len - frame + 1 if kind == 2 and it % 3 == 0 else w
            before = state[s]
            state[s], done = policy.step_reference(before, m, at[s] * F)
            tb, ta = before["totals"], state[s]["totals"]
            k = int(m.sum())
            seen["first"] |= bool(done[1]) and done[3] == at[s] * F and not m[0] and done[1] < top
            seen["last"] |= bool(done[1]) and done[3] == at[s] * F + F - 1 and done[1] < top
            seen["cut_last"] |= bool(done[1]) and done[1] == top and done[3] == (at[s] + 1) * F
            nxt = prog[s][at[s] + 1][0] if at[s] + 1 < len(prog[s]) else 0
            seen["cut_then_gap"] |= done[1] == top and (nxt == 0 if done[3] == (at[s] + 1) * F else m[done[3] - at[s] * F] == 0)
            seen["short"] |= ta[1] > tb[1]
            seen["reopened"] |= bool(done[1]) and state[s]["n"] > 0
            seen["two"] |= ta[0] > tb[0] and ta[1] > tb[1]
            if k and w + k * frame > ring_len:
                seen["wrap_vec" if w % 4 == 0 and frame % 4 == 0 else "wrap_scalar"] = True
            seen["open"][s].add(state[s]["open"])
            masks.append(m), wpos.append(w), g0.append(at[s] * F)
            at[s] += 1
        seen["sizes"].add(size)
        launches.append((slots, wpos, g0, np.stack(masks)))
        it += 1
    return launches, seen, ring_len


SHAPES = [(160, 25, 25, 100), (8, 4, 4, 8), (6, 5, 5, 7), (160, 512, 512, 600)]


def _turn(staging, ring_len, mask, hdr, A, F, frame, least, top, bufs, state, totals, done, S=5):
    from afx._lib import lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib().afx_k_turn(p(staging), S, ring_len, p(mask), p(hdr), A, F, frame, least, top, p(bufs), p(state), p(totals), p(done),
                          None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("frame,F,least,top", SHAPES)
def test_turn_kernel_equals_the_reference_launch_by_launch(frame, F, least, top):
    from afx.turns import TurnPolicy
    S, policy = 5, TurnPolicy(least)
    launches, seen, ring_len = _turn_cases(frame, F, least, top, seed=F + top)
    # the case set holds every case (asserted on the reference, before anything is compared)
    for case in ("first", "last", "cut_last", "cut_then_gap", "short", "reopened", "two"):
        assert seen[case], case
    assert seen["wrap_scalar"] and (seen["wrap_vec"] or frame % 4), seen
    assert all(o == {0, 1} for o in seen["open"]) and seen["sizes"] == {1, 2, 3, 4, 5} and len(launches) >= 12

    g = torch.Generator().manual_seed(frame + F)
    pattern = -1.0 - (torch.arange(S * 2 * top * frame) % 977).float().reshape(S, 2, top, frame)
    bufs, m_bufs = pattern.cuda(), pattern.numpy().copy()
    state = torch.zeros(S, 3, dtype=torch.int32, device="cuda")
    totals = torch.zeros(S, 4, dtype=torch.int32, device="cuda")
    mirror = [policy.new_state(top) for _ in range(S)]
    for it, (slots, wpos, g0, masks) in enumerate(launches):
        A = len(slots)
        ring = torch.randn(S, ring_len, generator=g)
        want = []
        for i, s in enumerate(slots):
            k = int(masks[i].sum())
            cols = (wpos[i] + np.arange(k * frame)) % ring_len
            mirror[s], done = policy.step_reference(mirror[s], masks[i], g0[i], ring[s].numpy()[cols].reshape(k, frame), m_bufs[s])
            want.append(done)
        before = bufs.clone()
        done = torch.full((A, 4), -9, dtype=torch.int32, device="cuda")
        hdr = torch.tensor(list(zip(slots, wpos, g0)), dtype=torch.int32).cuda()
        rc = _turn(ring.cuda(), ring_len, torch.from_numpy(masks).cuda(), hdr, A, F, frame, least, top, bufs, state, totals, done)
        assert rc == 0
        assert done.tolist() == [list(d) for d in want], (it, slots)
        assert state.tolist() == [[m["open"], m["n"], m["g"]] for m in mirror], (it, slots)
        assert totals.tolist() == [list(m["totals"]) for m in mirror], (it, slots)
        got = bufs.cpu().numpy()
        for i, s in enumerate(slots):
            o, n = mirror[s]["open"], mirror[s]["n"]
            assert got[s, o, :n].tobytes() == m_bufs[s, o, :n].tobytes(), (it, s, "the open turn")
            if want[i][1]:
                b, n = want[i][0], want[i][1]
                assert got[s, b, :n].tobytes() == m_bufs[s, b, :n].tobytes(), (it, s, "the completed turn")
        rest = [s for s in range(S) if s not in slots]
        assert _same_bits(bufs[rest], before[rest]), (it, "the buffers of the slots not named")


def test_turn_kernel_skips_bad_rows_whole_and_bad_arguments_launch_nothing():
    from afx._lib import lib
    from afx.turns import TurnPolicy
    frame, F, least, top, S = 8, 4, 4, 8, 3
    ring_len, policy = 6 * frame, TurnPolicy(least)
    g = torch.Generator().manual_seed(3)
    ring = torch.randn(S, ring_len, generator=g)
    bufs = torch.randn(S, 2, top, frame, generator=g).cuda()
    state = torch.tensor([[0, 3, 5], [1, 2, 9], [0, 0, 0]], dtype=torch.int32).cuda()
    totals = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8], [0, 0, 0, 0]], dtype=torch.int32).cuda()
    snap = lambda: [bufs.clone(), state.clone(), totals.clone()]  # noqa: E731
    same = lambda a, b: all(_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b))  # noqa: E731
    mask = torch.tensor([[1, 1, 0, 1]] * 8, dtype=torch.uint8).cuda()
    last = (1 << 31) - 1 - F  # the largest g0 that is taken: g0 + F = 2^31 - 1
    # slot outside [0, S), wpos outside the ring, g0 negative or g0 + F = 2^31: skipped; rows 2 (slot 1) and 6 (slot 2) are taken
    rows = [(-1, 0, 8), (3, 0, 8), (1, 8, 11), (0, -1, 8), (0, ring_len, 8), (0, 0, -1), (2, 4, last)]
    done = torch.full((8, 4), -9, dtype=torch.int32, device="cuda")
    before = snap()
    rc = _turn(ring.cuda(), ring_len, mask, torch.tensor(rows + [(0, 0, last + 1)], dtype=torch.int32).cuda(), 8, F, frame, least, top,
               bufs, state, totals, done, S=S)
    assert rc == 0
    m1, d1 = policy.step_reference(dict(policy.new_state(top), open=1, n=2, g=9, totals=(5, 6, 7, 8)), [1, 1, 0, 1], 11)
    m2, d2 = policy.step_reference(policy.new_state(top), [1, 1, 0, 1], last)
    assert d1 == (1, 4, 9, 13) and d2 == (0, 0, 0, 0) and m2["totals"] == (0, 1, 0, 3) and m2["g"] == last + 3
    skipped = [-1] * 4
    assert done.tolist() == [skipped, skipped, list(d1), skipped, skipped, skipped, list(d2), skipped]
    assert state.tolist() == [[0, 3, 5], [m1["open"], m1["n"], m1["g"]], [m2["open"], m2["n"], m2["g"]]]
    assert totals.tolist() == [[1, 2, 3, 4], list(m1["totals"]), list(m2["totals"])]
    assert _same_bits(bufs[0], before[0][0])  # slot 0 was named by skipped rows only
    assert _same_bits(bufs[1, 1, 2:4], ring[1, 8:8 + 2 * frame].reshape(2, frame)) and _same_bits(bufs[1, 0, 0], ring[1, 24:32])
    # a state that is not a turn state (n = max_frames; open = 2): the row is skipped too
    for bad in ([0, top, 0], [2, 0, 0], [0, -1, 0]):
        state[2] = torch.tensor(bad, dtype=torch.int32)
        before = snap()
        assert _turn(ring.cuda(), ring_len, mask, torch.tensor([(2, 0, 0)], dtype=torch.int32).cuda(), 1, F, frame, least, top, bufs,
                     state, totals, done, S=S) == 0
        assert done[0].tolist() == skipped and same(before, snap())
    # scalar arguments: an error that names the entry point, nothing launched
    hdr = torch.tensor([(1, 0, 0)], dtype=torch.int32).cuda()
    ok = dict(staging=ring.cuda(), ring_len=ring_len, mask=mask, hdr=hdr, A=1, F=F, frame=frame, least=least, top=top, bufs=bufs,
              state=state, totals=totals, done=done, S=S)
    before, marks = snap(), done.clone()
    for bad in (dict(A=0), dict(A=65536), dict(F=0), dict(F=513, least=513, top=600, ring_len=513 * frame), dict(frame=0),
                dict(frame=-8), dict(least=F - 1), dict(least=top + 1), dict(S=0), dict(ring_len=F * frame - 1), dict(staging=None),
                dict(mask=None), dict(hdr=None), dict(bufs=None), dict(state=None), dict(totals=None), dict(done=None)):
        a = dict(ok, **bad)
        assert _turn(**a) != 0 and b"turn:" in lib().afx_last_error(), bad
        assert same(before, snap()) and torch.equal(done, marks), bad


# ---- 2. afx_k_turn_collect against np.resize -------------------------------------------------------------------------------
def _collect(bufs, S, top, frame, rows, out):
    from afx._lib import lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    tab = None if rows is None else torch.tensor(rows, dtype=torch.int32).cuda()
    rc = lib().afx_k_turn_collect(p(bufs), S, top, frame, p(tab), 0 if rows is None else len(rows), p(out), None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("frame,top,odd,shift", [(160, 100, 37, 0), (6, 7, 3, 0), (160, 100, 37, 1), (8, 8, 3, 0)])
def test_collect_kernel_equals_numpy_resize(frame, top, odd, shift):
    """odd: a turn length in frames that does not divide the window; shift: the output begins that many floats off a 16-byte
    boundary, which takes a frame of 160 through the one-sample-per-lane path."""
    from afx._lib import lib
    S, Wn = 4, top * frame
    assert Wn % (odd * frame)
    g = torch.Generator().manual_seed(frame + top)
    bufs = torch.randn(S, 2, Wn, generator=g).cuda()
    host = bufs.cpu().numpy()
    # one frame, the window, a length that does not divide it; both buffers of slot 2; a bad row in the middle
    table = [(2, 0, odd), (2, 1, top), (0, 1, 1), (3, 0, top - 1), (1, 1, odd), (1, 0, 2), (0, 0, top)]
    for R in range(1, 8):
        flat = torch.full((R * Wn + 4,), -3.0, device="cuda")
        out = flat[shift:shift + R * Wn].view(R, Wn)
        assert (out.data_ptr() % 16 == 0) == (shift == 0)
        assert _collect(bufs, S, top, frame, table[:R], out) == 0
        want = np.stack([np.resize(host[s, b, :n * frame], Wn) for s, b, n in table[:R]])
        assert out.cpu().numpy().tobytes() == want.tobytes(), R
        assert flat[:shift].tolist() == [-3.0] * shift and flat[shift + R * Wn:].tolist() == [-3.0] * (4 - shift)
    # bad rows leave their output row as it was
    rows = [(0, 0, 2), (-1, 0, 2), (S, 0, 2), (1, 2, 2), (1, -1, 2), (2, 0, 0), (2, 0, top + 1), (3, 1, 5)]
    out = torch.full((len(rows), Wn), -3.0, device="cuda")
    assert _collect(bufs, S, top, frame, rows, out) == 0
    got = out.cpu().numpy()
    assert got[0].tobytes() == np.resize(host[0, 0, :2 * frame], Wn).tobytes() and got[7].tobytes() == np.resize(host[3, 1, :5 * frame], Wn).tobytes()
    assert (got[1:7] == -3.0).all()
    # bad scalar arguments launch nothing
    for bad in (dict(S=0), dict(top=0), dict(frame=0), dict(rows=[]), dict(rows=None), dict(bufs=None), dict(out=None),
                dict(rows=[(0, 0, 1)] * 65536)):
        a = dict(dict(bufs=bufs, S=S, top=top, frame=frame, rows=[(0, 0, 1)], out=out), **bad)
        assert _collect(**a) != 0 and b"turn_collect:" in lib().afx_last_error(), bad
    assert out.cpu().numpy().tobytes() == got.tobytes()


# ---- 3. streamed against offline ----------------------------------------------------------------------------------------------
def _tap(S):
    from afx.streaming import SlidingWindowScorer

    class Tap(SlidingWindowScorer):
        def __init__(self):
            super().__init__(None, S, window=W, hop=W, device="cuda")
            self.got = [[] for _ in range(S)]

        def push(self, chunk, slots=None):
            idx = self._slot_list(slots, ordered=True)
            assert chunk.is_cuda and chunk.dtype == torch.float32 and chunk.shape == (len(idx), W)
            for i, s in enumerate(idx):
                self.got[s].append(chunk[i].clone())
            self._seen[idx] += W
            return torch.tensor([float(10 * s + 1) for s in idx], device=chunk.device)

    return Tap()


_GATES = {}


def _gate(name):
    from afx import vad
    if name not in _GATES:
        _GATES[name] = getattr(vad, name)()
    return _GATES[name]


_REFS = {}


def _reference(name, offset, begin=0, end=128000):
    """``turns_reference`` of one session of a fixture stream, computed once: (turns, totals, open, the scored turns)."""
    from afx.turns import TurnPolicy
    key = (name, offset, begin, end)
    if key not in _REFS:
        turns, totals, still = TurnPolicy(LEAST).turns_reference(np.roll(FIX, -offset)[begin:end], _gate(name), TOP)
        _REFS[key] = (turns, totals, still, [t for t in turns if t["scored"]])
    return _REFS[key]


def _schedule(ticks=44, reset_at=17):
    """Which slots a tick names, in which order -> (per tick (named, reset slot 2 first?), the sessions (slot, begin, end))."""
    pos, plan, begin = [0, 0, 0], [], 0
    sessions = []
    for t in range(ticks):
        if t == reset_at:
            sessions.append((2, 0, pos[2]))
            begin = pos[2]
        named = [s for s in ([0, 1, 2] if t % 3 else [2, 0, 1]) if not (s == 1 and 10 <= t < 14) and not (s == 0 and t % 7 == 3)
                 and pos[s] + H <= 128000]
        for s in named:
            pos[s] += H
        plan.append((named, t == reset_at))
    return plan, [(0, 0, pos[0]), (1, 0, pos[1]), (2, begin, pos[2])] + sessions


@pytest.mark.parametrize("name", ["SpeechGate", "ToneGate"])
def test_streamed_turns_equal_the_reference(name):
    from afx.turns import TurnPolicy, TurnScorer
    S, gate, policy = 3, _gate(name), TurnPolicy(LEAST)
    for off in OFFSETS:  # each stream shows a natural end, a cut and a short turn
        turns = _reference(name, off)[0]
        assert any(t["scored"] and not t["cut"] for t in turns) and any(t["cut"] for t in turns) and any(not t["scored"] for t in turns)
    plan, sessions = _schedule()
    assert sessions[3][2] % H == 0 and 0 < sessions[3][2] < 128000 and all(e == 128000 for _, _, e in sessions[:2])
    refs = {(s, b): _reference(name, OFFSETS[s], b, e) for s, b, e in sessions}
    closes = {k: {t["close"] // (H // FRAME): t for t in r[3]} for k, r in refs.items()}
    assert sum(len(c) for c in closes.values()) >= 9 and len(closes[(2, 0)]) >= 1 and len(closes[(2, sessions[2][1])]) >= 1
    streams = [np.roll(FIX, -o) for o in OFFSETS]
    tap = _tap(S)
    ts = TurnScorer(tap, gate, policy, hop=H)
    pos, begin, mark, count = [0] * S, [0] * S, 0, 0
    for t, (named, reset) in enumerate(plan):
        if reset:  # slot 2 starts over midway (its stream goes on from where it is)
            first = refs[(2, 0)]
            assert ts.turn_totals[2].tolist() == list(first[1]) and int(ts.turns_scored[2]) == len(first[3])
            assert int(ts.stats()["open_frames"][2]) == (first[2][1] if first[2] else 0)
            ts.reset([2])
            begin[2], mark = pos[2], len(tap.got[2])
            assert ts.turn_totals[2].tolist() == [0] * 4 and ts.samples_seen.tolist()[2] == 0 and int(ts.turns_scored[2]) == 0
        if not named:
            continue
        chunk = torch.from_numpy(np.stack([streams[s][pos[s]:pos[s] + H] for s in named])).cuda()
        whole = len(named) == S and t % 2 == 0
        out = ts.push(chunk[[named.index(s) for s in range(S)]]) if whole else ts.push(chunk, named)
        order = list(range(S)) if whole else named
        assert out.shape == (len(order),) and out.dtype == torch.float32 and out.is_cuda
        want, spans = [], []
        for s in order:
            turn = closes[(s, begin[s])].get((pos[s] - begin[s]) // H)
            want.append(turn is not None)
            spans.append([turn["first"] * FRAME, turn["end"] * FRAME] if turn else [-1, -1])
            pos[s] += H
        assert ts.emitted(out).tolist() == want, t  # NaN exactly where the reference completes no turn
        assert out[ts.emitted(out)].tolist() == [float(10 * s + 1) for s, w in zip(order, want) if w]
        assert ts.last_turn.dtype == torch.int64 and ts.last_turn.is_cuda and ts.last_turn.tolist() == spans, t
        assert ts.samples_seen.tolist() == [p - b for p, b in zip(pos, begin)]
        count += sum(want)
    assert count == sum(len(c) for c in closes.values()) and pos[:2] == [128000, 128000]
    for s in range(S):
        turns, totals, still, scored = refs[(s, begin[s])]
        assert ts.turn_totals[s].tolist() == list(totals) and int(ts.turns_scored[s]) == len(scored), s
        got = tap.got[s][mark:] if s == 2 else tap.got[s]
        assert len(got) == len(scored)
        for clip, turn in zip(got, scored):  # the pushed clips: the reference's turns, tiled
            assert clip.cpu().numpy().tobytes() == policy.clip_reference(turn["audio"], W).tobytes(), (s, turn["first"])
    early = refs[(2, 0)][3]
    assert len(tap.got[2][:mark]) == len(early)
    assert all(c.cpu().numpy().tobytes() == policy.clip_reference(t["audio"], W).tobytes() for c, t in zip(tap.got[2], early))
    stats = ts.stats()
    assert stats["scored"].tolist() == [refs[(s, begin[s])][1][0] for s in range(S)]
    assert stats["open_frames"].tolist() == [refs[(s, begin[s])][2][1] if refs[(s, begin[s])][2] else 0 for s in range(S)]


# ---- 4. scores ---------------------------------------------------------------------------------------------------------------------
def _sliding(S):
    from afx.streaming import SlidingWindowScorer
    eng, sd = _engine("fp16")
    return SlidingWindowScorer(eng, S, window=W, hop=W, state_dict=sd)


def _run(ts, streams, hops, got=None, first=0):
    """Push hops [first, hops) of the streams (slot i = stream i) in varying row orders -> per slot the (hop, score) emitted."""
    got = [[] for _ in streams] if got is None else got
    S = len(streams)
    for t in range(first, hops):
        named = [list(range(S)), list(range(S))[::-1], list(range(1, S)) + [0]][t % 3]
        out = ts.push(torch.stack([streams[s][t * H:(t + 1) * H] for s in named]), named)
        for s, v, e in zip(named, out, ts.emitted(out).tolist()):
            if e:
                got[s].append((t, v.clone()))
    return got


def test_scores_equal_a_fresh_scorer_and_the_engine_on_the_reference_clips():
    from afx.turns import TurnPolicy, TurnScorer
    S, name, policy = 3, "SpeechGate", TurnPolicy(LEAST)
    ts = TurnScorer(_sliding(S), _gate(name), policy, hop=H)
    streams = [torch.from_numpy(np.roll(FIX, -o).copy()).cuda() for o in OFFSETS]
    got = _run(ts, streams, 128000 // H)
    eng, fresh = _engine("fp16")[0], _sliding(S)
    assert sum(len(g) for g in got) >= 9
    for s in range(S):
        scored = _reference(name, OFFSETS[s])[3]
        assert [t for t, _ in got[s]] == [turn["close"] // (H // FRAME) for turn in scored], s
        for (t, v), turn in zip(got[s], scored):
            clip = torch.from_numpy(policy.clip_reference(turn["audio"], W)).cuda()
            assert torch.equal(v.reshape(1), fresh.push(clip[None].contiguous(), [s])), (s, t)
            assert torch.equal(v, eng.forward(clip[None].contiguous())[0, 1]), (s, t)
    assert torch.equal(ts.turns_scored, torch.tensor([len(g) for g in got]))


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------
def test_around_the_verdict_layer_the_hop_index_counts_turns():
    from afx.turns import TurnPolicy, TurnScorer
    from afx.verdict import VerdictPolicy, VerdictScorer, new_state
    S = 3
    plain = _run(TurnScorer(_sliding(S), _gate("SpeechGate"), TurnPolicy(LEAST), hop=H),
                 [torch.from_numpy(np.roll(FIX, -o).copy()).cuda() for o in OFFSETS], 128000 // H)
    scores = sorted(float(v) for g in plain for _, v in g)
    vp = VerdictPolicy(enter=scores[len(scores) // 2] + 1e-6)  # (about half of the turn scores are below it: alarms rise and clear)
    vs = VerdictScorer(_sliding(S), vp)
    ts = TurnScorer(vs, _gate("SpeechGate"), TurnPolicy(LEAST), hop=H)
    got = _run(ts, [torch.from_numpy(np.roll(FIX, -o).copy()).cuda() for o in OFFSETS], 128000 // H)
    for s in range(S):
        assert [t for t, _ in got[s]] == [t for t, _ in plain[s]] and all(torch.equal(a[1], b[1]) for a, b in zip(got[s], plain[s]))
    slot, kind, hop_index, smoothed = vs.take_events()
    m, st = new_state(S)
    want = []
    for t in range(128000 // H):  # the turn scores in push order, hop index = the turn's ordinal in its slot
        rows = [(s, j + 1, v) for s in range(S) for j, (tt, v) in enumerate(got[s]) if tt == t]
        named = [list(range(S)), list(range(S))[::-1], list(range(1, S)) + [0]][t % 3]
        rows.sort(key=lambda r: named.index(r[0]))
        if rows:
            want += vp.step_reference([r[0] for r in rows], np.array([float(r[2]) for r in rows], dtype=np.float32),
                                      [r[1] for r in rows], m, st)
    assert len(want) >= 1 and 1 in {w[1] for w in want}  # (a score below the threshold raises at once)
    assert list(zip(slot.tolist(), kind.tolist(), hop_index.tolist(), smoothed.view(np.int32).tolist())) == want


def test_behind_the_packet_front():
    from afx.ingest import PacketScorer, decode
    from afx.resample import Resampler
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import emitted
    S, gate = 3, _gate("SpeechGate")
    ps = PacketScorer(TurnScorer(_sliding(S), gate, TurnPolicy(LEAST), hop=H), 8000, "mulaw")
    codes = [_mulaw_encode(np.roll(FIX, -o)[::2]) for o in OFFSETS]  # 8 kHz by plain slicing, 8 s each
    got = [[] for _ in range(S)]
    for k in range(0, codes[0].size, 160):  # 20-ms packets
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        res = ps.feed([codes[s][k:k + 160].tobytes() for s in named], named)
        for s, part in zip(named, res.split()):
            got[s] += [v.clone() for v in part[emitted(part)]]
    R = [Resampler(8000)(decode(c, "mulaw")[None])[0] for c in codes]
    hops = int(ps.samples_seen[0]) // H  # (the front counts what the turn scorer was pushed)
    assert hops >= 30 and ps.samples_seen.tolist() == [hops * H] * S and min(r.numel() for r in R) >= hops * H
    want = _run(TurnScorer(_sliding(S), gate, TurnPolicy(LEAST), hop=H), R, hops)
    assert sum(len(w) for w in want) >= 6
    for s in range(S):
        assert len(got[s]) == len(want[s]) and all(torch.equal(a, b[1]) for a, b in zip(got[s], want[s])), s


# ---- 6. sessions ------------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def _snap(ts):
    st = ts.export_slots(list(range(ts.S)))
    return [st.seen] + [st.tensors[k].clone() for k in sorted(st.tensors)] + [ts.bufs.clone(), ts.turn_state.clone()]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and (_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x.cpu(), y.cpu()))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["SpeechGate", "ToneGate"])
def test_moved_sessions_continue_bit_for_bit(name):
    from afx.streaming import StreamState
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import GatedScorer, SpeechGate
    gate, policy, t0, hops = _gate(name), TurnPolicy(LEAST), 13, 32
    streams = [torch.from_numpy(np.roll(FIX, -o).copy()).cuda() for o in OFFSETS[:2]]
    rows = lambda t: torch.stack([x[t * H:(t + 1) * H] for x in streams])  # noqa: E731
    never = TurnScorer(_sliding(3), gate, policy, hop=H)
    ref = torch.stack([never.push(rows(t), [0, 2]).clone() for t in range(hops)])  # (hops, 2)
    assert never.emitted(ref[t0:, 0]).any() and never.emitted(ref[t0:, 1]).any() and never.emitted(ref[:t0]).any()

    a = TurnScorer(_sliding(3), gate, policy, hop=H)
    for t in range(t0):
        assert _same_bits(a.push(rows(t).flip(0), [2, 0]), ref[t].flip(0))
    st = a.export_slots([0, 2])
    n = st.tensors["turn_frames"].tolist()
    assert min(n) > 0 and st.tensors["turn_first"].tolist() == [t0 * 25 - k for k in n]  # both mid-turn, up to the newest frame
    assert int(a.turn_state[0, 0]) == 1 or int(a.turn_state[2, 0]) == 1  # (an open turn in buffer 1 lands in buffer 0)
    b = TurnScorer(_sliding(4), gate, policy, hop=H)
    b.push(torch.from_numpy(np.stack([FIX[8000:12000], FIX[48000:52000]])).cuda(), [3, 0])  # the destination is in use
    moved = _move(st)

    def edited(**kw):
        t = {k: v.clone() for k, v in moved.tensors.items()}
        for k, (i, v) in kw.items():
            t[k][i] = v
        return StreamState(moved.meta, moved.seen, t)

    loud = moved.tensors["turn_open"].clone()
    loud[0, n[0] * FRAME] = 1e-3
    gated = GatedScorer(_sliding(4), gate)
    before, gated_before = _snap(b), gated.export_slots([0, 1, 2, 3])
    refused = [gated.export_slots([0, 1]),                                      # a GatedScorer state
               StreamState(dict(moved.meta, turn_params=[H, 50, TOP]), moved.seen, moved.tensors),  # other parameters
               edited(turn_frames=(0, TOP)), edited(turn_frames=(1, -1)),     # turn_frames outside [0, max_frames)
               StreamState(moved.meta, moved.seen, dict(moved.tensors, turn_open=loud)),  # samples after the open turn
               edited(turn_first=(0, t0 * 25 - n[0] + 1)),                     # turn_first + turn_frames > seen // frame
               edited(turn_totals=((1, 3), -1)),                                # negative totals
               edited(gate_hang=(0, gate.hang + 1)), edited(gate_nf=(1, float("nan")))]  # what the gate's checks refuse
    for i, state in enumerate(refused):
        with pytest.raises(ValueError):
            b.import_slots([3, 1], state)
        assert _same(before, _snap(b)), i
    with pytest.raises(ValueError):
        gated.import_slots([3, 1], moved)  # a turn state into a GatedScorer
    with pytest.raises(ValueError):
        TurnScorer(_sliding(4), SpeechGate(hang=10), policy, hop=H).import_slots([3, 1], moved)
    after = gated.export_slots([0, 1, 2, 3])
    assert _same([gated_before.tensors[k] for k in sorted(gated_before.tensors)], [after.tensors[k] for k in sorted(after.tensors)])

    b.import_slots([3, 1], moved)
    assert b.turn_state[[3, 1], 0].tolist() == [0, 0] and b.turn_state[[3, 1], 1].tolist() == n
    for t in range(t0, hops):
        assert _same_bits(b.push(rows(t).flip(0), [1, 3]), ref[t].flip(0)), t
    assert b.samples_seen.tolist() == [H, hops * H, 0, hops * H]
    assert torch.equal(b.turn_totals[[3, 1]].cpu(), never.turn_totals[[0, 2]].cpu())
    assert torch.equal(b.turns_scored[[3, 1]], never.turns_scored[[0, 2]])

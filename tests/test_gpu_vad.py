"""The speech gate on the GPU (afx/vad.py, afx_k_gate).  Every comparison is exact: the kernel against the numpy restatement
``gate_reference`` (kept counts, ring contents, noise-floor bits, hangover, untouched neighbours), ``GatedScorer`` streamed
against the offline ``SpeechGate.gate``, its scores against a fresh inner scorer pushed the gated stream hop by hop for
the three scorer kinds, the same behind the packet and jitter fronts, and sessions moved between scorers.

The KV-cached scorer keeps its 4-s window (as in every other streaming test: the mode is defined for it); the two exact
scorers run a 1-s window."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000


def fixture_stream():
    g = np.random.default_rng(0)
    x = (0.002 * g.standard_normal(128000)).astype(np.float32)
    t = np.arange(128000) / 16000
    for a, b in [(0.5, 1.3), (2.0, 2.15), (3.0, 5.0), (6.5, 6.52)]:
        m = (t >= a) & (t < b)
        x[m] += (0.2 * np.sin(2 * np.pi * 180 * t[m]) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t[m]))).astype(np.float32)
    x[112000:120000] = 0
    return x


FIX = fixture_stream()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


# ---- 1. the kernel against gate_reference ----------------------------------------------------------------------------------
class _Raw:
    """afx_k_gate driven directly, with a host mirror of ring, nf and h advanced by ``gate_reference``."""

    def __init__(self, gate, S, ring_len, seed):
        from afx.vad import SpeechGate
        self.gate, self.S, self.ring_len = gate, S, ring_len
        g = torch.Generator().manual_seed(seed)
        self.m_ring = torch.randn(S, ring_len, generator=g).numpy().copy()  # (not zeros: a stray write shows)
        self.ring = torch.from_numpy(self.m_ring).cuda()
        self.nf = torch.full((S,), float("inf"), device="cuda")
        self.h = torch.zeros(S, dtype=torch.int32, device="cuda")
        self.state = [SpeechGate.new_state() for _ in range(S)]
        self.wpos = [0] * S

    def launch(self, rows, slots, wpos=None, mask=False):
        """rows: (A, n) numpy -> (rc, kept list, mask or None) of one afx_k_gate call."""
        from afx._lib import call_on, lib, ptr
        g = self.gate
        x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        A, n = x.shape
        hdr = torch.tensor(list(zip(slots, [self.wpos[s] for s in slots] if wpos is None else wpos)), dtype=torch.int32).cuda()
        kept = torch.full((A,), -5, dtype=torch.int32, device="cuda")
        mk = torch.full((A, n // g.frame), 9, dtype=torch.uint8, device="cuda") if mask else None
        rc = call_on(x, lib().afx_k_gate, ptr(x), A, n, ptr(hdr), g.frame, float(g.E_floor), float(g.ratio32), float(g.rise32),
                     g.hang, ptr(self.nf), ptr(self.h), ptr(self.ring), self.S, self.ring_len, ptr(kept), ptr(mk))
        torch.cuda.synchronize()
        return rc, kept.tolist(), None if mk is None else mk.cpu().numpy()

    def reference(self, rows, slots, wpos=None):
        """Advance the mirror -> (kept list, masks)."""
        kept, masks = [], []
        for i, s in enumerate(slots):
            m, k, self.state[s] = self.gate.gate_reference(rows[i], self.state[s])
            w = self.wpos[s] if wpos is None else wpos[i]
            self.m_ring[s, (w + np.arange(k.size)) % self.ring_len] = k
            if wpos is None:
                self.wpos[s] = (w + k.size) % self.ring_len
            kept.append(k.size)
            masks.append(m)
        return kept, masks

    def check(self, what):
        assert self.ring.cpu().numpy().tobytes() == self.m_ring.tobytes(), what
        nf = np.array([st["nf"] for st in self.state], dtype=np.float32)
        assert self.nf.cpu().numpy().tobytes() == nf.tobytes(), (what, self.nf.tolist(), nf.tolist())
        assert self.h.tolist() == [st["h"] for st in self.state], what


def _sources(total):
    """Five streams: the fixture at two offsets (one off the frame grid), zeros, speech throughout, noise only."""
    t = np.arange(total) / 16000
    g = np.random.default_rng(11)
    speech = (0.2 * np.sin(2 * np.pi * 180 * t) * (1 + 0.8 * np.sin(2 * np.pi * 4 * t))).astype(np.float32)
    speech += (0.002 * g.standard_normal(total)).astype(np.float32)
    noise = (0.004 * g.standard_normal(total)).astype(np.float32)
    return [FIX[:total], np.roll(FIX, -(20000 + 37))[:total], np.zeros(total, dtype=np.float32), speech, noise]


@pytest.mark.parametrize("n,frame,launches", [(800, 160, 40), (4000, 160, 24), (1000, 200, 60)])
def test_kernel_equals_the_reference_launch_by_launch(n, frame, launches):
    from afx.vad import SpeechGate
    S = 5
    gate = SpeechGate(frame=frame)
    raw = _Raw(gate, S, 2 * n, seed=n)
    src = _sources(n * launches)
    pos = [0] * S
    rng = np.random.default_rng(n + frame)
    total_kept = [0] * S
    for it in range(launches):
        slots = [0, 1, 2, 3, 4] if it in (0, launches - 1) else rng.permutation(S)[:rng.integers(1, S + 1)].tolist()
        rows = np.stack([src[s][pos[s]:pos[s] + n] for s in slots])
        rc, kept, mask = raw.launch(rows, slots, mask=it % 2 == 0)
        assert rc == 0
        want, masks = raw.reference(rows, slots)
        assert kept == want, (it, slots)
        if mask is not None:
            assert np.array_equal(mask, np.stack(masks).astype(np.uint8)), it
        raw.check((it, slots))  # (the whole ring and state: the named slots' columns AND the unnamed slots' bytes)
        for s, k in zip(slots, kept):
            pos[s] += n
            total_kept[s] += k
    # the cases did something: the rings wrapped several times, zeros and noise kept nothing, speech throughout was gated too
    assert total_kept[0] > 3 * 2 * n and total_kept[1] > 3 * 2 * n, total_kept
    assert total_kept[2] == 0 and total_kept[4] == 0 and total_kept[3] > 0, total_kept


def test_a_row_longer_than_one_launch_takes_is_split_with_the_state_carried():
    from afx.vad import MAX_FRAMES, SpeechGate
    gate = SpeechGate()
    frames = MAX_FRAMES + 88  # 600 frames: two launches inside the library
    n = frames * 160
    raw = _Raw(gate, 3, n + 160, seed=3)
    rows = np.stack([FIX[:n], np.roll(FIX, -(16000 + 37))[:n]])
    slots, wpos = [2, 0], [n - 320, 5]  # (slot 2 wraps the ring inside the first launch's frames)
    rc, kept, mask = raw.launch(rows, slots, wpos=wpos, mask=True)
    assert rc == 0
    want, masks = raw.reference(rows, slots, wpos=wpos)
    assert kept == want and min(kept) > 100 * 160
    assert np.array_equal(mask, np.stack(masks).astype(np.uint8))
    assert masks[0][MAX_FRAMES:].any() and masks[0][:MAX_FRAMES].any()  # kept frames on both sides of the split
    raw.check("split row")


def test_bad_rows_are_skipped_whole_and_bad_arguments_launch_nothing():
    from afx._lib import lib
    from afx.vad import SpeechGate
    gate = SpeechGate()
    n = 800
    raw = _Raw(gate, 3, 2 * n, seed=5)
    rows = np.stack([FIX[7520:7520 + n]] * 4)  # three frames of noise, then the onset of the first talk spurt
    # slot 3 and slot -1 are outside the state, wpos 1600 is outside the ring: those rows are skipped, row 1 (slot 1) is gated
    slots, wpos = [3, 1, -1, 0], [0, 7, 0, 2 * n]
    rc, kept, _ = raw.launch(rows, slots, wpos=wpos)
    assert rc == 0
    want, _ = raw.reference(rows[1:2], [1], wpos=[7])
    assert kept == [0, want[0], 0, 0] and want[0] == 320
    raw.check("skipped rows")
    # a row longer than the ring: every row is skipped
    small = _Raw(gate, 2, n - 160, seed=6)
    rc, kept, _ = small.launch(rows[:2], [0, 1])
    assert rc == 0 and kept == [0, 0]
    small.check("n > ring_len")
    # scalar arguments: an error, nothing launched
    for bad in (dict(n=801), dict(frame=0), dict(A=0), dict(S=0), dict(ring_len=0), dict(hang=-1), dict(ratio=1.0),
                dict(floor=0.0), dict(rise=0.5)):
        a = dict(A=1, n=n, frame=160, floor=float(gate.E_floor), ratio=8.0, rise=1.01, hang=20, S=3, ring_len=2 * n)
        a.update(bad)
        x = torch.from_numpy(rows[:1].copy()).cuda()
        hdr = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
        kept = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = lib().afx_k_gate(p(x), a["A"], a["n"], p(hdr), a["frame"], a["floor"], a["ratio"], a["rise"], a["hang"], p(raw.nf),
                              p(raw.h), p(raw.ring), a["S"], a["ring_len"], p(kept), None, None)
        torch.cuda.synchronize()
        assert rc != 0 and b"gate" in lib().afx_last_error(), bad
        assert kept.tolist() == [-5]
    raw.check("bad arguments")
    assert lib().afx_k_gate(None, 1, n, None, 160, 1e-4, 8.0, 1.01, 20, None, None, None, 3, 2 * n, None, None, None) != 0


# ---- 2. streamed equals offline ----------------------------------------------------------------------------------------------
def _tap(S, hop):
    from afx.streaming import SlidingWindowScorer

    class Tap(SlidingWindowScorer):
        def __init__(self):
            super().__init__(None, S, window=4 * hop, hop=hop, device="cuda")
            self.got = [[] for _ in range(S)]

        def push(self, chunk, slots=None):
            idx = self._slot_list(slots, ordered=True)
            assert chunk.is_cuda and chunk.dtype == torch.float32 and chunk.shape == (len(idx), hop)
            for i, s in enumerate(idx):
                self.got[s].append(chunk[i].clone())
            self._seen[idx] += hop
            return torch.tensor([float(10 * s + 1) for s in idx], device=chunk.device)

    return Tap()


def test_streamed_gate_equals_the_offline_gate_and_the_reference():
    from afx.vad import GatedScorer, SpeechGate
    S, hop, ticks = 3, 800, 70
    gate = SpeechGate()
    tap = _tap(S, hop)
    gs = GatedScorer(tap, gate)
    streams = [FIX, np.roll(FIX, -(24000 + 13)), np.roll(FIX, -(52000 + 401))]
    pos, begin, mark = [0] * S, [0] * S, [0] * S  # samples pushed; where the current session began; tap hops before it
    state = [SpeechGate.new_state() for _ in range(S)]
    fill = [0] * S
    first_session = None
    for t in range(ticks):
        if t == 35:  # slot 2 starts over midway (its stream goes on from where it is)
            first_session = (begin[2], pos[2], len(tap.got[2]))
            gs.reset([2])
            begin[2], mark[2], state[2], fill[2] = pos[2], len(tap.got[2]), SpeechGate.new_state(), 0
        named = [s for s in ([0, 1, 2] if t % 3 else [2, 0, 1]) if not (s == 1 and 10 <= t < 30) and not (s == 0 and t % 7 == 3)]
        chunk = torch.from_numpy(np.stack([streams[s][pos[s]:pos[s] + hop] for s in named])).cuda()
        out = gs.push(chunk, named) if len(named) < S or t % 2 else gs.push(chunk[[named.index(s) for s in range(S)]])
        order = named if len(named) < S or t % 2 else list(range(S))
        assert out.shape == (len(order),) and out.dtype == torch.float32 and out.is_cuda
        want = []
        for s in order:
            _, k, state[s] = gate.gate_reference(streams[s][pos[s]:pos[s] + hop], state[s])
            pos[s] += hop
            fill[s] += k.size
            want.append(fill[s] >= hop)
            fill[s] -= hop if fill[s] >= hop else 0
        assert gs.emitted(out).tolist() == want, t  # NaN exactly where no hop completed
        assert out[gs.emitted(out)].tolist() == [float(10 * s + 1) for s, w in zip(order, want) if w]
        assert gs.pending.tolist() == fill and gs.samples_seen.tolist() == [p - b for p, b in zip(pos, begin)]
        assert gs.samples_kept.tolist() == [(len(tap.got[s]) - mark[s]) * hop + fill[s] for s in range(S)]
    sessions = [(s, begin[s], pos[s], tap.got[s][mark[s]:]) for s in range(S)] + [(2, first_session[0], first_session[1], tap.got[2][:first_session[2]])]
    offline = gate.gate([torch.from_numpy(streams[s][a:b].copy()).cuda() for s, a, b, _ in sessions])
    for (s, a, b, got), off in zip(sessions, offline):
        _, kept, _ = gate.gate_reference(streams[s][a:b])
        assert off.cpu().numpy().tobytes() == kept.tobytes()
        whole = kept.size // hop
        assert len(got) == whole and whole >= 3, (s, whole)
        assert torch.cat(got).cpu().numpy().tobytes() == kept[:whole * hop].tobytes(), s
    # the offline form: a (B, n) tensor, masks, trailing samples short of a frame dropped
    two = torch.from_numpy(np.stack([FIX[:8000 + 77], streams[1][:8000 + 77]])).cuda()
    outs, masks = gate.gate(two, return_mask=True)
    for row, o, m in zip(two.cpu().numpy(), outs, masks):
        rm, rk, _ = gate.gate_reference(row[:8000])
        assert m.dtype == torch.bool and m.cpu().numpy().tolist() == rm.tolist() and o.cpu().numpy().tobytes() == rk.tobytes()
    assert gate.gate([torch.zeros(100, device="cuda")])[0].numel() == 0


# ---- 3. scores -----------------------------------------------------------------------------------------------------------------
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES[dtype] = (eng, sd)
    return _ENGINES[dtype]


def _inner(kind, S):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    eng, sd = _engine("fp16x3" if kind == "kv-fp16x3" else "fp16")
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _gated_offline(gate, R):
    """R: (n,) fp32 CUDA -> the whole hops of its gated stream, (hops, H)."""
    g = gate.gate([R])[0]
    return g[:g.numel() // H * H].reshape(-1, H)


def _check_scores(kind, got, G, slots=None):
    """got[s]: the non-NaN scores slot s emitted, in order; G[s]: (hops, H) gated stream -> equal to a fresh inner scorer."""
    S = len(G)
    fresh = _inner(kind, S)
    for s in range(S):
        assert len(got[s]) == G[s].shape[0], (s, len(got[s]), G[s].shape[0])
        for j in range(G[s].shape[0]):
            ref = fresh.push(G[s][j:j + 1].contiguous(), [s])
            assert torch.equal(got[s][j].reshape(1), ref), (kind, s, j)


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv", "kv-fp16x3"])
def test_scores_equal_a_fresh_inner_scorer_pushed_the_gated_stream(kind):
    from afx.vad import GatedScorer, SpeechGate
    S, hops = 3, 12
    gate = SpeechGate()
    gs = GatedScorer(_inner(kind, S), gate)
    streams = [torch.from_numpy(np.roll(FIX, -o)[:hops * H].copy()).cuda() for o in (0, 30000 + 57, 44000)]
    got = [[] for _ in range(S)]
    for t in range(hops):
        named = [[0, 1, 2], [2, 1, 0], [1, 2, 0]][t % 3]
        out = gs.push(torch.stack([streams[s][t * H:(t + 1) * H] for s in named]), named)
        for s, v, e in zip(named, out, gs.emitted(out).tolist()):
            if e:
                got[s].append(v.clone())
    G = [_gated_offline(gate, x) for x in streams]
    assert sum(g.shape[0] for g in G) >= 12 and min(g.shape[0] for g in G) >= 2 and all(g.shape[0] < hops for g in G)
    _check_scores(kind, got, G)
    assert torch.equal(gs.scorer.samples_seen, torch.tensor([g.shape[0] * H for g in G]))


# ---- 4. behind the fronts --------------------------------------------------------------------------------------------------------
def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the reference decodes the same bytes)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def _collect(got, res, named):
    from afx.vad import emitted
    for s, part in zip(named, res.split()):
        got[s] += [v.clone() for v in part[emitted(part)]]


def test_gate_behind_the_packet_front():
    from afx.ingest import PacketScorer, decode
    from afx.resample import Resampler
    from afx.vad import GatedScorer, SpeechGate
    S, kind, gate = 3, "kv", SpeechGate()
    ps = PacketScorer(GatedScorer(_inner(kind, S), gate), 8000, "mulaw")
    codes = [_mulaw_encode(np.roll(FIX, -o)[:96000:2]) for o in (0, 30000 + 57, 44000)]  # 8 kHz by plain slicing, 6 s each
    got = [[] for _ in range(S)]
    for k in range(0, codes[0].size, 160):  # 20-ms packets
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        _collect(got, ps.feed([codes[s][k:k + 160].tobytes() for s in named], named), named)
    G = [_gated_offline(gate, Resampler(8000)(decode(c, "mulaw")[None])[0]) for c in codes]
    assert min(g.shape[0] for g in G) >= 2
    _check_scores(kind, got, G)
    assert ps.samples_seen.tolist() == [96000 // H * H] * S  # (the fronts count what the gate was pushed)


def test_gate_behind_the_jitter_front_with_a_withheld_run():
    from afx.ingest import decode
    from afx.jitter import JitterScorer
    from afx.resample import Resampler
    from afx.vad import GatedScorer, SpeechGate
    S, kind, gate = 3, "incremental", SpeechGate()
    js = JitterScorer(GatedScorer(_inner(kind, S), gate), 8000, "mulaw", depth=480, conceal="zero")
    offs = (0, 4000, 16000 + 57)
    codes = [_mulaw_encode(np.roll(FIX, -o)[:96000:2]) for o in offs]
    # 400 ms withheld per slot, inside the 2-s talk spurt of each stream (3.0 - 5.0 s of the fixture)
    lost = [((60000 - o) // 2 // 160 * 160, (60000 - o) // 2 // 160 * 160 + 3200) for o in offs]

    got = [[] for _ in range(S)]
    for k in range(0, codes[0].size, 160):
        named = [s for s in [[0, 1, 2], [1, 2, 0]][(k // 160) % 2] if not lost[s][0] <= k < lost[s][1]]
        _collect(got, js.feed([codes[s][k:k + 160].tobytes() for s in named], named, [k] * len(named)), named)
    _collect(got, js.flush(), list(range(S)))
    E = []
    for s in range(S):
        e = decode(codes[s], "mulaw").clone()
        e[lost[s][0]:lost[s][1]] = 0.0  # conceal="zero": the played-out stream is the decoded one with the gap zeroed
        E.append(e)
    R = [Resampler(8000)(e[None])[0] for e in E]
    G = [_gated_offline(gate, r) for r in R]
    _check_scores(kind, got, G)
    # the withheld run yields no score of its own: once the hangover has run out inside it, no frame of it is kept
    for s in range(S):
        _, (mask,) = gate.gate([R[s]], return_mask=True)
        a, b = 2 * lost[s][0] // 160 + 2 + gate.hang, 2 * lost[s][1] // 160
        assert b - a >= 15 and not mask[a:b].any() and mask[a - gate.hang - 3:a - 2].all(), s


# ---- 5. moving sessions ------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def _snap(gs):
    st = gs.export_slots(list(range(gs.S)))
    return [st.seen] + [st.tensors[k].clone() for k in sorted(st.tensors)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and _same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x.cpu(), y.cpu())
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_moved_sessions_continue_bit_for_bit(kind):
    from afx.ingest import PacketScorer
    from afx.vad import GatedScorer, SpeechGate
    gate, t0, ticks = SpeechGate(), 5, 14
    # slot 0: cut mid-hangover with pending samples; slot 1: cut in silence (zeros) after a 20-ms blip, speech again later
    streams = [np.roll(FIX, -2000)[:ticks * H], np.roll(FIX, -100000)[:ticks * H]]
    hopsof = lambda t, rows: torch.from_numpy(np.stack([streams[i][t * H:(t + 1) * H] for i in rows])).cuda()  # noqa: E731
    never = GatedScorer(_inner(kind, 3), gate)
    ref = torch.stack([never.push(hopsof(t, [0, 1]), [0, 2]).clone() for t in range(ticks)])  # (ticks, 2)
    assert never.emitted(ref[t0:]).sum() >= 3 and never.emitted(ref[t0:, 1]).any() and never.emitted(ref[:t0, 0]).any()

    a = GatedScorer(_inner(kind, 3), gate)
    for t in range(t0):
        assert _same_bits(a.push(hopsof(t, [1, 0]), [2, 0]), ref[t].flip(0))
    st = a.export_slots([0, 2])
    assert int(st.tensors["gate_hang"][0]) > 0 and int(st.tensors["gate_fill"][0]) > 0  # mid-hangover, samples pending
    assert int(st.tensors["gate_hang"][1]) == 0 and float(st.tensors["gate_nf"][1]) == float(gate.nf_min)  # in silence
    b = GatedScorer(_inner(kind, 4), gate)
    b.push(torch.from_numpy(np.stack([FIX[8000:12000], FIX[48000:52000]])).cuda(), [3, 0])  # the destination is in use
    other = GatedScorer(_inner(kind, 4), SpeechGate(hang=10))
    before = _snap(other)
    with pytest.raises(ValueError):
        other.import_slots([3, 1], _move(st))
    assert _same(before, _snap(other))  # refused with the destination unchanged
    with pytest.raises(ValueError):
        b.scorer.import_slots([3, 1], _move(st))  # a bare scorer refuses a gated state
    with pytest.raises(ValueError):
        b.import_slots([3, 1], a.scorer.export_slots([0, 2]))  # and the gated scorer a bare one
    b.import_slots([3, 1], _move(st))
    for t in range(t0, ticks):
        assert _same_bits(b.push(hopsof(t, [1, 0]), [1, 3]), ref[t].flip(0)), t
    assert b.samples_seen.tolist() == [H, ticks * H, 0, ticks * H]

    # once through the packet front's export / import around the gate (16 kHz float packets of one hop: one push per feed)
    pa = PacketScorer(GatedScorer(_inner(kind, 3), gate), 16000, "pcm_f32le")
    pb = PacketScorer(GatedScorer(_inner(kind, 2), gate), 16000, "pcm_f32le")
    for t in range(ticks):
        P, named = (pa, [0, 2]) if t < t0 else (pb, [1, 0])
        if t == t0:
            pb.import_slots([1, 0], _move(pa.export_slots([0, 2])))
        res = P.feed([streams[i][t * H:(t + 1) * H].tobytes() for i in (0, 1)], named)
        assert res.counts.tolist() == [1, 1] and _same_bits(res.scores, ref[t]), t

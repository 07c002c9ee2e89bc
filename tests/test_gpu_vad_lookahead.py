"""The look-ahead gate on the GPU (afx/vad.py LookaheadGate, afx_k_gate_la).  Every comparison is exact: the kernel driven
directly against a host mirror advanced by ``gate_reference`` (ring, kept, nf, h, flags, line, src, mask, untouched
neighbours), ``GatedScorer`` around it against a fresh inner scorer pushed the gated stream G' hop by hop (streamed, with a
reset, with a session moved mid-stream, behind the packet front), ``last_span`` against the reference's source indices and
the offline form against the dilated mask.

The input is the burst stream of tests/test_cpu_vad_lookahead.py: the plain gate keeps 300 of its 600 frames, look-ahead
adds 6, 30 and 186 for pre = 1, 5 and 31."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000


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
    """(keep, keep') over the whole of x from the plain decision: the definition, not the delay line."""
    _, speech, keep, _, _ = gate._decide(x, {"nf": np.float32(np.inf), "h": 0})
    out = keep.copy()
    for g in np.flatnonzero(speech):
        out[max(0, g - gate.pre):g] = True
    return keep, out


def _differs(gate, x):
    keep, kd = dilated(gate, x)
    return bool((kd != keep).any())


# ---- 1. the kernel against gate_reference ----------------------------------------------------------------------------------
class _Raw:
    """afx_k_gate_la driven directly, with a host mirror of ring, nf, h, flags, line and src advanced by ``gate_reference``."""

    def __init__(self, gate, S, ring_len, seed):
        self.gate, self.S, self.ring_len, self.ent = gate, S, ring_len, ring_len // gate.frame
        g = torch.Generator().manual_seed(seed)
        self.m_ring = torch.randn(S, ring_len, generator=g).numpy().copy()  # (not zeros: a stray write shows)
        self.m_line = torch.randn(S, gate.pre * gate.frame, generator=g).numpy().copy()
        self.m_src = np.full((S, self.ent), -7, dtype=np.int32)
        self.m_flags = np.zeros(S, dtype=np.int32)
        self.ring, self.line, self.src = (torch.from_numpy(a.copy()).cuda() for a in (self.m_ring, self.m_line, self.m_src))
        self.nf = torch.full((S,), float("inf"), device="cuda")
        self.h = torch.zeros(S, dtype=torch.int32, device="cuda")
        self.flags = torch.zeros(S, dtype=torch.int32, device="cuda")
        self.state = [gate.new_state() for _ in range(S)]
        self.wpos = [0] * S

    def launch(self, rows, slots, wpos=None, F=None, mask=False, **over):
        """rows: (A, n) numpy -> (rc, kept list, mask or None) of one afx_k_gate_la call."""
        from afx._lib import call_on, lib, ptr
        g = self.gate
        x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        A, n = x.shape
        wpos = [self.wpos[s] for s in slots] if wpos is None else wpos
        F = [self.state[s]["F"] if 0 <= s < self.S else 0 for s in slots] if F is None else F
        hdr = torch.tensor([[s, w, f, 0] for s, w, f in zip(slots, wpos, F)], dtype=torch.int32).cuda()
        kept = torch.full((A,), -5, dtype=torch.int32, device="cuda")
        mk = torch.full((A, n // g.frame), 9, dtype=torch.uint8, device="cuda") if mask else None
        a = dict(pre=g.pre, ring_len=self.ring_len, flags=ptr(self.flags))
        a.update(over)
        rc = call_on(x, lib().afx_k_gate_la, ptr(x), A, n, ptr(hdr), g.frame, float(g.E_floor), float(g.ratio32), float(g.rise32),
                     g.hang, a["pre"], ptr(self.nf), ptr(self.h), a["flags"], ptr(self.line), ptr(self.ring), ptr(self.src), self.S,
                     a["ring_len"], ptr(kept), ptr(mk))
        torch.cuda.synchronize()
        return rc, kept.tolist(), None if mk is None else mk.cpu().numpy()

    def reference(self, rows, slots, wpos=None):
        """Advance the mirror -> (kept list, mask rows as the kernel lays them out, emitted samples per row)."""
        g = self.gate
        kept, masks, outs = [], [], []
        for i, s in enumerate(slots):
            F, nfr = self.state[s]["F"], rows[i].size // g.frame
            m, out, src, st = g.gate_reference(rows[i], self.state[s])
            self.state[s] = st
            w = self.wpos[s] if wpos is None else wpos[i]
            self.m_ring[s, (w + np.arange(out.size)) % self.ring_len] = out
            self.m_src[s, (w // g.frame + np.arange(src.size)) % self.ent] = src
            for j, fr in enumerate(rows[i].reshape(nfr, g.frame)):  # frame F + j enters block (F + j) mod pre
                b = (F + j) % g.pre
                self.m_line[s, b * g.frame:(b + 1) * g.frame] = fr
            d = len(st["flags"])
            self.m_flags[s] = sum(int(f) << ((st["F"] - d + k) % g.pre) for k, f in enumerate(st["flags"]))
            if wpos is None:
                self.wpos[s] = (w + out.size) % self.ring_len
            full = np.zeros(nfr, dtype=np.uint8)  # entry j: frame F - pre + j, 0 where that is negative
            full[nfr - m.size:] = m
            kept.append(out.size), masks.append(full), outs.append(out)
        return kept, masks, outs

    def check(self, what):
        for name, dev, host in (("ring", self.ring, self.m_ring), ("line", self.line, self.m_line), ("src", self.src, self.m_src),
                                ("flags", self.flags, self.m_flags)):
            assert dev.cpu().numpy().tobytes() == host.tobytes(), (what, name)
        nf = np.array([st["nf"] for st in self.state], dtype=np.float32)
        assert self.nf.cpu().numpy().tobytes() == nf.tobytes(), (what, self.nf.tolist(), nf.tolist())
        assert self.h.tolist() == [st["h"] for st in self.state], what


def _streams(frame, total):
    """Five streams: the bursts at three offsets (one off the frame grid), the bursts with a NaN frame in the noise, an inf
    frame just before an onset and an overflowing one inside a burst, and zeros.  For one-sample frames the stream is
    decimated by 40 (bursts of 120 samples from sample 200 on, every 360) and scaled so that the noise stays under the floor."""
    base = X if frame > 1 else (np.float32(0.3) * X[::40]).astype(np.float32)
    bad = base.copy()
    nan, inf, big = (43 * 160 + 17, 138 * 160 + 5, 235 * 160) if frame > 1 else (150, 198, 260)
    bad[nan], bad[inf], bad[big] = np.nan, np.inf, 1e30
    reps = -(-total // base.size)
    return [np.tile(s, reps)[:total] for s in (base, np.roll(base, -(4000 + 37)), np.roll(base, -9920), bad, np.zeros_like(base))]


@pytest.mark.parametrize("frame,pre", [(160, 1), (160, 5), (160, 31), (200, 5), (1, 5)])
def test_kernel_equals_the_reference_launch_by_launch(frame, pre):
    from afx.vad import LookaheadGate
    S, launches, prefix = 5, 60, 250
    gate = LookaheadGate(frame=frame, pre=pre)
    sizes = [m for m in (1, pre - 1, pre, pre + 1, 25) if m > 0]  # frames per row: the line rotates through every phase
    src = _streams(frame, launches * 32 * frame)
    assert all(_differs(gate, s[:prefix * frame]) for s in src[:4])  # (no case passes vacuously: look-ahead adds frames)
    raw = _Raw(gate, S, 40 * frame, seed=frame + pre)
    pos, total, wraps = [0] * S, [0] * S, 0
    rng = np.random.default_rng(frame + pre)
    for it in range(launches):
        n = sizes[it % len(sizes)] * frame
        slots = rng.permutation(S)[:rng.integers(1, S + 1)].tolist() if it % 3 == 2 else rng.permutation(S).tolist()
        rows = np.stack([src[s][pos[s]:pos[s] + n] for s in slots])
        before = [raw.wpos[s] for s in slots]
        rc, kept, mask = raw.launch(rows, slots, mask=it % 2 == 0)
        assert rc == 0
        want, masks, _ = raw.reference(rows, slots)
        assert kept == want, (it, slots)
        if mask is not None:
            assert np.array_equal(mask, np.stack(masks)), it
        raw.check((it, slots))  # (everything: the named slots' state AND the unnamed slots' bytes)
        for s, k, w in zip(slots, kept, before):
            pos[s] += n
            total[s] += k
            wraps += w + k > raw.ring_len  # a copy that wrapped the ring
    assert min(pos[:4]) >= prefix * frame and min(total[:4]) > raw.ring_len and wraps >= 4 and total[4] == 0, (pos, total, wraps)


def test_a_row_across_the_launch_split_equals_the_same_audio_in_short_rows():
    from afx.vad import MAX_FRAMES, LookaheadGate
    gate = LookaheadGate()
    frames = MAX_FRAMES + 88  # 600 frames: two launches inside the library
    n = frames * 160
    rows = np.stack([X[:n], np.roll(X, -(4000 + 37))[:n]])
    assert _differs(gate, rows[0]) and _differs(gate, rows[1])
    slots, wpos = [2, 0], [n - 320, 160]  # (slot 2 wraps the ring inside the first launch's frames)
    one, many = _Raw(gate, 3, n + 160, seed=3), _Raw(gate, 3, n + 160, seed=3)
    rc, kept, mask = one.launch(rows, slots, wpos=wpos, mask=True)
    assert rc == 0
    want, masks, _ = one.reference(rows, slots, wpos=wpos)
    assert kept == want and min(kept) > 100 * 160
    assert np.array_equal(mask, np.stack(masks))
    assert masks[0][MAX_FRAMES:].any() and masks[0][:MAX_FRAMES].any()  # emitted frames on both sides of the split
    one.check("split row")
    many.wpos[2], many.wpos[0] = wpos
    for a in range(0, n, 25 * 160):
        part = rows[:, a:a + 25 * 160]
        rc, kept, _ = many.launch(part, slots)
        assert rc == 0 and kept == many.reference(part, slots)[0]
    many.check("short rows")
    for a, b in ((one.ring, many.ring), (one.src, many.src), (one.line, many.line), (one.flags, many.flags), (one.h, many.h)):
        assert torch.equal(a, b)
    assert one.nf.cpu().numpy().tobytes() == many.nf.cpu().numpy().tobytes()


def test_bad_rows_are_skipped_whole_and_bad_arguments_launch_nothing():
    from afx._lib import lib
    from afx.vad import LookaheadGate
    gate = LookaheadGate()
    n, L = 800, 1600
    raw = _Raw(gate, 3, L, seed=5)
    warm = np.stack([X[40 * 160:50 * 160]] * 3)  # ten frames of noise each: the lines are full, the floors set
    assert raw.launch(warm, [0, 1, 2])[0] == 0
    raw.reference(warm, [0, 1, 2])
    raw.check("warm")
    rows = np.stack([X[50 * 160:55 * 160]] * 8)  # the onset: the five delayed noise frames are flagged and emitted
    # slot 3 and -1: outside the state; wpos L and -160: outside the ring; wpos 7: off the frame grid; F + 5 = 2^31 and
    # F = -1: outside the count.  Row 3 (slot 1) is gated.
    slots = [3, -1, 0, 1, 0, 0, 2, 2]
    wpos = [0, 0, L, 320, -160, 7, 0, 0]
    F = [10, 10, 10, 10, 10, 10, (1 << 31) - 5, -1]
    rc, kept, mask = raw.launch(rows, slots, wpos=wpos, F=F, mask=True)
    assert rc == 0
    want, masks, _ = raw.reference(rows[3:4], [1], wpos=[320])
    assert kept == [0, 0, 0, want[0], 0, 0, 0, 0] and want[0] == 800
    assert np.array_equal(mask[3], masks[0]) and (np.delete(mask, 3, axis=0) == 9).all()  # (a skipped row's mask is not written)
    raw.check("skipped rows")
    # a row longer than the ring: every row is skipped
    small = _Raw(gate, 2, n - 160, seed=6)
    rc, kept, _ = small.launch(rows[:2], [0, 1])
    assert rc == 0 and kept == [0, 0]
    small.check("n > ring_len")
    # scalar arguments: an error, nothing launched
    for bad in (dict(pre=0), dict(pre=32), dict(ring_len=L - 1), dict(ring_len=0), dict(flags=None)):
        rc, kept, _ = raw.launch(rows[:1], [1], **bad)
        assert rc != 0 and b"gate_la" in lib().afx_last_error(), bad
        assert kept == [-5]
    raw.check("bad arguments")
    z = C.c_void_p(None)
    assert lib().afx_k_gate_la(z, 1, n, z, 160, 1e-4, 8.0, 1.01, 20, 5, z, z, z, z, z, z, 3, L, z, z, z) != 0


# ---- 2. scores -----------------------------------------------------------------------------------------------------------------
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
    from afx.streaming import IncrementalScorer, KVCachedScorer
    eng, sd = _engine("fp16")
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _check_scores(kind, got, G):
    """got[s]: the non-NaN scores of session s, in order; G[s]: its gated stream (numpy) -> equal to a fresh inner scorer
    pushed the whole hops of G[s]."""
    fresh = _inner(kind, len(G))
    for s, g in enumerate(G):
        hops = torch.from_numpy(g[:g.size // H * H].reshape(-1, H)).cuda()
        assert len(got[s]) == hops.shape[0], (s, len(got[s]), hops.shape[0])
        for j in range(hops.shape[0]):
            assert torch.equal(got[s][j].reshape(1), fresh.push(hops[j:j + 1].contiguous(), [s])), (kind, s, j)


def _spans(src):
    """The source indices of a session's emitted frames -> its hops' [first sample, one past the last) spans."""
    per = H // 160
    return [[int(src[j * per]) * 160, (int(src[(j + 1) * per - 1]) + 1) * 160] for j in range(src.size // per)]


STREAMS = [X, np.roll(X, -(30000 + 57)), np.roll(X, -44000)]


def test_scores_and_spans_equal_a_fresh_inner_scorer_pushed_the_gated_stream():
    from afx.vad import GatedScorer, LookaheadGate
    S, kind = 3, "incremental"
    gate = LookaheadGate(pre=5)
    assert all(_differs(gate, x) for x in STREAMS)
    gs = GatedScorer(_inner(kind, S), gate)
    dev = [torch.from_numpy(x.copy()).cuda() for x in STREAMS]
    refs = [gate.gate_reference(x) for x in STREAMS]
    spans = [_spans(r[2]) for r in refs]
    got, pos = [[] for _ in range(S)], [0] * S
    for t in range(30):
        named = [[0, 1, 2], [2, 1, 0], [1, 2], [0]][t % 4]  # (subsets in shuffled order: the slots advance at their own pace)
        out = gs.push(torch.stack([dev[s][pos[s]:pos[s] + H] for s in named]), named)
        for s in named:
            pos[s] += H
        span = gs.last_span
        assert span.is_cuda and span.dtype == torch.int64 and tuple(span.shape) == (len(named), 2)
        for s, v, e, sp in zip(named, out, gs.emitted(out).tolist(), span.tolist()):
            assert sp == (spans[s][len(got[s])] if e else [-1, -1]), (t, s)
            if e:
                got[s].append(v.clone())
    seen = gs.samples_seen.tolist()
    G = [gate.gate_reference(x[:n])[1] for x, n in zip(STREAMS, seen)]
    assert seen == pos and min(g.size // H for g in G) >= 5
    _check_scores(kind, got, G)
    assert gs.samples_kept.tolist() == [g.size for g in G]
    plain = GatedScorer(_inner(kind, 1))
    plain.push(dev[0][:H][None])
    assert plain.last_span is None and not hasattr(plain, "src")  # (a plain gate is what it was)


def test_a_reset_mid_stream_drops_the_line():
    from afx.vad import GatedScorer, LookaheadGate
    S, hops, kind, t0 = 2, 24, "incremental", 9
    gate = LookaheadGate(pre=5)
    gs = GatedScorer(_inner(kind, S), gate)
    dev = [torch.from_numpy(x.copy()).cuda() for x in STREAMS[:S]]
    got = [[], [], []]  # slot 0, slot 1 before its reset, slot 1 after it
    for t in range(hops):
        if t == t0:
            assert int(gs.flags[1]) != 0 and int(gs.pending[1]) > 0  # flagged frames delayed and frames pending: all dropped
            gs.reset([1])
            assert int(gs.flags[1]) == 0 and gs.pending.tolist()[1] == 0 and gs.samples_seen.tolist() == [t0 * H, 0]
        out = gs.push(torch.stack([d[t * H:(t + 1) * H] for d in dev]))
        for s, v, e, sp in zip(range(S), out, gs.emitted(out).tolist(), gs.last_span.tolist()):
            if e:
                got[s + (s == 1 and t >= t0)].append(v.clone())
                assert 0 <= sp[0] < sp[1] <= (t + 1 - (t0 if s == 1 and t >= t0 else 0)) * H - 5 * 160
    G = [gate.gate_reference(x)[1] for x in (STREAMS[0], STREAMS[1][:t0 * H], STREAMS[1][t0 * H:])]
    assert all(g.size >= 2 * H for g in G)
    # three sessions, each against a fresh scorer of its own slot
    fresh = _inner(kind, 3)
    for s, g in enumerate(G):
        hops_s = torch.from_numpy(g[:g.size // H * H].reshape(-1, H)).cuda()
        assert len(got[s]) == hops_s.shape[0], s
        for j in range(hops_s.shape[0]):
            assert torch.equal(got[s][j].reshape(1), fresh.push(hops_s[j:j + 1].contiguous(), [s])), (s, j)


def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def test_a_session_moved_with_frames_delayed_and_pending_continues_bit_for_bit():
    from afx.vad import GatedScorer, LookaheadGate, SpeechGate
    hops, kind, t0 = 24, "incremental", 9
    gate = LookaheadGate(pre=5)
    a, b = GatedScorer(_inner(kind, 2), gate), GatedScorer(_inner(kind, 3), gate)
    dev = [torch.from_numpy(x.copy()).cuda() for x in STREAMS[:2]]
    b.push(torch.stack([dev[0][8000:12000], dev[1][48000:52000]]), [2, 0])  # the destination is in use
    got, spans = [[], []], [[], []]
    for t in range(hops):
        if t == t0:
            st = a.export_slots([1, 0])
            assert st.tensors["gate_flags"].tolist()[0] != 0 and int(st.tensors["gate_fill"][0]) > 0
            assert int(st.tensors["gate_sources"][0, 0]) >= 0 and st.tensors["gate_line"][0].any()
            with pytest.raises(ValueError):
                GatedScorer(_inner(kind, 3), SpeechGate()).import_slots([2, 0], _move(st))
            with pytest.raises(ValueError):
                GatedScorer(_inner(kind, 3), LookaheadGate(pre=4)).import_slots([2, 0], _move(st))
            b.import_slots([2, 0], _move(st))  # session 1 -> slot 2, session 0 -> slot 0
        gs, named, order = (a, [0, 1], [0, 1]) if t < t0 else (b, [2, 0], [1, 0])
        out = gs.push(torch.stack([dev[i][t * H:(t + 1) * H] for i in order]), named)
        for i, v, e, sp in zip(order, out, gs.emitted(out).tolist(), gs.last_span.tolist()):
            if e:
                got[i].append(v.clone())
                spans[i].append(sp)
    refs = [gate.gate_reference(x) for x in STREAMS[:2]]
    assert all(len(g) > t0 // 2 for g in got)
    _check_scores(kind, got, [r[1] for r in refs])
    assert spans == [_spans(r[2]) for r in refs]  # (the source indices moved with the pending frames)
    assert b.samples_seen.tolist() == [hops * H, 0, hops * H]


def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the reference decodes the same bytes)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def test_lookahead_gate_behind_the_packet_front():
    from afx.ingest import PacketScorer, decode
    from afx.resample import Resampler
    from afx.vad import GatedScorer, LookaheadGate, emitted
    S, kind, gate = 3, "kv", LookaheadGate(pre=5)
    ps = PacketScorer(GatedScorer(_inner(kind, S), gate), 8000, "mulaw")
    codes = [_mulaw_encode(x[::2]) for x in STREAMS]  # 8 kHz by plain slicing, 6 s each
    got = [[] for _ in range(S)]
    for k in range(0, codes[0].size, 160):  # 20-ms packets
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        res = ps.feed([codes[s][k:k + 160].tobytes() for s in named], named)
        for s, part in zip(named, res.split()):
            got[s] += [v.clone() for v in part[emitted(part)]]
    seen = ps.samples_seen.tolist()
    R = [Resampler(8000)(decode(c, "mulaw")[None])[0].cpu().numpy()[:n] for c, n in zip(codes, seen)]
    assert all(_differs(gate, r) for r in R) and min(seen) >= 23 * H
    G = [gate.gate_reference(r)[1] for r in R]
    assert min(g.size // H for g in G) >= 5
    _check_scores(kind, got, G)


# ---- 3. the offline form ---------------------------------------------------------------------------------------------------------
def test_offline_gate_equals_the_dilated_mask():
    from afx.vad import LookaheadGate
    for pre in (1, 5, 31):
        gate = LookaheadGate(pre=pre)
        lens = [0, 1, pre, 600, 600]
        clips = [X[:m * 160].copy() for m in lens[:4]] + [np.roll(X, -(4000 + 37))[:600 * 160 + 77]]
        assert _differs(gate, clips[3]) and _differs(gate, clips[4][:96000])
        outs, masks, srcs = gate.gate([torch.from_numpy(c).cuda() for c in clips], return_mask=True, return_sources=True)
        for c, m, o, mk, sr in zip(clips, lens, outs, masks, srcs):
            c = c[:m * 160]
            kd = dilated(gate, c)[1] if m else np.zeros(0, dtype=bool)
            assert mk.dtype == torch.bool and mk.cpu().numpy().tolist() == kd.tolist(), (pre, m)
            assert sr.dtype == torch.int64 and sr.cpu().numpy().tolist() == np.flatnonzero(kd).tolist(), (pre, m)
            assert o.cpu().numpy().tobytes() == c.reshape(m, 160)[kd].tobytes(), (pre, m)
    only = LookaheadGate().gate(torch.from_numpy(np.stack([X[:8000], X[8000:16000]])).cuda())
    assert isinstance(only, list) and len(only) == 2 and only[1].numel() == dilated(LookaheadGate(), X[8000:16000])[1].sum() * 160

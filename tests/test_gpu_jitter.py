"""The jitter buffer on the GPU (afx/jitter.py, afx_k_jitter_place / _conceal / _release).  The reference for the played-out
stream E is oracle/jitter.py's ``RefSlot`` in numpy: decode tables, received-sample bookkeeping (first arrival wins, late
samples dropped), the playout rule and the concealment recurrence over E itself.  A slot's popped 16 kHz stream must be bit-identical to the
offline ``Resampler`` over that E (and within 2e-6 * max|x| of float64 upfirdn) at four rates, in all four encodings and
both concealment modes, under a network that drops 5 % of the packets, duplicates some and shuffles within the depth,
with two gaps closer than P in one release, a gap longer than F and a jump longer than the ring.  The corollaries:
shuffled lossless delivery with duplicates equals an in-order ``PacketScorer``, and ``depth = 0`` in-order delivery equals
it call by call.  And over each streaming scorer the scores equal, bit for bit and in the call that releases the hop's last
sample, those of a fresh inner scorer pushed the offline stream -- through a reset, a starving slot, buffered feeds with
drains, ``advance``, ``flush`` and a session exported mid-gap through torch.save into another scorer."""
import io
import random

import numpy as np
import pytest
import torch

from oracle.jitter import BPS, ENCODINGS, RefSlot, Schedule as _Schedule, packet
from packet_helpers import offline as _offline, ref64 as _ref64, tap as _tap

pytestmark = pytest.mark.gpu

H = 4000


def _stream(encoding, n, seed):
    return packet(encoding, n, np.random.default_rng(seed))


def Schedule(rate, encoding, seed, P=0, **kw):
    return _Schedule(rate, encoding, seed, short=max(1, P // 2), **kw)


@pytest.mark.parametrize("mode", ["repeat", "zero"])
@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("rate", [8000, 11025, 16000, 48000])
def test_played_out_stream_is_the_offline_resampling_of_the_numpy_stream(rate, encoding, mode):
    from afx.jitter import JitterScorer
    S = 3
    depth = 3 * (rate // 50)  # 60 ms
    tap = _tap(S)
    js = JitterScorer(tap, rate, encoding, depth, conceal=mode, max_pending=3)
    P, F = rate // 100, 3 * (rate // 100)
    assert (js.period, js.fade_len) == ((P, F) if mode == "repeat" else (0, 0))
    seed = rate + 31 * ENCODINGS.index(encoding) + (7 if mode == "zero" else 0)
    rng = random.Random(seed)
    sch = [Schedule(rate, encoding, seed + 1000 * s, jump=js.J + 123 + s, P=P, origin=(1 << 32) - 3000 if s == 0 else None)
           for s in range(S)]
    refs = [RefSlot(depth, mode, P, F) for sc in sch]
    hops = [0] * S
    while not all(sc.done() for sc in sch):
        ticks = {s: sch[s].tick() for s in range(S) if not sch[s].done() and rng.random() < 0.8}
        order = [s for s, r in ticks.items() for _ in r]
        if not order:
            continue
        rng.shuffle(order)  # the slots' rows interleaved, each slot's own rows in their order of arrival
        its = {s: iter(r) for s, r in ticks.items()}
        rows = [(s,) + next(its[s]) for s in order]
        named = []
        for s, ts, t, raw, x, e in rows:
            refs[s].packet(t, x)
            named += [s] if s not in named else []
        for s in named:
            refs[s].after_feed()
        made = {s: -(-refs[s].next * js.L // js.M) for s in named}
        score = rng.random() < 0.6 or any(made[s] - hops[s] * H > 3 * H for s in named)
        res = js.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows], score=score)
        assert res.counts.shape == (len(rows),) and res.scores.shape == (int(res.counts.sum()),)
        for s in named:
            if score:  # every hop whose last input sample has been released is out, in this call
                assert len(tap.got[s]) == made[s] // H and int(js.pending[s]) == made[s] % H
            assert int(js.pending[s]) + H * len(tap.got[s]) == made[s] and int(js.samples_in[s]) == refs[s].next
            assert int(js.buffered[s]) == refs[s].hi - refs[s].next <= depth
            hops[s] = len(tap.got[s])
    js.flush()
    st = js.stats()
    for s in range(S):
        r = refs[s]
        r.release(r.hi)
        assert int(js.samples_in[s]) == r.next == r.hi and int(js.buffered[s]) == 0
        assert (int(st["received"][s]), int(st["late"][s]), int(st["duplicate"][s]), int(st["concealed"][s])) == \
            tuple(r.stats[k] for k in ("received", "late", "duplicate", "concealed"))
        # the traffic was what the issue asks for: two gaps closer than P in one release, a gap beyond the fade, a jump beyond J
        assert any(len(g) >= 2 and any(b[0] - a[1] < max(P, 1) for a, b in zip(g, g[1:])) for g in r.releases)
        lens = [e - a for a, e in r.spans]
        assert max(lens) > js.J and sum(1 for n in lens if F + P < n < js.J) >= 1 and r.stats["duplicate"] > 0 and len(sch[s].lost) >= 6
        E = np.array(r.E, dtype=np.float32)
        if mode == "repeat":  # concealed samples are there, and they are not zeros
            a, e = next((a, e) for a, e in r.spans if a >= 10 * (rate // 50))
            assert np.count_nonzero(E[a:min(e, a + F)]) > 0.8 * min(e - a, F) - 1
        whole = _offline(E, rate)
        n_h = whole.numel() // H
        assert len(tap.got[s]) == n_h >= 6 and int(js.pending[s]) == whole.numel() - n_h * H
        got = torch.cat(tap.got[s])
        assert torch.equal(got, whole[: n_h * H]), (rate, encoding, mode, s)
        assert np.abs(got.cpu().double().numpy() - _ref64(E, rate)[: n_h * H]).max() <= 2e-6 * float(np.abs(E).max())
        ex = js.export_slots([s])
        k = int(ex.tensors["jitter_fill"][0])
        assert torch.equal(ex.tensors["jitter_pending"][0, :k], whole[n_h * H:]) and not ex.tensors["jitter_pending"][0, k:].any()


@pytest.mark.parametrize("rate,encoding", [(8000, "alaw"), (11025, "pcm_s16le"), (48000, "pcm_f32le"), (16000, "mulaw")])
def test_shuffled_lossless_delivery_with_duplicates_equals_an_in_order_packet_scorer(rate, encoding):
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    S, depth = 2, 3 * (rate // 50)
    tj, tp = _tap(S), _tap(S)
    js, ps = JitterScorer(tj, rate, encoding, depth), PacketScorer(tp, rate, encoding)
    sch = [Schedule(rate, encoding, 5 * rate + s, lossy=False, origin=(1 << 32) - 777 if s else 12345) for s in range(S)]
    while not all(sc.done() for sc in sch):
        rows = [(s,) + r for s in range(S) if not sch[s].done() for r in sch[s].tick()]
        js.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
    js.flush()
    ps.feed([sc.raw for sc in sch], [0, 1])
    st = js.stats()
    assert st["late"].tolist() == [0, 0] and st["concealed"].tolist() == [0, 0] and min(st["duplicate"].tolist()) > 0
    assert min(st["out_of_order"].tolist()) > 5 and st["received"].tolist() == [len(sc.x) for sc in sch]
    for s in range(S):
        assert len(tj.got[s]) == len(tp.got[s]) >= 5 and torch.equal(torch.cat(tj.got[s]), torch.cat(tp.got[s]))
        assert int(js.pending[s]) == int(ps.pending[s]) and int(js.samples_in[s]) == int(ps.samples_in[s])
        k = int(js.pending[s])
        assert torch.equal(js.export_slots([s]).tensors["jitter_pending"][0, :k], ps.export_slots([s]).tensors["ingest_pending"][0, :k])


@pytest.mark.parametrize("rate,encoding", [(8000, "mulaw"), (44100, "pcm_s16le"), (16000, "pcm_f32le")])
def test_depth_zero_in_order_is_the_packet_scorer_call_by_call(rate, encoding):
    from afx.ingest import PacketScorer
    from afx.jitter import JitterScorer
    S = 3
    tj, tp = _tap(S), _tap(S)
    js, ps = JitterScorer(tj, rate, encoding, 0, ts_bits=None), PacketScorer(tp, rate, encoding)
    rng = random.Random(rate)
    raw, _ = _stream(encoding, 6 * H * rate // 16000, rate)
    bps, fed = BPS[encoding], [0] * S
    sizes = [0, 1, 7, rate // 50, rate // 50, 3 * rate // 100 + 1, int(2.3 * H * rate / 16000)]
    for step in range(60):
        named = rng.sample(range(S), rng.randint(1, S))
        ns = [min(rng.choice(sizes), len(raw) // bps - fed[s]) for s in named]
        score = step % 3 != 1 or any(int(ps.pending[s]) + 2 * n + 2 > 4 * H for s, n in zip(named, ns))
        pk = [raw[fed[s] * bps:(fed[s] + n) * bps] for s, n in zip(named, ns)]
        a = js.feed(pk, named, [10 ** 12 + fed[s] for s in named], score=score)
        b = ps.feed(pk, named, score=score)
        assert a.counts.tolist() == b.counts.tolist()
        for s, n in zip(named, ns):
            fed[s] += n
        if step % 5 == 4:
            assert js.drain().counts.tolist() == ps.drain().counts.tolist()
        assert js.pending.tolist() == ps.pending.tolist() and js.samples_in.tolist() == ps.samples_in.tolist() == fed
        for s in range(S):
            assert len(tj.got[s]) == len(tp.got[s]) and (not tj.got[s] or torch.equal(tj.got[s][-1], tp.got[s][-1]))
    assert min(len(g) for g in tj.got) >= 3
    for s in range(S):
        assert torch.equal(torch.cat(tj.got[s]), torch.cat(tp.got[s]))


# ---- the contract, over the real scorers -----------------------------------------------------------------------------------
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


class _Pair:
    """A JitterScorer and the reference it must equal: per slot the numpy stream E, and a fresh inner scorer of the same
    kind pushed ``Resampler(rate)(E)`` hop by hop (with the same resets)."""

    def __init__(self, kind, S, rate, encoding, depth, mode, max_pending):
        from afx.jitter import JitterScorer
        self.P = JitterScorer(_inner(kind, S), rate, encoding, depth, conceal=mode, max_pending=max_pending)
        self.R, self.rate = _inner(kind, S), rate
        self.ref, self.sch, self.checked, self.begun = {}, {}, {}, set()

    def start(self, s, sch):
        self.sch[s], self.checked[s] = sch, 0
        self.begun.discard(s)  # (a session's origin is its first packet: before it there is nothing to play out)
        self.ref[s] = RefSlot(self.P.depth, self.P.conceal, self.P.period, self.P.fade_len)

    def made(self, s):
        return -(-self.ref[s].next * self.P.L // self.P.M)

    def check(self, res, named, scoring=True):
        """``named``: the distinct slots of the call in the order of their first rows; res.counts may carry zeros for the
        later rows of a slot."""
        want = [self.made(s) // H - self.checked[s] if scoring else 0 for s in named]
        counts = [c for c in res.counts.tolist()]
        assert sum(counts) == sum(want) and res.scores.is_cuda and res.scores.numel() == sum(want)
        parts = [p for p in res.split() if p.numel()]
        assert [p.numel() for p in parts] == [w for w in want if w]
        parts = iter(parts)
        for s, w in zip(named, want):
            got = next(parts) if w else res.scores[:0]
            offline = _offline(self.ref[s].E, self.rate) if w else None
            for j in range(w):  # every emitted score of every slot
                hop = offline[self.checked[s] * H:(self.checked[s] + 1) * H]
                ref = self.R.push(hop[None].contiguous(), [s])
                assert torch.equal(got[j:j + 1], ref), (s, self.checked[s])
                self.checked[s] += 1
            assert int(self.P.pending[s]) == self.made(s) - self.checked[s] * H and int(self.P.samples_in[s]) == self.ref[s].next
        assert torch.equal(self.P.samples_seen, self.R.samples_seen)

    def feed(self, slots_ticks, score=True):
        """One ``feed`` with the next tick of each named slot (rows shuffled by the caller's order)."""
        rows = [(s,) + r for s in slots_ticks for r in self.sch[s].tick()]
        named = []
        for s, ts, t, raw, x, e in rows:
            self.ref[s].packet(t, x)
            named += [s] if s not in named else []
        for s in named:
            self.ref[s].after_feed()
        self.begun.update(named)
        if not score and any(self.made(s) - self.checked[s] * H > self.P.max_pending * H for s in named):
            score = True
        res = self.P.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows], score=score)
        self.check(res, named, scoring=score)
        return res


_FRONT = ("jitter_pending", "jitter_fill", "jitter_ring", "jitter_book", "jitter_stats", "jitter_intervals")


def _snap(P, slots):
    st = P.export_slots(slots)
    out = [st.seen] + [st.tensors[k].clone() for k in _FRONT]
    begun = [s for s, n in zip(slots, st.seen.tolist()) if n > 0]
    inner = P.scorer.export_slots(begun)
    return out + [inner.seen] + [inner.tensors[k].clone() for k in sorted(inner.tensors)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


@pytest.mark.parametrize("rate,encoding,mode", [(8000, "mulaw", "repeat"), (11025, "pcm_s16le", "zero")])
@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv", "kv-fp16x3"])
def test_jitter_scores_equal_inner_on_the_offline_stream(kind, rate, encoding, mode):
    from afx.ingest import PacketScorer
    from afx.streaming import ResamplingScorer, StreamState
    rng = random.Random(rate + len(kind))
    depth = 3 * (rate // 50)
    seeds = iter(range(1000 * len(kind) + rate, 10 ** 9, 17))
    X = _Pair(kind, 3, rate, encoding, depth, mode, max_pending=4)
    P = X.P
    new = lambda jump=0: Schedule(rate, encoding, next(seeds), jump=jump, P=P.period, n_pk=150)
    for s in range(3):
        X.start(s, new(jump=P.J + 50 if s == 2 else 0))
    moved = None
    for t in range(400):
        if all(X.sch[s].done() for s in X.sch) or moved is not None:
            break
        if t == 9:  # a reset mid-stream: slot 1 starts a new session
            P.reset([1])
            X.R.reset([1])
            X.start(1, new())
            assert int(P.pending[1]) == 0 and int(P.samples_in[1]) == 0 and int(P.buffered[1]) == 0
        live = [s for s in ([0, 1] if 3 <= t < 20 else [0, 1, 2]) if not X.sch[s].done()]  # slot 2 starves for many feeds
        if not live:
            continue
        named = rng.sample(live, rng.randint(1, len(live)))
        idle = [s for s in range(3) if s not in named]
        before = _snap(P, idle)
        X.feed(named, score=t % 4 != 2)
        assert _same(before, _snap(P, idle))  # slots not named are untouched, byte for byte
        if t % 4 == 3:  # the hops buffered by the feed before this one come out of a drain
            sub = rng.sample(range(3), 2) if t % 8 == 3 else None
            X.check(P.drain(sub), list(range(3)) if sub is None else sub)
        if t % 11 == 6 and X.begun & set(live):  # clock-driven playout: half the depth further, or beyond everything received
            s = rng.choice(sorted(X.begun & set(live)))
            upto = X.ref[s].next + (depth // 2 if t % 2 else depth + 33)
            X.ref[s].release(upto)
            X.check(P.advance([s], upto), [s])
        if t % 13 == 8:
            s = rng.choice(live)
            X.ref[s].release(X.ref[s].hi)
            X.check(P.flush([s]), [s])
        # move slot 0's session, while its playout point stands in a gap, into slot 1 of a 2-slot scorer
        if t > 12 and X.ref[0].gap is not None and X.ref[0].hi > X.ref[0].next and not X.sch[0].done():
            moved = t
    assert moved is not None and X.checked[0] >= 1
    assert int(P.export_slots([0]).tensors["jitter_book"][0, 4]) == X.ref[0].gap >= 0  # mid-gap: the open gap's origin travels
    Y = _Pair(kind, 2, rate, encoding, depth, mode, max_pending=5)
    for s in range(2):
        Y.start(s, Schedule(rate, encoding, next(seeds), P=P.period, n_pk=150))
    for t in range(5):
        Y.feed([1, 0])
    src_before, keep_before = _snap(P, [0, 1, 2]), _snap(Y.P, [0])
    st = P.export_slots([0])
    assert set(st.tensors) >= set(_FRONT) and "resample_hist" not in st.tensors
    assert st.meta["input_rate"] == rate and st.meta["jitter"] == 1 and st.meta["jitter_depth"] == depth
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    st2 = StreamState.from_state_dict(torch.load(buf, weights_only=True))
    Y.P.import_slots([1], st2)
    Y.R.import_slots([1], X.R.export_slots([0]))
    assert _same(src_before, _snap(P, [0, 1, 2])) and _same(keep_before, _snap(Y.P, [0]))
    a, b = _snap(P, [0]), _snap(Y.P, [1])
    assert _same(a[:1] + a[2:7], b[:1] + b[2:7]) and torch.equal(a[1].cpu(), b[1][:, :4 * H].cpu())  # the jitter part arrives as it left
    Y.sch[1], Y.ref[1], Y.checked[1] = X.sch[0], X.ref[0], X.checked[0]
    assert {k: int(v[1]) for k, v in Y.P.stats().items()} == {k: int(v[0]) for k, v in P.stats().items()}
    n0 = Y.checked[1]
    Y.check(Y.P.drain([1]), [1])
    while not Y.sch[1].done():
        named = [1] if Y.sch[0].done() or rng.random() < 0.5 else [1, 0]
        Y.feed(named)
    for s in (1, 0):
        Y.ref[s].release(Y.ref[s].hi)
    Y.check(Y.P.flush([1, 0]), [1, 0])
    assert Y.checked[1] >= n0 + 3 and Y.ref[1].stats["concealed"] > 0
    assert int(Y.P.stats()["concealed"][1]) == Y.ref[1].stats["concealed"] and int(Y.P.stats()["late"][1]) == Y.ref[1].stats["late"]
    # a packet, a resampling and a bare state are refused before anything changes, and the reverse
    keep = _snap(Y.P, [0, 1])
    for foreign in (PacketScorer(_inner(kind, 2), rate, encoding).export_slots([0]), X.R.export_slots([0]),
                    ResamplingScorer(_inner(kind, 2), 8000).export_slots([0])):
        with pytest.raises(ValueError):
            Y.P.import_slots([0], foreign)
    for dst in (X.R, PacketScorer(_inner(kind, 2), rate, encoding), ResamplingScorer(_inner(kind, 2), 8000)):
        with pytest.raises(ValueError):
            dst.import_slots([0], st2)
    assert _same(keep, _snap(Y.P, [0, 1]))


def test_feed_rtp_on_the_gpu_equals_feed():
    import struct
    from afx.jitter import JitterScorer
    rate, n = 8000, 160
    ta, tb = _tap(1), _tap(1)
    a, b = JitterScorer(ta, rate, "mulaw", 480), JitterScorer(tb, rate, "mulaw", 480)
    raw, _ = _stream("mulaw", 60 * n, 3)
    order = [k for k in range(60) if k not in (7, 20, 21)]
    order[30], order[32], order[40], order[41] = order[32], order[30], order[41], order[40]
    for k in order:
        ts = ((1 << 32) - 1000 + k * n) % (1 << 32)
        pay = raw[k * n:(k + 1) * n]
        d = struct.pack("!BBHII", 0x80, 0, (65530 + k) & 0xFFFF, ts, 0xABCD) + pay
        a.feed_rtp([d], [0])
        b.feed([pay], [0], [ts])
    a.flush()
    b.flush()
    assert len(ta.got[0]) == len(tb.got[0]) >= 4 and torch.equal(torch.cat(ta.got[0]), torch.cat(tb.got[0]))
    assert int(a.stats()["concealed"][0]) == 3 * n == int(b.stats()["concealed"][0])

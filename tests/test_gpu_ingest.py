"""The packet front on the GPU (afx/ingest.py, afx_k_ingest / afx_k_ingest_pop): ``decode`` is exact for every G.711 code
and every int16 value; a slot's popped 16 kHz stream is bit-identical to the offline ``Resampler`` over its whole decoded
stream (and within 2e-6 * max|x| of float64 upfirdn) whatever the packet sizes, named subsets, order, rate and encoding;
and a ``PacketScorer`` over each streaming scorer emits, bit for bit and in the feed / drain where the hop completes, the
scores of a fresh inner scorer pushed that offline stream hop by hop -- through a reset, a slot that starves, buffered
feeds with drains, a packet of three hops, and a session moved through host memory and torch.save into another scorer."""
import copy
import io
import random

import numpy as np
import pytest
import torch

from oracle.jitter import BPS, ENCODINGS, TABLES, packet
from packet_helpers import ref64 as _ref64, tap as _tap

pytestmark = pytest.mark.gpu

H = 4000


def _stream(encoding, n, seed):
    """n random samples as ``encoding`` (16-bit ones at full scale) -> (the bytes, their host-decoded fp32 values)."""
    return packet(encoding, n, np.random.default_rng(seed), div=1)


def test_decode_is_exact_for_every_code_and_every_int16():
    from afx.ingest import decode
    codes = bytes(range(256))
    for law in ("mulaw", "alaw"):
        got = decode(codes, law)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (256,)
        assert torch.equal(got.cpu(), torch.from_numpy(TABLES[law]))
        assert torch.equal(decode(np.frombuffer(codes, dtype=np.uint8)[::-1].copy(), law).cpu().flip(0), got.cpu())
    v = np.arange(-32768, 32768, dtype=np.int16)
    want = torch.from_numpy(v.astype(np.float32) / np.float32(32768))
    assert torch.equal(decode(v, "pcm_s16le").cpu(), want)
    assert torch.equal(decode(v.astype("<i2").tobytes(), "pcm_s16le").cpu(), want)
    f = np.array([0.0, -0.0, 1.0, -1.5, 3e-39, np.float32(np.pi), -65504.0], dtype=np.float32)
    assert decode(f, "pcm_f32le").cpu().numpy().tobytes() == f.tobytes()  # bit for bit, the sign of zero and denormals included
    assert decode(b"", "mulaw").shape == (0,)
    with pytest.raises(ValueError):
        decode(b"abc", "pcm_s16le")


# ---- ragged resampling alone: a scorer that only records what it is pushed -----------------------------------------------
def _sizes(rate, T):
    hop_in = H * rate / 16000
    out = [0, 1, 7, rate // 50, {8000: 263, 11025: 367, 16000: 523, 22050: 727, 44100: 1453, 48000: 1583, 96000: 3167}[rate],
           int(2.3 * hop_in)]
    if T - 2 > 0:
        out.append(T - 2)
    return out


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("rate", [8000, 11025, 22050, 44100, 48000, 96000, 16000])
def test_ragged_packets_resample_like_the_whole_stream(rate, encoding):
    from afx.ingest import PacketScorer, decode, plan
    from afx.resample import Resampler
    S, MAXP = 5, 3
    rs = Resampler(rate)
    tap = _tap(S)
    ps = PacketScorer(tap, rate, encoding, max_pending=MAXP)
    rng = random.Random(rate * 7 + len(encoding))
    sizes, bps = _sizes(rate, rs.T), BPS[encoding]
    total = int(5.4 * H * rate / 16000) + 11  # samples per slot
    streams = [_stream(encoding, total, seed=rate + 97 * s + len(encoding)) for s in range(S)]
    fed, hops = [0] * S, [0] * S
    guard = 0
    while min(fed) < total:
        guard += 1
        assert guard < 5000
        named = [s for s in range(S) if fed[s] < total and rng.random() < 0.7]
        rng.shuffle(named)
        if not named:
            continue
        ns = [min(total - fed[s], rng.choice(sizes)) for s in named]
        score = rng.random() < 0.6 or any(
            int(ps.pending[s]) + plan(fed[s], n, rs.L, rs.M)[0] > MAXP * H for s, n in zip(named, ns))
        res = ps.feed([streams[s][0][fed[s] * bps:(fed[s] + n) * bps] for s, n in zip(named, ns)], named, score=score)
        for s, n in zip(named, ns):
            fed[s] += n
        if rng.random() < 0.25:  # a drain of some slots, named or not
            sub = rng.sample(range(S), rng.randint(1, S))
            res2 = ps.drain(sub)
            assert res2.counts.tolist() == [len(tap.got[s]) - hops[s] - (res.counts[named.index(s)].item() if s in named else 0)
                                            for s in sub]
            assert all(int(ps.pending[s]) < H for s in sub)
        for i, s in enumerate(named):
            made = -(-fed[s] * rs.L // rs.M)
            if score:  # every hop the slot's stream has completed is out, in this call
                assert len(tap.got[s]) == made // H and int(ps.pending[s]) == made % H
            assert int(ps.pending[s]) + H * len(tap.got[s]) == made
        assert res.scores.shape == (int(res.counts.sum()),) and (score or int(res.counts.sum()) == 0)
        hops = [len(g) for g in tap.got]
        assert ps.samples_in.tolist() == fed
    ps.drain()
    for s in range(S):
        x = streams[s][1]
        dec = decode(streams[s][0], encoding)
        assert torch.equal(dec.cpu(), torch.from_numpy(x))
        whole = rs(dec[None])[0]
        n_h = whole.numel() // H
        assert len(tap.got[s]) == n_h >= 5 and int(ps.pending[s]) == whole.numel() - n_h * H
        got = torch.cat(tap.got[s])
        assert torch.equal(got, whole[: n_h * H]), (rate, encoding, s)
        assert np.abs(got.cpu().double().numpy() - _ref64(x, rate)[: n_h * H]).max() <= 2e-6 * float(np.abs(x).max())
        # what is still pending is the stream's tail
        st = ps.export_slots([s])
        k = int(st.tensors["ingest_fill"][0])
        assert torch.equal(st.tensors["ingest_pending"][0, :k], whole[n_h * H:]) and not st.tensors["ingest_pending"][0, k:].any()


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


class _Session:
    """One stream: its bytes, and the offline kernel's 16 kHz version of the whole decoded stream."""

    def __init__(self, rate, encoding, n, seed):
        from afx.ingest import decode
        from afx.resample import Resampler
        self.bytes, _ = _stream(encoding, n, seed)
        if encoding == "pcm_s16le":  # speech-like levels rather than full-scale noise
            v = (np.frombuffer(self.bytes, dtype="<i2") // 8).astype("<i2")
            self.bytes = v.tobytes()
        self.offline = Resampler(rate)(decode(self.bytes, encoding)[None])[0]
        self.n, self.bps, self.fed, self.checked = n, BPS[encoding], 0, 0

    def take(self, n):
        n = min(n, self.n - self.fed)
        b = self.bytes[self.fed * self.bps:(self.fed + n) * self.bps]
        self.fed += n
        return b


class _Pair:
    """A PacketScorer and the reference it must equal: a fresh inner scorer of the same kind and S, pushed each session's
    offline stream hop by hop (with the same resets)."""

    def __init__(self, kind, S, rate, encoding, max_pending):
        from afx.ingest import PacketScorer
        self.P, self.R = PacketScorer(_inner(kind, S), rate, encoding, max_pending=max_pending), _inner(kind, S)
        self.sess = {}

    def expect(self, s):
        """Hops of slot s's session that are complete but not yet emitted."""
        se = self.sess[s]
        return -(-se.fed * self.P.L // self.P.M) // H - se.checked

    def check(self, res, named, scoring=True):
        want = [self.expect(s) if scoring else 0 for s in named]
        assert res.counts.tolist() == want, (res.counts.tolist(), want)
        parts = res.split()
        assert len(parts) == len(named) and res.scores.is_cuda and res.scores.numel() == sum(want)
        for s, got in zip(named, parts):
            se = self.sess[s]
            for j in range(got.numel()):  # every emitted score of every slot
                hop = se.offline[se.checked * H:(se.checked + 1) * H]
                ref = self.R.push(hop[None].contiguous(), [s])
                assert torch.equal(got[j:j + 1], ref), (s, se.checked)
                se.checked += 1
            assert int(self.P.pending[s]) == -(-se.fed * self.P.L // self.P.M) - se.checked * H
        assert torch.equal(self.P.samples_seen, self.R.samples_seen)


_FRONT = ("ingest_pending", "ingest_fill", "ingest_in", "resample_hist")


def _snap(P, slots):
    """Everything the named slots hold: the packet front's part of every slot, and the inner scorer's part of every slot
    whose session has been pushed a hop (before that an inner session is empty, and the width of its empty conv carries
    follows the scorer's other slots)."""
    st = P.export_slots(slots)
    out = [st.seen] + [st.tensors[k].clone() for k in _FRONT]
    begun = [s for s, n in zip(slots, st.seen.tolist()) if n > 0]
    inner = P.scorer.export_slots(begun)
    return out + [inner.seen] + [inner.tensors[k].clone() for k in sorted(inner.tensors)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


@pytest.mark.parametrize("rate,encoding", [(8000, "mulaw"), (11025, "pcm_s16le")])
@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv", "kv-fp16x3"])
def test_packet_scores_equal_inner_on_the_offline_stream(kind, rate, encoding):
    from afx.ingest import PacketScorer
    from afx.streaming import StreamState
    rng = random.Random(rate + len(kind))
    hop_in = H * rate // 16000 + 1
    n_sess = 60 * hop_in
    seeds = iter(range(1000 * len(kind) + rate, 10 ** 9))
    new = lambda: _Session(rate, encoding, n_sess, next(seeds))
    X = _Pair(kind, 3, rate, encoding, max_pending=4)
    P = X.P
    X.sess = {s: new() for s in range(3)}
    small = [rate // 50, rate // 50, 3 * rate // 100 + 1, 0, 1, 7, rate // 100]
    for t in range(30):
        if t == 9:  # a reset mid-stream: slot 1 starts a new session
            P.reset([1])
            X.R.reset([1])
            X.sess[1] = new()
            assert int(P.pending[1]) == 0 and int(P.samples_in[1]) == 0
        live = [0, 1] if 3 <= t < 20 else [0, 1, 2]  # slot 2 receives nothing for many feeds
        named = rng.sample(live, rng.randint(1, len(live)))
        ns = [rng.choice(small) * rng.choice([1, 6, 12]) for _ in named]
        score = t % 4 != 2
        if t == 12:  # one packet that completes three hops at once
            named, ns, score = [0, 1], [int(3.1 * hop_in), rate // 50], True
        if t == 21:  # the starved slot comes back with more than two hops
            named, ns, score = [2, 1], [int(2.2 * hop_in), int(2.2 * hop_in)], True
        if not score and any(int(P.pending[s]) + 2 * n + 2 > 4 * H for s, n in zip(named, ns)):  # (at most 2 outputs per input)
            score = True
        idle = [s for s in range(3) if s not in named]
        before = _snap(P, idle)
        res = P.feed([X.sess[s].take(n) for s, n in zip(named, ns)], named, score=score)
        assert _same(before, _snap(P, idle))  # slots not named are untouched, byte for byte
        if t == 12:
            assert int(res.counts[0]) >= 3
        X.check(res, named, scoring=score)
        if t % 4 == 3:  # the hops buffered by the feed before this one (and anything else complete) come out of a drain
            sub = rng.sample(range(3), 2) if t % 8 == 3 else None
            order = list(range(3)) if sub is None else sub
            X.check(P.drain(sub), order)
    assert X.sess[0].checked >= 3 and all(X.sess[s].checked >= 2 for s in range(3))
    X.check(P.drain(), [0, 1, 2])

    # move slot 0's session, with more than a hop pending, into slot 1 of a 2-slot scorer with another max_pending
    named = [0]
    res = P.feed([X.sess[0].take(int(1.3 * hop_in))], named, score=False)
    X.check(res, named, scoring=False)
    assert int(P.pending[0]) >= H
    Y = _Pair(kind, 2, rate, encoding, max_pending=3)
    Y.sess = {0: new(), 1: new()}
    for t in range(3):
        Y.check(Y.P.feed([Y.sess[s].take(rate // 50 * 7) for s in (1, 0)], [1, 0]), [1, 0])
    src_before, keep_before = _snap(P, [0, 1, 2]), _snap(Y.P, [0])
    st = P.export_slots([0])
    assert set(st.tensors) >= {"ingest_pending", "ingest_fill", "ingest_in", "resample_hist"}
    assert st.meta["input_rate"] == rate and st.meta["resampler"] == "kaiser5-hl10" and st.meta["ingest"] == 1
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    st2 = StreamState.from_state_dict(torch.load(buf, weights_only=True))
    Y.P.import_slots([1], st2)
    Y.R.import_slots([1], X.R.export_slots([0]))
    assert _same(src_before, _snap(P, [0, 1, 2])) and _same(keep_before, _snap(Y.P, [0]))
    moved = X.sess[0]
    Y.sess[1] = copy.copy(moved)
    assert int(Y.P.pending[1]) == int(P.pending[0]) and int(Y.P.samples_in[1]) == moved.fed
    Y.check(Y.P.drain([1]), [1])  # the pending hop it brought along
    for t in range(6):
        named = [[1, 0], [1], [0, 1]][t % 3]
        Y.check(Y.P.feed([Y.sess[s].take(rng.choice(small) * 5) for s in named], named), named)
    assert Y.sess[1].checked > moved.checked
    # the source keeps going, untouched by the export
    X.check(P.feed([X.sess[s].take(rate // 50 * 9) for s in (2, 0, 1)], [2, 0, 1]), [2, 0, 1])
    # a state of another rate, a bare and a resampling state are refused before anything changes
    from afx.streaming import ResamplingScorer
    other = PacketScorer(_inner(kind, 2), 48000, "pcm_s16le")
    keep = _snap(Y.P, [0, 1])
    for foreign in (other.export_slots([0]), X.R.export_slots([0]), ResamplingScorer(_inner(kind, 2), 8000).export_slots([0])):
        with pytest.raises(ValueError):
            Y.P.import_slots([0], foreign)
    with pytest.raises(ValueError):
        X.R.import_slots([0], st2)
    assert _same(keep, _snap(Y.P, [0, 1]))

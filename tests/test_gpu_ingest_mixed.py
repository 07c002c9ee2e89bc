"""Several formats on one packet front, on the GPU (afx/ingest.py MixedPacketScorer, afx_k_ingest_mixed; afx/jitter.py with
a tuple of encodings, afx_k_jitter_place_mixed).  The reference is what this change leaves alone: the offline ``Resampler``
over ``decode`` of a slot's whole stream, the single-format ``PacketScorer`` and the single-encoding ``JitterScorer``.  Every
comparison is exact (``torch.equal``): the mixed launch gives an output the fmaf chain the one-format launch gives it."""
import random

import numpy as np
import pytest
import torch

from oracle.jitter import BPS, TABLES, packet, rtp
from packet_helpers import tap

pytestmark = pytest.mark.gpu

H = 4000
PRIME = {8000: 263, 11025: 367, 16000: 523, 22050: 727, 44100: 1453, 48000: 1583, 96000: 3167}


def _stream(encoding, n, seed, quiet=False):
    """n random samples as ``encoding`` -> their bytes (quiet: speech-like levels rather than full-scale noise)."""
    return packet(encoding, n, np.random.default_rng(seed), div=8 if quiet else 1)[0]


def _tap(S):
    return tap(S, clear_on_reset=True)


def _offline(data, rate, encoding):
    """The reference: the offline kernel over the whole decoded stream."""
    from afx.ingest import decode
    from afx.resample import Resampler
    return Resampler(rate)(decode(data, encoding)[None])[0]


def _sizes(rate, T):
    out = [0, 1, 7, rate // 50, PRIME[rate], int(2.3 * H * rate / 16000)]
    return out + ([T - 2] if T - 2 > 0 else [])


def _made(n, rate):
    from afx.resample import ratio
    L, M = ratio(rate)
    return -(-n * L // M)


RAGGED = [(8000, "mulaw"), (8000, "alaw"), (11025, "pcm_s16le"), (16000, "pcm_f32le"), (44100, "pcm_s16le"), (48000, "pcm_f32le")]


def test_ragged_mixed_feed_resamples_every_slot_like_its_whole_stream():
    from afx.ingest import MixedPacketScorer
    from afx.resample import Resampler
    S, MAXP, of = 7, 3, [0, 0, 1, 2, 3, 4, 5]
    tap = _tap(S)
    ms = MixedPacketScorer(tap, RAGGED, max_pending=MAXP)
    ms.reset(list(range(S)), of)
    fm = [RAGGED[f] for f in of]
    # the launch shapes this test is about: LDS taps with R = 1 and R = 8, taps from global memory, the identity, M / L = 3
    shape = {r: (x.L * (x.T | 1), x.identity) for r, x in ms._rs.items()}
    assert shape[8000][0] <= 1024 and shape[11025][0] == 13440 > 12288 and shape[16000][1] and 8 * 1024 <= shape[44100][0] <= 12288
    assert (ms._rs[48000].L, ms._rs[48000].M) == (1, 3) and ms.Hs == 60
    rng = random.Random(20260)
    total = [int(5.4 * H * r / 16000) + 11 for r, _ in fm]
    data = [_stream(e, total[s], seed=1000 + s) for s, (r, e) in enumerate(fm)]
    sizes = [_sizes(r, Resampler(r).T) for r, _ in fm]
    fed, hops, guard, buffered, drains = [0] * S, [0] * S, 0, 0, 0
    while min(f - t for f, t in zip(fed, total)) < 0:
        guard += 1
        assert guard < 5000
        named = [s for s in range(S) if fed[s] < total[s] and rng.random() < 0.7]
        rng.shuffle(named)
        if not named:
            continue
        ns = [min(total[s] - fed[s], rng.choice(sizes[s])) for s in named]
        score = rng.random() < 0.6 or any(int(ms.pending[s]) + _made(fed[s] + n, fm[s][0]) - _made(fed[s], fm[s][0]) > MAXP * H
                                          for s, n in zip(named, ns))
        buffered += not score
        res = ms.feed([data[s][fed[s] * BPS[fm[s][1]]:(fed[s] + n) * BPS[fm[s][1]]] for s, n in zip(named, ns)], named, score=score)
        for s, n in zip(named, ns):
            fed[s] += n
        assert res.scores.shape == (int(res.counts.sum()),) and (score or int(res.counts.sum()) == 0)
        if score:  # every hop a named slot's stream has completed is out, in this call
            assert all(len(tap.got[s]) == _made(fed[s], fm[s][0]) // H for s in named)
            assert res.counts.tolist() == [len(tap.got[s]) - hops[s] for s in named]
        hops = [len(g) for g in tap.got]
        if rng.random() < 0.25:  # a drain of some slots, named or not
            sub = rng.sample(range(S), rng.randint(1, S))
            res2 = ms.drain(sub)
            drains += 1
            assert res2.counts.tolist() == [len(tap.got[s]) - hops[s] for s in sub] and all(int(ms.pending[s]) < H for s in sub)
            hops = [len(g) for g in tap.got]
        # the host arithmetic, after every call
        assert ms.samples_in.tolist() == fed
        assert ms.pending.tolist() == [_made(fed[s], fm[s][0]) - H * hops[s] for s in range(S)]
        assert ms.samples_seen.tolist() == [H * h for h in hops]
    assert buffered >= 3 and drains >= 3
    ms.drain()
    assert ms.format_of.tolist() == of
    for s, (r, e) in enumerate(fm):
        whole = _offline(data[s], r, e)
        n_h = whole.numel() // H
        assert len(tap.got[s]) == n_h >= 5 and int(ms.pending[s]) == whole.numel() - n_h * H
        assert torch.equal(torch.cat(tap.got[s]), whole[: n_h * H]), (s, r, e)
        st = ms.export_slots([s])  # what is still pending is the stream's tail
        k = int(st.tensors["ingest_fill"][0])
        assert torch.equal(st.tensors["ingest_pending"][0, :k], whole[n_h * H:]) and not st.tensors["ingest_pending"][0, k:].any()
        own = 0 if r == 16000 else Resampler(r).T - 1
        assert not st.tensors["resample_hist"][0, own:].any() and (own == 0 or st.tensors["resample_hist"][0, :own].any())


def test_a_feed_of_every_format_is_one_ingest_call_per_round(monkeypatch):
    from afx._lib import lib
    from afx.ingest import MixedPacketScorer
    S, of = 7, [0, 0, 1, 2, 3, 4, 5]
    tap = _tap(S)
    ms = MixedPacketScorer(tap, RAGGED)
    ms.reset(list(range(S)), of)
    fm = [RAGGED[f] for f in of]
    l = lib()
    calls = {"afx_k_ingest_mixed": [], "afx_k_ingest": []}
    for name in calls:
        real = getattr(l, name)

        def counted(*args, _real=real, _name=name):
            calls[_name].append(args[3])  # rows
            return _real(*args)

        monkeypatch.setattr(l, name, counted)
    n = [int(0.6 * H * r / 16000) for r, _ in fm]  # less than a hop of audio each
    data = [_stream(e, 2 * n[s], seed=50 + s) for s, (r, e) in enumerate(fm)]
    order = [4, 0, 6, 2, 5, 1, 3]
    res = ms.feed([data[s][:n[s] * BPS[fm[s][1]]] for s in order], order)
    # one entry call = one ingest launch over all seven rows plus one history launch, whatever the number of formats
    assert calls == {"afx_k_ingest_mixed": [7], "afx_k_ingest": []} and int(res.counts.sum()) == 0
    assert ms.pending.tolist() == [_made(n[s], fm[s][0]) for s in range(S)]
    res = ms.feed([data[s][n[s] * BPS[fm[s][1]]:] for s in order], order)  # the second half completes one hop per slot
    assert calls == {"afx_k_ingest_mixed": [7, 7], "afx_k_ingest": []} and res.counts.tolist() == [1] * 7
    monkeypatch.undo()
    for s, (r, e) in enumerate(fm):
        assert torch.equal(tap.got[s][0], _offline(data[s], r, e)[:H]), (s, r, e)


def test_a_slot_changes_its_format_at_reset():
    from afx.ingest import MixedPacketScorer
    formats = [(48000, "pcm_f32le"), (8000, "alaw"), (11025, "pcm_s16le")]
    tap = _tap(3)
    ms = MixedPacketScorer(tap, formats)
    ms.reset([0, 1, 2], [0, 1, 2])
    fm = list(formats)
    total = [int(4.3 * H * r / 16000) + 5 for r, _ in fm]
    data = [_stream(e, total[s], seed=700 + s) for s, (r, e) in enumerate(fm)]
    fed = [0, 0, 0]

    def step(k):  # 20-ms packets times k, for every slot that has samples left
        named = [s for s in (2, 0, 1) if fed[s] < total[s]]
        ns = [min(total[s] - fed[s], k * fm[s][0] // 50 + s + 1) for s in named]
        ms.feed([data[s][fed[s] * BPS[fm[s][1]]:(fed[s] + n) * BPS[fm[s][1]]] for s, n in zip(named, ns)], named)
        for s, n in zip(named, ns):
            fed[s] += n

    for k in (3, 7, 1, 9, 5):  # two hops in 20-ms packets times k, and a few samples
        step(k)
    assert len(tap.got[0]) >= 1 and int(ms.pending[0]) > 0 and ms.hist[0].any()
    old = _offline(data[0][:fed[0] * 4], 48000, "pcm_f32le")
    assert torch.equal(torch.cat(tap.got[0]), old[: len(tap.got[0]) * H])
    others = ms.export_slots([1, 2])
    ms.reset([0], (8000, "alaw"))  # the 48 kHz slot starts an A-law call
    now = ms.export_slots([1, 2])
    assert all(torch.equal(others.tensors[k], now.tensors[k]) for k in others.tensors) and torch.equal(others.seen, now.seen)
    assert ms.format_of.tolist() == [1, 1, 2] and ms.rates.tolist() == [8000, 8000, 11025] and ms.delays.tolist()[0] == 20.0
    assert int(ms.pending[0]) == 0 and int(ms.samples_in[0]) == 0 and not ms.hist[0].any() and tap.got[0] == []
    fm[0], total[0], fed[0] = (8000, "alaw"), int(3.2 * H * 8000 / 16000) + 3, 0
    data[0] = _stream("alaw", total[0], seed=799)
    while min(f - t for f, t in zip(fed, total)) < 0:
        step(4)
    for s, (r, e) in enumerate(fm):  # slot 0 matches a fresh A-law stream, its neighbours their streams through the reset
        whole = _offline(data[s], r, e)
        n_h = whole.numel() // H
        assert len(tap.got[s]) == n_h >= 3 and torch.equal(torch.cat(tap.got[s]), whole[: n_h * H]), s
        assert int(ms.pending[s]) == whole.numel() - n_h * H


# ---- over the real scorers ---------------------------------------------------------------------------------------------------
_ENGINE = []


def _inner(kind, S):
    from afx import engine, synth
    from afx.streaming import IncrementalScorer, KVCachedScorer
    if not _ENGINE:
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINE.append((eng, sd))
    eng, sd = _ENGINE[0]
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


REAL = [(8000, "mulaw"), (8000, "alaw"), (16000, "pcm_s16le"), (48000, "pcm_s16le")]


def _cut(data, rate, encoding, rng):
    """A stream's bytes cut into packets of 20 ms times 1..12, a few odd ones among them."""
    out, at, bps = [], 0, BPS[encoding]
    while at < len(data):
        n = rng.choice([1, 1, 2, 6, 12]) * (rate // 50) + rng.choice([0, 0, 0, 1, 7])
        out.append(data[at:at + n * bps])
        at += n * bps
    return out


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_mixed_scores_equal_the_single_format_packet_scorers(kind):
    from afx.ingest import MixedPacketScorer, PacketScorer
    S = 4
    ms = MixedPacketScorer(_inner(kind, S), REAL)
    ms.reset([0, 1, 2, 3], [0, 1, 2, 3])
    refs = [PacketScorer(_inner(kind, S), r, e) for r, e in REAL]  # slot s's reference: a fresh inner scorer, fed slot s alone
    rng = random.Random(len(kind))
    packets = [_cut(_stream(e, int(5.3 * H * r / 16000), seed=300 + s, quiet=True), r, e, rng) for s, (r, e) in enumerate(REAL)]
    at, emitted = [0] * S, [0] * S
    while any(at[s] < len(packets[s]) for s in range(S)):
        named = [s for s in range(S) if at[s] < len(packets[s]) and rng.random() < 0.8]
        rng.shuffle(named)
        if not named:
            continue
        score = rng.random() < 0.8
        pk = [packets[s][at[s]] for s in named]
        if not score and any(int(ms.pending[s]) + 2 * len(p) + 2 > 4 * H for s, p in zip(named, pk)):
            score = True
        res = ms.feed(pk, named, score=score)
        for s, p, got in zip(named, pk, res.split()):
            want = refs[s].feed([p], [s], score=score)
            assert torch.equal(got, want.scores) and got.numel() == int(want.counts[0]), (kind, s, at[s])
            emitted[s] += got.numel()
            at[s] += 1
        assert torch.equal(ms.pending, torch.stack([refs[s].pending[s] for s in range(S)]))
    res = ms.drain()
    for s, got in enumerate(res.split()):
        assert torch.equal(got, refs[s].drain([s]).scores)
        emitted[s] += got.numel()
    assert all(e >= 5 for e in emitted) and ms.samples_seen.tolist() == [H * e for e in emitted]


def test_sessions_move_between_mixed_scorers_and_from_a_plain_packet_scorer():
    from afx.ingest import MixedPacketScorer, PacketScorer
    kind = "incremental"
    A = MixedPacketScorer(_inner(kind, 3), [(8000, "mulaw"), (48000, "pcm_s16le"), (16000, "pcm_s16le")])
    A.reset([0, 1], [0, 1])
    B = MixedPacketScorer(_inner(kind, 3), [(48000, "pcm_s16le"), (16000, "pcm_f32le"), (8000, "mulaw")], max_pending=3)
    P = PacketScorer(_inner(kind, 2), 48000, "pcm_s16le")
    rng = random.Random(5)
    fm = [(8000, "mulaw"), (48000, "pcm_s16le"), (48000, "pcm_s16le")]  # A's slot 0, A's slot 1, P's slot 1
    packets = [_cut(_stream(e, int(6.4 * H * r / 16000), seed=400 + s, quiet=True), r, e, rng) for s, (r, e) in enumerate(fm)]
    half = [len(p) // 2 for p in packets]
    for s in (0, 1):
        for p in packets[s][:half[s]]:
            A.feed([p], [s])
    for p in packets[2][:half[2]]:
        P.feed([p], [1])
    # one more packet each, buffered: the sessions move with pending samples
    A.feed([packets[0][half[0]], packets[1][half[1]]], [0, 1], score=False)
    P.feed([packets[2][half[2]]], [1], score=False)
    st = A.export_slots([1, 0])
    assert st.tensors["ingest_rate"].tolist() == [48000, 8000] and (st.tensors["ingest_fill"] > 0).all()
    assert st.tensors["resample_hist"][0].any() and st.tensors["resample_hist"][1, :20].any() and not st.tensors["resample_hist"][1, 20:].any()
    assert (st.seen > 0).all()
    B.import_slots([2, 0], st.to("cpu").to("cuda"))
    B.import_slots([1], P.export_slots([1]).to("cpu").to("cuda"))
    assert B.format_of.tolist() == [2, 0, 0] and B.rates.tolist() == [8000, 48000, 48000]
    assert B.pending.tolist() == [int(A.pending[0]), int(P.pending[1]), int(A.pending[1])]
    moved = {0: (A, 0, 0), 2: (A, 1, 1), 1: (P, 1, 2)}  # B's slot -> (the unmoved scorer, its slot, the stream)
    got = B.drain([0, 2, 1])
    for b, part in zip([0, 2, 1], got.split()):
        src, s, _ = moved[b]
        assert torch.equal(part, src.drain([s]).scores)
    nxt = {b: half[k] + 1 for b, (_, _, k) in moved.items()}
    scores = 0
    while any(nxt[b] < len(packets[moved[b][2]]) for b in moved):
        named = [b for b in moved if nxt[b] < len(packets[moved[b][2]]) and rng.random() < 0.8]
        rng.shuffle(named)
        if not named:
            continue
        pk = [packets[moved[b][2]][nxt[b]] for b in named]
        res = B.feed(pk, named)
        for b, p, part in zip(named, pk, res.split()):
            src, s, _ = moved[b]
            assert torch.equal(part, src.feed([p], [s]).scores), b
            scores += part.numel()
            nxt[b] += 1
    assert scores >= 6 and B.samples_in.tolist() == [int(A.samples_in[0]), int(P.samples_in[1]), int(A.samples_in[1])]


# ---- jitter: PT 0 and PT 8 on one scorer -------------------------------------------------------------------------------------
def _rtp(seq, ts, pt, payload, ssrc):
    return rtp(seq & 0xFFFF, ts & 0xFFFFFFFF, pt=pt, ssrc=ssrc, payload=payload)  # (the callers' counters run past the wrap)


def test_jitter_scores_do_not_depend_on_how_a_packet_was_encoded():
    from afx.jitter import JitterScorer
    depth, n = 480, 160
    J = JitterScorer(_inner("incremental", 2), 8000, ("mulaw", "alaw"), depth)
    R = JitterScorer(_inner("incremental", 2), 8000, "pcm_f32le", depth)  # the same decoded audio as pcm_f32le
    law = {0: "mulaw", 8: "alaw"}
    g = np.random.default_rng(9)
    count = int(5.2 * H / 2 / n)  # 5.2 hops of 8 kHz audio in 20-ms datagrams
    t0 = [(1 << 32) - 40 * n, 123456]  # slot 0's timestamps pass 2**32
    items = []  # (slot, datagram, timestamp, the payload decoded as pcm_f32le)
    for s in (0, 1):
        for k in range(count):
            pt = 0 if s == 0 or k % 2 == 0 else 8
            codes = g.integers(0, 256, n).astype(np.uint8)
            ts = t0[s] + k * n
            items.append((s, _rtp(k + 7, ts, pt, codes.tobytes(), 0xA0 + s), ts & 0xFFFFFFFF,
                          TABLES[law[pt]][codes].astype("<f4").tobytes()))
    per = {s: [it for it in items if it[0] == s] for s in (0, 1)}
    for s, (i, j, lost) in ((0, (11, 12, 30)), (1, (20, 21, 41))):  # a reordered pair and a lost datagram per slot
        per[s][i], per[s][j] = per[s][j], per[s][i]
        del per[s][lost]
    assert {it[1][1] & 0x7F for it in per[1]} == {0, 8} and {it[1][1] & 0x7F for it in per[0]} == {0}
    emitted = [0, 0]
    k, call = 0, 0
    while k < count - 1:  # one to three datagrams per slot per call (a slot named once continues at its `hi`: the plan's fast path)
        step = (3, 1, 1, 2)[call % 4]
        batch = per[1][k:k + step] + per[0][k:k + step]
        k, call = k + step, call + 1
        slots = [it[0] for it in batch]
        got = J.feed_rtp([it[1] for it in batch], slots)
        want = R.feed([it[3] for it in batch], slots, [it[2] for it in batch])
        assert got.counts.tolist() == want.counts.tolist() and torch.equal(got.scores, want.scores), k
        for s, c in zip(slots, got.counts.tolist()):
            emitted[s] += c
    got, want = J.flush(), R.flush()
    assert got.counts.tolist() == want.counts.tolist() and torch.equal(got.scores, want.scores)
    assert all(e + c >= 5 for e, c in zip(emitted, got.counts.tolist()))
    sj, sr = J.stats(), R.stats()
    assert all(torch.equal(sj[k], sr[k]) for k in ("received", "late", "duplicate", "concealed"))
    assert sj["concealed"].tolist() == [n, n] and sj["out_of_order"].tolist() == [1, 1]
    assert torch.equal(J.export_slots([0, 1]).tensors["jitter_ring"], R.export_slots([0, 1]).tensors["jitter_ring"])

"""Provenance through onset pre-roll and through turns, on the GPU (afx/provenance.py, ``ProvenancePolicy(through="all")``):
the three new kernels against numpy at their edges, all exact, then the two chains -- a jitter front over a ``TurnScorer`` and
over a look-ahead gate -- on lossy ``oracle.jitter.Schedule`` traffic of talk spurts against the reference: c16 computed from
``RefSlot.kinds`` by the formula, summed per frame, cut by ``cut_reference`` / compacted by the look-ahead mask of
``gate_reference``, tiled by ``clip_count``, and ``ProvenancePolicy.run_reference`` over the counts.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import RefSlot, Schedule, decode_ref
from test_gpu_provenance import Summing, _call, _dev

pytestmark = pytest.mark.gpu
H, FRAME, PER = 4000, 160, 25
RATIO = {8000: (2, 1), 48000: (1, 3)}


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def _resampled(E, rate):
    """The 16 kHz stream a front pushes for the played-out stream E: the device's resampler over the whole stream."""
    return packet_helpers.offline(E, rate).cpu().numpy()


# ---- 1. afx_k_prov_compact_la ---------------------------------------------------------------------------------------------------
def compact_la_reference(counts, mask, hdr, frame, pre, gline, gsyn):
    """include/afx.h's statement, row by row, in place."""
    S, RF = gsyn.shape
    n = counts.shape[1]
    for i, (slot, wpos, F, _) in enumerate(hdr.tolist()):
        if not (0 <= slot < S and 0 <= wpos < RF * frame and wpos % frame == 0 and F >= 0 and F + n < 1 << 31):
            continue
        if ((counts[i] < 0) | (counts[i] > frame)).any():
            continue
        old, r = gline[slot].copy(), 0
        for j in range(n):
            g = F - pre + j
            if g >= 0 and mask[i, j] & 1:
                gsyn[slot, (wpos // frame + r) % RF] = old[g % pre] if j < pre else counts[i, j - pre]
                r += 1
        for j in range(max(0, n - pre), n):
            gline[slot, (F + j) % pre] = counts[i, j]


@pytest.mark.parametrize("pre", [1, 3, 31])
@pytest.mark.parametrize("n", [1, 5, 512])
def test_compact_la_scatters_the_emitted_frames_counts_and_keeps_the_line(built, pre, n):
    S, frame, RF = 3, FRAME, 2 * n
    g = np.random.default_rng(100 * pre + n)
    gsyn = g.integers(-9, 0, (S, RF)).astype(np.int32)   # poisoned: what is not written is recognised
    gline = g.integers(-9, 0, (S, pre)).astype(np.int32)
    d_gsyn, d_gline = _dev(gsyn), _dev(gline)
    F, wpos = {0: 0, 2: 1000}, {0: 0, 2: (RF - 1) * frame}  # slot 0 starts new; slot 2's first scatter wraps; slot 1 is never named
    for launch in range(4):
        counts = g.integers(0, frame + 1, (6, n)).astype(np.int32)
        mask = g.integers(0, 4, (6, n)).astype(np.uint8)     # bit 0 keeps; bit 1 is not read
        if launch == 1:
            mask[0] = 3                                      # every frame that can leave does
        counts[4, n - 1] = frame + 1                         # a count that is no frame's
        hdr = np.array([[0, wpos[0], F[0], 0], [2, wpos[2], F[2], 0],
                        [S, 0, 5, 0], [1, frame + 1, 5, 0], [1, 0, 5, 0], [1, 0, -1, 0]], dtype=np.int32)  # skipped whole
        before = gsyn.copy()
        compact_la_reference(counts, mask, hdr, frame, pre, gline, gsyn)
        _call(built.lib().afx_k_prov_compact_la, _dev(counts), _dev(mask), _dev(hdr), len(hdr), n, frame, pre, d_gline, d_gsyn, S, RF)
        assert np.array_equal(d_gsyn.cpu().numpy(), gsyn) and np.array_equal(d_gline.cpu().numpy(), gline), launch
        for s in (0, 2):
            r = int((gsyn[s] != before[s]).sum())  # (at least that many entries were written: the write position moves on)
            emitted = sum(1 for j in range(n) if F[s] - pre + j >= 0 and mask[(0, None, 1)[s], j] & 1)
            assert r <= emitted
            wpos[s], F[s] = (wpos[s] + emitted * frame) % (RF * frame), F[s] + n
    assert (gsyn[1] < 0).all() and (gline[1] < 0).all() and (gline[0] >= 0).sum() == min(pre, 4 * n)
    assert n < pre or (gsyn[0] >= 0).any()  # (launch 1 of slot 0: F = n >= pre and every mask bit set)


# ---- 2. afx_k_prov_turn with afx_k_turn ---------------------------------------------------------------------------------------------
def test_prov_turn_stores_the_counts_where_the_turn_kernel_stores_the_frames(built):
    from afx.turns import TurnPolicy
    S, F, least, top, frame = 3, 5, 5, 12, FRAME
    policy, l = TurnPolicy(least), built.lib()
    masks = {0: [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1],   # cut inside push 3; two short runs; open at the end
             2: [1, 1, 1, 1, 1, 1, 1, 0, 3, 1, 1, 1, 1, 1, 1, 0, 2, 1, 1, 1]}   # a natural close and a new onset in push 2
    g = np.random.default_rng(9)
    staging = torch.zeros(S, F * frame, device="cuda")
    bufs = torch.zeros(S, 2, top * frame, device="cuda")
    state = torch.zeros(S, 3, dtype=torch.int32, device="cuda")
    totals = torch.zeros(S, 4, dtype=torch.int32, device="cuda")
    poison = g.integers(-9, 0, (S, 2, top)).astype(np.int32)
    bsyn = _dev(poison)
    mirror = {s: (policy.new_state(top), np.zeros((2, top, 1), dtype=np.float32)) for s in masks}
    seen = {"cut": 0, "natural": 0, "flip": 0}
    for push in range(4):
        counts = g.integers(0, frame + 1, (3, F)).astype(np.int32)
        mask = np.array([masks[0][F * push:F * push + F], masks[2][F * push:F * push + F], [1] * F], dtype=np.uint8)
        hdr = np.array([[0, 0, F * push], [2, 0, F * push], [1, 0, -1]], dtype=np.int32)  # slot 1: g0 = -1, skipped by both kernels
        done = torch.full((3, 4), -7, dtype=torch.int32, device="cuda")
        before = state.cpu().numpy().copy()
        _call(l.afx_k_prov_turn, _dev(counts), _dev(mask), _dev(hdr), 3, F, frame, least, top, state, bsyn, S)
        assert np.array_equal(state.cpu().numpy(), before)  # it reads the state and never writes it
        _call(l.afx_k_turn, staging, S, F * frame, _dev(mask), _dev(hdr), 3, F, frame, least, top, bufs, state, totals, done)
        done, st, got = done.cpu().numpy(), state.cpu().numpy(), bsyn.cpu().numpy()
        assert done[2].tolist() == [-1] * 4 and np.array_equal(got[1], poison[1])
        for i, s in enumerate((0, 2)):
            kept = counts[i][(mask[i] & 1) != 0].astype(np.float32)[:, None]
            opened = mirror[s][0]["open"]
            new, d = policy.step_reference(mirror[s][0], mask[i], F * push, kept, mirror[s][1])
            mirror[s] = (new, mirror[s][1])
            assert done[i].tolist() == list(d) and st[s, :2].tolist() == [new["open"], new["n"]]
            if d[1] > 0:  # the completed turn's counts
                assert np.array_equal(got[s, d[0], :d[1]], mirror[s][1][d[0], :d[1], 0].astype(np.int32)), (push, s)
                seen["cut" if d[1] == top else "natural"] += 1
            assert np.array_equal(got[s, new["open"], :new["n"]], mirror[s][1][new["open"], :new["n"], 0].astype(np.int32)), (push, s)
            seen["flip"] += int(new["open"] != opened and new["n"] > 0)  # counts of one row landed in both buffers
    assert seen == {"cut": 1, "natural": 2, "flip": 3} and totals.cpu()[0].tolist() == [1, 2, 1, 17]
    # a row with a count that is no frame's is skipped whole, whatever its mask
    counts = np.full((1, F), 7, dtype=np.int32)
    counts[0, 3] = frame + 1
    was = bsyn.cpu().numpy().copy()
    _call(l.afx_k_prov_turn, _dev(counts), _dev(np.ones((1, F), dtype=np.uint8)), _dev(np.array([[1, 0, 0]], dtype=np.int32)), 1, F, frame,
          least, top, state, bsyn, S)
    assert np.array_equal(bsyn.cpu().numpy(), was)
    state[1] = torch.tensor([2, 0, 0], dtype=torch.int32)  # a state that is no turn state: skipped, as afx_k_turn skips it
    counts[0, 3] = 0
    _call(l.afx_k_prov_turn, _dev(counts), _dev(np.ones((1, F), dtype=np.uint8)), _dev(np.array([[1, 0, 0]], dtype=np.int32)), 1, F, frame,
          least, top, state, bsyn, S)
    assert np.array_equal(bsyn.cpu().numpy(), was)


# ---- 3. afx_k_prov_turn_sum ---------------------------------------------------------------------------------------------------
def test_turn_sum_is_the_clip_count_of_the_tiled_turn(built):
    from afx.provenance import clip_count
    S, top = 3, 12
    g = np.random.default_rng(4)
    bsyn = g.integers(0, FRAME + 1, (S, 2, top)).astype(np.int32)
    bsyn[1, 0, 2] = -1
    rows = np.array([[0, 0, 1], [0, 1, 5], [2, 0, 7], [2, 1, 12],                       # (q, rem) = (12, 0), (2, 2), (1, 5), (1, 0)
                     [1, 2, 5], [1, -1, 5], [S, 0, 5], [-1, 0, 5], [0, 0, 13], [0, 0, 0],  # afx_k_turn_collect would skip them
                     [1, 0, 5], [1, 0, 2], [1, 0, 10]], dtype=np.int32)                    # the negative entry: read, read, read (not in the tail)
    want = [clip_count(bsyn[s, b, :m], top) for s, b, m in rows[:4].tolist()] + [-1] * 7 + [clip_count(bsyn[1, 0, :2], top), -1]
    out = torch.full((len(rows),), -7, dtype=torch.int32, device="cuda")
    _call(built.lib().afx_k_prov_turn_sum, _dev(bsyn), S, top, _dev(rows), len(rows), out)
    assert out.cpu().tolist() == want and want[0] == 12 * int(bsyn[0, 0, 0])


# ---- 4. the chains, end to end ------------------------------------------------------------------------------------------------------
LOUD = ((6, 20), (25, 56), (62, 67), (74, 91), (98, 109))  # the loud packets: five talk spurts
S, RATE, DEPTH, N_PK, WINDOW_T, TOP = 3, 8000, 480, 110, 8000, 50
# per mode the slots' Schedule seeds, chosen on the reference for the conditions the chain tests assert
SEEDS = {"repeat": (2, 4, 6), "pitch_sync": (2, 4, 6), "zero": (2, 4, 6)}


def spurts(rate, encs, sizes, seed):
    """A Schedule's payloads: talk spurts.  The packets of ``LOUD`` are loud (any mu-law code; 16-bit PCM: any sample up to
    20 000), the rest quiet (the mu-law codes 124-127 and 252-255, the eight lowest levels; PCM: |x| <= 8)."""
    g = np.random.default_rng(seed)
    low = np.array([124, 125, 126, 127, 252, 253, 254, 255], dtype=np.uint8)
    out = []
    for k, n in enumerate(sizes):
        loud = any(a <= k <= b for a, b in LOUD)
        if encs[k] == "mulaw":
            raw = (g.integers(0, 256, n).astype(np.uint8) if loud else low[g.integers(0, 8, n)]).tobytes()
        else:
            raw = g.integers(-20000, 20001, n).astype("<i2").tobytes() if loud else g.integers(-8, 9, n).astype("<i2").tobytes()
        out.append((raw, decode_ref(raw, encs[k])))
    return out


def _gates():
    from afx.vad import LookaheadGate, SpeechGate
    return dict(turns=SpeechGate(hang=3), lookahead=LookaheadGate(hang=3, pre=5))


def _stack(chain, layer, log):
    """[gate or turns ->] [layer ->] scorer for ``chain`` (``layer``: True, or the layer's policy); the layer records every
    push's rows in ``log``."""
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.streaming import SlidingWindowScorer
    from afx.turns import TurnPolicy, TurnScorer
    from afx.vad import GatedScorer

    class Recording(ProvenanceScorer):
        def push(self, chunk, slots=None):
            out = super().push(chunk, slots)
            log.append((self._named(slots), self.last_meas, out))
            return out

    s = SlidingWindowScorer(Summing(), S, WINDOW_T, WINDOW_T) if chain == "turns" else SlidingWindowScorer(Summing(), S, 16000, H)
    if layer:
        s = Recording(s, ProvenancePolicy(through="all") if layer is True else layer)
    return TurnScorer(s, _gates()[chain], TurnPolicy(PER), hop=H) if chain == "turns" else GatedScorer(s, _gates()[chain])


def _chain(chain, mode, layer, log=None):
    from afx.jitter import JitterScorer
    return JitterScorer(_stack(chain, layer, log), RATE, "mulaw", DEPTH, conceal=mode)


def _traffic(mode):
    return [Schedule(RATE, "mulaw", SEEDS[mode][s], short=40, n_pk=N_PK, payload=spurts) for s in range(S)]


def _refs(mode, rates=(RATE,) * S):
    return [RefSlot(3 * (r // 50), mode, r // 100, 3 * (r // 100)) if mode == "repeat" else
            RefSlot(3 * (r // 50), mode, rate=r) if mode == "pitch_sync" else RefSlot(3 * (r // 50), mode) for r in rates]


def _by_slot(res, rows):
    named = list(dict.fromkeys(r[0] for r in rows))
    return zip(named, res.scores.split([int(res.counts[[r[0] for r in rows].index(s)]) for s in named]))


def _drive(js, sch, refs=None, slot_of=None, encodings=False, until=None):
    """Feeds the traffic tick by tick (``until(step)``: stop when it says so) -> per slot the list of its scores, feed by feed."""
    got, step = [[] for _ in range(len(sch))], 0
    while not all(x.done() for x in sch) and not (until is not None and until(step)):
        step += 1
        rows = [(s,) + pk for s in range(len(sch)) if not sch[s].done() for pk in sch[s].tick()]
        kw = dict(encodings=[r[5] for r in rows]) if encodings else {}
        res = js.feed([r[3] for r in rows], [r[0] if slot_of is None else slot_of[r[0]] for r in rows], [r[1] for r in rows], **kw)
        for s, sc in _by_slot(res, rows):
            got[s].append(sc)
        if refs is not None:
            for s, ts, t, raw, x, e in rows:
                refs[s].packet(t, x)
            for s in dict.fromkeys(r[0] for r in rows):
                refs[s].after_feed()
    return got


def _flush(js, got, refs=None, slots=None):
    res = js.flush(slots)
    for s, sc in enumerate(res.split()):
        got[s].append(sc)
    for r in refs or ():
        r.release(r.hi)
    return [torch.cat(g).cpu().numpy() for g in got]


def _frame_counts(ref, rate):
    """-> (n hops the front pushed, the 16 kHz stream of those hops, n[f] per gate frame)."""
    from afx.provenance import marks16
    c16 = marks16(ref.kinds, *RATIO[rate])
    n = len(c16) // H
    return n, _resampled(ref.E, rate)[:n * H], c16[:n * H].reshape(-1, FRAME).sum(axis=1)


def turns_reference(ref, policy, rate=RATE):
    """One slot's reference through turns -> (turns, their clip counts, meas, valid, the push that returns each turn's score,
    short runs, the open turn (first, frames), the open turn's clip count or None where a flush drops it, hops)."""
    from afx.provenance import clip_count
    from afx.turns import TurnPolicy
    n, x, nf = _frame_counts(ref, rate)
    keep = _gates()["turns"].gate_reference(x)[0]
    turns, totals, still = TurnPolicy(PER).cut_reference(keep, TOP, close_end=False)
    counts = [clip_count(nf[t["first"]:t["end"]], TOP) for t in turns]
    at = [(t["end"] - 1 if t["cut"] else t["end"]) // PER for t in turns]
    last = clip_count(nf[still[0]:still[0] + still[1]], TOP) if still[1] >= PER else None
    meas, valid = policy.run_reference(np.array(counts + ([] if last is None else [last]), dtype=np.int64), WINDOW_T, WINDOW_T)
    return turns, counts, meas, valid, at, totals[1], still, last, n


def lookahead_reference(ref, policy, rate=RATE):
    """One slot's reference behind the look-ahead gate -> (the counts of the gated hops, meas, valid, the gated hop each push
    of the front completed or -1)."""
    n, x, nf = _frame_counts(ref, rate)
    mask = _gates()["lookahead"].gate_reference(x)[0]  # keep' of the decided frames: all but the newest pre
    per_frame = nf[:mask.size][mask]
    m = per_frame.size // PER
    counts = per_frame[:m * PER].reshape(m, PER).sum(axis=1)
    decided = np.maximum(PER * np.arange(1, n + 1) - 5, 0)
    done = np.array([int(mask[:d].sum()) for d in decided]) // PER
    inner = np.where(np.diff(np.concatenate([[0], done])) > 0, done - 1, -1)
    meas, valid = policy.run_reference(counts, H, 16000)
    return counts, meas, valid, inner


def _rows_by_slot(log, n_slots=S, slot_of=None):
    per = [[] for _ in range(n_slots)]
    back = {b: s for s, b in enumerate(slot_of)} if slot_of is not None else None
    for idx, meas, out in log:
        for i, b in enumerate(idx):
            per[b if back is None else back[b]].append(meas[i].cpu().numpy())
    return [np.stack(p) if p else np.zeros((0, 3), dtype=np.int32) for p in per]


def _withheld(base, at, valid):
    """``base`` (a slot's scores without the layer) with the quiet NaN at the pushes ``at`` whose turn or hop is not valid."""
    want = base.copy()
    for k, v in zip(at, valid):
        if not v:
            want.view(np.int32)[k] = 0x7fc00000
    return want


def _check_turn_chain(js, plain, ts_flush, refs, log, policy, rates=(RATE,) * S, conditions=True):
    """``js`` and ``plain`` were driven and flushed (``ts_flush``: each slot's scores of the turn scorers' own flush, with and
    without the layer); asserts the issue's list against the reference of every slot."""
    got, base, last_got, last_base = ts_flush
    rows = _rows_by_slot(log, len(refs))
    withheld = []
    for s, ref in enumerate(refs):
        turns, counts, meas, valid, at, short, still, last, n = turns_reference(ref, policy, rates[s])
        if conditions:  # the conditions the seeds were chosen for
            assert any(t["cut"] for t in turns) and any(not t["cut"] for t in turns) and short >= 2 and still[1] > 0, s
            assert any(c > 0 and v for c, v in zip(counts, valid)) and not valid[:len(counts)].all(), s
            assert any(c > int(sum(_frame_counts(ref, rates[s])[2][t["first"]:t["end"]])) for c, t in zip(counts, turns)), s  # tiled: repeated
        assert np.array_equal(rows[s], meas), s
        assert len(got[s]) == len(base[s]) == n
        closes = np.zeros(n, dtype=bool)
        closes[at] = True
        assert len(set(at)) == len(at) and np.array_equal(np.isnan(base[s]), ~closes)
        assert np.array_equal(got[s].view(np.int32), _withheld(base[s], at, valid).view(np.int32)), s
        if last is None:
            assert np.isnan(last_got[s]) and np.isnan(last_base[s])
        else:  # the open turn, closed by the turn scorer's flush: the last row of meas
            assert not np.isnan(last_base[s]) and meas[-1, 0] == last
            assert last_got[s].view(np.int32) == (last_base[s].view(np.int32) if valid[-1] else 0x7fc00000)
        withheld.append(int((~valid).sum()))
    return withheld


@pytest.mark.parametrize("mode", ["repeat", "pitch_sync", "zero"])
def test_the_turn_chain_counts_the_tiled_clip_and_withholds_as_the_reference_says(built, mode):
    from afx.provenance import ProvenancePolicy
    log = []
    js, plain = _chain("turns", mode, True, log), _chain("turns", mode, False)
    refs = _refs(mode)
    got = _flush(js, _drive(js, _traffic(mode), refs), refs)
    base = _flush(plain, _drive(plain, _traffic(mode)))
    last_got, last_base = js.scorer.flush().cpu().numpy(), plain.scorer.flush().cpu().numpy()
    withheld = _check_turn_chain(js, plain, (got, base, last_got, last_base), refs, log, ProvenancePolicy(through="all"))
    assert js.scorer.scorer.stats()["withheld"].tolist() == withheld
    assert js.scorer.stats()["scored"].tolist() == plain.scorer.stats()["scored"].tolist()


def _check_lookahead_chain(got, base, refs, log, policy, rates=(RATE,) * S, conditions=True):
    rows = _rows_by_slot(log, len(refs))
    withheld = []
    for s, ref in enumerate(refs):
        counts, meas, valid, inner = lookahead_reference(ref, policy, rates[s])
        if conditions:  # the conditions the seeds were chosen for: a hop with synthetic samples, a withheld and a passed score
            assert (counts > 0).any() and (~valid).any() and valid.any(), s
        assert np.array_equal(rows[s], meas), s
        assert len(got[s]) == len(base[s]) == len(inner)
        emitted = inner >= 0
        assert np.array_equal(np.isnan(base[s]), ~emitted)
        want = base[s].copy()
        want.view(np.int32)[emitted & ~np.where(emitted, valid[np.maximum(inner, 0)], True)] = 0x7fc00000
        assert np.array_equal(got[s].view(np.int32), want.view(np.int32)), s
        withheld.append(int((~valid).sum()))
    return withheld


@pytest.mark.parametrize("mode", ["repeat", "pitch_sync", "zero"])
def test_the_lookahead_chain_counts_the_emitted_frames_as_the_reference_says(built, mode):
    from afx.provenance import ProvenancePolicy
    log = []
    js, plain = _chain("lookahead", mode, True, log), _chain("lookahead", mode, False)
    refs = _refs(mode)
    got = _flush(js, _drive(js, _traffic(mode), refs), refs)
    base = _flush(plain, _drive(plain, _traffic(mode)))
    withheld = _check_lookahead_chain(got, base, refs, log, ProvenancePolicy(through="all"))
    assert js.scorer.scorer.stats()["withheld"].tolist() == withheld


@pytest.mark.parametrize("chain", ["turns", "lookahead"])
def test_mixed_rates_carry_the_counts_through_both_chains(built, chain):
    from afx.jitter import MixedJitterScorer
    from afx.provenance import ProvenancePolicy
    formats, rates = [(8000, "mulaw"), (48000, "pcm_s16le")], (8000, 48000, 8000)
    sch = lambda: [Schedule(r, "mulaw" if r == 8000 else "pcm_s16le", SEEDS["repeat"][s], short=r // 200, n_pk=N_PK, payload=spurts)  # noqa: E731
                   for s, r in enumerate(rates)]
    log, runs, refs = [], [], _refs("repeat", rates)
    for layer in (True, False):
        ms = MixedJitterScorer(_stack(chain, layer, log), formats, 60)
        ms.reset(list(range(S)), list(rates))
        mine = refs if layer else None
        runs.append((ms, _flush(ms, _drive(ms, sch(), mine, encodings=True), mine)))
    (ms, got), (plain, base) = runs
    policy = ProvenancePolicy(through="all")
    if chain == "turns":
        last = (ms.scorer.flush().cpu().numpy(), plain.scorer.flush().cpu().numpy())
        withheld = _check_turn_chain(ms, plain, (got, base) + last, refs, log, policy, rates, conditions=False)
    else:
        withheld = _check_lookahead_chain(got, base, refs, log, policy, rates, conditions=False)
    assert ms.scorer.scorer.stats()["withheld"].tolist() == withheld and int(ms.scorer.scorer.stats()["synthetic"].min()) > 0


# ---- 5. sessions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["turns", "lookahead"])
def test_a_session_moved_mid_turn_and_mid_gap_continues_as_the_unmoved_one(built, chain):
    mode, perm = "repeat", [2, 0, 1]
    loga, logb = [], []
    A, B = _chain(chain, mode, True, loga), _chain(chain, mode, True, logb)
    key = "turn_syn" if chain == "turns" else "gate_syn_line"

    def ready(step):  # a slot inside a gap of its stream whose open turn / delay line holds made-up samples
        if step < 8 or not (A._b.gap >= 0).any():
            return False
        return int(A.scorer.export_slots([0, 1, 2]).tensors[key].clamp(min=0).sum()) > 0

    sch = _traffic(mode)
    _drive(A, sch, until=ready)
    assert not all(x.done() for x in sch), "no step of the traffic is mid-gap with made-up samples in the open turn / the line"
    at = [x.at for x in sch]
    st = A.export_slots([0, 1, 2])
    assert int(st.tensors[key].clamp(min=0).sum()) > 0 and int(st.tensors["jitter_syn"].sum()) > 0
    if chain == "turns":
        assert int(st.tensors["turn_frames"].max()) > 0
    B.import_slots(perm, st.to("cpu").to("cuda"))

    def go_on(js, slot_of):
        sch = _traffic(mode)
        for x, a in zip(sch, at):
            x.at = a
        got = _flush(js, _drive(js, sch, slot_of=slot_of), slots=slot_of)
        tail = js.scorer.flush(slot_of).cpu().numpy() if chain == "turns" else np.zeros(0, dtype=np.float32)
        return got, tail

    na, nb = len(loga), len(logb)
    (ga, ta), (gb, tb) = go_on(A, [0, 1, 2]), go_on(B, perm)
    for s in range(S):
        assert np.array_equal(ga[s].view(np.int32), gb[s].view(np.int32)), s
    assert np.array_equal(ta.view(np.int32), tb.view(np.int32))
    rows_a, rows_b = _rows_by_slot(loga[na:]), _rows_by_slot(logb[nb:], slot_of=perm)
    assert all(np.array_equal(a, b) for a, b in zip(rows_a, rows_b)) and sum(int(r[:, 0].sum()) for r in rows_a) > 0
    ea, eb = A.export_slots([0, 1, 2]), B.export_slots(perm)
    assert sorted(ea.tensors) == sorted(eb.tensors) and key in ea.tensors
    for k in ea.tensors:
        assert torch.equal(ea.tensors[k].cpu(), eb.tensors[k].cpu()), k


# ---- 6. nothing else moved ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", ["turns", "lookahead"])
def test_the_lane_changes_no_score_bit_and_adds_only_its_own_keys(built, chain):
    """The chain without the layer against the same chain over a ``through="all"`` layer that only counts (``abstain`` off):
    every score of every feed, the turn scorers' flush included, has the same bits; the layered chain's export adds exactly
    the provenance keys; the chain without the layer carries none of them and no new attribute."""
    from afx.provenance import ProvenancePolicy
    mode, log = "repeat", []
    plain, js = _chain(chain, mode, False), _chain(chain, mode, ProvenancePolicy(abstain=False, through="all"), log)
    base = _flush(plain, _drive(plain, _traffic(mode)))
    got = _flush(js, _drive(js, _traffic(mode)))
    for s in range(S):
        assert np.array_equal(got[s].view(np.int32), base[s].view(np.int32)) and not np.isnan(base[s]).all(), s
    if chain == "turns":
        assert torch.equal(js.scorer.flush().view(torch.int32), plain.scorer.flush().view(torch.int32))
    assert int(js.scorer.scorer.stats()["withheld"].sum()) > 0  # (hops that would have been withheld: the lane did count)
    keys = set(plain.export_slots([0, 1, 2]).tensors)
    extra = set(js.export_slots([0, 1, 2]).tensors) - keys
    assert extra == {"jitter_syn", "prov_ring", "prov_state", "prov_totals"} | ({"turn_syn"} if chain == "turns" else {"gate_syn", "gate_syn_line"})
    assert not {"jitter_syn", "gate_syn", "gate_syn_line", "turn_syn", "prov_ring"} & keys
    assert not any(hasattr(plain.scorer, a) for a in ("gsyn", "gline", "bsyn")) and not plain.scorer._syn and plain._prov is None
    for k in keys:
        assert torch.equal(plain.export_slots([0, 1, 2]).tensors[k].cpu(), js.export_slots([0, 1, 2]).tensors[k].cpu()), k

"""Provenance on the GPU (afx/provenance.py): each of the five kernels against numpy at its edges, all exact, then whole
chains -- a jitter front over the layer, over a gate and the layer, over a tone gate, a verdict layer and the layer -- on
lossy ``oracle.jitter.Schedule`` traffic against the reference: c16 computed from ``RefSlot.kinds`` by the formula, behind a
gate compacted by ``gate_reference``'s keep mask, and ``ProvenancePolicy.run_reference`` over the hop counts."""
import ctypes

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import RefSlot, Schedule, decode_ref
from packet_helpers import offline as _offline

pytestmark = pytest.mark.gpu
H, WINDOW, FRAME = 4000, 16000, 160


@pytest.fixture(scope="module", autouse=True)
def built():
    return packet_helpers.built()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(fn, *args):
    from afx._lib import check, stream_ptr
    check(fn(*[ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args], stream_ptr()))


# ---- 1. each kernel against numpy at its edges ---------------------------------------------------------------------------------
def test_spans_fill_byte_ranges_across_the_ring_end(built):
    S, R = 3, 1003  # (an odd ring: rows 1 and 2 start at unaligned addresses)
    g = np.random.default_rng(1)
    ring = g.integers(0, 2, (S, R)).astype(np.uint8)
    rows = np.array([[0, 998, 9, 1],      # wraps the ring end
                     [0, 7, 0, 1],        # n = 0: nothing
                     [0, 13, 1, 0], [0, 14, 2, 1], [0, 16, 3, 0], [0, 19, 5, 1],  # shorter than a dword, at every alignment
                     [1, 501, R, 1],      # n = ring_len: the whole row, from the middle
                     [2, 1, 600, 0], [2, 601, 399, 1],
                     [3, 0, 4, 1], [-1, 0, 4, 1], [2, R, 1, 1], [2, -1, 1, 1], [2, 0, R + 1, 1], [2, 0, -1, 1], [2, 0, 2, 2]],  # skipped whole
                    dtype=np.int32)
    want = ring.copy()
    for s, w, n, v in rows[:9].tolist():
        want[s, (w + np.arange(n)) % R] = v
    d = _dev(ring)
    _call(built.lib().afx_k_prov_spans, d, S, R, _dev(rows), len(rows), R)
    assert np.array_equal(d.cpu().numpy(), want)
    d = _dev(ring)  # the grid of a launch whose longest row is empty still covers its rows
    _call(built.lib().afx_k_prov_spans, d, S, R, _dev(rows[1:2]), 1, 0)
    assert np.array_equal(d.cpu().numpy(), ring)


@pytest.mark.parametrize("frame", [FRAME, H])
def test_frames_count_the_marks_of_popped_hops(built, frame):
    S, R = 3, 5 * H
    g = np.random.default_rng(2)
    ring = (g.random((S, R)) < 0.3).astype(np.uint8)
    ring[1, :7] = 255  # (any non-zero byte is one mark)
    table = np.array([[1, R - 3], [0, 0], [2, H + 1], [3, 0], [0, R], [-1, 5], [1, -1]], dtype=np.int32)  # head 3 before the ring end
    F = H // frame
    want = np.full((len(table), F), -1, dtype=np.int32)
    for i, (s, h) in enumerate(table[:3].tolist()):
        want[i] = (ring[s, (h + np.arange(H)) % R] != 0).reshape(F, frame).sum(axis=1)
    out = torch.full((len(table), F), -7, dtype=torch.int32, device="cuda")
    _call(built.lib().afx_k_prov_frames, _dev(ring), S, R, _dev(table), len(table), H, frame, out)
    assert np.array_equal(out.cpu().numpy(), want) and want[0].sum() > 0


@pytest.mark.parametrize("F", [25, 512])
def test_compact_scatters_the_kept_frames_counts_in_order(built, F):
    S, frame = 4, FRAME
    RF = 2 * F
    g = np.random.default_rng(3 + F)
    counts = g.integers(0, frame + 1, (7, F)).astype(np.int32)
    mask = (g.integers(0, 4, (7, F))).astype(np.uint8)  # bit 0 keeps; bit 1 (a tone gate's) is not read
    mask[1], mask[2] = 2, 3                             # all dropped, all kept
    counts[5, F - 1] = frame + 1                        # a count that is no frame's: the row is skipped whole
    hdr = np.array([[0, 3 * frame], [1, 0], [2, (RF - 1) * frame],  # the write position at the last ring entry
                    [3, RF * frame], [3, frame + 1], [3, 5 * frame], [-1, 0]], dtype=np.int32)
    ring = g.integers(-9, 0, (S, RF)).astype(np.int32)
    want = ring.copy()
    for i in range(3):
        s, w = hdr[i, 0], hdr[i, 1] // frame
        kept = counts[i][(mask[i] & 1) != 0]
        want[s, (w + np.arange(kept.size)) % RF] = kept
    d = _dev(ring)
    _call(built.lib().afx_k_prov_compact, _dev(counts), _dev(mask), _dev(hdr), len(hdr), F, frame, d, S, RF)
    assert np.array_equal(d.cpu().numpy(), want) and (want[2] >= 0).sum() == F and np.array_equal(want[1], ring[1])


def test_take_and_the_layer_update_at_three_slots(built):
    from afx.provenance import Provenance, ProvenancePolicy, ProvenanceState
    S, per, frame, RF = 3, 25, FRAME, 50
    g = np.random.default_rng(5)
    ring = g.integers(0, frame + 1, (S, RF)).astype(np.int32)
    ring[2, 3] = -1
    table = np.array([[1, 40 * frame], [0, 0], [2, 0], [2, 25 * frame], [3, 0], [0, RF * frame], [0, 7]], dtype=np.int32)
    want = np.array([ring[1, (40 + np.arange(per)) % RF].sum(), ring[0, :per].sum(), -1, ring[2, 25:].sum(), -1, -1, -1], dtype=np.int32)
    out = torch.full((len(table),), -7, dtype=torch.int32, device="cuda")
    _call(built.lib().afx_k_prov_take, _dev(ring), S, RF, _dev(table), len(table), per, frame, out)
    assert np.array_equal(out.cpu().numpy(), want)
    # the layer update: W = 4, young sessions, the wrap, a skipped row, a reset, against the numpy statement
    for abstain in (True, False):
        policy = ProvenancePolicy(abstain=abstain)
        pv, st = Provenance(S, policy, H, WINDOW), ProvenanceState(S, 4)
        k = np.zeros(S, dtype=np.int64)
        for step in range(14):
            slots = [[0, 1, 2], [2, 0], [1], [0, 1, 2]][step % 4]
            if step == 9:
                pv.reset([1])
                st.reset([1])
                k[1] = 0
            c = g.choice([0, 0, 100, 300, 801, H], len(slots)).astype(np.int32)
            if step == 6:
                c[0] = H + 1  # skipped whole (the hop index moves on: that hop's ring entry stays what it was)
            k[slots] += 1
            hop_index = k[slots].copy()
            s = g.standard_normal(len(slots)).astype(np.float32)
            scores = torch.zeros(len(slots), 3, device="cuda")
            scores[:, 1] = _dev(s)
            out, meas = pv.update(_dev(c), slots, hop_index=hop_index, scores=scores[:, 1])  # (a column: read in place)
            ro, rm = policy.step_reference(slots, c, hop_index, s, st, H)
            assert np.array_equal(meas.cpu().numpy(), rm) and np.array_equal(out.cpu().numpy().view(np.int32), ro.view(np.int32)), step
            assert np.array_equal(pv.ring.cpu().numpy(), st.ring) and np.array_equal(pv.st.cpu().numpy(), st.st)
            assert np.array_equal(pv.totals.cpu().numpy(), st.totals)
            none, meas = pv.update(_dev(c), slots, hop_index=hop_index)  # without scores: measured all the same
            policy.step_reference(slots, c, hop_index, None, st, H)
            assert none is None and np.array_equal(pv.st.cpu().numpy(), st.st)
        stats = pv.stats()
        assert stats["hops"].tolist() == st.totals[:, 0].tolist() and stats["synthetic"].tolist() == st.totals[:, 1].tolist()
        assert stats["withheld"].tolist() == st.totals[:, 2].tolist() and int(stats["withheld"].sum()) > 0
        assert pv.valid.tolist() == (st.st[:, 1] != 0).tolist() and pv.synthetic.tolist() == st.st[:, 0].tolist()


# ---- 2. end to end --------------------------------------------------------------------------------------------------------------
class Summing:
    """The stand-in for a model: (A, window) -> (A, 2), column 1 the sum of the window."""

    def forward(self, batch):
        s = batch.sum(dim=1)
        return torch.stack([-s, s], dim=1)

    def state_dict(self):  # (a session names the weights it was scored with)
        return {"w": torch.ones(3)}


def bursts(rate, encs, sizes, seed):
    """A Schedule's payloads in mu-law: loud packets (any code) with two quiet ones (codes of low level) after every six, so
    that a speech gate keeps some frames and drops others."""
    g = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(sizes):
        raw = (g.integers(120, 136, n) if k % 8 >= 6 else g.integers(0, 256, n)).astype(np.uint8).tobytes()
        out.append((raw, decode_ref(raw, "mulaw")))
    return out


SEEDS = {"repeat": 2, "pitch_sync": 22, "zero": 7}  # (chosen on the reference, for the conditions the chain test asserts)
S, RATE, DEPTH, N_PK = 3, 8000, 480, 110


def _chain(kind, mode, layer, log=None):
    """jitter -> [gate ->] [verdict ->] [layer ->] scorer; ``log``: the layer records every push's rows there."""
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenanceScorer
    from afx.streaming import SlidingWindowScorer
    from afx.vad import GatedScorer, ToneGate
    from afx.verdict import VerdictPolicy, VerdictScorer

    class Recording(ProvenanceScorer):
        def push(self, chunk, slots=None):
            out = super().push(chunk, slots)
            log.append((self._named(slots), self.last_meas, out))
            return out

    s = SlidingWindowScorer(Summing(), S, WINDOW, H)
    if layer:
        s = Recording(s)
    if kind == "tone":
        s = GatedScorer(VerdictScorer(s, VerdictPolicy(1e30)), ToneGate())  # (every score the verdict layer takes raises the alarm)
    elif kind == "gate":
        s = GatedScorer(s)
    return JitterScorer(s, RATE, "mulaw", DEPTH, conceal=mode)


def _traffic(mode):
    return [Schedule(RATE, "mulaw", SEEDS[mode] + 7 * s, short=40, n_pk=N_PK, payload=bursts) for s in range(S)]


def _drive(js, mode, refs=None, stop=None, skip=()):
    """Feeds the traffic tick by tick (``stop``: only so many steps; a slot in ``skip`` is not named) -> per slot the list
    of its scores, feed by feed."""
    sch, got, step = _traffic(mode), [[] for _ in range(S)], 0
    while not all(x.done() for x in sch) and (stop is None or step < stop):
        step += 1
        rows = [(s,) + pk for s in range(S) if s not in skip and not sch[s].done() for pk in sch[s].tick()]
        res = js.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        named = list(dict.fromkeys(r[0] for r in rows))
        for s, sc in zip(named, res.scores.split([int(res.counts[[r[0] for r in rows].index(s)]) for s in named])):
            got[s].append(sc)
        if refs is not None:
            for s, ts, t, raw, x, e in rows:
                refs[s].packet(t, x)
            for s in named:
                refs[s].after_feed()
    return got, sch


def _flush(js, got, refs=None):
    res = js.flush()
    for s, sc in enumerate(res.split()):
        got[s].append(sc)
    for r in refs or ():
        r.release(r.hi)
    return [torch.cat(g).cpu().numpy() for g in got]


def _reference(ref, kind, policy):
    """One slot's reference -> (the counts of the hops the layer sees, ``run_reference`` over them: meas and valid, the inner
    hop of each hop the front pushed or -1 where the gate completed none)."""
    from afx.provenance import marks16
    from afx.vad import SpeechGate, ToneGate
    c16 = marks16(ref.kinds, 2, 1)
    n = len(c16) // H
    if kind == "jitter":
        counts, inner = c16[:n * H].reshape(n, H).sum(axis=1), np.arange(n)
    else:
        x = _offline(ref.E, RATE).cpu().numpy()[:n * H]  # the 16 kHz stream the gate was pushed: Resampler(E), hop by hop
        keep = (ToneGate() if kind == "tone" else SpeechGate()).gate_reference(x)[0]
        per_frame = c16[:n * H].reshape(-1, FRAME).sum(axis=1)[keep]
        m = per_frame.size // (H // FRAME)
        counts = per_frame[:m * (H // FRAME)].reshape(m, H // FRAME).sum(axis=1)
        done = np.cumsum(keep.reshape(n, H // FRAME).sum(axis=1)) // (H // FRAME)  # gated hops completed after each push
        inner = np.where(np.diff(np.concatenate([[0], done])) > 0, done - 1, -1)
    meas, valid = policy.run_reference(counts, H, WINDOW)
    return counts, meas, valid, inner


@pytest.mark.parametrize("mode", ["repeat", "pitch_sync", "zero"])
def test_chains_count_and_withhold_as_the_reference_says(built, mode):
    from afx.provenance import ProvenancePolicy
    policy = ProvenancePolicy()
    for kind in ("jitter", "gate", "tone"):
        log = []
        js, plain = _chain(kind, mode, True, log), _chain(kind, mode, False)
        refs = [RefSlot(DEPTH, mode, 80, 240) if mode == "repeat" else RefSlot(DEPTH, mode, rate=RATE) if mode == "pitch_sync" else RefSlot(DEPTH, mode)
                for _ in range(S)]
        got = _flush(js, _drive(js, mode, refs)[0], refs)
        base = _flush(plain, _drive(plain, mode)[0])
        layer = js.scorer if kind == "jitter" else js.scorer.scorer.scorer if kind == "tone" else js.scorer.scorer
        per_slot = [[] for _ in range(S)]
        for idx, meas, out in log:
            for i, s in enumerate(idx):
                per_slot[s].append(meas[i])
        for s in range(S):
            counts, meas, valid, inner = _reference(refs[s], kind, policy)
            mine = torch.stack(per_slot[s]).cpu().numpy()
            # the conditions the seeds were chosen for: a hop with synthetic samples, a withheld and a passed score, per slot
            assert (counts > 0).any() and (~valid).any() and valid.any(), (kind, s)
            assert np.array_equal(mine, meas), (kind, s)  # the per-hop counts, window totals and flags
            assert len(got[s]) == len(base[s]) == len(inner)
            emitted = inner >= 0
            assert np.array_equal(np.isnan(base[s]), ~emitted)  # (without the layer: NaN only where the gate completed no hop)
            want = base[s].copy()
            want.view(np.int32)[emitted & ~np.where(emitted, valid[np.maximum(inner, 0)], True)] = 0x7fc00000
            assert np.array_equal(got[s].view(np.int32), want.view(np.int32)), (kind, s)
            assert np.isnan(got[s][emitted]).sum() == (~valid).sum()
        st = layer.stats()
        assert st["withheld"].tolist() == [int((~_reference(refs[s], kind, policy)[2]).sum()) for s in range(S)]
        if kind == "tone":  # the verdict layer took the passed scores only, and raised nothing on a withheld hop
            verdict = js.scorer.scorer
            ev = verdict.take_events()
            taken = verdict.verdicts.st[:, 0].cpu().tolist()
            for s in range(S):
                valid = _reference(refs[s], kind, policy)[2]
                assert taken[s] == int(valid.sum())
                hops = [int(k) for b, kd, k, _ in zip(*ev) if b == s]
                assert hops == [int(np.flatnonzero(valid)[0]) + 1]  # raised by the first score that passed, at its hop: no earlier one


def test_a_note_is_for_the_next_push_of_exactly_its_slots(built):
    """Layer and attached gate alike: a push that names other slots than the note's is a ValueError before anything changes,
    the note is then gone (the same push again counts zeros), and a push of the note's slots consumes it."""
    from afx.jitter import JitterScorer
    from afx.provenance import ProvenanceScorer
    from afx.streaming import SlidingWindowScorer
    from afx.vad import GatedScorer
    g = torch.Generator().manual_seed(3)
    hops = lambda n: torch.randn(n, H, generator=g).cuda()  # noqa: E731
    counts = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    layer = ProvenanceScorer(SlidingWindowScorer(Summing(), S, WINDOW, H))
    layer.note_synthetic(counts(5, 900), [0, 2])
    for other in ([0, 1], [2, 0], [0], None):
        layer.note_synthetic(counts(5, 900), [0, 2])
        with pytest.raises(ValueError, match="note"):
            layer.push(hops(S if other is None else len(other)), other)
        assert layer.samples_seen.tolist() == [0] * S and layer.stats()["hops"].tolist() == [0] * S  # nothing was pushed
        assert layer._note is None
    layer.push(hops(2), [2, 0])  # the note is gone: this push counts zeros
    assert layer.last_meas.cpu().tolist() == [[0, 0, 1], [0, 0, 1]]
    layer.note_synthetic(counts(5, 900), [0, 2])
    out = layer.push(hops(2), [0, 2])
    assert layer.last_meas.cpu().tolist() == [[5, 5, 1], [900, 900, 0]] and torch.isnan(out).tolist() == [False, True]
    layer.push(hops(2), [0, 2])  # consumed: zeros again
    assert layer.last_meas.cpu().tolist() == [[0, 5, 1], [0, 900, 0]]
    # the attached gate: per-frame counts
    inner = ProvenanceScorer(SlidingWindowScorer(Summing(), S, WINDOW, H))
    gate = GatedScorer(inner)
    JitterScorer(gate, RATE, "mulaw", DEPTH)  # (a jitter front over the layer attaches the gate)
    frames = torch.full((2, H // FRAME), 7, dtype=torch.int32, device="cuda")
    for other in ([1, 2], [2, 0], [0]):
        gate.note_synthetic(frames, [0, 2])
        with pytest.raises(ValueError, match="note"):
            gate.push(hops(len(other)), other)
        assert gate.samples_seen.tolist() == [0] * S and gate._syn_note is None and int(gate.gsyn.abs().sum()) == 0
    loud = lambda n: (hops(n) * (torch.arange(H, device="cuda") % 800 < 400)).contiguous()  # noqa: E731  (bursts: the gate keeps some frames)
    for _ in range(3):
        gate.push(loud(2), [0, 2])  # no note: zeros
    assert int(gate.gsyn.sum()) == 0
    gate.note_synthetic(frames, [0, 2])
    gate.push(loud(2), [0, 2])
    kept = gate.samples_kept
    assert int(gate.gsyn.sum()) > 0 and set(gate.gsyn.unique().tolist()) <= {0, 7} and int(kept[0]) > 0


def test_around_a_cascade_the_layer_hands_on_what_stands_directly_below(built):
    """``Verdict(Provenance(Quality(Cascade)))``: every slot is verified at every hop from 2 H on, and any verifier score the
    verdict layer is given raises.  Slot 1 is clipped throughout (quality-invalid, nothing synthetic), slot 2 is noted a whole
    synthetic hop at every push (provenance-invalid, clean audio): neither may raise, and ``last_verified()`` has NaN for both;
    slot 0 raises.  Without the two layers every slot raises."""
    import test_gpu_quality as q
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    INF, ticks = float("inf"), 5
    teacher, tsd = q._teacher()
    cpol = CascadePolicy(INF, S, 0, 2 * H)
    vp = VerdictPolicy(-INF, INF, verifier_enter=INF, latch=True)
    streams = [np.roll(q.FIX, -o)[:ticks * H].copy() for o in (0, 30057, 44000)]
    streams[1] = q._clipped(streams[1])
    hops = lambda t: torch.from_numpy(np.stack([s[t * H:(t + 1) * H] for s in streams])).cuda()  # noqa: E731
    qvalid = np.stack([QualityPolicy().run_reference(s, H, 64000)[1] for s in streams], axis=1)
    assert qvalid[:, [0, 2]].all() and not qvalid[:, 1].any(), "the fixture"
    plain = VerdictScorer(CascadeScorer(q._screen("kv", S), teacher, cpol, state_dict=tsd), vp)
    dry = [plain.push(hops(t)).clone() for t in range(ticks)]
    assert sorted(plain.take_events()[0].tolist()) == [0, 1, 2]
    ps = ProvenanceScorer(QualityScorer(CascadeScorer(q._screen("kv", S), teacher, cpol, state_dict=tsd), QualityPolicy()), ProvenancePolicy())
    vs = VerdictScorer(ps, vp)
    assert vs._verified and ps._cascade
    note = torch.tensor([0, 0, H], dtype=torch.int32, device="cuda")
    for t in range(ticks):
        ps.note_synthetic(note, None)
        sc = vs.push(hops(t))
        assert torch.equal(sc[:1].view(torch.int32), dry[t][:1].view(torch.int32)) and torch.isnan(sc[1:]).all(), t
        assert ps.last_meas.cpu().tolist() == [[0, 0, 1], [0, 0, 1], [H, min(t + 1, 16) * H, 0]]
        if t >= 1:  # verified: the verifier scores of the two invalid slots are NaN, whichever layer withheld them
            chosen, v = ps.last_verified()
            assert sorted(chosen.tolist()) == [0, 1, 2]
            assert torch.isnan(v.cpu()[chosen != 0]).all() and not torch.isnan(v.cpu()[chosen == 0]).any(), t
    slot, kind, k, _ = vs.take_events()
    assert slot.tolist() == [0] and kind.tolist() == [2] and vs.alarm.cpu().tolist() == [True, False, False]
    assert not torch.isnan(ps.verified).any()  # all three WERE verified (the cascade's own results, forwarded)
    assert ps.valid.cpu().tolist() == [True, True, False] and ps.scorer.valid.cpu().tolist() == [True, False, True]


def test_a_slot_that_is_not_named_keeps_its_rings_and_its_layer_state(built):
    js = _chain("gate", "repeat", True, [])
    _drive(js, "repeat", stop=30)
    gate = js.scorer
    layer = gate.scorer
    snap = lambda: [t[1].clone() for t in (js.psyn, js.ring, gate.gsyn, gate.ring, layer.provenance.ring, layer.provenance.st,  # noqa: E731
                                            layer.provenance.totals)]
    before = snap()
    sch = _traffic("repeat")
    for _ in range(30):
        [x.tick() for x in sch]
    for _ in range(25):  # slots 0 and 2 go on, slot 1 is not named
        rows = [(s,) + pk for s in (0, 2) for pk in sch[s].tick()]
        js.feed([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    assert int(layer.stats()["hops"][0]) > 2


def test_a_session_moved_in_mid_gap_continues_as_the_unmoved_one(built):
    mode = "repeat"
    loga, logb = [], []
    A, B = _chain("gate", mode, True, loga), _chain("gate", mode, True, logb)
    stop = next(i for i, t in enumerate(_traffic(mode)[0].ticks) if 29 in t)  # packets 25..28 are lost: with packet 29 in, slot 0 has played out into the gap
    sa, _ = _drive(A, mode, stop=stop + 1)
    assert int(A._b.gap[0]) >= 0, "slot 0 has an open gap"
    st = A.export_slots([0, 1, 2])
    assert int(st.tensors["jitter_syn"].sum()) > 0
    B.import_slots([2, 0, 1], st.to("cpu").to("cuda"))
    perm = [2, 0, 1]

    def go_on(js, slot_of):
        sch, got = _traffic(mode), [[] for _ in range(S)]
        for _ in range(stop + 1):
            [x.tick() for x in sch if not x.done()]
        while not all(x.done() for x in sch):
            rows = [(s,) + pk for s in range(S) if not sch[s].done() for pk in sch[s].tick()]
            res = js.feed([r[3] for r in rows], [slot_of[r[0]] for r in rows], [r[1] for r in rows])
            named = list(dict.fromkeys(r[0] for r in rows))
            for s, sc in zip(named, res.scores.split([int(res.counts[[r[0] for r in rows].index(s)]) for s in named])):
                got[s].append(sc)
        res = js.flush([slot_of[s] for s in range(S)])
        return [torch.cat(got[s] + [sc]).cpu().numpy() for s, sc in enumerate(res.split())]

    na, nb = len(loga), len(logb)
    ga, gb = go_on(A, [0, 1, 2]), go_on(B, perm)
    for s in range(S):
        assert np.array_equal(ga[s].view(np.int32), gb[s].view(np.int32)), s
    rows_a = [[m[idx.index(s)].tolist() for idx, m, _ in loga[na:] if s in idx] for s in range(S)]
    rows_b = [[m[idx.index(perm[s])].tolist() for idx, m, _ in logb[nb:] if perm[s] in idx] for s in range(S)]
    assert rows_a == rows_b and sum(r[0] for r in rows_a[0]) > 0 and any(r[2] == 0 for r in rows_a[0])
    ea, eb = A.export_slots([0, 1, 2]), B.export_slots(perm)
    for k in ("jitter_syn", "gate_syn", "prov_ring", "prov_state", "prov_totals"):
        assert torch.equal(ea.tensors[k].cpu(), eb.tensors[k].cpu()), k


def test_a_loss_free_feed_counts_nothing_and_changes_nothing_else(built):
    logs = []
    js, plain = _chain("gate", "repeat", True, logs), _chain("gate", "repeat", False)
    sch = [Schedule(RATE, "mulaw", 50 + s, lossy=False, n_pk=N_PK, payload=bursts) for s in range(S)]
    for x in sch:
        x.ticks = [[k] for k in range(N_PK)]  # in order
    for t in range(N_PK):
        rows = [(s,) + sch[s].tick()[0] for s in range(S)]
        args = ([r[3] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
        pa, pb = js._plan_feed(*args)[0], plain._plan_feed(*args)[0]
        assert [op[0] for op in pa.ops if op[0] != "spans"] == [op[0] for op in pb.ops]
        for x, y in zip([op for op in pa.ops if op[0] != "spans"], pb.ops):
            assert np.array_equal(x[1], y[1])
        assert all(op[1][:, 3].max() == 0 for op in pa.ops if op[0] == "spans")
        a, b = js.feed(*args), plain.feed(*args)
        assert torch.equal(a.counts, b.counts) and torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    ea, eb = js.export_slots([0, 1, 2]), plain.export_slots([0, 1, 2])
    mine = {"jitter_syn", "gate_syn", "prov_ring", "prov_state", "prov_totals"}
    assert set(ea.tensors) - set(eb.tensors) == mine and set(ea.meta) - set(eb.meta) == {"provenance", "provenance_window"}
    for k in eb.tensors:
        assert torch.equal(ea.tensors[k].cpu(), eb.tensors[k].cpu()), k
    assert int(ea.tensors["jitter_syn"].sum()) == 0 and int(ea.tensors["gate_syn"].clamp(min=0).sum()) == 0
    assert len(logs) >= 3 and all(int(m[:, :2].abs().sum()) == 0 and bool((m[:, 2] == 1).all()) for _, m, _ in logs)
    assert js.scorer.scorer.stats()["synthetic"].tolist() == [0, 0, 0]

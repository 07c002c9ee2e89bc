"""The whole streaming stack on the GPU (afx/_layer.py): a live session of the longest chain,
``PacketScorer(GatedScorer(EvidenceScorer(VerdictScorer(ProvenanceScorer(QualityScorer(CascadeScorer(...)))))), 8000, "mulaw")``, moves between
scorers through host memory and a file and continues bit for bit in every layer.  Every comparison is exact.

The audio is cut from the fixture stream of the per-layer tests: 0.1 s of noise (the gate sets its floor), the 2-s tone, noise,
0.1 s of noise, the 0.8-s tone: the gate keeps nearly 13 hops of 14.  Session 1 passes a saturating stage over ticks 2-4, so
the quality layer withholds its scores.  No threshold is tuned: the cascade's is 1e30 (every scored slot is a candidate) and so
is the verdict's ``enter`` (every score counts towards the alarm), which ``min_scores`` and ``confirm`` put at the seventh
score.  The move comes after tick 5: five scores in, no alarm yet, nothing recording; the alarm, its clip (whose pre-roll
begins with a hop pushed in the source) and further verifications come in the destination.

Tiny engines as in tests/test_gpu_quality.py: a 1-layer Conformer student scores, a 1-layer XLSR_AASIST teacher verifies."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
T_MOVE, TICKS = 5, 14


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
_ENGINES = {}


def _student(dtype="fp16"):
    if dtype not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES[dtype] = (eng, sd)
    return _ENGINES[dtype]


def _teacher():
    if "teacher" not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype="fp16")
        eng.load_state_dict(sd)
        _ENGINES["teacher"] = (eng, sd)
    return _ENGINES["teacher"]


def _clipped(x):
    """The stream through a saturating input stage: 40 dB of gain into a hard limiter."""
    return np.clip(x * np.float32(100), -1, 1).astype(np.float32)


def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the scorers are held against each other)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def _same_bits(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def _chain(kind, S):
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.evidence import EvidencePolicy, EvidenceScorer
    from afx.ingest import PacketScorer
    from afx.provenance import ProvenancePolicy, ProvenanceScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.streaming import IncrementalScorer, KVCachedScorer
    from afx.vad import GatedScorer
    from afx.verdict import VerdictPolicy, VerdictScorer
    (eng, sd), (teacher, tsd) = _student(), _teacher()
    screen = IncrementalScorer(eng, sd, S, window=16000, hop=H) if kind == "incremental" else KVCachedScorer(eng, sd, S, window=64000, hop=H)
    cascade = CascadeScorer(screen, teacher, CascadePolicy(threshold=1e30, budget=2, cooldown=1, min_samples=2 * H), state_dict=tsd)
    verdict = VerdictScorer(ProvenanceScorer(QualityScorer(cascade, QualityPolicy()), ProvenancePolicy()),
                            VerdictPolicy(enter=1e30, confirm=2, min_scores=6))
    return PacketScorer(GatedScorer(EvidenceScorer(verdict, EvidencePolicy(pre=2, post=2, clips=8))), 8000, "mulaw")


def _layers(front):
    gate = front.scorer
    evidence = gate.scorer
    verdict = evidence.scorer
    provenance = verdict.scorer
    quality = provenance.scorer
    return dict(gate=gate, evidence=evidence.evidence, verdicts=verdict.verdicts, provenance=provenance.provenance, quality=quality.quality,
                cascade=quality.scorer,
                take_events=evidence.take_events, take_clips=evidence.take_clips)


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_a_live_session_of_the_whole_stack_moves_bit_for_bit(kind):
    streams = [np.concatenate([FIX[46400 - o:84000 - o], FIX[6400 - o:]])[:TICKS * H].copy() for o in (0, 557)]
    streams[1][2 * H:5 * H] = _clipped(streams[1][2 * H:5 * H])
    codes = [_mulaw_encode(s[::2]) for s in streams]
    other = [_mulaw_encode(np.roll(FIX, -o)[:2 * H:2]) for o in (8000, 48000)]
    packets = lambda t: [c[t * 2000:(t + 1) * 2000].tobytes() for c in codes]  # noqa: E731  (2000 bytes at 8 kHz: one hop at 16 kHz)

    never, a, b = _chain(kind, 3), _chain(kind, 3), _chain(kind, 4)
    N, A, B = _layers(never), _layers(a), _layers(b)
    ref = []
    for t in range(TICKS):
        r = never.feed(packets(t), [0, 2])
        ref.append((r.counts.clone(), r.scores.clone()))
        if t == T_MOVE:
            early = N["take_events"]()
    for t in range(T_MOVE + 1):
        r = a.feed(packets(t), [0, 2])
        assert torch.equal(r.counts, ref[t][0]) and _same_bits(r.scores, ref[t][1]), t
    assert A["evidence"].rec[[0, 2]].tolist() == [-1, -1] and a.scorer.scorer.take_clips() == []  # nothing is recording at the move
    assert early[0].size == 0                                                                      # and no alarm was raised yet
    b.feed([c.tobytes() for c in other], [0, 2])  # the destination is in use
    b.import_slots([3, 1], _move(a.export_slots([0, 2])))
    B["take_events"]()
    for t in range(T_MOVE + 1, TICKS):
        r = b.feed(packets(t), [3, 1])
        assert torch.equal(r.counts, ref[t][0]) and _same_bits(r.scores, ref[t][1]), t

    # the fixture: it gets through the gate, the quality layer withheld a score, and after the move a verdict was raised, a
    # clip completed and the teacher ran
    scored = N["cascade"].samples_seen[[0, 2]] // H  # (the hops the gate let through to the models)
    assert scored.tolist() == (B["cascade"].samples_seen[[3, 1]] // H).tolist() and int(scored.min()) >= 8
    flagged = N["quality"].stats()["clipped"][[0, 2]]
    assert int(flagged[1]) >= 1 and int(flagged[0]) == 0
    taken = N["verdicts"].st[[0, 2], 0].cpu()  # the scores the verdict layer was given: a withheld one is a NaN row, not counted
    assert int(taken[0]) == int(scored[0]) and int(taken[1]) < int(scored[1])
    assert int(B["cascade"].stats()["verified"][[3, 1]].sum()) >= 1

    # every layer's state of the moved sessions, against the sessions that never moved
    for name, fields in (("verdicts", ("m", "st")), ("quality", ("ring", "st", "totals")),
                         ("provenance", ("ring", "st", "totals")), ("cascade", ("verified", "wait", "verified_at")),
                         ("gate", ("nf", "h")), ("evidence", ("hist", "sring"))):
        for f in fields:
            assert _same_bits(getattr(B[name], f)[[3, 1]], getattr(N[name], f)[[0, 2]]), (name, f)
    want, got = never.export_slots([0, 2]), b.export_slots([3, 1])
    assert torch.equal(want.seen, got.seen) and set(want.tensors) == set(got.tensors)
    for k in want.tensors:
        if k.split("_")[0] in ("cascade", "quality", "prov", "verdict", "evidence", "gate", "ingest", "resample"):
            assert _same_bits(want.tensors[k], got.tensors[k]), k

    # events and clips after the move, up to the renaming of the slots
    rename = {0: 3, 2: 1}
    slot, evkind, k, sm = N["take_events"]()
    slot2, evkind2, k2, sm2 = B["take_events"]()
    assert [rename[s] for s in slot.tolist()] == slot2.tolist() and evkind.tolist() == evkind2.tolist() and k.tolist() == k2.tolist()
    assert sm.view(np.int32).tolist() == sm2.view(np.int32).tolist()
    assert (evkind == 1).sum() >= 1 and int(k.min()) > T_MOVE
    clips, clips2 = N["take_clips"](), B["take_clips"]()
    assert a.scorer.scorer.take_clips() == [] and len(clips) == len(clips2) >= 1 and any(c.complete for c in clips2)
    for c, c2 in zip(clips, clips2):
        assert (rename[c.slot], c.raised_at, c.first_hop, c.complete) == (c2.slot, c2.raised_at, c2.first_hop, c2.complete)
        assert c.audio.tobytes() == c2.audio.tobytes() and c.scores.tobytes() == c2.scores.tobytes()
        assert c.first_hop <= T_MOVE < c.raised_at  # the pre-roll begins with a hop pushed in the source

"""Per-slot streaming sessions (afx/streaming.py ``reset``): slots start and restart at any hop while every slot still
advances one hop per push.  The contract: a slot reset before tick t0 emits at tick t0 + j, bit for bit, the score that
slot emits at tick j of a FRESH scorer with the same number of slots fed the same audio from tick 0 -- while the other
slots of the two scorers hold different audio at different phases."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-3
S, W, H, TICKS = 4, 16000, 4000, 14
# (slot, reset tick): slot 0 is a session from tick 0 (reset before the first push), slots 1 / 2 start at odd / even ticks,
# slot 3 starts at tick 5 and again at tick 9 -- its second session begins after its ring has wrapped
SESSIONS = [(0, 0), (1, 1), (2, 2), (3, 5), (3, 9)]


def _engine(arch):
    from afx import engine, synth
    if arch == "conformer":
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1)
    else:
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype="fp16")
    eng.load_state_dict(sd)
    return eng, sd


def _make(kind, eng, sd):
    from afx.streaming import IncrementalScorer, SlidingWindowScorer
    return SlidingWindowScorer(eng, S, window=W, hop=H) if kind == "sliding" else IncrementalScorer(eng, sd, S, window=W, hop=H)


def _audio():
    """Per session its own audio from its reset on; per slot the audio it hears before its first session."""
    from afx import synth
    sess = {(k, t0): synth.waveforms(1, (TICKS - t0) * H, batch_idx=4100 + 10 * k + t0)[0] for k, t0 in SESSIONS}
    before = synth.waveforms(S, TICKS * H, batch_idx=4177)
    return sess, before


def _staggered_run(sc, sess, before, sessions=SESSIONS, ticks=TICKS):
    """Drive ``sc`` through the schedule; returns the (ticks, S) scores and the samples_seen after every tick."""
    starts = {}
    scores, seen = [], []
    for t in range(ticks):
        named = [k for k, t0 in sessions if t0 == t]
        if named:
            sc.reset(named)
            starts.update({k: t for k in named})
        chunk = torch.stack([sess[(k, starts[k])][(t - starts[k]) * H:(t - starts[k] + 1) * H] if k in starts
                             else before[k, t * H:(t + 1) * H] for k in range(S)]).cuda()
        scores.append(sc.push(chunk).clone().cpu())
        seen.append(sc.samples_seen)
    return torch.stack(scores), torch.stack(seen)


def _fresh_run(sc, feed, ticks=TICKS):
    """A fresh scorer, no reset: slot k is fed feed[k] (ticks * H samples) from tick 0."""
    return torch.stack([sc.push(torch.stack([f[t * H:(t + 1) * H] for f in feed]).cuda()).clone().cpu() for t in range(ticks)])


@pytest.mark.parametrize("kind", ["sliding", "incremental"])
@pytest.mark.parametrize("arch", ["conformer", "xlsr_aasist"])
def test_staggered_sessions_are_bit_identical_to_fresh_streams(arch, kind):
    eng, sd = _engine(arch)
    sess, before = _audio()
    got, seen = _staggered_run(_make(kind, eng, sd), sess, before)
    for t in range(TICKS):  # samples_seen counts each slot's samples since its (last) reset
        last = [max((t0 for k2, t0 in SESSIONS if k2 == k and t0 <= t), default=0) for k in range(S)]
        assert seen[t].tolist() == [(t - t0 + 1) * H for t0 in last], t
    pad = lambda x: torch.cat([x, torch.zeros(TICKS * H - x.numel())])
    # fresh scorer A: the first four sessions, each in its own slot from tick 0 (all slots in lockstep: the original path);
    # fresh scorer B: slot 3's second session, the other slots fed other audio
    feed_a = [pad(sess[s]) for s in SESSIONS[:4]]
    feed_b = [before[0], before[1], before[2], pad(sess[(3, 9)])]
    ref_a, ref_b = _fresh_run(_make(kind, eng, sd), feed_a), _fresh_run(_make(kind, eng, sd), feed_b)
    for i, (k, t0) in enumerate(SESSIONS):
        ref = ref_a if i < 4 else ref_b
        t1 = 9 if (k, t0) == (3, 5) else TICKS  # slot 3's first session ends at its second reset
        for j in range(t1 - t0):
            assert torch.equal(got[t0 + j, k], ref[j, k]), \
                f"{arch} {kind}: slot {k} session from tick {t0}, its tick {j}: {(got[t0 + j, k] - ref[j, k]).abs().item():.2e}"


@pytest.mark.parametrize("kind", ["sliding", "incremental"])
def test_a_reset_slot_scores_the_reference_window_of_its_own_session(kind):
    """The reset slot's score is the reference model's on the window of ITS session: while the session is younger than the
    window, its history so far repeated (the reference's pad policy); then its last `window` samples."""
    from oracle import models, pre
    eng, sd = _engine("conformer")
    sess, before = _audio()
    got, _ = _staggered_run(_make(kind, eng, sd), sess, before)
    audio = sess[(3, 9)]
    for j in range(TICKS - 9):
        hist = audio[: (j + 1) * H]
        win = pre.adjust_duration(hist, W) if hist.numel() < W else hist[-W:]
        ref = models.conformer_forward(sd, win[None])[0, 1]
        assert (got[9 + j, 3] - ref).abs().item() <= SCORE_TOL, j


def test_resetting_one_slot_changes_no_byte_of_the_others():
    """Same audio in every slot at every tick; slot 3 restarts at ticks 5 and 9 in both runs, slot 2 is reset at tick 2 in
    one run only: slots 0, 1 and 3 emit the same bytes in both."""
    from afx import synth
    eng, sd = _engine("xlsr_aasist")
    audio = synth.waveforms(S, TICKS * H, batch_idx=4300).cuda()
    runs = []
    for resets in ({2: [2], 5: [3], 9: [3]}, {5: [3], 9: [3]}):
        sc = _make("incremental", eng, sd)
        out = []
        for t in range(TICKS):
            if t in resets:
                sc.reset(resets[t])
            out.append(sc.push(audio[:, t * H:(t + 1) * H]).clone().cpu())
        runs.append(torch.stack(out))
    assert not torch.equal(runs[0][2:, 2], runs[1][2:, 2])  # (the reset did something to its own slot)
    for k in (0, 1, 3):
        assert torch.equal(runs[0][:, k], runs[1][:, k]), k


def test_reset_refuses_bad_slots_before_touching_the_device():
    eng, sd = _engine("conformer")
    for kind in ("sliding", "incremental"):
        sc = _make(kind, eng, sd)
        for bad in ([S], [-1], [1, 1], torch.ones(S + 1, dtype=torch.bool)):
            with pytest.raises(ValueError):
                sc.reset(bad)
        assert sc.samples_seen.tolist() == [0] * S


# ---- KV-cached mode (labelled non-reference, oracle/streaming.py): per-stream tables in the library ---------------------
# 22 ticks: the 16-group ring wraps; slot 3's second session starts at tick 18, after the wrap.  Odd and even start ticks
# put 12- and 13-frame chunks into one step (a stream's chunk sizes run 12, 12, 13, 12, 13, ... from its own first sample).
KV_TICKS = 22
KV_SESSIONS = [(0, 0), (1, 1), (2, 2), (3, 5), (3, 18)]


def _kv_audio():
    from afx import synth
    sess = {(k, t0): synth.waveforms(1, (KV_TICKS - t0) * H, batch_idx=4500 + 10 * k + t0)[0] for k, t0 in KV_SESSIONS}
    return sess, synth.waveforms(S, KV_TICKS * H, batch_idx=4577)


def _kv_engine(arch, dtype):
    from afx import engine, synth
    if arch == "conformer":
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
    else:
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype=dtype)
    eng.load_state_dict(sd)
    return eng, sd


def _kv_staggered(eng, sd):
    """(staggered scores, fresh-scorer scores per session) of the KV-cached scorer over KV_SESSIONS."""
    from afx.streaming import KVCachedScorer
    sess, before = _kv_audio()
    got, _ = _staggered_run(KVCachedScorer(eng, sd, S, window=64000, hop=H), sess, before, KV_SESSIONS, KV_TICKS)
    pad = lambda x: torch.cat([x, torch.zeros(KV_TICKS * H - x.numel())])
    ref_a = _fresh_run(KVCachedScorer(eng, sd, S, window=64000, hop=H), [pad(sess[s]) for s in KV_SESSIONS[:4]], KV_TICKS)
    ref_b = _fresh_run(KVCachedScorer(eng, sd, S, window=64000, hop=H), [before[0], before[1], before[2], pad(sess[(3, 18)])], KV_TICKS)
    return got, ref_a, ref_b, sess


def _kv_check_bits(got, ref_a, ref_b, what):
    for i, (k, t0) in enumerate(KV_SESSIONS):
        ref = ref_a if i < 4 else ref_b
        t1 = 18 if (k, t0) == (3, 5) else KV_TICKS
        for j in range(t1 - t0):
            assert torch.equal(got[t0 + j, k], ref[j, k]), \
                f"{what}: slot {k} session from tick {t0}, its tick {j}: {(got[t0 + j, k] - ref[j, k]).abs().item():.2e}"


@pytest.mark.parametrize("arch", ["conformer", "xlsr_aasist"])
def test_kv_cached_staggered_sessions_are_bit_identical_to_fresh_streams(arch):
    from oracle import streaming as ostream
    sizes = ostream.chunk_sizes(8 * H, H)
    assert sizes[:4] == [12, 12, 13, 12]  # (slots started at ticks 1 and 2 bring 12 and 13 frames at tick 3)
    eng, sd = _kv_engine(arch, "fp16")
    got, ref_a, ref_b, _ = _kv_staggered(eng, sd)
    _kv_check_bits(got, ref_a, ref_b, f"{arch} kv-cached")


def test_kv_cached_sessions_in_split_precision_hold_bits_and_the_offline_restatement():
    """dtype fp16x3 (split-precision ring attention): the staggered run is bit-identical to fresh streams, and every hop of
    the re-started slot is within 1e-3 of oracle/streaming.py on that slot's own audio from its reset."""
    from oracle import streaming as ostream
    eng, sd = _kv_engine("xlsr_aasist", "fp16x3")
    got, ref_a, ref_b, sess = _kv_staggered(eng, sd)
    _kv_check_bits(got, ref_a, ref_b, "xlsr_aasist fp16x3 kv-cached")
    for k, t0, t1 in ((3, 18, KV_TICKS), (2, 2, KV_TICKS)):
        want, _ = ostream.block_causal_scores(sd, sess[(k, t0)][None, :(t1 - t0) * H], H)
        for j in range(t1 - t0):
            assert (got[t0 + j, k] - want[j][0, 1]).abs().item() <= 1e-3, (k, t0, j)


def test_kv_cached_refusals():
    from afx._lib import AfxError
    from afx.streaming import KVCachedScorer
    eng, sd = _kv_engine("conformer", "fp16")
    sc = KVCachedScorer(eng, sd, S, window=64000, hop=H)
    for bad in ([S], [-1], [1, 1]):
        with pytest.raises(ValueError):
            sc.reset(bad)
    kv = eng.kv_state(S)
    f = torch.zeros(S, 13, 512, device=eng.device)
    for nf in ([13, 13, 14, 13], [13, 0, 12, 12]):
        with pytest.raises(AfxError):
            kv.step(f, n_frames=nf)
    with pytest.raises(AfxError):
        kv.reset([0, 0])
    kv.reset([1])
    with pytest.raises(AfxError):  # per-stream state: the lock-stepped step refuses it
        kv.step(f)
    assert kv.step(f, n_frames=[13, 12, 13, 12]).shape == (S, 2)

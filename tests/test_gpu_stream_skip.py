"""Non-paced streams (afx/streaming.py ``push(chunk, slots)``): a push brings hops for the named slots only.  The contract:
a slot's j-th score, whatever ticks its hops arrive on and whatever the other slots do meanwhile, equals, bit for bit, its
score at tick j of a FRESH scorer with the same number of slots in which every slot is pushed on every tick and the slot
is fed its hops back to back."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

S, H, TICKS = 4, 4000, 24
W = 16000  # exact scorers (the KV-cached mode keeps the 4-s window: its slot 0 makes 24 hops, its ring wraps)
# Activity per tick: slot 0 every tick; slot 1 on odd ticks; slot 2 silent until tick 10; slot 3 a burst (ticks 0-4), a gap,
# a reset while idle (tick 7) and a second session from tick 9.  Named in a different order on different ticks.
RESET = {7: [3]}


def _active(t):
    on = [0] + ([1] if t % 2 else []) + ([2] if t >= 10 else []) + ([3] if t < 5 or t >= 9 else [])
    return on[::-1] if t % 3 == 0 else on


def _streams():
    """Per stream (slot, session): its hops in order."""
    from afx import synth
    n = {(0, 0): TICKS, (1, 0): TICKS // 2, (2, 0): TICKS - 10, (3, 0): 5, (3, 1): TICKS - 9}
    return {key: synth.waveforms(1, m * H, batch_idx=5100 + 7 * i)[0].reshape(m, H) for i, (key, m) in enumerate(n.items())}


def _engine(arch, dtype="fp16"):
    from afx import engine, synth
    if arch == "conformer":
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
    else:
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype=dtype)
    eng.load_state_dict(sd)
    return eng, sd


def _make(kind, eng, sd):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=W, hop=H)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=W, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _skip_run(sc, streams):
    """The schedule above -> {(slot, session): [scores in order]} and samples_seen after every tick."""
    pos, sess, got, seen = {}, {k: 0 for k in range(S)}, {}, []
    for t in range(TICKS):
        for k in RESET.get(t, []):
            sc.reset([k])
            sess[k] += 1
        on = _active(t)
        before = sc.samples_seen
        keys = [(k, sess[k]) for k in on]
        chunk = torch.stack([streams[key][pos.get(key, 0)] for key in keys]).cuda()
        out = sc.push(chunk, slots=on).clone().cpu()
        assert out.shape == (len(on),)
        for key, v in zip(keys, out):
            pos[key] = pos.get(key, 0) + 1
            got.setdefault(key, []).append(v)
        after = sc.samples_seen
        assert torch.equal(after - before, torch.tensor([H if k in on else 0 for k in range(S)])), t  # (named slots only)
        seen.append(after)
    return {k: torch.stack(v) for k, v in got.items()}, seen


def _fresh(sc, feed):
    """Lock-stepped fresh scorer: slot k fed feed[k] ((n, H) hops, zero-padded to TICKS) on every tick."""
    pad = [torch.cat([f, torch.zeros(TICKS - f.shape[0], H)]) for f in feed]
    return torch.stack([sc.push(torch.stack([p[t] for p in pad]).cuda()).clone().cpu() for t in range(TICKS)])


def _check(kind, eng, sd, what):
    streams = _streams()
    got, _ = _skip_run(_make(kind, eng, sd), streams)
    ref_a = _fresh(_make(kind, eng, sd), [streams[(0, 0)], streams[(1, 0)], streams[(2, 0)], streams[(3, 0)]])
    ref_b = _fresh(_make(kind, eng, sd), [streams[(1, 0)], streams[(2, 0)], streams[(0, 0)], streams[(3, 1)]])
    for (k, j), ref in (((0, 0), ref_a[:, 0]), ((1, 0), ref_a[:, 1]), ((2, 0), ref_a[:, 2]), ((3, 0), ref_a[:, 3]), ((3, 1), ref_b[:, 3])):
        g = got[(k, j)]
        for i in range(g.shape[0]):
            assert torch.equal(g[i], ref[i]), f"{what}: slot {k} session {j}, its hop {i}: {(g[i] - ref[i]).abs().item():.2e}"
    # the always-active slot: the same bytes whether the others skip (this run) or not (fresh scorer A)
    assert torch.equal(got[(0, 0)], ref_a[:, 0])
    return got, streams


@pytest.mark.parametrize("kind", ["sliding", "incremental"])
@pytest.mark.parametrize("arch", ["conformer", "xlsr_aasist"])
def test_skipping_slots_score_bit_identical_to_fresh_lockstep_streams(arch, kind):
    eng, sd = _engine(arch)
    _check(kind, eng, sd, f"{arch} {kind}")


@pytest.mark.parametrize("arch", ["conformer", "xlsr_aasist"])
def test_kv_cached_skipping_slots_score_bit_identical_to_fresh_lockstep_streams(arch):
    eng, sd = _engine(arch)
    _check("kv", eng, sd, f"{arch} kv-cached")


def test_kv_cached_forms_agree_in_bf16():
    """The three forms of the KV-cached step through the bf16 ring attention.  Skipping slots (list steps) score bit for bit
    as fresh lock-stepped streams; then lock-stepped pushes, a reset and per-stream (ragged) steps: the restarted slot scores
    as a fresh stream fed its audio, the others as if nothing happened.  No bf16 accuracy against the oracle is claimed
    (measured, not gated)."""
    from afx import synth
    eng, sd = _engine("xlsr_aasist", "bf16")
    _check("kv", eng, sd, "xlsr_aasist bf16 kv-cached")
    n, at = 20, 3  # (17 per-stream steps: the 16-group ring wraps in this form too)
    audio = synth.waveforms(S, n * H, batch_idx=5500).reshape(S, n, H)
    a, b, c = _make("kv", eng, sd), _make("kv", eng, sd), _make("kv", eng, sd)
    for t in range(n):
        if t == at:
            a.reset([1])
        got = a.push(audio[:, t].cuda()).clone().cpu()
        ref = b.push(audio[:, t].cuda()).clone().cpu()  # never reset: lock-stepped throughout
        keep = [0, 2, 3] if t >= at else [0, 1, 2, 3]
        assert torch.equal(got[keep], ref[keep]), f"bf16 ragged step, tick {t}: the slots that were not reset"
        if t >= at:
            fresh = c.push(audio[:, t].cuda()).clone().cpu()  # slot 1's session from its first hop
            assert torch.equal(got[1], fresh[1]), f"bf16 ragged step, tick {t}: the restarted slot"


def test_kv_cached_skipping_in_split_precision_holds_bits_and_the_offline_restatement():
    from oracle import streaming as ostream
    eng, sd = _engine("xlsr_aasist", "fp16x3")
    got, streams = _check("kv", eng, sd, "xlsr_aasist fp16x3 kv-cached")
    for key in ((1, 0), (3, 1)):  # a slot active on alternate ticks, and a session started after a reset while idle
        audio = streams[key].reshape(1, -1)
        want, _ = ostream.block_causal_scores(sd, audio, H)
        for j in range(got[key].shape[0]):
            assert (got[key][j] - want[j][0, 1]).abs().item() <= 1e-3, (key, j)


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_naming_every_slot_equals_the_lockstep_push(kind):
    """push(chunk, slots=range(S)) == push(chunk), bit for bit; a permuted list returns the permuted scores."""
    from afx import synth
    eng, sd = _engine("conformer")
    audio = synth.waveforms(S, 5 * H, batch_idx=5300).reshape(S, 5, H)
    a, b, c = _make(kind, eng, sd), _make(kind, eng, sd), _make(kind, eng, sd)
    perm = [2, 0, 3, 1]
    for t in range(5):
        x = audio[:, t].cuda()
        ra = a.push(x).cpu()
        rb = b.push(x, slots=range(S)).cpu()
        rc = c.push(x[perm], slots=perm).cpu()
        assert torch.equal(ra, rb), (kind, t)
        assert torch.equal(ra[perm], rc), (kind, t)
    assert torch.equal(b.push(audio[:, 0].cuda()).cpu(), a.push(audio[:, 0].cuda()).cpu())  # slots=None after: every slot


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_an_empty_slot_list_changes_nothing(kind):
    from afx import synth
    eng, sd = _engine("conformer")
    audio = synth.waveforms(S, 3 * H, batch_idx=5400).reshape(S, 3, H)
    a, b = _make(kind, eng, sd), _make(kind, eng, sd)
    for t in range(3):
        if t == 1:
            for mask in ([], torch.zeros(S, dtype=torch.bool)):
                out = a.push(torch.empty(0, H, device="cuda"), slots=mask)
                assert out.shape == (0,) and out.is_cuda
        assert torch.equal(a.push(audio[:, t].cuda(), slots=range(S)).cpu(), b.push(audio[:, t].cuda(), slots=range(S)).cpu())
    assert torch.equal(a.samples_seen, b.samples_seen)


def test_refusals_of_the_scorers_and_of_the_library():
    from afx import _lib
    from afx._lib import AfxError
    eng, sd = _engine("conformer")
    for kind in ("sliding", "incremental", "kv"):
        sc = _make(kind, eng, sd)
        for slots, rows in (([S], 1), ([-1], 1), ([1, 1], 2), ([0, 2], 3), ([0, 2], 1)):
            with pytest.raises(ValueError):
                sc.push(torch.zeros(rows, H, device="cuda"), slots=slots)
        with pytest.raises(ValueError):
            sc.push(torch.zeros(2, H), slots=[0, 1])  # host tensor
        assert sc.samples_seen.tolist() == [0] * S
    kv = eng.kv_state(S)
    f = torch.zeros(2, 13, 512, device=eng.device)
    for slots in ([1, 1], [0, S], [-1, 0]):  # straight to afx_kv_step_active: duplicate or out-of-range ids
        with pytest.raises(AfxError):
            kv.step(f, slots=slots)
    with pytest.raises(AfxError):
        kv.step(f, n_frames=[13, 14], slots=[0, 1])
    with pytest.raises(ValueError):
        kv.step(f, slots=[0, 1, 2])
    l = _lib.lib()
    assert l.afx_kv_step_active(kv._k, None, 0, None, 13, None, None, None, 0, None) == 0  # an empty list: nothing to launch
    assert kv.step(f, slots=[3, 1]).shape == (2, 2)
    with pytest.raises(AfxError):  # per-stream ring positions: the lock-stepped and the ragged steps refuse the state
        kv.step(torch.zeros(S, 13, 512, device=eng.device))
    with pytest.raises(AfxError):
        kv.step(torch.zeros(S, 13, 512, device=eng.device), n_frames=[13] * S)
    kv.reset([1])
    assert kv.step(f, n_frames=[13, 12], slots=[1, 2]).shape == (2, 2)

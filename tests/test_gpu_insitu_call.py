"""Per-launch fp64 parity on CALL AUDIO on an MI355X: the forwards of tests/test_gpu_insitu.py and the KV-cached step of
tests/test_gpu_insitu_kv.py, fed ``afx.synth.call_waveforms`` -- digital silence, a burst cut to silence, DC, a full-scale
square wave, one PCM step, a click, a tone, G.711 steps, comfort noise, "repeat" concealment -- instead of white noise.
Such audio gives the launches hundreds of bit-identical rows, exactly flat attention logits, a GroupNorm variance of
exactly 0, full-scale levels and levels of one PCM step.  Same references, same bounds, same constants (oracle/insitu.py);
the rounding-bias statistic is taken over distinct rows and store-dominated elements (``check(..., unique_rows=True,
rounding_only=True)``: tests/test_cpu_insitu_call.py shows why) and asserted from 16 384 elements on.  The launch classes
are recorded under a ``_call`` suffix; the file's last test prints them with what ``check_finite`` said about the
full-scale kinds and the whole-model figures."""
import pytest
import torch

import test_gpu_insitu as G
import test_gpu_insitu_kv as KV
from conftest import teacher_conditioning

pytestmark = pytest.mark.gpu

SUMMARY, NOTES = {}, []
CALL = dict(suffix="_call", summary=SUMMARY)
FULL_SCALE = ("clipped", "click")  # (10x every level the other tests feed: the README's range contract may speak here)
L1 = 16000  # 49 frames


@pytest.fixture(scope="module")
def mods():
    from afx import engine, synth
    from oracle import insitu, ssl_trunk
    return engine, synth, insitu, ssl_trunk


def in_range(mods, what, dt, kinds, run):
    """run(kinds) on the whole batch.  The range contract (README): a half-precision engine may refuse the full-scale kinds
    -- ``check_finite`` raises ``AfxError`` -- while fp32 and fp16x3 must not; then the other kinds are run, and checked,
    without them.  Whichever occurs goes into the summary."""
    from afx._lib import AfxError
    try:
        run(list(kinds))
        NOTES.append(f"{what} [{dt}]: finite on every kind")
    except AfxError as e:
        assert dt in mods[2].HALF, f"{what} [{dt}]: check_finite raised in a full-range mode: {e}"
        NOTES.append(f"{what} [{dt}]: check_finite raised on the full batch ({str(e)[:80]}); run again without {FULL_SCALE}")
        run([k for k in kinds if k not in FULL_SCALE])


# (a) ---- trunk, layer_norm ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_trunk_layer_norm_every_kind(mods, dt):
    synth = mods[1]
    eng, sd = G._trunk(mods, 2, dt)
    in_range(mods, "trunk layer_norm", dt, synth.CALL_KINDS,
             lambda kinds: G.trunk_checks(mods, eng, sd, synth.call_waveforms(kinds, L1), dt, call=CALL))


def test_trunk_layer_norm_199_frames_fp16(mods):
    """burst_silence, silence and mulaw at 4 s: 199 frames, the <7,7> attention family."""
    synth = mods[1]
    eng, sd = G._trunk(mods, 2, "fp16")
    G.trunk_checks(mods, eng, sd, synth.call_waveforms(["burst_silence", "silence", "mulaw"], 64000), "fp16", call=CALL)


# (b) ---- trunk, group_norm: silence has variance exactly 0 in every channel, the click normalised values near 50 ------------
@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_trunk_group_norm_every_kind(mods, dt):
    synth = mods[1]
    eng, sd = G._trunk(mods, 1, dt, mode="group_norm")
    in_range(mods, "trunk group_norm", dt, synth.CALL_KINDS,
             lambda kinds: G.trunk_checks(mods, eng, sd, synth.call_waveforms(kinds, L1), dt, mode="group_norm", call=CALL))


# (c) ---- ragged: a short silence clip beside zero padding -- real zeros and pad zeros are told apart by lens alone ---------
RAGGED = (("burst_silence", 49), ("silence", 30), ("tone", 17), ("mulaw", 49), ("idle", 1))


@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_trunk_ragged_call_clips(mods, dt):
    synth = mods[1]
    eng, sd = G._trunk(mods, 1, dt)
    clips = [synth.call_waveforms([k], 400 + 320 * (t - 1))[0] for k, t in RAGGED]
    G.trunk_checks(mods, eng, sd, None, dt, clips=clips, frames=[t for _, t in RAGGED], call=CALL)


# (d) ---- Conformer head and logits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,fused", [("fp16", 1), ("bf16", 1), ("fp16x3", 0), ("fp32", 0)])
def test_conformer_forward_on_call_audio(mods, dt, fused):
    synth = mods[1]
    eng, sd = G._head(mods, dt, fused)
    in_range(mods, "conformer head", dt, synth.CALL_KINDS,
             lambda kinds: G.head_checks(mods, eng, sd, None, dt, fused, wave=synth.call_waveforms(kinds, L1), call=CALL))


# (e) ---- AASIST back-end on the trunk's own output: silence makes GraphPool's candidates exact ties -------------------------
AAS_KINDS = ("silence", "burst_silence", "tone", "mulaw", "noise")


@pytest.mark.parametrize("dt", ["fp16", "fp32", "fp16x3"])
def test_aasist_on_the_trunks_own_output(mods, dt):
    synth = mods[1]
    eng, sd = G._aasist(mods, dt)
    feats = eng.ssl(synth.call_waveforms(AAS_KINDS, L1).cuda()).cpu()
    eng.check_finite()
    assert feats.shape == (len(AAS_KINDS), 49, 1024)
    same = int((feats[0, 1:] == feats[0, :-1]).all(1).sum())
    NOTES.append(f"aasist [{dt}]: {same} of 48 neighbouring frame pairs of the silence clip are bit-identical")
    G.aasist_checks(mods, eng, sd, feats, dt, call=CALL)  # (aas_border == 0 and all six pools are asserted there)


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_aasist_exact_ties_in_every_pool(mods, dt):
    """At 49 frames no two frames of the silence clip leave the trunk bit-identical (the 128-tap positional conv sees
    another share of the zero padding at every frame), so the ties are made exact here: 400 frames, clip 0 holds ONE frame
    of the silence clip's trunk output 400 times (133 identical temporal nodes: what a long zero-concealed gap hands the
    back-end), clip 1 the trunk's output on noise.  ``pool_check`` then assigns the kept rows among identical candidates;
    the kernel's choice among ties is free, its rows, their order and the membership are not."""
    synth = mods[1]
    eng, sd = G._aasist(mods, dt)
    feats = eng.ssl(synth.call_waveforms(["silence", "noise"], 400 + 320 * 399).cuda()).cpu()
    eng.check_finite()
    assert feats.shape == (2, 400, 1024)
    same = int((feats[0, 1:] == feats[0, :-1]).all(1).sum())
    NOTES.append(f"aasist ties [{dt}]: {same} of 399 neighbouring frame pairs of 8 s of silence leave the trunk bit-identical")
    feats[0] = feats[0, 200].clone()
    G.aasist_checks(mods, eng, sd, feats, dt, call=dict(CALL, suffix="_call_ties"))


# (f) ---- the KV-cached step -------------------------------------------------------------------------------------------------
KV_KINDS = ("silence", "burst_silence", "mulaw")
_FRAMES = {}


def kv_frames():
    """(3, 275, 512): conv-layer-6 frames of 5.5 s of each kind from the oracle's conv stack in float64."""
    if "f" not in _FRAMES:
        from afx import synth
        from oracle import ssl_trunk as ST
        _eng, sd = KV._engine("fp16")
        sd64 = {k: v.double() for k, v in sd.items() if k.startswith("feature_extractor.")}
        wave = synth.call_waveforms(KV_KINDS, 400 + 320 * 274).double()
        _FRAMES["f"] = ST.feature_extractor(sd64, wave).float()
        assert _FRAMES["f"].shape == (3, 275, 512)
    return _FRAMES["f"]


@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_kv_lockstep_22_steps_on_call_audio(dt):
    f = kv_frames()
    w = KV.Walker(dt, call=CALL)
    pos = 0
    for i in range(22):  # 12 / 13-frame chunks: the ring (256 slots) wraps
        n = 12 + i % 2
        w.step(f[:, pos:pos + n])
        pos += n
    assert pos == 275 and w.model.hop == 22
    w.done()


@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_kv_active_lists_silence_sits_out_and_returns(dt):
    f = kv_frames()
    w = KV.Walker(dt, call=CALL)
    pos = [0, 0, 0]

    def chunk(slots, n_max, ns=None):
        ns_ = ns or [n_max] * len(slots)
        blk = torch.zeros(len(slots), n_max, 512)
        for i, (s, n) in enumerate(zip(slots, ns_)):
            blk[i, :n] = f[s, pos[s]:pos[s] + n]
            pos[s] += n
        return blk, ns

    for i in range(8):
        blk, _ = chunk([0, 1, 2], 12 + i % 2)
        w.step(blk)
    for slots, n_max, ns in (([1, 2], 12, None), ([2, 1], 13, [13, 5]), ([1], 16, None), ([1, 2], 12, [1, 12]),
                             ([0], 13, None), ([0, 2, 1], 12, [12, 5, 9])):  # stream 0 (silence) sits out four steps
        blk, ns = chunk(slots, n_max, ns)
        w.step(blk, ns, slots)
    assert w.model.active
    w.done()


# (g) ---- whole models against the CPU oracle ----------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.detach().float().cpu().reshape(-1), b.detach().float().cpu().reshape(-1)
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("dt,tol", [("fp16", 1e-3), ("fp16x3", 1e-5)])
def test_conformer_model_scores_on_call_audio(mods, dt, tol):
    """The tolerances of tests/test_gpu_models.py: |dlogit| <= 1e-3 in fp16 (features 2e-3, blocks 3e-3 relative L2),
    1e-5 in split precision."""
    engine, synth, I, ST = mods
    from oracle import models
    sd = synth.model_state_dict("ConformerModel", n_layers=2, n_encoders=2)
    eng = engine.Engine("conformer", n_layers=2, dtype=dt, conf_blocks=2)
    eng.load_state_dict(sd)

    def run(kinds):
        wave = synth.call_waveforms(kinds, L1)
        taps = {}
        ref = models.conformer_forward(sd, wave, taps=taps)
        eng.enable_taps()
        got = eng.forward(wave.cuda()).cpu()
        eng.check_finite()
        err = (got - ref).abs().amax(1)
        NOTES.append(f"ConformerModel [{dt}]: |dlogit| " + ", ".join(f"{k} {e:.1e}" for k, e in zip(kinds, err.tolist())))
        if dt == "fp16":
            assert rel_l2(eng.tap("ssl"), taps["ssl"]) < 2e-3
            assert rel_l2(eng.tap("tokens"), taps["tokens"]) < 2e-3
            for b in range(2):
                assert rel_l2(eng.tap(f"block{b}"), taps[f"block{b}"]) < 3e-3
        eng.enable_taps(False)
        assert float(err.max()) <= tol, dict(zip(kinds, err.tolist()))

    in_range(mods, "ConformerModel", dt, synth.CALL_KINDS, run)


def test_teacher_scores_on_call_audio_fp16x3(mods):
    """XLSR_AASIST (two trunk layers, the lively head of tests/test_gpu_teacher.py), fp16x3, with that file's tolerances:
    back-end 1e-5 on the engine's own features, |dlogit| <= 1e-3 wherever the reference keeps its GraphPool decisions,
    3e-2 elsewhere.  A flipped decision is reported with the reference's own margin (0 on silence: exact ties)."""
    engine, synth, I, ST = mods
    sd = synth.model_state_dict("XLSR_AASIST", n_layers=2, head_scale=1.5)
    eng = engine.Engine("xlsr_aasist", n_layers=2, dtype="fp16x3")
    eng.load_state_dict(sd)
    wave = synth.call_waveforms(synth.CALL_KINDS, L1)
    _ref, _got, rows = teacher_conditioning(sd, wave, eng)
    eng.check_finite()
    for k, r in zip(synth.CALL_KINDS, rows):
        NOTES.append(f"teacher [fp16x3] {k}: |dlogit| {r['dlogit']:.1e}, back-end {r['backend']:.1e}, features {r['feat_rel_l2']:.1e}, "
                     f"top-k {'kept' if r['same_topk'] else 'FLIPPED'} (smallest margin {r['margin']:.1e})")
    assert max(r["backend"] for r in rows) <= 1e-5
    assert all(r["dlogit"] <= 1e-3 for r in rows if r["same_topk"]), [(k, r) for k, r in zip(synth.CALL_KINDS, rows) if r["dlogit"] > 1e-3]
    assert max((r["dlogit"] for r in rows if not r["same_topk"]), default=0.0) <= 3e-2


# ---- the module's summary (the last test of the file: it reports what the tests above measured) -----------------------------
def test_summary_of_worst_ratios_on_call_audio(capsys):
    lines = ["in-place parity on call audio: worst |got - ref| / bound, rounding bias (mean signed ulps, distinct rows)"]
    for (cls, dt), (r, b) in sorted(SUMMARY.items()):
        lines.append(f"  {cls:18s} {dt:7s} ratio {r:.3f}" + (f"  bias {b:+.4f}" if b is not None else ""))
    lines += ["  " + n for n in NOTES]
    with capsys.disabled():  # (printed past pytest's output capture)
        print("\n" + "\n".join(lines))
    assert all(r <= 1.0 for r, _b in SUMMARY.values()), SUMMARY

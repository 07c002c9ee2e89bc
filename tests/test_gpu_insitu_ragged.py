"""Per-launch parity under key-padding masks on an MI355X (``forward_ragged`` / ``ssl_ragged``), in every family of the
trunk attention and of the Shaw attention, and the statement that rows nobody reads do not matter: whatever the workspace
held before a ragged forward (zeros, NaN bit patterns, fp16 infinities), the logits, the valid rows of every tap and the
overflow guard (``check_finite``) are the same.  The per-launch checks are tests/test_gpu_insitu.py's (``trunk_checks``,
``head_checks``, its ``gate`` and ``SUMMARY``) with ``clips`` given; this module's last test prints the worst ratio
per launch class and dtype, the masked classes among them."""
import pytest
import torch

import test_gpu_insitu as base
from test_gpu_insitu import mods  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

DTYPES = ["fp16", "bf16", "fp32", "fp16x3"]


def samples(T):
    """The smallest clip with T frames."""
    return 400 + 320 * (T - 1)


def clips_of(synth, frames, seed):
    return [synth.waveforms(1, samples(T), batch_idx=seed + i)[0] for i, T in enumerate(frames)]


# ---- rows nobody reads must not matter --------------------------------------------------------------------------------
FILLS = ("stale", "zeros", "nan", "inf16")


def fill_workspace(eng, kind):
    """Overwrite the engine's whole workspace: zeros, 0xFF bytes (a NaN in fp16, bf16 and fp32), or the fp16 +inf pattern
    0x7C00 in every half-word ("stale": leave what the earlier forwards left)."""
    ws = eng._ws
    if kind == "zeros":
        ws.zero_()
    elif kind == "nan":
        ws.fill_(0xFF)
    elif kind == "inf16":
        ws[: ws.numel() // 2 * 2].view(torch.int16).fill_(0x7C00)
    torch.cuda.synchronize()


def finite_or_message(eng):
    from afx._lib import AfxError
    try:
        eng.check_finite()
    except AfxError as e:
        return str(e)
    return None


E_FRAMES = [199, 49, 125, 21]
TRUNK_TAPS = ["conv", "feats", "proj", "pos"] + [f"l{l}.{t}" for l in range(2) for t in ("ln1", "qkv", "att", "mid", "ln2", "ff")] + \
             ["layer0", "layer1", "ssl", "ssl.op"]
HEAD_TAPS = ["tokens"] + [f"b{b}.{t}" for b in range(2) for t in ("xa", "qkv", "ao", "xb", "glu", "u")] + ["block0", "block1"]


def tap_valid_rows(eng, ST, frames, arch):
    """The valid rows of every tap of the last (ragged) forward: {name: tensor}."""
    B, Tmax = len(frames), max(frames)
    out = {}
    per_layer = [ST.conv_out_lengths(samples(T)) for T in frames]
    per_max = ST.conv_out_lengths(samples(Tmax))
    for i in range(6):
        t = eng.tap(f"c{i}").reshape(B, per_max[i], -1)
        out[f"c{i}"] = torch.cat([t[b, :per_layer[b][i]] for b in range(B)]).cpu()
    for n in TRUNK_TAPS:
        t = eng.tap(n).reshape(B, Tmax, -1)
        out[n] = torch.cat([t[b, :frames[b]] for b in range(B)]).cpu()
    out["xpad"] = eng.tap("xpad").cpu()  # (whole: the rows past a clip's frames are zeros by contract)
    if arch == "conformer":
        for n in HEAD_TAPS:
            t = eng.tap(n).reshape(B, Tmax + 1, -1)
            if n.endswith(".u"):  # (the fused path neither writes nor reads the pad columns of u)
                t = t[:, :, :288]
            out[n] = torch.cat([t[b, :frames[b] + 1] for b in range(B)]).cpu()
    return out


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("arch", ["conformer", "xlsr_aasist"])
def test_ragged_forward_ignores_unread_rows(mods, arch, dt):
    """Clips of 199, 49, 125 and 21 frames after a larger uniform forward, the workspace left as it is, zeroed, filled with
    NaN bit patterns and with fp16 infinities: the logits and the valid rows of every tap keep every bit, the overflow
    guard stays quiet (it judges the rows of a clip's own length only), the next uniform forward passes it too, and each
    clip equals itself alone."""
    engine, synth, I, ST = mods
    if arch == "conformer":
        sd = synth.model_state_dict("ConformerModel", n_layers=2, n_encoders=2)
        eng = engine.Engine("conformer", n_layers=2, dtype=dt, conf_blocks=2)
    else:
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=2)
        eng = engine.Engine("xlsr_aasist", n_layers=2, dtype=dt)
    eng.load_state_dict(sd)
    clips = [c.cuda() for c in clips_of(synth, E_FRAMES, 2100)]
    for c, T in zip(clips, E_FRAMES):
        assert ST.conv_out_lengths(c.numel())[-1] == T
    other = synth.waveforms(6, 72080, batch_idx=2199).cuda()
    eng.forward(other)
    assert finite_or_message(eng) is None
    eng.forward_ragged(clips)  # (sizes the workspace for the ragged call: the fills below cover all of it)
    finite_or_message(eng)  # (counter cleared; this run's verdict is the "stale" one below)
    eng.forward(other)
    assert finite_or_message(eng) is None
    eng.enable_taps()
    runs, fails = {}, []
    for kind in FILLS:
        fill_workspace(eng, kind)
        ws = eng._ws.data_ptr()
        logits = eng.forward_ragged(clips).cpu()
        assert eng._ws.data_ptr() == ws
        msg = finite_or_message(eng)
        if msg is not None:
            fails.append(f"[{kind}] check_finite raised after a healthy ragged batch: {msg}")
        runs[kind] = (logits, tap_valid_rows(eng, ST, E_FRAMES, arch))
    eng.enable_taps(False)
    l0, t0 = runs["zeros"]
    if not bool(torch.isfinite(l0).all()):
        fails.append(f"logits not finite: {l0.tolist()}")
    for kind in FILLS:
        l, t = runs[kind]
        if not torch.equal(l, l0):
            fails.append(f"[{kind}] logits depend on the workspace's earlier contents: {l.tolist()} / {l0.tolist()}")
        for n in t0:
            if not torch.equal(t[n], t0[n]):
                fails.append(f"[{kind}] valid rows of tap {n} depend on the workspace's earlier contents")
    eng.forward(other)
    msg = finite_or_message(eng)
    if msg is not None:
        fails.append(f"uniform forward after the ragged ones: {msg}")
    for b, c in enumerate(clips):
        alone = eng.forward(c[None]).cpu()[0]
        if not torch.equal(l0[b], alone):
            fails.append(f"clip {b} ({E_FRAMES[b]} frames) differs from itself alone by {(l0[b] - alone).abs().max().item():.2e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", DTYPES)
def test_ragged_ssl_features_ignore_unread_rows(mods, dt):
    """The same for ``ssl_ragged``: valid rows equal across the fills and equal to the clip alone, padded rows exactly 0."""
    engine, synth, I, ST = mods
    eng = engine.Engine("ssl", n_layers=2, dtype=dt)
    eng.load_state_dict(synth.ssl_state_dict(2))
    clips = [c.cuda() for c in clips_of(synth, E_FRAMES, 2100)]
    other = synth.waveforms(6, 72080, batch_idx=2199).cuda()
    eng.ssl(other)
    eng.ssl_ragged(clips)
    finite_or_message(eng)
    fails, ref = [], None
    for kind in FILLS:
        fill_workspace(eng, kind)
        feats, frames = eng.ssl_ragged(clips)
        assert frames == E_FRAMES
        msg = finite_or_message(eng)
        if msg is not None:
            fails.append(f"[{kind}] check_finite raised after a healthy ragged batch: {msg}")
        feats = feats.cpu()
        for b, T in enumerate(E_FRAMES):
            if not bool((feats[b, T:] == 0).all()):
                fails.append(f"[{kind}] clip {b}: rows past its {T} frames are not 0")
        ref = feats if ref is None else ref
        if not torch.equal(feats, ref):
            fails.append(f"[{kind}] features depend on the workspace's earlier contents")
    for b, c in enumerate(clips):
        if not torch.equal(ref[b, :E_FRAMES[b]], eng.ssl(c[None])[0].cpu()):
            fails.append(f"clip {b} differs from itself alone")
    assert finite_or_message(eng) is None
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("form", ["ragged", "active"])
@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp16x3"])
def test_kv_step_ignores_unread_rows(mods, dt, form):
    """The KV-cached per-stream steps (afx_kv_step_ragged, afx_kv_step_active) carve the same workspace: a step whose
    streams bring 1, 7 and 16 frames of a 16-row block, after each fill.  Same logits, a quiet overflow guard."""
    import torch.nn.functional as F
    engine, synth, I, ST = mods
    sd = synth.model_state_dict("ConformerModel", n_layers=2, n_encoders=1)
    eng = engine.Engine("conformer", n_layers=2, dtype=dt, conf_blocks=1)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(77)
    first, second = (F.gelu(torch.randn(3, 16, 512, generator=g)).cuda() for _ in range(2))
    slots = [2, 0, 1] if form == "active" else None
    fails, ref = [], None
    for kind in FILLS:
        kv = eng.kv_state(3)
        kv.step(first, [16, 16, 16], slots)  # (sizes the workspace and gives the rings 16 live slots)
        finite_or_message(eng)
        fill_workspace(eng, kind)
        out = kv.step(second, [1, 7, 16], slots).cpu()
        msg = finite_or_message(eng)
        if msg is not None:
            fails.append(f"[{kind}] check_finite raised after a healthy step: {msg}")
        ref = out if ref is None else ref
        if not (torch.equal(out, ref) and bool(torch.isfinite(out).all())):
            fails.append(f"[{kind}] logits depend on the workspace's earlier contents: {out.tolist()} / {ref.tolist()}")
    assert not fails, "\n".join(fails)


# ---- the trunk under masks, across every attention family ---------------------------------------------------------------
# Frames per clip, each set on a tile, block or split edge of launch_mhsa_t / launch_mhsa_split (the longest clip picks
# the kernel, H * B the z-split: 16 heads).  The profile has ONE class ("mhsa_kernel") for every trunk-attention kernel,
# the fp32 VALU attention included, so the family is known from the dispatch code only; what the profile does tell apart
# is the positional conv: "posconv_kernel" launches (sliding form, <= 224 frames, fp16 / bf16) or none (product form).
FAMILIES = {
    "k24": [64, 63, 17, 1],                                            # mhsa_kernel<2,4>
    "k44_z2": [128, 65, 64, 16, 1],                                    # <4,4>, two workgroups per (utterance, head)
    "k44_z1": [65] + [(64, 33, 1)[i % 3] for i in range(24)],          # <4,4>, H * B = 400 > 384: one workgroup
    "k77": [224, 199, 129, 33, 1],                                     # <7,7>
    "long2": [225, 224, 129, 128, 64, 1],                              # blocked kernel, 2 key blocks
    "long4": [449, 257, 256, 1],                                       # blocked kernel, 4 key blocks
}
CONV_FAMILY = "k24"  # (the conv stack under masks runs in this family, once per dtype)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_trunk_launches_under_masks(mods, family, dt):
    """``ssl_ragged`` on a one-layer trunk: every launch against its reference under the key-padding masks.  fp16x3 runs
    the split-precision families up to 224 frames and, beyond, the fp32 VALU attention and the product-form posconv."""
    engine, synth, I, ST = mods
    frames = FAMILIES[family]
    assert len(frames) * 16 > 384 if family == "k44_z1" else len(frames) * 16 <= 384
    eng, sd = base._trunk(mods, 1, dt)
    clips = clips_of(synth, frames, 3000 + 10 * len(frames))
    prof = base.trunk_checks(mods, eng, sd, None, dt, conv=family == CONV_FAMILY, clips=clips, frames=frames)
    assert prof["mhsa_kernel"]["launches"] == 1
    if dt in I.HALF:
        assert prof["posconv_kernel"]["launches"] == (1 if max(frames) <= 224 else 0)


# ---- the Conformer head under masks -------------------------------------------------------------------------------------
HEAD_FRAMES = {
    "one_pass_limit": [208, 124, 1],        # N = 209 tokens: the one-pass limit of the Shaw attention
    "blocked": [209, 208, 13],              # the 128-key blocked form
    "clamp": [600, 513, 512, 30],           # distances beyond +-512: the clamp is active
}


@pytest.mark.parametrize("dt,fused", [("fp16", 1), ("bf16", 1), ("fp16x3", 0), ("fp32", 0)])
@pytest.mark.parametrize("shape", list(HEAD_FRAMES))
def test_head_launches_under_masks(mods, shape, dt, fused):
    """``forward_ragged`` on a conformer engine with a one-layer trunk: tokens, both blocks' launches and the logits, the
    attention and the depthwise conv masked at each clip's frames + 1 tokens."""
    engine, synth, I, ST = mods
    frames = HEAD_FRAMES[shape]
    eng, sd = base._head(mods, dt, fused)
    base.head_checks(mods, eng, sd, None, dt, fused, clips=clips_of(synth, frames, 4000 + frames[0]), frames=frames)


# ---- the attention kernels alone on lively logits -------------------------------------------------------------------------
KB, KH = 2, 3
PLANT_ROWS = (3, -1, 17, 0)  # the query rows (mod T) that get a dominating key at key 0, 127, 128, T - 1


def lively_qkv(T, dt, seed):
    """q, k = 3 randn (logit spread ~9), v = randn, rounded to the operand type; per utterance and head one dominating
    key for each planted row: k = c q / |q| with c set 12 above the row's largest other logit.  -> (qkv (B T, 3 H 64)
    float64 operand values, planted (row, key) pairs)."""
    from oracle import insitu as I
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(KB, T, 3, KH, 64, generator=g, dtype=torch.float64)
    x[:, :, :2] *= 3.0
    x = I.op(x, dt)
    keys = sorted({k for k in (0, 127, 128, T - 1) if k < T})
    plant = [(PLANT_ROWS[j] % T, k) for j, k in enumerate(keys)]
    assert len({r for r, _ in plant}) == len(plant)
    for b in range(KB):
        for h in range(KH):
            for r, k in plant:
                q = x[b, r, 0, h]
                others = (x[b, :, 1, h] @ q) / 8.0
                x[b, k, 1, h] = I.op((8.0 * (float(others.max()) + 12.0) / float(q.norm())) * q / q.norm(), dt)
    return x.reshape(KB * T, 3 * KH * 64), plant


@pytest.mark.parametrize("T,dt", [(T, dt) for T in (64, 65, 128, 129, 224, 225, 256, 257, 449) for dt in ("fp16", "bf16", "fp16x3")
                                  if dt != "fp16x3" or T <= 224])
def test_mhsa_kernel_on_lively_logits(mods, T, dt):
    """``afx.kernels.mhsa`` alone, judged with ``insitu.mhsa``'s bound and bias statistic (no tolerance): a wrong rescale
    of a running maximum or one mis-weighted key is far outside it.  Up to 224 frames the one-pass family AND the blocked
    kernel (mhsa_force_long); beyond, the blocked kernel either way.  fp16x3: the split-precision face takes fp32 rows
    and 1 .. 224 frames."""
    engine, synth, I, ST = mods
    from afx import kernels
    from afx._lib import lib, check
    qkv, plant = lively_qkv(T, dt, 7000 + T)
    rows = torch.arange(KB * T)
    # the adversarial inputs, on the reference alone
    x = qkv.reshape(KB, T, 3, KH, 64)
    p = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1]) / 8.0, -1)
    for r, k in plant:
        assert bool((p[:, :, r].amax(-1) > 0.9).all()) and bool((p[:, :, r].argmax(-1) == k).all()), (r, k)
    assert bool((p[:, :, plant[-1][0]].argmax(-1) >= 128 * ((T - 1) // 128)).all())  # (a maximum in the last key block)
    dev = qkv.to(engine.torch_dtype(dt)).cuda()
    fails = []
    # (the knob is the half-precision launcher's; beyond 224 frames the blocked kernel runs either way: once)
    forms = [0, 1] if dt != "fp16x3" and T <= 224 else [0]
    for force in forms:
        blocked = bool(force) or T > 224
        ref = I.mhsa(qkv, rows, T, dt, heads=KH, bias_ref=True, blocked=blocked)
        check(lib().afx_debug_set(b"mhsa_force_long", force))
        try:
            out = kernels.mhsa(dt, dev, KB, T, KH).cpu().double()
        finally:
            check(lib().afx_debug_set(b"mhsa_force_long", 0))
        cls = "mhsa_k_long" if blocked else "mhsa_k"
        base.gate(cls, dt, f"mhsa T={T} force_long={force}", I.check(out, ref[0], ref[1], dt, rows, bias_ref=ref[2]), I, fails, True)
    assert not fails, "\n".join(fails)


# ---- the summary line (this file's last test) ---------------------------------------------------------------------------
def test_summary_of_worst_ratios_per_launch_class(capsys):
    """Worst ratio and bias per (launch class, dtype) of every in-place check run so far in this session
    (tests/test_gpu_insitu.py's ``SUMMARY``: the masked classes of this module among them)."""
    lines = ["in-place parity under masks (cumulative): worst |got - ref| / bound, rounding bias (mean signed ulps)"]
    for (cls, dt), (r, b) in sorted(base.SUMMARY.items()):
        lines.append(f"  {cls:13s} {dt:7s} ratio {r:.3f}" + (f"  bias {b:+.4f}" if b is not None else ""))
    with capsys.disabled():  # (printed past pytest's output capture)
        print("\n" + "\n".join(lines))
    assert all(r <= 1.0 for r, _b in base.SUMMARY.values()), base.SUMMARY

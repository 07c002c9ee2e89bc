"""Per-launch parity inside real forwards on an MI355X: every tapped launch of the SSL trunk, of the Conformer head and
of the AASIST back-end against its fp64 reference (oracle/insitu.py) built from the launch's own tapped inputs, element by element within the
bounds stated there, from the conv stack to the final LayerNorm's two outputs and from the Conformer's tokens to its
logits.  Large products are checked on a deterministic subset of rows (``check_rows``).  ``trunk_checks`` and
``head_checks`` also take ragged batches (``clips``); tests/test_gpu_insitu_ragged.py runs those.  The module's
summary line gives, per launch class and dtype, the worst |got - ref| / bound and the rounding-bias statistic."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SUMMARY = {}


@pytest.fixture(scope="module", autouse=True)
def _summary(request):
    yield
    lines = ["in-place parity: worst |got - ref| / bound, rounding bias (mean signed ulps)"]
    for (cls, dt), (r, b) in sorted(SUMMARY.items()):
        lines.append(f"  {cls:10s} {dt:7s} ratio {r:.3f}" + (f"  bias {b:+.4f}" if b is not None else ""))
    cm = request.config.pluginmanager.get_plugin("capturemanager")
    with cm.global_and_fixture_disabled():  # (printed past pytest's output capture)
        print("\n" + "\n".join(lines))


@pytest.fixture(scope="module")
def mods():
    from afx import engine, synth
    from oracle import insitu, ssl_trunk
    return engine, synth, insitu, ssl_trunk


def check_rows(B, T):
    """The subset of flat rows (B utterances of T) a large launch is checked on: every row of the first and the last
    utterance, every row whose index mod 256 is in {0, 15, 16, 63, 64, 127, 128, 255}, the last row of every
    utterance, every 7th row."""
    M = B * T
    r = torch.arange(M)
    m = (r < T) | (r >= M - T) | (r % 7 == 0) | ((r + 1) % T == 0)
    for k in (0, 15, 16, 63, 64, 127, 128, 255):
        m |= r % 256 == k
    return r[m]


def conv_rows(B, T):
    """Lighter subset for the conv stack's long row counts: the first and last 64 rows of the first and the last
    utterance, the last row of every utterance, the rows mod 256 in the set above, every 61st row."""
    M = B * T
    r = torch.arange(M)
    t = r % T
    m = ((r < T) | (r >= M - T)) & ((t < 64) | (t >= T - 64))
    m |= (t == T - 1) | (r % 61 == 0)
    for k in (0, 15, 16, 63, 64, 127, 128, 255):
        m |= r % 256 == k
    return r[m]


MIN_BIAS_N = 16384  # (tests/test_gpu_insitu_kv.py derives it: one element's rounding error has sigma 0.29 ulp against BIAS_MAX)


def gate(cls, dt, where, res, insitu, fails, op_dt=False, suffix="", summary=None, min_n=0):
    """Record one launch's result; a launch past its bound (or biased) is added to `fails` (every launch of the forward
    is checked before the test asserts, so one run names all of them).  suffix: appended to the class in the summary
    (`summary`: another module's table); min_n: the bias statistic is asserted and recorded only where it rests on at
    least that many elements (``check(..., unique_rows=True)`` may leave few)."""
    key = (cls + suffix, dt)
    table = SUMMARY if summary is None else summary
    r0, b0 = table.get(key, (0.0, None))
    if res["bias"] is not None and res["n"] < min_n:
        res = dict(res, bias=None)
    b = res["bias"] if op_dt else None
    table[key] = (max(r0, res["ratio"]), b if b0 is None or (b is not None and abs(b) > abs(b0)) else b0)
    if not res["ratio"] <= 1.0:
        fails.append(f"{where} [{dt}]: |got - ref| = {res['ratio']:.2f} x bound at row {res['row']}, col {res['col']} "
                     f"(got {res['got']:.6e}, ref {res['ref']:.6e}, bound {res['bound']:.2e})")
    if op_dt and dt in insitu.HALF and cls not in insitu.BIAS_REPORTED and res["bias"] is not None and \
            abs(res["bias"]) > insitu.BIAS_MAX:
        fails.append(f"{where} [{dt}]: rounding bias {res['bias']:+.3f} ulp")


def _call_kw(call):
    """-> (keywords of insitu.check, keywords of gate) for the `call` argument of the *_checks functions."""
    if call is None:
        return {}, {}
    return dict(unique_rows=True, rounding_only=True), dict(suffix=call["suffix"], summary=call["summary"], min_n=MIN_BIAS_N)


def _ragged(ST, clips):
    """clips (1-D waveforms) -> (zero-padded batch (B, Lmax), per conv layer the valid lengths of every clip)."""
    L = max(c.numel() for c in clips)
    wave = torch.zeros(len(clips), L)
    for b, c in enumerate(clips):
        wave[b, :c.numel()] = c
    per = [ST.conv_out_lengths(c.numel()) for c in clips]
    return wave, [[p[i] for p in per] for i in range(7)]


def trunk_checks(mods, eng, sd, wave, dt, mode="layer_norm", conv=True, clips=None, frames=None, few=False, call=None):
    """Run one taps-on forward of `eng` on `wave` and check every tapped launch of the trunk.  clips (a list of 1-D
    waveforms, `wave` ignored): the forward is ``eng.ssl_ragged(clips)`` and every launch is judged under the
    key-padding masks, on the rows of each clip's own length only (``insitu.masked_rows``); frames: the frame counts the
    clips were cut for (asserted with ``conv_out_lengths``).  call (tests/test_gpu_insitu_call.py: dict(suffix, summary)):
    degenerate audio -- the bias statistic over distinct rows and store-dominated elements only, asserted from MIN_BIAS_N
    elements on, the classes recorded under the suffix in that module's summary, ``eng.check_finite()`` after the forward.
    -> the forward's profile (``Engine.profile_end``)."""
    engine, synth, I, ST = mods
    lens_i = None
    if clips is not None:
        wave, lens_i = _ragged(ST, clips)
        assert frames is None or lens_i[6] == list(frames), (lens_i[6], frames)
    B, L = wave.shape
    Ts = ST.conv_out_lengths(L)
    T = Ts[-1]
    lens = lens_i[6] if clips is not None else None
    eng.enable_taps()
    eng.profile_begin()
    if clips is not None:
        _, got_frames = eng.ssl_ragged([c.cuda() for c in clips])
        assert got_frames == lens
    else:
        eng.ssl(wave.cuda())
    prof = eng.profile_end()
    torch.cuda.synchronize()
    if call is not None:
        eng.check_finite()
    tap = lambda n: eng.tap(n).cpu().double()

    fails = []
    ck, gk = _call_kw(call)

    def g(cls, where, got, ref_bnd, op_dt, rows=None):
        gate(cls, dt, where, I.check(got, ref_bnd[0], ref_bnd[1], dt if op_dt else None, rows, **ck), I, fails, op_dt, **gk)

    C = 512
    if conv:
        prev = None
        for i in range(6):
            cur = tap(f"c{i}").reshape(B * Ts[i], C)
            rows = conv_rows(B, Ts[i]) if lens is None else I.masked_rows(lens_i[i], Ts[i])
            ref = I.conv0(sd, wave, rows, dt, mode) if i == 0 else I.conv_layer(sd, i, prev, B, rows, dt, mode)
            g("conv0" if i == 0 else "conv", f"c{i}", cur[rows], ref, True, rows)
            prev = cur
        rows = conv_rows(B, T) if lens is None else I.masked_rows(lens, T)
        g("conv", "conv", tap("conv").reshape(B * T, C)[rows], I.conv_layer(sd, 6, prev, B, rows, dt, mode, out="f32"), False, rows)
    # (group_norm mode differs in the conv stack alone: the launches from here on are the same pre-LN sequence)
    # every valid row (row-local launches checked whole) and the subset the large launches are checked on
    vr = torch.arange(B * T) if lens is None else I.valid_rows(lens, T)
    rows = check_rows(B, T) if lens is None else I.masked_rows(lens, T)
    conv6 = tap("conv").reshape(B * T, C)
    g("layernorm", "feats", tap("feats").reshape(B * T, C)[vr],
      I.layernorm(conv6[vr], sd["layer_norm.weight"], sd["layer_norm.bias"], dt), True, vr)
    feats = tap("feats").reshape(B * T, C)
    D = 1024
    proj = tap("proj").reshape(B * T, D)
    g("product", "proj", proj[rows], I.product(feats[rows], sd["post_extract_proj.weight"], sd["post_extract_proj.bias"], dt), False, rows)
    xpad = tap("xpad").reshape(B, T + 128, D)
    assert bool((xpad[:, :64] == 0).all()) and bool((xpad[:, 64 + T:] == 0).all()), f"xpad [{dt}]: nonzero pad rows"
    g("product", "xpad", xpad[:, 64:64 + T].reshape(B * T, D)[rows],
      I.product(feats[rows], sd["post_extract_proj.weight"], sd["post_extract_proj.bias"], dt, out="op"), True, rows)
    x = tap("pos").reshape(B * T, D)
    g("posconv", "pos", x[rows], I.posconv(sd, xpad, proj, rows, T, dt, lens=lens), False, rows)
    wqkv = lambda p, k: torch.cat([sd[p + f"self_attn.{n}_proj.{k}"] for n in "qkv"], 0)
    # "mhsa": the uniform batches this module has always run, bias asserted against the exact reference as ever.  The new
    # batches -- under masks ("mhsa_masked"; "mhsa_long" from 225 frames on, the blocked any-length kernel) or uniform with
    # few clips (`few`: "mhsa_few" / "mhsa_long") -- assert it too, against the reference that rounds P as the kernel does
    # (insitu._p_rounded): with 1 .. 25 clips the exact reference's statistic carries P's own rounding, shared by all
    # elements of an (utterance, head), and says nothing about the store
    p_ref = lens is not None or few or call is not None
    att_cls = "mhsa" if not p_ref else "mhsa_long" if T > 224 else "mhsa_few" if lens is None else "mhsa_masked"
    for l in range(ST.num_layers(sd)):
        p, n = f"encoder.layers.{l}.", f"l{l}."
        ln1 = tap(n + "ln1").reshape(B * T, D)
        g("layernorm", n + "ln1", ln1[vr], I.layernorm(x[vr], sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"], dt), True, vr)
        qkv = tap(n + "qkv").reshape(B * T, 3 * D)
        g("product", n + "qkv", qkv[rows], I.product(ln1[rows], wqkv(p, "weight"), wqkv(p, "bias"), dt, out="op"), True, rows)
        att = tap(n + "att").reshape(B * T, D)
        ar = I.mhsa(qkv, rows, T, dt, lens=lens, bias_ref=p_ref)
        gate(att_cls, dt, n + "att", I.check(att[rows], ar[0], ar[1], dt, rows, bias_ref=ar[2] if p_ref else None, **ck), I, fails, True, **gk)
        mid = tap(n + "mid").reshape(B * T, D)
        g("product", n + "mid", mid[rows], I.product(att[rows], sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"],
                                                      dt, resid=x[rows]), False, rows)
        ln2 = tap(n + "ln2").reshape(B * T, D)
        g("layernorm", n + "ln2", ln2[vr], I.layernorm(mid[vr], sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], dt), True, vr)
        ff = tap(n + "ff").reshape(B * T, 4096)
        g("product", n + "ff", ff[rows], I.product(ln2[rows], sd[p + "fc1.weight"], sd[p + "fc1.bias"], dt, act="gelu", out="op"), True, rows)
        x = tap(f"layer{l}").reshape(B * T, D)
        g("product", f"layer{l}", x[rows], I.product(ff[rows], sd[p + "fc2.weight"], sd[p + "fc2.bias"], dt, resid=mid[rows]), False, rows)
    # the final LayerNorm: one launch, the fp32 feature rows and the operand copy the back-end reads
    r32, rop = I.final_layernorm(x[vr], sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], dt)
    g("final_ln", "ssl", tap("ssl").reshape(B * T, D)[vr], r32, False, vr)
    g("final_ln", "ssl.op", tap("ssl.op").reshape(B * T, D)[vr], rop, True, vr)
    eng.enable_taps(False)
    assert not fails, "\n".join(fails)
    return prof


def _trunk(mods, n_layers, dt, mode="layer_norm"):
    engine, synth, I, ST = mods
    full = synth.ssl_state_dict(n_layers, extractor_mode=mode)
    eng = engine.Engine("ssl", n_layers=n_layers, dtype=dt, extractor_mode=mode)
    eng.load_state_dict(full)
    return eng, {k[len(synth.SSL_PREFIX):]: v for k, v in full.items()}


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_trunk_launches_teacher_batch(mods, dt):
    eng, sd = _trunk(mods, 2, dt)
    trunk_checks(mods, eng, sd, mods[1].waveforms(16, 64000), dt)


@pytest.mark.parametrize("B,L", [(64, 64000), (3, 64600), (1, 400), (2, 72080)])
def test_trunk_launches_other_shapes_fp16(mods, B, L):
    eng, sd = _trunk(mods, 1, "fp16")
    trunk_checks(mods, eng, sd, mods[1].waveforms(B, L, batch_idx=B + L), "fp16", conv=B < 64)


# uniform batches in the attention families the shapes above never reach: (3, 100) = mhsa_kernel<4,4> with the z-split,
# (2, 449) = the blocked any-length kernel over four 128-key blocks (fp16x3: the fp32 VALU attention and the product-form
# positional conv), and in the dtypes that had run (16, 199) only (3, 201) = <7,7> and (1, 1) = <2,4>.  The profile has
# ONE class for every trunk-attention kernel, so it cannot tell the families apart: the family follows from T and H * B by
# launch_mhsa_t's dispatch; the positional conv's two forms are told apart by the "posconv_kernel" class.
@pytest.mark.parametrize("B,T,dt", [(B, T, dt) for B, T in ((3, 100), (2, 449)) for dt in ("fp16", "bf16", "fp32", "fp16x3")] +
                         [(B, T, dt) for B, T in ((3, 201), (1, 1)) for dt in ("bf16", "fp32", "fp16x3")])
def test_trunk_launches_uniform_attention_families(mods, B, T, dt):
    engine, synth, I, ST = mods
    L = 400 + 320 * (T - 1)
    assert ST.conv_out_lengths(L)[-1] == T
    eng, sd = _trunk(mods, 1, dt)
    prof = trunk_checks(mods, eng, sd, synth.waveforms(B, L, batch_idx=3 * B + T), dt, conv=False, few=True)
    assert prof["mhsa_kernel"]["launches"] == 1
    if dt in I.HALF:
        assert prof["posconv_kernel"]["launches"] == (1 if T <= 224 else 0)


def test_trunk_posconv_gemm_form(mods):
    eng, sd = _trunk(mods, 1, "fp16")
    eng.set("posconv_sliding", 0)
    trunk_checks(mods, eng, sd, mods[1].waveforms(4, 64000, batch_idx=5), "fp16", conv=False)


def test_trunk_group_norm_extractor(mods):
    eng, sd = _trunk(mods, 1, "fp16", mode="group_norm")
    trunk_checks(mods, eng, sd, mods[1].waveforms(2, 64000, batch_idx=6), "fp16", mode="group_norm")


# ---- Conformer head ------------------------------------------------------------------------------------------------------
def head_checks(mods, eng, sd, feats, dt, fused, clips=None, wave=None, frames=None, call=None):
    """One taps-on forward and every tapped launch of the Conformer head, from the tokens to the classifier's logits.
    feats (B, T, 1024): ``eng.head(feats)``.  wave (B, L): a whole ``eng.forward(wave)``, the head reads the trunk's
    operand copy ("ssl.op").  clips (a list of 1-D waveforms): ``eng.forward_ragged(clips)``, every launch judged under
    the key-padding masks on the tokens of each clip's own length (its frames + 1) only.  call: as in ``trunk_checks``."""
    engine, synth, I, ST = mods
    eng.enable_taps()
    ck, gk = _call_kw(call)
    lens = None
    if clips is not None:
        lens = [ST.conv_out_lengths(c.numel())[-1] for c in clips]
        assert frames is None or lens == list(frames), (lens, frames)
        B, T = len(clips), max(lens)
        logits = eng.forward_ragged([c.cuda() for c in clips])
    elif wave is not None:
        B, T = wave.shape[0], ST.conv_out_lengths(wave.shape[1])[-1]
        logits = eng.forward(wave.cuda())
    else:
        B, T, _ = feats.shape
        logits = eng.head(feats.cuda())
    N, E = T + 1, 144
    M = B * N
    torch.cuda.synchronize()
    if call is not None:
        eng.check_finite()
    tap = lambda n: eng.tap(n).cpu().double()

    fails = []

    def g(cls, where, got, ref_bnd, op_dt, rows=None):
        gate(cls, dt, where, I.check(got, ref_bnd[0], ref_bnd[1], dt if op_dt else None, rows, **ck), I, fails, op_dt, **gk)

    # vr: every token row that means something; rows: the subset the attention is checked on
    vr = torch.arange(M) if lens is None else I.valid_rows([n + 1 for n in lens], N)
    rows = check_rows(B, N) if lens is None else I.masked_rows([n + 1 for n in lens], N)
    # the head's input as its first product reads it: the trunk's operand copy, or the given features rounded
    ssl_op = I.op(I.d(feats).reshape(B * T, 1024), dt) if feats is not None else tap("ssl.op").reshape(B * T, 1024)
    x = tap("tokens").reshape(M, E)
    tok = I.conf_tokens(sd, ssl_op, B, T, dt)
    g("tokens", "tokens", x[vr], (tok[0][vr], tok[1][vr]), False, vr)
    Ep = eng.tap("b0.ao").numel() // M  # (operand rows padded to whole 64-column K-steps)
    shaw_cls, dw_cls = ("shaw", "dwconv") if lens is None else ("shaw_masked", "dwconv_masked")
    for b in range(2):
        p, n = f"conformer.encoder_blocks.{b}.", f"b{b}."
        (xa_r, qkv_r) = I.chain_a(sd, p, x[vr], dt)
        xa, qkv = tap(n + "xa").reshape(M, E), tap(n + "qkv").reshape(M, 3 * E)
        g("chain_a", n + "xa", xa[vr], xa_r, False, vr)
        g("chain_a", n + "qkv", qkv[vr], qkv_r, False, vr)
        ao = tap(n + "ao").reshape(M, Ep)
        if not bool((ao[:, E:] == 0).all()):
            fails.append(f"{n}ao [{dt}]: nonzero pad columns")
        g(shaw_cls, n + "ao", ao[rows, :E], I.shaw(qkv, sd[p + "attn.fn.rel_pos_emb.weight"], rows, N, dt, lens=lens), True, rows)
        xb_r, glu_r = I.chain_b(sd, p, xa[vr], ao[vr, :E], dt)
        xb, glu = tap(n + "xb").reshape(M, E), tap(n + "glu").reshape(M, 576)
        g("chain_b", n + "xb", xb[vr], xb_r, False, vr)
        g("chain_b", n + "glu", glu[vr], glu_r, False, vr)
        u = tap(n + "u").reshape(M, -1)
        dw = I.glu_dwconv(sd, p, glu, B, N, dt, lens=lens)
        g(dw_cls, n + "u", u[vr, :288], (dw[0][vr], dw[1][vr]), True, vr)
        if not fused:  # (the fused chain C reads the 288 real columns of u only; the per-op product reads them all)
            if not bool((u[:, 288:] == 0).all()):
                fails.append(f"{n}u [{dt}]: nonzero pad columns")
            for h in ("ff1.hc", "attn.hc", "conv.hc", "ff2.hc", "ff1.hid", "ff2.hid"):
                t = tap(n + h).reshape(M, -1)
                k = E if h.endswith("hc") else 576
                if not bool((t[:, k:] == 0).all()):
                    fails.append(f"{n}{h} [{dt}]: nonzero pad columns")
        blk = tap(f"block{b}").reshape(M, E)
        g("chain_c", f"block{b}", blk[vr], I.chain_c(sd, p, xb[vr], u[vr, :288], dt), False, vr)
        x = blk
    # the classifier reads token 0 of every utterance
    first = torch.arange(B) * N
    g("logits", "logits", logits.cpu().double(), I.conf_logits(sd, x[first], B, 1), False)
    eng.enable_taps(False)
    assert not fails, "\n".join(fails)


def _head(mods, dt, fused, kernel=31):
    engine, synth, I, ST = mods
    head = synth.conformer_head_state_dict(emb_size=144, heads=4, kernel_size=kernel, n_encoders=2)
    full = dict(synth.ssl_state_dict(1))
    full.update(head)
    eng = engine.Engine("conformer", n_layers=1, dtype=dt, conf_kernel=kernel, conf_blocks=2)
    eng.load_state_dict(full)
    eng.set("fuse_conformer", 1 if fused else 0)
    return eng, head


def _feats(B, T, seed):
    return torch.randn(B, T, 1024, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("dt,fused", [("fp16", 1), ("fp16", 0), ("bf16", 1), ("bf16", 0), ("fp16x3", 1), ("fp16x3", 0), ("fp32", 0)])
def test_head_launches_student_batch(mods, dt, fused):
    eng, sd = _head(mods, dt, fused)
    head_checks(mods, eng, sd, _feats(64, 199, 1), dt, fused)


@pytest.mark.parametrize("B,T", [(3, 124), (1, 1), (2, 208), (2, 209), (1, 1100)])
@pytest.mark.parametrize("dt,fused", [("fp16", 1), ("fp16x3", 0)])
def test_head_launches_edge_shapes(mods, B, T, dt, fused):
    eng, sd = _head(mods, dt, fused)
    head_checks(mods, eng, sd, _feats(B, T, B * 1000 + T), dt, fused)


def test_head_launches_even_kernel(mods):
    eng, sd = _head(mods, "fp16", 1, kernel=16)
    head_checks(mods, eng, sd, _feats(3, 124, 7), "fp16", 1)


@pytest.mark.parametrize("dt,fused", [("fp16", 1), ("bf16", 1), ("fp16x3", 0), ("fp32", 0)])
def test_conformer_forward_both_ends(mods, dt, fused):
    """A whole ``forward``: the head's tokens from the trunk's own operand copy of the final LayerNorm ("ssl.op", the
    second output of that launch), every head launch, and the classifier's logits as the call returns them."""
    eng, sd = _head(mods, dt, fused)
    head_checks(mods, eng, sd, None, dt, fused, wave=mods[1].waveforms(3, 16000, batch_idx=31))


# ---- AASIST back-end ---------------------------------------------------------------------------------------------------------
_AAS = {}


def _aasist(mods, dt):
    """One xlsr_aasist engine per dtype (one-layer trunk, the lively head), shared by the tests of this module."""
    engine, synth, I, ST = mods
    if "sd" not in _AAS:
        _AAS["sd"] = synth.model_state_dict("XLSR_AASIST", n_layers=1, head_scale=1.5)
    if dt not in _AAS:
        _AAS[dt] = engine.Engine("xlsr_aasist", n_layers=1, dtype=dt)
        _AAS[dt].load_state_dict(_AAS["sd"])
    return _AAS[dt], _AAS["sd"]


AAS_TAPS = ["aa.ll", "aa.x1", "aa.b0.y", "aa.b0.d", "aa.b0", "aa.b1.y", "aa.b1", "aa.b2.y", "aa.b2.d", "aa.b2", "aa.b3.y", "aa.b3",
            "aa.b4.y", "aa.b4", "aa.b5.y", "aa.b5", "aa.w1", "aa.w2", "e_S", "e_T", "gat_S", "gat_T", "out_S", "out_T"] + \
           [f"b{k}_{t}" for k in (1, 2) for t in ("xp", "T1", "S1", "m1", "T1p", "S1p", "xp2", "Ta", "Sa", "ma")] + ["hidden", "logits"]


def aasist_checks(mods, eng, sd, feats, dt, call=None):
    """One taps-on forward of the back-end; every launch against its reference (oracle/insitu.py::aasist_walk).
    call: as in ``trunk_checks`` (the back-end is fp32: no bias statistic, the suffix and the summary only)."""
    engine, synth, I, ST = mods
    eng.enable_taps()
    eng.head(feats.cuda())
    torch.cuda.synchronize()
    if call is not None:
        eng.check_finite()
    res, zeros = I.aasist_walk(sd, feats, lambda n: eng.tap(n).cpu().double(), dt != "fp32")
    eng.enable_taps(False)
    fails = []
    for cls, name, r in res:
        gate(cls, dt, name, r, I, fails, **_call_kw(call)[1])
    fails += [f"{name} [{dt}]: {n} nonzero floats in the image head / at invalid virtual pixels" for name, n in zeros if n]
    assert sum(1 for cls, _, _ in res if cls == "pool") == 6  # (every pool is checked: near ties are tolerated, not skipped)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_aasist_launches_ragged_last_tile(mods, dt):
    eng, sd = _aasist(mods, dt)
    aasist_checks(mods, eng, sd, _feats(2, 49, 2049), dt)


def test_aasist_conv_many_tiles_per_workgroup(mods):
    """Three workgroups walk the 26 tiles of (2, 49): nine tiles each, the prefetch of the next tile and its clamp at the
    last pixel; every tap equals the automatic grid's bit for bit."""
    from afx._lib import lib, check
    eng, sd = _aasist(mods, "fp16")
    feats = _feats(2, 49, 2049)
    eng.enable_taps()
    eng.head(feats.cuda())
    auto = _all_taps(eng, AAS_TAPS)
    eng.enable_taps(False)
    check(lib().afx_debug_set(b"aasist_conv_slots", 3))
    try:
        aasist_checks(mods, eng, sd, feats, "fp16")
        capped = _all_taps(eng, AAS_TAPS)
    finally:
        check(lib().afx_debug_set(b"aasist_conv_slots", 0))
    for n in AAS_TAPS:
        assert torch.equal(auto[n], capped[n]), f"tap {n} depends on the conv kernel's grid"


@pytest.mark.parametrize("B,T,dt", [(3, 200, "fp16"), (3, 200, "fp32"), (1, 6, "fp16"), (2, 10, "fp16"), (2, 17, "fp16"), (16, 199, "fp16"),
                                    (1, 573, "fp16"), (1, 1887, "fp16")])
def test_aasist_launches_edge_shapes(mods, B, T, dt):
    eng, sd = _aasist(mods, dt)
    aasist_checks(mods, eng, sd, _feats(B, T, B * 1000 + T), dt)


def test_aasist_documented_maximum(mods):
    """629 temporal nodes (T <= 1889) is what the graph kernel's LDS slab holds: T = 1889 scores, T = 1890 is refused by
    aasist_forward's own message before anything is launched."""
    from afx._lib import AfxError
    eng, sd = _aasist(mods, "fp16")
    assert bool(torch.isfinite(eng.head(_feats(1, 1889, 2889).cuda())).all())
    try:
        out = eng.head(_feats(1, 1890, 2890).cuda())
        assert bool(torch.isfinite(out).all())
    except AfxError as e:
        assert "clip too long for the graph kernels" in str(e), str(e)


# ---- taps change nothing; a stale workspace changes nothing ----------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_taps_do_not_change_the_forward(mods, dt):
    engine, synth, I, ST = mods
    sd = synth.model_state_dict("ConformerModel", n_layers=2, n_encoders=2)
    eng = engine.Engine("conformer", n_layers=2, dtype=dt, conf_blocks=2)
    eng.load_state_dict(sd)
    wave = synth.waveforms(3, 64600, batch_idx=11).cuda()
    off = eng.forward(wave).cpu()
    eng.enable_taps()
    on = eng.forward(wave).cpu()
    eng.enable_taps(False)
    assert torch.equal(on, off), f"[{dt}] taps moved the logits by {(on - off).abs().max().item():.3e}"
    eng, _ = _aasist(mods, dt)
    off = eng.forward(wave).cpu()
    eng.enable_taps()
    on = eng.forward(wave).cpu()
    eng.enable_taps(False)
    assert torch.equal(on, off), f"[{dt}] xlsr_aasist: taps moved the logits by {(on - off).abs().max().item():.3e}"


def _all_taps(eng, names):
    return {n: eng.tap(n).cpu() for n in names}


def _stale_vs_fresh(eng, run_other, run, names, fused):
    run_other()
    eng.enable_taps()
    stale_out = run().cpu()
    stale = _all_taps(eng, names)
    eng._ws = torch.zeros_like(eng._ws)
    fresh_out = run().cpu()
    fresh = _all_taps(eng, names)
    eng.enable_taps(False)
    assert torch.equal(stale_out, fresh_out), "logits depend on the workspace's earlier contents"
    for n in names:
        a, b = stale[n], fresh[n]
        if n.endswith(".u") and fused:  # (the fused path neither writes nor reads the pad columns of u)
            a, b = a.reshape(-1, 320)[:, :288], b.reshape(-1, 320)[:, :288]
        assert torch.equal(a, b), f"tap {n} depends on the workspace's earlier contents"


def test_stale_workspace_trunk_fp16(mods):
    engine, synth, I, ST = mods
    sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=2)
    eng = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=2)
    eng.load_state_dict(sd)
    other, wave = synth.waveforms(5, 72080, batch_idx=1).cuda(), synth.waveforms(3, 64600, batch_idx=2).cuda()
    names = [f"c{i}" for i in range(6)] + ["conv", "feats", "proj", "xpad", "pos", "l0.ln1", "l0.qkv", "l0.att", "l0.mid",
                                           "l0.ln2", "l0.ff", "layer0", "ssl", "tokens"] + \
            [f"b{b}.{t}" for b in range(2) for t in ("xa", "qkv", "ao", "xb", "glu", "u")] + ["block0", "block1"]
    _stale_vs_fresh(eng, lambda: eng.forward(other), lambda: eng.forward(wave), names, True)


def test_stale_workspace_head_fp16x3_unfused(mods):
    eng, sd = _head(mods, "fp16x3", 0)
    names = ["tokens"] + [f"b{b}.{t}" for b in range(2) for t in ("ff1.hc", "ff1.hid", "xa", "attn.hc", "qkv", "ao", "xb",
                                                                   "conv.hc", "glu", "u", "xc", "ff2.hc", "ff2.hid", "xd")] + \
            ["block0", "block1"]
    other, feats = _feats(5, 230, 3).cuda(), _feats(3, 124, 4).cuda()
    _stale_vs_fresh(eng, lambda: eng.head(other), lambda: eng.head(feats), names, False)


@pytest.mark.parametrize("dt", ["fp16", "fp32"])
def test_stale_workspace_aasist(mods, dt):
    eng, sd = _aasist(mods, dt)
    other, feats = _feats(5, 230, 5230).cuda(), _feats(3, 124, 3124).cuda()
    _stale_vs_fresh(eng, lambda: eng.head(other), lambda: eng.head(feats), AAS_TAPS, False)

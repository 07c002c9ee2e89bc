"""Per-launch parity inside real forwards on an MI355X: every tapped launch of the SSL trunk, of the Conformer head and
of the AASIST back-end against its fp64 reference (oracle/insitu.py) built from the launch's own tapped inputs, element by element within the
bounds stated there.  Large products are checked on a deterministic subset of rows (``check_rows``).  The module's
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


def gate(cls, dt, where, res, insitu, fails, op_dt=False):
    """Record one launch's result; a launch past its bound (or biased) is added to `fails` (every launch of the forward
    is checked before the test asserts, so one run names all of them)."""
    key = (cls, dt)
    r0, b0 = SUMMARY.get(key, (0.0, None))
    b = res["bias"] if op_dt else None
    SUMMARY[key] = (max(r0, res["ratio"]), b if b0 is None or (b is not None and abs(b) > abs(b0)) else b0)
    if not res["ratio"] <= 1.0:
        fails.append(f"{where} [{dt}]: |got - ref| = {res['ratio']:.2f} x bound at row {res['row']}, col {res['col']} "
                     f"(got {res['got']:.6e}, ref {res['ref']:.6e}, bound {res['bound']:.2e})")
    if op_dt and dt in insitu.HALF and cls not in insitu.BIAS_REPORTED and res["bias"] is not None and \
            abs(res["bias"]) > insitu.BIAS_MAX:
        fails.append(f"{where} [{dt}]: rounding bias {res['bias']:+.3f} ulp")


def trunk_checks(mods, eng, sd, wave, dt, mode="layer_norm", conv=True):
    """Run one taps-on forward of `eng` on `wave` and check every tapped launch of the trunk."""
    engine, synth, I, ST = mods
    B, L = wave.shape
    Ts = ST.conv_out_lengths(L)
    T = Ts[-1]
    eng.enable_taps()
    eng.ssl(wave.cuda())
    torch.cuda.synchronize()
    tap = lambda n: eng.tap(n).cpu().double()

    fails = []

    def g(cls, where, got, ref_bnd, op_dt, rows=None):
        gate(cls, dt, where, I.check(got, ref_bnd[0], ref_bnd[1], dt if op_dt else None, rows), I, fails, op_dt)

    C = 512
    if conv:
        prev = None
        for i in range(6):
            cur = tap(f"c{i}").reshape(B * Ts[i], C)
            rows = conv_rows(B, Ts[i])
            ref = I.conv0(sd, wave, rows, dt, mode) if i == 0 else I.conv_layer(sd, i, prev, B, rows, dt, mode)
            g("conv0" if i == 0 else "conv", f"c{i}", cur[rows], ref, True, rows)
            prev = cur
        rows = conv_rows(B, T)
        g("conv", "conv", tap("conv").reshape(B * T, C)[rows], I.conv_layer(sd, 6, prev, B, rows, dt, mode, out="f32"), False, rows)
    if mode != "layer_norm":
        eng.enable_taps(False)
        assert not fails, "\n".join(fails)
        return
    conv6 = tap("conv").reshape(B * T, C)
    g("layernorm", "feats", tap("feats").reshape(B * T, C),
      I.layernorm(conv6, sd["layer_norm.weight"], sd["layer_norm.bias"], dt), True)
    feats = tap("feats").reshape(B * T, C)
    rows = check_rows(B, T)
    D = 1024
    proj = tap("proj").reshape(B * T, D)
    g("product", "proj", proj[rows], I.product(feats[rows], sd["post_extract_proj.weight"], sd["post_extract_proj.bias"], dt), False)
    xpad = tap("xpad").reshape(B, T + 128, D)
    assert bool((xpad[:, :64] == 0).all()) and bool((xpad[:, 64 + T:] == 0).all()), f"xpad [{dt}]: nonzero pad rows"
    g("product", "xpad", xpad[:, 64:64 + T].reshape(B * T, D)[rows],
      I.product(feats[rows], sd["post_extract_proj.weight"], sd["post_extract_proj.bias"], dt, out="op"), True)
    x = tap("pos").reshape(B * T, D)
    g("posconv", "pos", x[rows], I.posconv(sd, xpad, proj, rows, T, dt), False)
    wqkv = lambda p, k: torch.cat([sd[p + f"self_attn.{n}_proj.{k}"] for n in "qkv"], 0)
    for l in range(ST.num_layers(sd)):
        p, n = f"encoder.layers.{l}.", f"l{l}."
        ln1 = tap(n + "ln1").reshape(B * T, D)
        g("layernorm", n + "ln1", ln1, I.layernorm(x, sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"], dt), True)
        qkv = tap(n + "qkv").reshape(B * T, 3 * D)
        g("product", n + "qkv", qkv[rows], I.product(ln1[rows], wqkv(p, "weight"), wqkv(p, "bias"), dt, out="op"), True)
        att = tap(n + "att").reshape(B * T, D)
        g("mhsa", n + "att", att[rows], I.mhsa(qkv, rows, T, dt), True)
        mid = tap(n + "mid").reshape(B * T, D)
        g("product", n + "mid", mid[rows], I.product(att[rows], sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"],
                                                      dt, resid=x[rows]), False)
        ln2 = tap(n + "ln2").reshape(B * T, D)
        g("layernorm", n + "ln2", ln2, I.layernorm(mid, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], dt), True)
        ff = tap(n + "ff").reshape(B * T, 4096)
        g("product", n + "ff", ff[rows], I.product(ln2[rows], sd[p + "fc1.weight"], sd[p + "fc1.bias"], dt, act="gelu", out="op"), True)
        x = tap(f"layer{l}").reshape(B * T, D)
        g("product", f"layer{l}", x[rows], I.product(ff[rows], sd[p + "fc2.weight"], sd[p + "fc2.bias"], dt, resid=mid[rows]), False)
    eng.enable_taps(False)
    assert not fails, "\n".join(fails)


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


def test_trunk_posconv_gemm_form(mods):
    eng, sd = _trunk(mods, 1, "fp16")
    eng.set("posconv_sliding", 0)
    trunk_checks(mods, eng, sd, mods[1].waveforms(4, 64000, batch_idx=5), "fp16", conv=False)


def test_trunk_group_norm_extractor(mods):
    eng, sd = _trunk(mods, 1, "fp16", mode="group_norm")
    trunk_checks(mods, eng, sd, mods[1].waveforms(2, 64000, batch_idx=6), "fp16", mode="group_norm")


# ---- Conformer head ------------------------------------------------------------------------------------------------------
def head_checks(mods, eng, sd, feats, dt, fused):
    engine, synth, I, ST = mods
    B, T, _ = feats.shape
    N, E = T + 1, 144
    M = B * N
    eng.enable_taps()
    eng.head(feats.cuda())
    torch.cuda.synchronize()
    tap = lambda n: eng.tap(n).cpu().double()

    fails = []

    def g(cls, where, got, ref_bnd, op_dt, rows=None):
        gate(cls, dt, where, I.check(got, ref_bnd[0], ref_bnd[1], dt if op_dt else None, rows), I, fails, op_dt)

    x = tap("tokens").reshape(M, E)
    Ep = eng.tap("b0.ao").numel() // M  # (operand rows padded to whole 64-column K-steps)
    rows = check_rows(B, N)
    for b in range(2):
        p, n = f"conformer.encoder_blocks.{b}.", f"b{b}."
        (xa_r, qkv_r) = I.chain_a(sd, p, x, dt)
        xa, qkv = tap(n + "xa").reshape(M, E), tap(n + "qkv").reshape(M, 3 * E)
        g("chain_a", n + "xa", xa, xa_r, False)
        g("chain_a", n + "qkv", qkv, qkv_r, False)
        ao = tap(n + "ao").reshape(M, Ep)
        if not bool((ao[:, E:] == 0).all()):
            fails.append(f"{n}ao [{dt}]: nonzero pad columns")
        g("shaw", n + "ao", ao[rows, :E], I.shaw(qkv, sd[p + "attn.fn.rel_pos_emb.weight"], rows, N, dt), True, rows)
        xb_r, glu_r = I.chain_b(sd, p, xa, ao[:, :E], dt)
        xb, glu = tap(n + "xb").reshape(M, E), tap(n + "glu").reshape(M, 576)
        g("chain_b", n + "xb", xb, xb_r, False)
        g("chain_b", n + "glu", glu, glu_r, False)
        u = tap(n + "u").reshape(M, -1)
        g("dwconv", n + "u", u[:, :288], I.glu_dwconv(sd, p, glu, B, N, dt), True)
        if not fused:  # (the fused chain C reads the 288 real columns of u only; the per-op product reads them all)
            if not bool((u[:, 288:] == 0).all()):
                fails.append(f"{n}u [{dt}]: nonzero pad columns")
            for h in ("ff1.hc", "attn.hc", "conv.hc", "ff2.hc", "ff1.hid", "ff2.hid"):
                t = tap(n + h).reshape(M, -1)
                k = E if h.endswith("hc") else 576
                if not bool((t[:, k:] == 0).all()):
                    fails.append(f"{n}{h} [{dt}]: nonzero pad columns")
        blk = tap(f"block{b}").reshape(M, E)
        g("chain_c", f"block{b}", blk, I.chain_c(sd, p, xb, u[:, :288], dt), False)
        x = blk
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


def aasist_checks(mods, eng, sd, feats, dt):
    """One taps-on forward of the back-end; every launch against its reference (oracle/insitu.py::aasist_walk)."""
    engine, synth, I, ST = mods
    eng.enable_taps()
    eng.head(feats.cuda())
    torch.cuda.synchronize()
    res, zeros = I.aasist_walk(sd, feats, lambda n: eng.tap(n).cpu().double(), dt != "fp32")
    eng.enable_taps(False)
    fails = []
    for cls, name, r in res:
        gate(cls, dt, name, r, I, fails)
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

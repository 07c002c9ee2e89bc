"""The AASIST back-end's in-place bounds (oracle/insitu.py, ``aasist_walk``) must catch what they claim, without a GPU.
A simulated CORRECT back-end -- a torch fp32 restatement of every launch in the engine's own buffer layouts, the split
form as hi / lo fp16 operands with fp32 accumulation -- passes every bound at every shape the GPU tests run, GraphPool's
near ties included (the smallest fp64 score gap per shape is printed), and each injected defect fails its launch's bound
by at least 10x (a nonzero border pixel: by the exact-zero count)."""
import pytest
import torch
import torch.nn.functional as F

from afx import synth
from oracle import insitu as I

SHAPES = [(2, 49), (3, 200), (1, 6), (2, 10), (2, 17), (16, 199), (1, 573), (1, 1887)]


@pytest.fixture(scope="module")
def sd():
    return synth.lively(synth.aasist_head_state_dict(), 1.5)


def feats_of(B, T):
    return torch.randn(B, T, 1024, generator=torch.Generator().manual_seed(B * 1000 + T))


# ---- the simulated kernels (fp32) ----------------------------------------------------------------------------------------
def sim_mm(a, w, split, cor=True, scale=1.0 / 2048):
    if not split:
        return a @ w.t()
    ah, wh = a.half().float(), w.half().float()
    al, wl = ((a - ah) * 2048).half().float(), ((w - wh) * 2048).half().float()
    acc = ah @ wh.t()
    return acc + (ah @ wl.t() + al @ wh.t()) * scale if cor else acc


def fold(sd, p):
    sc = sd[p + "weight"] / torch.sqrt(sd[p + "running_var"] + 1e-5)
    return sc, sd[p + "bias"] - sd[p + "running_mean"] * sc


def sim_epi(z, bias, resid=None, bn=None, post=0, valid=None, resid_after_bn=False):
    z = z + bias
    if resid is not None and not resid_after_bn:
        z = z + resid
    if post == 1:
        z = F.selu(z * bn[0] + bn[1])
    elif post == 2:
        z = F.selu(z) * bn[0] + bn[1]
    if resid is not None and resid_after_bn:
        z = z + resid
    return z * valid[:, None] if valid is not None else z


def sim_conv(image, w, bias, split, B, T, kh, a_off, hout, resid=None, bn=None, post=0, flip_taps=False, chunk_off=0, resid_after_bn=False, **kw):
    """-> the whole padded output image ((M + wp + 1), cout), fp32."""
    wd, wp, img = I.aas_dims(T)
    M, cin, cout = B * img, w.shape[1], w.shape[0]
    x = torch.cat([image.reshape(-1, cin), torch.zeros(3 * wp + 16, cin)])  # (the slack past the image: masked pixels only)
    m = torch.arange(M)
    idx = a_off + m[:, None, None] + (wp * torch.arange(kh) + chunk_off * (torch.arange(kh) > 0))[None, :, None] + torch.arange(3)[None, None, :]
    a = x[idx.reshape(M, -1)].reshape(M, -1)
    if flip_taps:
        w = w.flip(3)
    z = sim_mm(a, I.pack_conv(w), split, **kw)
    valid = I.aas_valid(m, T, hout).float()
    out = torch.zeros(M + wp + 1, cout)
    out[wp + 1:] = sim_epi(z, bias, None if resid is None else resid.reshape(-1, cout)[wp + 1:wp + 1 + M], bn, post, valid, resid_after_bn)
    return out


def sim_gat(sd, p, x, n1, temp, master=None, hetero=True, v12_everywhere=False, master_from_updated=False):
    B, N, _ = x.shape
    t1 = torch.arange(N) < n1
    if hetero:
        v11, v22, v12 = (sd[p + f"att_weight{k}"][:, 0] for k in ("11", "22", "12"))
    else:
        v11 = v22 = v12 = sd[p + "att_weight"][:, 0]
    same = t1[:, None] == t1[None, :]
    v = torch.where(same[:, :, None], torch.where(t1[:, None, None], v11[None, None], v22[None, None]), v12[None, None])
    if v12_everywhere:
        v = v12[None, None].expand(N, N, -1)
    y = []
    for i0 in range(0, N, 64):
        xi = x[:, i0:i0 + 64]
        h = torch.tanh(F.linear(xi[:, :, None] * x[:, None], sd[p + "att_proj.weight"], sd[p + "att_proj.bias"]))
        att = torch.softmax((h * v[i0:i0 + 64]).sum(-1) / temp, -1)
        y.append(F.linear(att @ x, sd[p + "proj_with_att.weight"], sd[p + "proj_with_att.bias"]) +
                 F.linear(xi, sd[p + "proj_without_att.weight"], sd[p + "proj_without_att.bias"]))
    sc, sh = fold(sd, p + "bn.")
    y = F.selu(torch.cat(y, 1) * sc + sh)
    if master is None:
        return y
    m = master.reshape(-1, 1, x.shape[2]).expand(B, 1, -1)
    xm = y if master_from_updated else x
    a = torch.tanh(F.linear(xm * m, sd[p + "att_projM.weight"], sd[p + "att_projM.bias"]))
    a = torch.softmax((a @ sd[p + "att_weightM"]) / temp, 1)  # (B, N, 1)
    mo = F.linear((a * xm).sum(1), sd[p + "proj_with_attM.weight"], sd[p + "proj_with_attM.bias"]) + \
        F.linear(m[:, 0], sd[p + "proj_without_attM.weight"], sd[p + "proj_without_attM.bias"])
    return y, mo


def sim_pool(sd, p, h, keep):
    s = torch.sigmoid(F.linear(h, sd[p + "proj.weight"], sd[p + "proj.bias"]))
    idx = torch.topk(s, keep, dim=1)[1]
    return torch.gather(h * s, 1, idx.expand(-1, -1, h.shape[2]))


def sim_readout(sd, a, b, plus_one=True):
    (t1, ta1, s1, _, m1, ma1), (t2, ta2, s2, sa2, m2, ma2) = a, b
    vt = torch.maximum(t1 + ta1, t2 + ta2)
    vs = torch.maximum(s1 + 1.0 if plus_one else s1, s2 + sa2)
    hid = torch.cat([vt.abs().amax(1), vt.mean(1), vs.abs().amax(1), vs.mean(1), torch.maximum(m1 + ma1, m2 + ma2)], 1)
    return hid, F.linear(hid, sd["out_layer.weight"], sd["out_layer.bias"])


def sim_forward(sd, feats, split):
    """Every tap of one forward, fp32, in the engine's layouts."""
    B, T, _ = feats.shape
    wd, wp, img = I.aas_dims(T)
    M = B * img
    t = {}
    ll = t["aa.ll"] = sim_mm(feats.reshape(B * T, 1024), sd["LL.weight"], split) + sd["LL.bias"]
    pooled = F.max_pool2d(ll.reshape(B, T, 128).transpose(1, 2)[:, None], (3, 3))[:, 0]
    sc, sh = fold(sd, "first_bn.")
    x1 = torch.zeros(M + 3 * wp + 16)
    x1[:M].reshape(B, I.AAS_HP, wp)[:, 1:I.AAS_F + 1, 1:wd + 1] = F.selu(pooled * sc + sh)
    t["aa.x1"] = x1
    p = "encoder.0.0."
    Y = t["aa.b0.y"] = sim_conv(x1, sd[p + "conv1.weight"], sd[p + "conv1.bias"], False, B, T, 2, 0, I.AAS_F + 1, bn=fold(sd, p + "bn2."), post=1)
    D = t["aa.b0.d"] = sim_conv(x1, sd[p + "conv_downsample.weight"], sd[p + "conv_downsample.bias"], False, B, T, 1, wp, I.AAS_F)
    X = t["aa.b0"] = sim_conv(Y, sd[p + "conv2.weight"], sd[p + "conv2.bias"], split, B, T, 2, wp, I.AAS_F, resid=D)
    for i in range(1, 6):
        p, (cin, cout) = f"encoder.{i}.0.", I.AAS_FILT[i]
        Y = t[f"aa.b{i}.y"] = sim_conv(X, sd[p + "conv1.weight"], sd[p + "conv1.bias"], split, B, T, 2, 0, I.AAS_F + 1, bn=fold(sd, p + "bn2."), post=1)
        resid = X
        if cin != cout:
            resid = t[f"aa.b{i}.d"] = sim_conv(X, sd[p + "conv_downsample.weight"], sd[p + "conv_downsample.bias"], split, B, T, 1, wp, I.AAS_F)
        last = dict(bn=fold(sd, "first_bn1."), post=1) if i == 5 else {}
        X = t[f"aa.b{i}"] = sim_conv(Y, sd[p + "conv2.weight"], sd[p + "conv2.bias"], split, B, T, 2, wp, I.AAS_F, resid=resid, **last)
    w1 = t["aa.w1"] = sim_epi(sim_mm(X[:M], sd["attention.0.weight"][:, :, 0, 0], split), sd["attention.0.bias"], bn=fold(sd, "attention.2."), post=2)
    w2 = t["aa.w2"] = sim_epi(sim_mm(w1, sd["attention.3.weight"][:, :, 0, 0], split), sd["attention.3.bias"])
    v = lambda u: u[:M].reshape(B, I.AAS_HP, wp, 64)[:, 1:I.AAS_F + 1, 1:wd + 1]
    xv, wv = v(X), v(w2)
    eS = t["e_S"] = (xv * torch.softmax(wv, 2)).sum(2) + sd["pos_S"]
    eT = t["e_T"] = (xv * torch.softmax(wv, 1)).sum(1)
    gS = t["gat_S"] = sim_gat(sd, "GAT_layer_S.", eS, I.AAS_F, 2.0, hetero=False)
    gT = t["gat_T"] = sim_gat(sd, "GAT_layer_T.", eT, wd, 2.0, hetero=False)
    nS, nT = I.AAS_F // 2, max(wd // 2, 1)
    nS1, nT1 = max(nS // 2, 1), max(nT // 2, 1)
    oS, oT = sim_pool(sd, "pool_S.", gS, nS), sim_pool(sd, "pool_T.", gT, nT)
    t["out_S"], t["out_T"] = oS, oT
    br = []
    for k in (1, 2):
        h1, h2, n = f"HtrgGAT_layer_ST{k}1.", f"HtrgGAT_layer_ST{k}2.", f"b{k}_"
        xp = t[n + "xp"] = torch.cat([F.linear(oT, sd[h1 + "proj_type1.weight"], sd[h1 + "proj_type1.bias"]),
                                      F.linear(oS, sd[h1 + "proj_type2.weight"], sd[h1 + "proj_type2.bias"])], 1)
        y, m1 = sim_gat(sd, h1, xp, nT, 100.0, master=sd[f"master{k}"])
        T1, S1 = y[:, :nT], y[:, nT:]
        t[n + "T1"], t[n + "S1"], t[n + "m1"] = T1, S1, m1
        S1p, T1p = sim_pool(sd, f"pool_hS{k}.", S1, nS1), sim_pool(sd, f"pool_hT{k}.", T1, nT1)
        t[n + "S1p"], t[n + "T1p"] = S1p, T1p
        xp2 = t[n + "xp2"] = torch.cat([F.linear(T1p, sd[h2 + "proj_type1.weight"], sd[h2 + "proj_type1.bias"]),
                                        F.linear(S1p, sd[h2 + "proj_type2.weight"], sd[h2 + "proj_type2.bias"])], 1)
        y, ma = sim_gat(sd, h2, xp2, nT1, 100.0, master=m1)
        t[n + "Ta"], t[n + "Sa"], t[n + "ma"] = y[:, :nT1], y[:, nT1:], ma
        br.append((T1p, y[:, :nT1], S1p, y[:, nT1:], m1, ma))
    t["hidden"], t["logits"] = sim_readout(sd, br[0], br[1])
    return {k: v.contiguous() for k, v in t.items()}, br


def walk(sd, feats, taps, split):
    res, zeros = I.aasist_walk(sd, feats, lambda n: taps[n].double().reshape(-1), split)
    return {name: r for _, name, r in res}, dict(zeros), res


# ---- a correct back-end passes everywhere --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,split", [(B, T, True) for B, T in SHAPES] + [(2, 49, False), (3, 200, False)])
def test_correct_backend_passes_every_bound(sd, B, T, split):
    feats = feats_of(B, T)
    taps, _ = sim_forward(sd, feats, split)
    by, zeros, res = walk(sd, feats, taps, split)
    worst = {}
    for cls, name, r in res:
        worst[cls] = max(worst.get(cls, 0.0), r["ratio"])
    margin = min(r["margin"] for cls, _, r in res if cls == "pool")
    print(f"\n({B}, {T}) split={split}: smallest fp64 pool margin {margin:.3e}; worst ratios " +
          ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    bad = [f"{name}: {r['ratio']:.2f} x bound at row {r['row']}, col {r['col']}" for _, name, r in res if not r["ratio"] <= 1.0]
    assert not bad, "\n".join(bad)
    assert not any(zeros.values()), zeros
    assert sum(1 for cls, _, _ in res if cls == "pool") == 6  # (no pool is left out)


# ---- injected defects: each fails its launch's bound by >= 10x ------------------------------------------------------------
DB, DT_ = 2, 49  # (M = 1 656 virtual pixels = 25.9 tiles of 64: the last tile is partial)


@pytest.fixture(scope="module")
def good(sd):
    feats = feats_of(DB, DT_)
    taps, br = sim_forward(sd, feats, True)
    return feats, taps, br


def ratio_with(sd, good, name, value, where=None):
    """The walk's result for launch `where` (default: `name`) with tap `name` replaced by `value`."""
    feats, taps, _ = good
    t = dict(taps)
    t[name] = value.contiguous()
    by, zeros, _ = walk(sd, feats, t, True)
    return by[where or name], zeros


def conv2_of(sd, taps, i, **kw):
    p = f"encoder.{i}.0."
    last = dict(bn=fold(sd, "first_bn1."), post=1) if i == 5 else {}
    last.update(kw)
    return sim_conv(taps[f"aa.b{i}.y"], sd[p + "conv2.weight"], sd[p + "conv2.bias"], True, DB, DT_, 2, I.aas_dims(DT_)[1], I.AAS_F,
                    resid=taps[f"aa.b{i - 1}"], **last)


def test_the_undisturbed_launches_pass(sd, good):
    assert ratio_with(sd, good, "aa.b3", conv2_of(sd, good[1], 3))[0]["ratio"] <= 1.0
    assert ratio_with(sd, good, "aa.b5", conv2_of(sd, good[1], 5))[0]["ratio"] <= 1.0


def test_dropped_correction_term_fails(sd, good):  # plain fp16 weights and activations
    w1 = sim_epi(sim_mm(good[1]["aa.b5"][:DB * I.aas_dims(DT_)[2]], sd["attention.0.weight"][:, :, 0, 0], True, cor=False),
                 sd["attention.0.bias"], bn=fold(sd, "attention.2."), post=2)
    assert ratio_with(sd, good, "aa.w1", w1)[0]["ratio"] >= 10
    assert ratio_with(sd, good, "aa.b3", conv2_of(sd, good[1], 3, cor=False))[0]["ratio"] >= 10


def test_missing_low_half_scale_fails(sd, good):
    assert ratio_with(sd, good, "aa.b3", conv2_of(sd, good[1], 3, scale=1.0))[0]["ratio"] >= 10


def test_conv_taps_in_the_wrong_order_fail(sd, good):
    assert ratio_with(sd, good, "aa.b3", conv2_of(sd, good[1], 3, flip_taps=True))[0]["ratio"] >= 10


def test_second_chunk_one_image_row_off_fails(sd, good):
    assert ratio_with(sd, good, "aa.b3", conv2_of(sd, good[1], 3, chunk_off=I.aas_dims(DT_)[1]))[0]["ratio"] >= 10


def test_nonzero_border_pixel_is_counted(sd, good):
    wd, wp, img = I.aas_dims(DT_)
    for row in (0, wp, wp + 1 + wd, wp + 1 + img - 1, wp + 1 + DB * img - 1):  # head, head's last pixel, a pad column, slack rows
        x = good[1]["aa.b3"].clone()
        assert bool((x[row] == 0).all())
        x[row, 5] = 1e-30
        assert ratio_with(sd, good, "aa.b3", x)[1]["aa.b3"] == 1


def test_stale_row_in_the_last_partial_tile_fails(sd, good):
    wd, wp, img = I.aas_dims(DT_)
    M = DB * img
    assert M % 64
    x = good[1]["aa.b3"].clone()
    x[wp + 1 + M - 1] = good[1]["aa.b3"][wp + 1 + 5 * wp + 3]  # (what an earlier, larger forward left there)
    r, zeros = ratio_with(sd, good, "aa.b3", x)
    assert r["ratio"] >= 10 and r["row"] == M - 1 and zeros["aa.b3"] > 0


def test_swapped_post_ops_fail(sd, good):
    assert ratio_with(sd, good, "aa.b5", conv2_of(sd, good[1], 5, post=2))[0]["ratio"] >= 10
    w1 = sim_epi(sim_mm(good[1]["aa.b5"][:DB * I.aas_dims(DT_)[2]], sd["attention.0.weight"][:, :, 0, 0], True),
                 sd["attention.0.bias"], bn=fold(sd, "attention.2."), post=1)
    assert ratio_with(sd, good, "aa.w1", w1)[0]["ratio"] >= 10


def test_residual_after_bn_fails(sd, good):
    assert ratio_with(sd, good, "aa.b5", conv2_of(sd, good[1], 5, resid_after_bn=True))[0]["ratio"] >= 10


def test_cross_type_vector_in_a_same_type_block_fails(sd, good):
    nT = I.aas_dims(DT_)[0] // 2
    y, _ = sim_gat(sd, "HtrgGAT_layer_ST11.", good[1]["b1_xp"], nT, 100.0, master=sd["master1"], v12_everywhere=True)
    assert ratio_with(sd, good, "b1_T1", y[:, :nT])[0]["ratio"] >= 10
    assert ratio_with(sd, good, "b1_S1", y[:, nT:])[0]["ratio"] >= 10


def test_master_from_updated_nodes_fails(sd, good):
    nT1 = I.aas_dims(DT_)[0] // 4
    _, ma = sim_gat(sd, "HtrgGAT_layer_ST12.", good[1]["b1_xp2"], nT1, 100.0, master=good[1]["b1_m1"], master_from_updated=True)
    assert ratio_with(sd, good, "b1_ma", ma)[0]["ratio"] >= 10


def _scores(sd, p, h):
    return torch.sigmoid(F.linear(h.double(), sd[p + "proj.weight"].double(), sd[p + "proj.bias"].double()))[..., 0]


def test_two_kept_nodes_swapped_fail(sd, good):
    out = good[1]["out_T"].clone()  # (B, 8, 64) in descending score order: rows 0 and 7 are far more than delta apart
    out[1, [0, -1]] = out[1, [-1, 0]]
    assert ratio_with(sd, good, "out_T", out)[0]["ratio"] >= 10


def test_kept_node_replaced_by_the_best_dropped_one_fails(sd, good):
    h = good[1]["gat_T"]
    s = _scores(sd, "pool_T.", h)
    keep = h.shape[1] // 2
    order = s[0].argsort(descending=True)
    out = good[1]["out_T"].clone()
    out[0, 0] = h[0, order[keep]] * s[0, order[keep]].float()  # the top node gives way to the best dropped one
    assert ratio_with(sd, good, "out_T", out)[0]["ratio"] >= 10


def test_readout_without_the_plus_one_fails(sd, good):
    hid, logits = sim_readout(sd, good[2][0], good[2][1], plus_one=False)
    assert ratio_with(sd, good, "hidden", hid)[0]["ratio"] >= 10
    feats, taps, _ = good
    t = dict(taps, hidden=hid, logits=logits)  # (the logits follow the stored hidden vector: only `hidden` names the defect)
    by, _, _ = walk(sd, feats, t, True)
    assert by["hidden"]["ratio"] >= 10 and by["logits"]["ratio"] <= 1.0


def test_one_node_graph_has_an_infinite_margin(sd):
    from oracle import aasist as oa
    taps = {}
    oa.graph_pool(sd, "pool_hT1.", torch.randn(2, 1, 32, generator=torch.Generator().manual_seed(1)), 0.5, taps)
    assert bool(torch.isinf(taps["pool_margin"]["pool_hT1."]).all())
    assert torch.isfinite(oa.aasist_backend(sd, feats_of(1, 6), {})).all()

"""The in-place bounds (oracle/insitu.py) must catch what they claim, without a GPU: a simulated CORRECT kernel (fp32
accumulation on the rounded operands, round-to-nearest outputs) passes every bound, and each injected defect fails its
bound by at least 10x (the pad and rounding-bias checks: by their own measure)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import insitu as I

DT = "fp16"
G = torch.Generator().manual_seed(5)


def rnd(*shape, scale=1.0):
    return torch.randn(*shape, generator=G, dtype=torch.float64) * scale


def op16(x):
    return I.op(x, DT)


def ratio(got, rb, rows=None):
    return I.check(got, rb[0], rb[1], DT, rows)


def sim_product(a, w, b):
    """Correct kernel: fp32 accumulation of the fp16 operands, fp32 bias, round-to-nearest fp16 out."""
    return (a.float() @ op16(w).float().t() + b.float()).double()


@pytest.fixture(scope="module")
def prod():
    M, N, K = 64, 64, 256
    a, w, b = op16(rnd(M, K)), rnd(N, K, scale=1 / math.sqrt(K)), rnd(N, scale=0.1)
    return a, w, b, I.product(a, w, b, DT, out="op"), sim_product(a, w, b)


def test_correct_product_passes(prod):
    a, w, b, rb, z = prod
    r = ratio(op16(z), rb)
    assert r["ratio"] <= 1.0 and abs(r["bias"]) <= I.BIAS_MAX, r


def test_missing_k_step_in_one_tile_fails(prod):
    a, w, b, rb, z = prod
    bad = z.clone()
    bad[16:32, 32:48] -= (a[16:32, 32:64].float() @ op16(w)[32:48, 32:64].float().t()).double()
    assert ratio(op16(bad), rb)["ratio"] >= 10


def test_swapped_rows_in_a_tile_fail(prod):
    a, w, b, rb, z = prod
    bad = z.clone()
    bad[[3, 7]] = bad[[7, 3]]
    assert ratio(op16(bad), rb)["ratio"] >= 10


def test_stale_last_row_fails(prod):
    a, w, b, rb, z = prod
    bad = z.clone()
    bad[-1] = sim_product(op16(rnd(1, a.shape[1])), w, b)[0]  # (what an earlier forward left there)
    r = ratio(op16(bad), rb)
    assert r["ratio"] >= 10 and r["row"] == a.shape[0] - 1


def test_round_toward_zero_fails_the_bias_check(prod):
    a, w, b, rb, z = prod
    t = z.float().half()
    over = t.float().abs() > z.float().abs()
    bits = t.view(torch.int16).clone()
    bits[over] -= 1  # one step toward zero where nearest rounding went away from it
    r = ratio(bits.view(torch.float16).double(), rb)
    assert r["ratio"] <= 1.0  # (every element is still within its bound: only the bias statistic sees it)
    assert r["bias"] <= -10 * I.BIAS_MAX, r


def test_nonzero_pad_column_is_seen():
    t = torch.zeros(8, 192, dtype=torch.float64)
    t[:, :144] = rnd(8, 144)
    assert bool((t[:, 144:] == 0).all())
    t[5, 150] = 2.0 ** -24
    assert not bool((t[:, 144:] == 0).all())


# ---- posconv --------------------------------------------------------------------------------------------------------------
def _pos_sd(D=128, K=128, groups=2):
    v = rnd(D, D // groups, K, scale=math.sqrt(4.0 / (K * D)))
    g = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1 + 0.1 * rnd(1, 1, K))
    return {"encoder.pos_conv.0.weight_v": v.float(), "encoder.pos_conv.0.weight_g": g.float(),
            "encoder.pos_conv.0.bias": rnd(D, scale=0.1).float()}


def sim_posconv(sd, xpad, x, T, groups, shift_group=None):
    w = op16(I.pos_weight({k: v.float() for k, v in sd.items()}).float()).float()
    B = xpad.shape[0]
    xp = xpad.float().transpose(1, 2)  # (B, D, T + 128)
    if shift_group is not None:  # one 64-channel group's window one frame late
        cpg = xp.shape[1] // groups
        xp = xp.clone()
        xp[:, shift_group * cpg:(shift_group + 1) * cpg, :-1] = xp[:, shift_group * cpg:(shift_group + 1) * cpg, 1:].clone()
    z = F.conv1d(xp, w, sd["encoder.pos_conv.0.bias"].float(), groups=groups)[:, :, :T]
    return (x.float() + F.gelu(z.transpose(1, 2).reshape(B * T, -1))).double()


def test_posconv_correct_and_window_off_by_one():
    D, groups, B, T = 128, 2, 2, 40
    sd = _pos_sd(D, groups=groups)
    x = rnd(B * T, D)
    xpad = torch.zeros(B, T + 128, D, dtype=torch.float64)
    xpad[:, 64:64 + T] = op16(x).reshape(B, T, D)
    rows = torch.arange(B * T)
    rb = I.posconv(sd, xpad, x, rows, T, DT, groups=groups)
    assert ratio(sim_posconv(sd, xpad, x, T, groups), rb)["ratio"] <= 1.0
    assert ratio(sim_posconv(sd, xpad, x, T, groups, shift_group=1), rb)["ratio"] >= 10


# ---- attention ------------------------------------------------------------------------------------------------------------
def sim_attention(q, k, v, bias=None, drop=None):
    """q (R, H, dh) scaled, k / v (R, keys, H, dh) operand values: fp32 logits, P rounded to fp16 before P.v."""
    s = torch.einsum("rhd,rthd->rht", q.float(), k.float())
    if bias is not None:
        s = s + bias.float()
    if drop is not None:
        s[..., drop] = -float("inf")
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = torch.einsum("rht,rthd->rhd", p.half().float(), v.float()) / p.sum(-1, keepdim=True)
    return o.reshape(o.shape[0], -1).double()


def test_mhsa_correct_and_dropped_key_past_a_128_block():
    B, T, H, dh = 2, 200, 2, 64
    qkv = op16(rnd(B * T, 3 * H * dh))
    rows = torch.arange(B * T)
    rb = I.mhsa(qkv, rows, T, DT, heads=H)
    x = qkv.reshape(B, T, 3, H, dh)
    q, k, v = x[rows // T, rows % T, 0] * dh ** -0.5, x[rows // T, :, 1], x[rows // T, :, 2]
    assert ratio(sim_attention(q, k, v), rb)["ratio"] <= 1.0
    assert ratio(sim_attention(q, k, v, drop=130), rb)["ratio"] >= 10


def test_shaw_correct_and_distance_clamp_at_511():
    B, N, H, dh = 1, 600, 4, 36
    qkv = rnd(B * N, 3 * H * dh)
    rel = rnd(2 * I.MAX_POS + 1, dh)
    rows = torch.arange(B * N)
    rb = I.shaw(qkv, rel, rows, N, DT, heads=H)
    x = qkv.reshape(B, N, 3, H, dh)
    q = op16((x[0, :, 0].float() * torch.tensor(1 / math.sqrt(dh), dtype=torch.float32)).double())
    k, v = op16(x[0, :, 1])[None].expand(N, -1, -1, -1), op16(x[0, :, 2])[None].expand(N, -1, -1, -1)

    def bias(clamp):
        dist = (torch.arange(N)[:, None] - torch.arange(N)[None, :]).clamp(-clamp, clamp) + I.MAX_POS
        return torch.einsum("rhd,rtd->rht", q.float(), op16(rel)[dist].float()).double()

    assert ratio(sim_attention(q, k, v, bias(I.MAX_POS)), rb)["ratio"] <= 1.0
    assert ratio(sim_attention(q, k, v, bias(I.MAX_POS - 1)), rb)["ratio"] >= 10


# ---- GLU + depthwise conv + BatchNorm + swish -----------------------------------------------------------------------------
def test_dwconv_correct_and_halo_off_by_one_at_a_chunk_edge():
    B, N, C2, k = 1, 1100, 16, 31
    p = "blk."
    sd = {p + "conv.net.4.conv.weight": rnd(C2, 1, k, scale=0.2).float(), p + "conv.net.4.conv.bias": rnd(C2, scale=0.1).float(),
          p + "conv.net.5.running_mean": rnd(C2, scale=0.1).float(), p + "conv.net.5.running_var": (1 + rnd(C2).abs()).float(),
          p + "conv.net.5.weight": (1 + 0.1 * rnd(C2)).float(), p + "conv.net.5.bias": rnd(C2, scale=0.1).float()}
    glu = rnd(B * N, 2 * C2).float().double()
    rb = I.glu_dwconv(sd, p, glu, B, N, DT)

    def sim(edge_shift):
        a, g = glu.float().reshape(B, N, -1).chunk(2, dim=-1)
        h = (a * torch.sigmoid(g)).transpose(1, 2)
        if edge_shift:  # the rows past 1024 seen one row late by the last outputs of the first chunk
            h = torch.cat([h[..., :1024], h[..., 1025:], torch.zeros_like(h[..., :1])], -1)
        z = F.conv1d(F.pad(h, (k // 2, k // 2)), sd[p + "conv.net.4.conv.weight"], sd[p + "conv.net.4.conv.bias"], groups=C2)
        sc = sd[p + "conv.net.5.weight"] / torch.sqrt(sd[p + "conv.net.5.running_var"] + 1e-5)
        sh = sd[p + "conv.net.5.bias"] - sd[p + "conv.net.5.running_mean"] * sc
        y = F.silu(z * sc[None, :, None] + sh[None, :, None]).transpose(1, 2).reshape(B * N, -1)
        return y.double()

    good = sim(False)
    assert ratio(op16(good), rb)["ratio"] <= 1.0
    bad = good.clone()
    bad[1024 - k // 2:1024] = sim(True)[1024 - k // 2:1024]
    assert ratio(op16(bad), rb)["ratio"] >= 10

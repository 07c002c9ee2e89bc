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


# ---- key-padding masks, the key-blocked form, the two ends of a forward -----------------------------------------------------
# Adversarial inputs, stated here and asserted on the reference alone (test_masked_inputs_are_adversarial): B = 2 utterances
# of T = 300 rows, lens = (300, 173), two heads; q, k, v = fp16(randn) (logit spread ~1), and per head h and utterance b one
# planted query row PLANT[b] whose dominating key k = 12 q / |q| (logit ~12: max P > 0.9) sits at the LAST valid key -- key
# 299 of utterance 0 (the third 128-key block), key 172 of utterance 1 (its last block, and the key before the first masked
# one); row FLAT[b] has q = 2^-10 randn: logits ~0, a near-uniform P.  The rows past lens[1] hold ordinary finite data
# (what a zero-padded clip leaves there), so a mask that lets one of them in moves the output.
MB, MT, MH, MDH = 2, 300, 2, 64
MLENS = (300, 173)
PLANT, FLAT = (40, 100), (41, 101)


@pytest.fixture(scope="module")
def masked():
    x = rnd(MB, MT, 3, MH, MDH)
    for b in range(MB):
        for h in range(MH):
            q = x[b, PLANT[b], 0, h]
            x[b, MLENS[b] - 1, 1, h] = 12.0 * q / q.norm()
        x[b, FLAT[b], 0] *= 2.0 ** -10
    qkv = op16(x.reshape(MB * MT, 3 * MH * MDH))
    rows = I.valid_rows(MLENS, MT)
    return qkv, rows, I.mhsa(qkv, rows, MT, DT, heads=MH, lens=MLENS)


def _masked_parts(qkv, rows):
    x = qkv.reshape(MB, MT, 3, MH, MDH)
    b_i, t_i = rows // MT, rows % MT
    return x[b_i, t_i, 0] * MDH ** -0.5, x[b_i, :, 1], x[b_i, :, 2], b_i


def sim_masked(qkv, rows, lens_of_row, live=None, stale_v=None):
    """One-pass kernel under a key-padding mask: keys >= lens_of_row[r] staged as zeros and masked (P exactly 0); fp32
    logits, P rounded to fp16 before P.v.  live (R,) key index or -1: that one masked key is staged from memory
    (k as stored, v = stale_v) and takes part -- the staging and the mask share one predicate."""
    q, k, v, _ = _masked_parts(qkv, rows)
    dead = torch.arange(MT)[None, :] >= lens_of_row[:, None]
    if live is not None:
        hit = torch.arange(MT)[None, :] == live[:, None]
        dead = dead & ~hit
        if stale_v is not None:
            v = torch.where(hit[:, :, None, None], torch.full_like(v, stale_v), v)
    s = torch.einsum("rhd,rthd->rht", q.float(), k.float()).masked_fill(dead[:, None, :], -float("inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = torch.einsum("rht,rthd->rhd", p.half().float(), v.float()) / p.sum(-1, keepdim=True)
    return o.reshape(o.shape[0], -1).double()


def sim_blocked(qkv, rows, lens_of_row, no_rescale=False, sum_before_rescale=False, block=128):
    """The key-blocked form: running maximum m, running sum l and accumulator acc over 128-key blocks,
    acc = acc alpha + fp16(P) v and l = l alpha + sum P with alpha = exp(m_old - m_new), out = acc / l."""
    q, k, v, _ = _masked_parts(qkv, rows)
    q, k, v = q.float(), k.float(), v.float()
    R = q.shape[0]
    m = torch.full((R, MH), -float("inf"))
    l = torch.zeros(R, MH)
    acc = torch.zeros(R, MH, MDH)
    for k0 in range(0, MT, block):
        keys = torch.arange(k0, min(k0 + block, MT))
        dead = keys[None, :] >= lens_of_row[:, None]
        s = torch.einsum("rhd,rthd->rht", q, k[:, keys]).masked_fill(dead[:, None, :], -float("inf"))
        m_new = torch.maximum(m, s.amax(-1))
        m_new = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)  # (a block of masked keys only)
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new[..., None])
        pv = torch.einsum("rht,rthd->rhd", p.half().float(), v[:, keys])
        acc = (acc if no_rescale else acc * alpha[..., None]) + pv
        l = (l + p.sum(-1)) * alpha if sum_before_rescale else l * alpha + p.sum(-1)
        m = m_new
    return (acc / l[..., None]).reshape(R, -1).double()


def test_masked_inputs_are_adversarial(masked):
    """On the reference alone: per head a row whose largest logit lies in the LAST key block, a row with max P > 0.9, a
    row with a near-uniform P (max P within 1 % of 1 / keys)."""
    qkv, rows, _ = masked
    q, k, _, b_i = _masked_parts(qkv, rows)
    n = torch.tensor(MLENS)[b_i]
    s = torch.einsum("rhd,rthd->rht", q, k).masked_fill((torch.arange(MT)[None, :] >= n[:, None])[:, None, :], -float("inf"))
    p = torch.softmax(s, -1)
    for h in range(MH):
        last_block = (s[:, h].argmax(-1) >= ((n - 1) // 128) * 128) & (n > 128)
        assert bool(last_block[b_i == 0].any()) and bool(last_block[b_i == 1].any())
        assert int((p[:, h].amax(-1) > 0.9).sum()) >= 2
        assert bool((p[:, h].amax(-1) * n < 1.01).any())
    for b in range(MB):
        r = int((rows == b * MT + PLANT[b]).nonzero())
        assert bool((p[r].amax(-1) > 0.9).all()) and bool((s[r].argmax(-1) == MLENS[b] - 1).all())


def test_masked_mhsa_correct_kernel_passes_one_pass_and_blocked(masked):
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[rows // MT]
    for got in (sim_masked(qkv, rows, n), sim_blocked(qkv, rows, n)):
        r = ratio(op16(got), rb, rows)
        assert r["ratio"] <= 1.0 and abs(r["bias"]) <= I.BIAS_MAX, r


def test_masked_mhsa_without_lens_is_the_unmasked_reference():
    qkv = op16(rnd(2 * 40, 3 * MH * MDH))
    rows = torch.arange(80)
    a, b = I.mhsa(qkv, rows, 40, DT, heads=MH), I.mhsa(qkv, rows, 40, DT, heads=MH, lens=(40, 40))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_mask_off_by_one_fails(masked):
    """Key lens[b] is included (utterance 1: the row after its last frame, ordinary data)."""
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[rows // MT]
    r = ratio(op16(sim_masked(qkv, rows, torch.clamp(n + 1, max=MT))), rb, rows)
    assert r["ratio"] >= 10 and r["row"] // MT == 1, r


def test_mask_from_the_neighbouring_utterance_fails(masked):
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[1 - rows // MT]
    assert ratio(op16(sim_masked(qkv, rows, n)), rb, rows)["ratio"] >= 10


def test_masked_key_staged_from_stale_memory_fails(masked):
    """The first masked key of utterance 1 is staged from memory instead of zero, and what lies there has a large v."""
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[rows // MT]
    live = torch.where(rows // MT == 1, torch.tensor(MLENS[1]), torch.tensor(-1))
    assert ratio(op16(sim_masked(qkv, rows, n, live=live, stale_v=1000.0)), rb, rows)["ratio"] >= 10


def test_blocked_form_without_the_rescale_fails(masked):
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[rows // MT]
    assert ratio(op16(sim_blocked(qkv, rows, n, no_rescale=True)), rb, rows)["ratio"] >= 10


def test_blocked_form_sum_added_before_the_rescale_fails(masked):
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[rows // MT]
    assert ratio(op16(sim_blocked(qkv, rows, n, sum_before_rescale=True)), rb, rows)["ratio"] >= 10


def test_masked_rows_helper():
    """Valid rows only; the last valid row of every utterance; every valid row whose frame index mod 16 is 0 or 15 (so
    mod 64: 0, 15, 63); every row of the first and the last utterance."""
    lens, T = (225, 1, 129, 64, 17), 225
    r = I.masked_rows(lens, T)
    b, t = r // T, r % T
    assert bool((t < torch.tensor(lens)[b]).all()) and len(set(r.tolist())) == len(r)
    have = set(r.tolist())
    for u, n in enumerate(lens):
        assert u * T + n - 1 in have
        for f in range(n):
            if f % 16 in (0, 15) or f % 64 in (0, 15, 63) or u in (0, len(lens) - 1):
                assert u * T + f in have
    assert len(r) < sum(lens)
    assert I.valid_rows(lens, T).tolist() == [u * T + f for u, n in enumerate(lens) for f in range(n)]


def test_masked_shaw_and_dwconv_ignore_the_rows_past_a_clip():
    """The masked references select: NaN in the rows past a clip's tokens changes nothing, and a clip's rows equal the
    clip's own unmasked reference."""
    B, N, H, dh, frames = 2, 50, 4, 36, (49, 20)
    qkv = rnd(B * N, 3 * H * dh)
    rel = rnd(2 * I.MAX_POS + 1, dh)
    poisoned = qkv.clone()
    poisoned.reshape(B, N, -1)[1, frames[1] + 1:] = float("nan")
    rows = I.valid_rows([f + 1 for f in frames], N)
    a = I.shaw(poisoned, rel, rows, N, DT, heads=H, lens=frames)
    alone = I.shaw(qkv.reshape(B, N, -1)[1, :frames[1] + 1].reshape(-1, 3 * H * dh), rel, torch.arange(frames[1] + 1), frames[1] + 1, DT, heads=H)
    assert bool(torch.isfinite(a[0]).all()) and (a[0][N:] - alone[0]).abs().max() < 1e-12 and (a[1][N:] - alone[1]).abs().max() < 1e-12
    C2, k, p = 16, 31, "blk."
    sd = {p + "conv.net.4.conv.weight": rnd(C2, 1, k, scale=0.2).float(), p + "conv.net.4.conv.bias": rnd(C2, scale=0.1).float(),
          p + "conv.net.5.running_mean": rnd(C2, scale=0.1).float(), p + "conv.net.5.running_var": (1 + rnd(C2).abs()).float(),
          p + "conv.net.5.weight": (1 + 0.1 * rnd(C2)).float(), p + "conv.net.5.bias": rnd(C2, scale=0.1).float()}
    glu = rnd(B * N, 2 * C2)
    bad = glu.clone()
    bad.reshape(B, N, -1)[1, frames[1] + 1:] = float("nan")
    y, e = I.glu_dwconv(sd, p, bad, B, N, DT, lens=frames)
    ya, ea = I.glu_dwconv(sd, p, glu.reshape(B, N, -1)[1, :frames[1] + 1].reshape(-1, 2 * C2), 1, frames[1] + 1, DT)
    own = y.reshape(B, N, -1)[1, :frames[1] + 1]
    assert bool(torch.isfinite(own).all()) and (own - ya.reshape(own.shape)).abs().max() < 1e-12
    z = torch.zeros(B, N + 128, 8, dtype=torch.float64)
    with pytest.raises(AssertionError, match="nonzero rows past"):
        z[1, 64 + 20] = 1.0
        I.posconv(_pos_sd(8, groups=1), z, rnd(B * N, 8), torch.arange(4), N, DT, groups=1, lens=(50, 20))


# ---- final LayerNorm (two outputs), tokens, logits ---------------------------------------------------------------------------
def test_final_layernorm_correct_and_operand_copy_of_the_unnormalised_row():
    M, D = 48, 256
    x = (rnd(M, D) * 3 + 1).float().double()
    g, b = (1 + 0.1 * rnd(D)).float(), rnd(D, scale=0.1).float()
    (r32, rop) = I.final_layernorm(x, g, b, DT)
    y = F.layer_norm(x.float(), (D,), g, b, 1e-5)
    assert I.check(y.double(), r32[0], r32[1])["ratio"] <= 1.0
    r = ratio(y.half().double(), rop)
    assert r["ratio"] <= 1.0 and abs(r["bias"]) <= I.BIAS_MAX, r
    assert ratio(x.float().half().double(), rop)["ratio"] >= 10  # (the copy taken before the normalisation)
    assert I.check(x, r32[0], r32[1])["ratio"] >= 10


def _conf_sd(E=144, K=1024):
    return {"LL.weight": rnd(E, K, scale=1 / math.sqrt(K)).float(), "LL.bias": rnd(E, scale=0.1).float(),
            "first_bn.weight": torch.tensor([1.3]), "first_bn.bias": torch.tensor([-0.2]),
            "first_bn.running_mean": torch.tensor([0.1]), "first_bn.running_var": torch.tensor([0.7]),
            "conformer.class_token": torch.rand(1, E, generator=G, dtype=torch.float64).float(),
            "conformer.fc5.weight": rnd(2, E, scale=1 / 12).float(), "conformer.fc5.bias": rnd(2, scale=0.1).float()}


def test_tokens_correct_and_class_token_at_the_last_row():
    B, T, E = 2, 9, 144
    sd = _conf_sd(E)
    a = op16(rnd(B * T, 1024))
    rb = I.conf_tokens(sd, a, B, T, DT)
    ll = a.float() @ op16(sd["LL.weight"].double()).float().t() + sd["LL.bias"]
    sc = sd["first_bn.weight"] / torch.sqrt(sd["first_bn.running_var"] + 1e-5)
    sh = sd["first_bn.bias"] - sd["first_bn.running_mean"] * sc
    y = F.selu(ll * sc + sh).reshape(B, T, E)
    cls = sd["conformer.class_token"].reshape(1, 1, E).expand(B, 1, E)
    good = torch.cat([cls, y], 1).reshape(B * (T + 1), E).double()
    assert I.check(good, rb[0], rb[1])["ratio"] <= 1.0
    assert bool((y < 0).any()) and bool((y > 0).any())  # (both sides of SELU)
    bad = torch.cat([y, cls], 1).reshape(B * (T + 1), E).double()
    assert I.check(bad, rb[0], rb[1])["ratio"] >= 10
    rl = I.conf_logits(sd, good, B, T + 1)
    x0 = good.reshape(B, T + 1, E)[:, 0].float()
    assert I.check((x0 @ sd["conformer.fc5.weight"].t() + sd["conformer.fc5.bias"]).double(), rl[0], rl[1])["ratio"] <= 1.0
    x1 = good.reshape(B, T + 1, E)[:, 1].float()  # (the classifier on the first frame's token instead of the class token)
    assert I.check((x1 @ sd["conformer.fc5.weight"].t() + sd["conformer.fc5.bias"]).double(), rl[0], rl[1])["ratio"] >= 10


# ---- the bias statistic of an attention output: against the P-rounded reference ---------------------------------------------
def _sim_bf16(qkv, T, H, block=None):
    """Correct bf16 kernel on every row: fp32 logits, P~ rounded to bf16 for P.v, the row's sum unrounded, round-to-nearest
    store (block: the key-blocked form)."""
    B = qkv.shape[0] // T
    x = qkv.reshape(B, T, 3, H, 64).float()
    outs = []
    for b in range(B):
        s = torch.einsum("qhd,khd->qhk", x[b, :, 0], x[b, :, 1]) * 0.125
        if block is None:
            p = torch.exp(s - s.amax(-1, keepdim=True))
            o = torch.einsum("qhk,khd->qhd", p.bfloat16().float(), x[b, :, 2]) / p.sum(-1)[..., None]
        else:
            m, l, acc = torch.full(s.shape[:2], -1e30), torch.zeros(s.shape[:2]), torch.zeros(T, H, 64)
            for j0 in range(0, T, block):
                sb = s[..., j0:j0 + block]
                mn = torch.maximum(m, sb.amax(-1))
                corr, p = torch.exp(m - mn), torch.exp(sb - mn[..., None])
                l, m = l * corr + p.sum(-1), mn
                acc = acc * corr[..., None] + torch.einsum("qhk,khd->qhd", p.bfloat16().float(), x[b, j0:j0 + block, 2])
            o = acc / l[..., None]
        outs.append(o.reshape(T, -1))
    return torch.cat(outs).double()


@pytest.mark.parametrize("T,block", [(100, None), (300, 128)])
def test_attention_bias_is_judged_against_the_p_rounded_reference(T, block):
    """Three clips, two heads, nearly flat logits (what synthetic weights give): every weight P~ of a row lies in the same
    bf16 bin and rounds the same way, so a CORRECT kernel's output differs from the exact one by a shared relative offset
    and the statistic against the exact reference leaves +-BIAS_MAX, whatever the store does.  Against the P-rounded
    reference the correct kernel measures ~0 and a truncating store its -0.5 ulp."""
    B, H = 3, 2
    x = rnd(B, T, 3, H, 64)
    x[:, :, 0] *= 0.0005  # logits within ~ +-0.002: every P~ in (0.996, 1], one bf16 bin wide
    qkv = I.op(x.reshape(B * T, 3 * H * 64), "bf16")
    rows = torch.arange(B * T)
    ref, bnd, pref = I.mhsa(qkv, rows, T, "bf16", heads=H, bias_ref=True, blocked=block is not None)
    good = _sim_bf16(qkv, T, H, block)
    got = good.bfloat16().double()
    exact = I.check(got, ref, bnd, "bf16", rows)
    fine = I.check(got, ref, bnd, "bf16", rows, bias_ref=pref)
    assert exact["ratio"] <= 1.0 and fine["ratio"] == exact["ratio"]
    assert abs(exact["bias"]) > I.BIAS_MAX, exact  # (P's rounding, not the store)
    assert abs(fine["bias"]) <= I.BIAS_MAX / 5, fine
    t = good.float().bfloat16()
    bits = t.view(torch.int16).clone()
    bits[t.float().abs() > good.float().abs()] -= 1  # round toward zero
    cut = I.check(bits.view(torch.bfloat16).double(), ref, bnd, "bf16", rows, bias_ref=pref)
    assert cut["bias"] <= -8 * I.BIAS_MAX, cut


def test_p_rounded_reference_follows_masks_and_blocks(masked):
    qkv, rows, rb = masked
    n = torch.tensor(MLENS)[rows // MT]
    for blocked, sim in ((False, sim_masked(qkv, rows, n)), (True, sim_blocked(qkv, rows, n))):
        ref, bnd, pref = I.mhsa(qkv, rows, MT, DT, heads=MH, lens=MLENS, bias_ref=True, blocked=blocked)
        assert torch.equal(ref, rb[0]) and torch.equal(bnd, rb[1])
        r = I.check(op16(sim), ref, bnd, DT, rows, bias_ref=pref)
        assert r["ratio"] <= 1.0 and abs(r["bias"]) <= I.BIAS_MAX / 5, r


def test_fp16_floor_does_not_swallow_a_defect_on_tiny_values():
    """fp16x3 rows with v ~ 2^-10 (where the unscaled pairs' floor of 2 x 2^-25 is most of the bound): a correct
    split-precision result passes, an error of 2^-20 on one element does not, and a dropped key fails by >= 10x."""
    B, T, H = 1, 40, 2
    x = rnd(B, T, 3, H, 64)
    x[:, :, 2] *= 2.0 ** -10
    qkv = I.op(x.reshape(B * T, 3 * H * 64), "fp16x3")
    rows = torch.arange(B * T)
    ref, bnd = I.mhsa(qkv, rows, T, "fp16x3", heads=H)
    assert 2 * I.F16_FLOOR < float(bnd.min()) and float(bnd.max()) < 2.0 ** -21  # (the floor terms are a good part of it)
    assert I.check(ref.float().double(), ref, bnd)["ratio"] <= 1.0
    bad = ref.clone()
    bad[7, 5] += 2.0 ** -20
    assert I.check(bad, ref, bnd)["ratio"] > 2
    xq = qkv.reshape(B, T, 3, H, 64)
    s = torch.einsum("qhd,khd->qhk", xq[0, :, 0], xq[0, :, 1]) * 0.125
    s[..., 13] = -float("inf")
    dropped = torch.einsum("qhk,khd->qhd", torch.softmax(s, -1), xq[0, :, 2]).reshape(T, -1)
    assert I.check(dropped, ref, bnd)["ratio"] >= 10

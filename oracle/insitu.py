"""Per-launch fp64 references for the in-place checks (TEST INFRASTRUCTURE).

``Engine`` taps (``afx/engine.py::Engine.tap``) expose the inputs and outputs of every launch of a forward.  Each function
below takes the tapped inputs of ONE launch plus the state dict (the oracle's key names, no ``ssl_model.model.`` prefix
for the trunk) and returns ``(ref, bound)``: the launch's exact result in float64 (before the output's own rounding to
the operand type) and a per-element error bound.  Operands are
rounded exactly where the kernels round them (``op``), every sum is exact in float64, and the bound is what a correct
kernel may differ by:

  * fp32 outputs of a product:   ``c_acc * S + c_poly``, where ``S = sum |a||w| + |bias| + |resid|`` per element (the
    magnitude the accumulation errors are relative to) and ``c_poly`` = 3e-6 covers the GELU / swish polynomials of the
    epilogues (``test_epilogue_gelu_polynomial_is_erf_gelu_to_3e6``) per unit of |output|;
  * operand-type outputs:        one ulp of the operand type at ``ref`` plus the term above times the epilogue's
    derivative (a LayerNorm divides by the row's sigma and multiplies by |gamma|);
  * a rounding point INSIDE a launch (the fused chains round the LayerNorm output before W1 and the swish hidden layer
    before W2; attention rounds P before P.V): the kernel's fp32 value and the fp64 value may round to neighbouring
    operand values.  ``C_FLIP`` such one-ulp disagreements per row are allowed, each weighted by the largest weight it
    can meet (``flip`` below);
  * unbiased rounding:           for every fp16 / bf16 operand output, ``bias_stat`` = the mean of
    ``sign(ref) (got - ref) / ulp(ref)`` over the normal-range elements is within +-BIAS_MAX.  Round-to-nearest-even
    gives ~0, truncation -0.5.  (fp32-typed operands carry several ulps of accumulation noise, so the statistic is
    reported for them, not asserted);
  * pad columns (144..159 of ``ao`` / ``hc`` / ``u`` / ``hid``, the pad rows of ``xpad``) are exactly 0.

Constants, calibrated once per operand dtype on an MI355X (tests/test_gpu_insitu.py prints, per launch class and dtype,
the worst ratio |got - ref| / bound):

  C_ACC  2^-19 for fp16 / bf16 / fp32 operands, 2^-18 for fp16x3 (hi / lo pairs carry ~22 significant bits).
         Worst measured ratio over all legs: fp16 0.496, bf16 0.499 (products, conv, LayerNorm, dwconv: the output's own
         half-ulp rounding dominates), chains 0.33 (chain B), posconv 0.28, trunk attention 0.36; fp32 0.225, fp16x3 0.071.
  C_FLIP 3 one-ulp flips per row at an internal rounding point (and per output column for the posconv weights, whose
         weight norm the device computes in fp32 before it rounds them).
  Bias   fp16 / bf16 operand outputs measured within +-0.015 ulp (BIAS_MAX 0.05).
"""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-5
BN_EPS = 1e-5
MAX_POS = 512

C_ACC = {"fp16": 2.0 ** -19, "bf16": 2.0 ** -19, "fp32": 2.0 ** -19, "fp16x3": 2.0 ** -18}
C_POLY = 3e-6
C_FLIP = 3.0
BIAS_MAX = 0.05
# launch classes whose bias statistic is reported, not asserted: the Shaw attention's output error is dominated by the
# rounding of P (several ulps of the output), and its mean signed error measured +0.06 .. +0.30 ulp (fp16 / bf16) on the
# first MI355X run -- an open item, not a rounding-mode defect of the output store
BIAS_REPORTED = ("shaw",)
# unit roundoff of the operand copies (fp16x3: the pair form of an fp32 value, ~2^-22)
U_OP = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp32": 2.0 ** -24, "fp16x3": 2.0 ** -22}
_MANT = {"fp16": 10, "bf16": 7, "fp32": 23, "fp16x3": 23}
_EMIN = {"fp16": -14, "bf16": -126, "fp32": -126, "fp16x3": -126}
HALF = ("fp16", "bf16")


def op(x, dt):
    """Round to the operand type of `dt` (fp32 / fp16x3 operand buffers hold fp32 values)."""
    t = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(dt, torch.float32)
    return x.to(t).to(torch.float64)


def ulp(x, dt):
    """Spacing of the operand type of `dt` at |x| (subnormal spacing below the smallest normal)."""
    _, e = torch.frexp(x.abs().to(torch.float64))
    e = torch.clamp(e - 1, min=_EMIN[dt])
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - _MANT[dt])


def d(t):
    return t.detach().to("cpu", torch.float64)


def gelu(z):
    return F.gelu(z)


def dgelu(z):  # |d gelu / dz| <= 1.13
    return (0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)).abs()


def swish(z):
    return z * torch.sigmoid(z)


def dswish(z):
    s = torch.sigmoid(z)
    return (s + z * s * (1 - s)).abs()


def flip(r, dt, wmax):
    """Allowance for C_FLIP one-ulp disagreements of an internal rounding point (values r: (M, K)) feeding weights whose
    largest magnitude per output column is wmax (N,): (M, N)."""
    if dt not in HALF:
        return torch.zeros(r.shape[0], wmax.shape[0], dtype=torch.float64)
    return C_FLIP * ulp(r, dt).amax(1, keepdim=True) * wmax[None, :]


# ---- products ---------------------------------------------------------------------------------------------------------
def linear(a, w, b, dt):
    """a (M, K) operand values (already rounded), w (N, K) fp32 weights -> (z, S): z = a.op(w)^T + b, S = |a||w|^T + |b|."""
    w = op(d(w), dt)
    z = a @ w.t()
    s = (a.abs().float() @ w.abs().float().t()).double()  # (a magnitude: fp32 is plenty)
    if b is not None:
        z = z + d(b)
        s = s + d(b).abs()
    return z, s


def product(a, w, b, dt, act=None, alpha=1.0, resid=None, out="f32"):
    """GEMM launch: out = resid + alpha act(a w^T + b), fp32 (out="f32") or operand type (out="op")."""
    z, s = linear(a, w, b, dt)
    if act == "gelu":
        y, g = gelu(z), dgelu(z)
    elif act == "swish":
        y, g = swish(z), dswish(z)
    else:
        y, g = z, torch.ones_like(z)
    y = alpha * y
    e = alpha * (C_ACC[dt] * s * g + (C_POLY * (1 + z.abs()) if act else 0))
    if resid is not None:
        y = y + resid
        e = e + C_ACC[dt] * resid.abs()
    if out == "op":  # (the exact value: the kernel's rounding of it is what the ulp term allows)
        return y, e + ulp(y, dt)
    return y, e


def layernorm(x, g, b, dt, out="op", acc=None):
    """Row LayerNorm of fp32 rows x (M, C) (acc: an accumulation error bound on x, fed through 1 / sigma)."""
    g, b = d(g), d(b)
    mu = x.mean(1, keepdim=True)
    sig = torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + LN_EPS)
    xh = (x - mu) / sig
    y = xh * g + b
    # fp32 row statistics: the mean's error is relative to |mu| + sigma, not to |x - mu|
    e = C_ACC["fp16x3" if dt == "fp16x3" else "fp32"] * 16 * ((xh.abs() + 1 + mu.abs() / sig) * g.abs() + b.abs())
    if acc is not None:
        e = e + g.abs() * (acc + acc.amax(1, keepdim=True)) / sig
    if out == "op":
        return y, e + ulp(y, dt)
    return y, e


# ---- SSL trunk --------------------------------------------------------------------------------------------------------
def conv_layer(sd, i, prev, B, rows, dt, mode="layer_norm", out="op"):
    """Conv layer i >= 1 as the engine launches it, for the flat output rows `rows`: prev (B * T_{i-1}, 512) operand
    values -> (R, 512); layer_norm mode: conv + bias -> LayerNorm(512) -> GELU in the epilogue, group_norm mode: bias-free
    conv -> GELU.  out="f32" for the last layer (fp32 rows for the feature LayerNorm)."""
    k, st = (3, 2) if i < 5 else (2, 2)
    w = sd[f"feature_extractor.conv_layers.{i}.0.weight"]  # (512, 512, k)
    C = w.shape[0]
    x = prev.reshape(B, -1, C)
    Tn = (x.shape[1] - k) // st + 1
    b_i, t_i = rows // Tn, rows % Tn
    a = x[b_i[:, None], st * t_i[:, None] + torch.arange(k)[None, :]].reshape(len(rows), k * C)  # K = tap * C + channel
    wk = w.permute(0, 2, 1).reshape(C, k * C)
    if mode != "layer_norm":
        return product(a, wk, None, dt, act="gelu", out=out)
    z, s = linear(a, wk, sd[f"feature_extractor.conv_layers.{i}.0.bias"], dt)
    y, e = layernorm(z, sd[f"feature_extractor.conv_layers.{i}.2.1.weight"], sd[f"feature_extractor.conv_layers.{i}.2.1.bias"],
                     dt, out="f32", acc=C_ACC[dt] * s)
    g, e = gelu(y), dgelu(y) * e + C_POLY * (1 + y.abs())  # (the polynomial's error is on GELU's output)
    return (g, e + ulp(g, dt)) if out == "op" else (g, e)


def conv0(sd, wave, rows, dt, mode="layer_norm"):
    """Conv layer 0 on the fp32 waveform (B, L) for the flat output rows `rows`: k = 10, s = 5 -> LayerNorm (group_norm
    mode: GroupNorm over each utterance's time axis) -> GELU, operand type.  The half-precision engines run it at fp32
    accuracy (the split-precision matrix-core form): the accumulation bound is fp32-level."""
    x = d(wave)
    w = d(sd["feature_extractor.conv_layers.0.0.weight"])[:, 0, :]  # (512, 10)
    cols = x.unfold(1, 10, 5)  # (B, T0, 10)
    T0 = cols.shape[1]
    b_i, t_i = rows // T0, rows % T0
    c = cols[b_i, t_i]
    z = c @ w.t()
    s = c.abs() @ w.abs().t()
    ca = C_ACC["fp16x3"]
    if mode == "layer_norm":
        bias = d(sd["feature_extractor.conv_layers.0.0.bias"])
        y, e = layernorm(z + bias, sd["feature_extractor.conv_layers.0.2.1.weight"], sd["feature_extractor.conv_layers.0.2.1.bias"],
                         "fp16x3", out="f32", acc=ca * (s + bias.abs()))
    else:  # statistics over the whole utterance (every frame), per channel
        zf = cols @ w.t()  # (B, T0, 512)
        mu, var = zf.mean(1), zf.var(1, unbiased=False)
        sig = torch.sqrt(var + LN_EPS)[b_i]
        g, b = d(sd["feature_extractor.conv_layers.0.2.weight"]), d(sd["feature_extractor.conv_layers.0.2.bias"])
        xh = (z - mu[b_i]) / sig
        y = xh * g + b
        sm = (cols.abs() @ w.abs().t()).amax(1)[b_i]
        e = ca * 16 * (xh.abs() * g.abs() + b.abs()) + g.abs() * ca * 4 * (s + sm) / sig
    g = gelu(y)
    return g, dgelu(y) * e + C_POLY * (1 + y.abs()) + ulp(g, dt)


def pos_weight(sd):
    if "encoder.pos_conv.0.weight" in sd:
        return d(sd["encoder.pos_conv.0.weight"])
    v, g = d(sd["encoder.pos_conv.0.weight_v"]), d(sd["encoder.pos_conv.0.weight_g"])
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def posconv(sd, xpad, x, rows, T, dt, groups=16):
    """Positional conv launch: x (B T, D) fp32 += GELU(conv(xpad) + bias) for the flat rows `rows`.  xpad: the operand
    copy (B, T + 128, D), frame t of utterance b at padded row t + 64; output frame t reads padded rows t .. t + 127."""
    w32 = pos_weight({k: v.float() if torch.is_tensor(v) else v for k, v in sd.items() if k.startswith("encoder.pos_conv")})
    w = op(w32.float(), dt)  # (D, D / groups, 128): the device computes the weight norm in fp32, then rounds
    D, cpg, K = w.shape
    b_i, t_i = rows // T, rows % T
    win = xpad[b_i[:, None], t_i[:, None] + torch.arange(K)[None, :]]  # (R, 128, D)
    win = win.reshape(len(rows), K, groups, cpg).permute(2, 0, 3, 1).reshape(groups, len(rows), cpg * K)  # k = c * 128 + j
    wg = w.reshape(groups, cpg, cpg * K)  # (G, out, c * 128 + j)
    z = torch.bmm(win, wg.transpose(1, 2)).permute(1, 0, 2).reshape(len(rows), D) + d(sd["encoder.pos_conv.0.bias"])
    s = torch.bmm(win.abs(), wg.abs().transpose(1, 2)).permute(1, 0, 2).reshape(len(rows), D) + d(sd["encoder.pos_conv.0.bias"]).abs()
    xr = x[rows]
    # (a weight whose fp32 weight norm lands on the other side of a rounding boundary: C_FLIP of them per output column)
    wflip = C_FLIP * win.abs().amax(2).t()[:, :, None] * ulp(w.abs().amax((1, 2)), dt).reshape(1, groups, cpg)
    wflip = wflip.reshape(len(rows), D) if dt in HALF else 0
    return xr + gelu(z), (C_ACC[dt] * s + wflip) * dgelu(z) + C_ACC[dt] * xr.abs() + C_POLY * (1 + z.abs())


def mhsa(qkv, rows, T, dt, heads=16):
    """Trunk self-attention launch for the flat query rows `rows`: qkv (B T, 3 D) operand values (q unscaled) -> (R, D)
    operand type.  The kernel scales the fp32 logits by dh^-0.5 and rounds P to the operand type before P.V."""
    D = qkv.shape[1] // 3
    dh = D // heads
    B = qkv.shape[0] // T
    x = qkv.reshape(B, T, 3, heads, dh)
    b_i, t_i = rows // T, rows % T
    q = x[b_i, t_i, 0]  # (R, H, dh)
    k = x[b_i, :, 1]  # (R, T, H, dh)
    v = x[b_i, :, 2]
    s = torch.einsum("rhd,rthd->rht", q, k) * dh ** -0.5
    sa = torch.einsum("rhd,rthd->rht", q.abs(), k.abs()) * dh ** -0.5
    return _softmax_av(s, sa, v, dt)


def _softmax_av(s, sa, v, dt, extra=None):
    """P = softmax(s) over the last axis, out = P.v (v: (R, keys, H, dh)) -> (R, H * dh) operand type and its bound: P's
    rounding (u_op per weight), the logits' accumulation (C_ACC * sa) moving P, the output's own ulp."""
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("rht,rthd->rhd", p, v)
    pv = torch.einsum("rht,rthd->rhd", p, v.abs())
    es = C_ACC[dt] * sa + (extra if extra is not None else 0)
    # |d out| <= sum_j P_j |v_j - out| (|ds_j| + max |ds|) <= 2 max |ds| sum_j P_j (|v_j| + |out|)
    ds = es.amax(-1)[..., None]
    e = U_OP[dt] * 1.01 * pv + 2 * ds * (pv + out.abs()) + C_ACC[dt] * 16 * pv
    R = out.shape[0]
    out, e = out.reshape(R, -1), e.reshape(R, -1)
    return out, e + ulp(out, dt)


def shaw(qkv32, rel, rows, N, dt, heads=4):
    """Conformer Shaw attention launch for flat query rows `rows`: qkv32 (B N, 3 inner) fp32 -> (R, inner) operand type.
    logits[i, j] = q_i.k_j + q_i.E[clamp(i - j, +-512) + 512] with q scaled by dh^-0.5 before it is rounded (fp16 / bf16),
    k, v and the table rounded to the operand type."""
    inner = qkv32.shape[1] // 3
    dh = inner // heads
    B = qkv32.shape[0] // N
    x = qkv32.reshape(B, N, 3, heads, dh)
    b_i, t_i = rows // N, rows % N
    sc = 1.0 / math.sqrt(dh)
    if dt in HALF:
        q = op(x[b_i, t_i, 0].float() * torch.tensor(sc, dtype=torch.float32), dt)
        qs = 1.0
    else:
        q, qs = x[b_i, t_i, 0], sc
    k, v = op(x[b_i, :, 1], dt), op(x[b_i, :, 2], dt)
    dist = (t_i[:, None] - torch.arange(N)[None, :]).clamp(-MAX_POS, MAX_POS) + MAX_POS  # (R, N)
    E = op(d(rel), dt)[dist]  # (R, N, dh)
    s = (torch.einsum("rhd,rthd->rht", q, k) + torch.einsum("rhd,rtd->rht", q, E)) * qs
    sa = (torch.einsum("rhd,rthd->rht", q.abs(), k.abs()) + torch.einsum("rhd,rtd->rht", q.abs(), E.abs())) * qs
    return _softmax_av(s, sa, v, dt)


# ---- Conformer chains --------------------------------------------------------------------------------------------------
def _ff(sd, p, x, dt):
    """x + 1/2 FF(x) as the chain computes it: LN -> op -> W1 + b1 -> swish -> op -> W2 + b2."""
    y, ey = layernorm(x, sd[p + "fn.norm.weight"], sd[p + "fn.norm.bias"], dt)
    y = op(y, dt)
    w1, w2 = sd[p + "fn.fn.net.0.weight"], sd[p + "fn.fn.net.3.weight"]
    z, s1 = linear(y, w1, sd[p + "fn.fn.net.0.bias"], dt)
    ez = C_ACC[dt] * s1 + flip(y, dt, op(d(w1), dt).abs().amax(1))
    if dt not in HALF:
        ez = ez + (ey - ulp(y, dt)) @ op(d(w1), dt).abs().t()
    h = op(swish(z), dt)
    eh = dswish(z) * ez + C_POLY * (1 + z.abs())
    o, s2 = linear(h, w2, sd[p + "fn.fn.net.3.bias"], dt)
    w2a = op(d(w2), dt).abs()
    eo = C_ACC[dt] * s2 + eh @ w2a.t() + flip(h, dt, w2a.amax(1))
    return x + 0.5 * o, 0.5 * eo + C_ACC[dt] * x.abs()


def chain_a(sd, p, x, dt):
    """Chain A of block prefix p: x (M, E) fp32 -> (xa, qkv): x += 1/2 FF1(x); q | k | v = W_qkv op(LN(x)) (no bias)."""
    xa, ea = _ff(sd, p + "ff1.", x, dt)
    y = op(layernorm(xa, sd[p + "attn.norm.weight"], sd[p + "attn.norm.bias"], dt)[0], dt)
    w = torch.cat([sd[p + "attn.fn.to_q.weight"], sd[p + "attn.fn.to_kv.weight"]], 0)
    z, s = linear(y, w, None, dt)
    wa = op(d(w), dt).abs()
    return (xa, ea), (z, C_ACC[dt] * s + flip(y, dt, wa.amax(1)) + _ln_prop(xa, ea, sd, p + "attn.norm.", wa, dt))


def _ln_prop(x, ex, sd, p, wa, dt):
    """An error ex on the rows x moves LN(x) by <= |gamma| (ex + max ex) / sigma; through the weights |W| that follow."""
    sig = torch.sqrt(x.var(1, unbiased=False, keepdim=True) + LN_EPS)
    ey = d(sd[p + "weight"]).abs() * (ex + ex.amax(1, keepdim=True)) / sig
    return ey @ wa.t()


def chain_b(sd, p, x, ao, dt):
    """Chain B: x += W_out ao + b (ao (M, inner) operand values); glu_in = W_pw1 op(LN(x)) + b, fp32."""
    o, s = linear(ao, sd[p + "attn.fn.to_out.weight"], sd[p + "attn.fn.to_out.bias"], dt)
    xb, eb = x + o, C_ACC[dt] * (s + x.abs())
    y = op(layernorm(xb, sd[p + "conv.net.0.weight"], sd[p + "conv.net.0.bias"], dt)[0], dt)
    w = sd[p + "conv.net.2.weight"][:, :, 0]
    z, s2 = linear(y, w, sd[p + "conv.net.2.bias"], dt)
    wa = op(d(w), dt).abs()
    return (xb, eb), (z, C_ACC[dt] * s2 + flip(y, dt, wa.amax(1)) + _ln_prop(xb, eb, sd, p + "conv.net.0.", wa, dt))


def chain_c(sd, p, x, u, dt):
    """Chain C: x += W_pw2 u + b (u (M, C2) operand values); x += 1/2 FF2(x); x = LN_post(x), fp32."""
    o, s = linear(u, sd[p + "conv.net.7.weight"][:, :, 0], sd[p + "conv.net.7.bias"], dt)
    xc, ec = x + o, C_ACC[dt] * (s + x.abs())
    xd, ed = _ff(sd, p + "ff2.", xc, dt)
    return layernorm(xd, sd[p + "post_norm.weight"], sd[p + "post_norm.bias"], dt, out="f32", acc=ed + ec)


def glu_dwconv(sd, p, glu, B, N, dt):
    """GLU -> depthwise conv (same padding) -> BatchNorm (eval) -> swish, glu (B N, 2 C2) fp32 -> (B N, C2) operand type."""
    a, g = glu.reshape(B, N, -1).chunk(2, dim=-1)
    h = (a * torch.sigmoid(g)).transpose(1, 2)  # (B, C2, N)
    w = d(sd[p + "conv.net.4.conv.weight"])
    k = w.shape[-1]
    pad = (k // 2, k // 2 - (k + 1) % 2)
    z = F.conv1d(F.pad(h, pad), w, d(sd[p + "conv.net.4.conv.bias"]), groups=h.shape[1])
    s = F.conv1d(F.pad(h.abs(), pad), w.abs(), d(sd[p + "conv.net.4.conv.bias"]).abs(), groups=h.shape[1])
    m, v = d(sd[p + "conv.net.5.running_mean"]), d(sd[p + "conv.net.5.running_var"])
    sc = d(sd[p + "conv.net.5.weight"]) / torch.sqrt(v + BN_EPS)
    sh = d(sd[p + "conv.net.5.bias"]) - m * sc
    zz = z * sc[None, :, None] + sh[None, :, None]
    y = swish(zz).transpose(1, 2).reshape(B * N, -1)
    e = (dswish(zz) * C_ACC["fp16x3"] * 16 * (s * sc.abs()[None, :, None] + zz.abs() + sh.abs()[None, :, None] + 1) +
         C_POLY * (1 + zz.abs())).transpose(1, 2).reshape(B * N, -1)
    return y, e + ulp(y, dt)


# ---- the check ---------------------------------------------------------------------------------------------------------
def check(got, ref, bound, dt=None, rows=None):
    """-> dict(ratio = max |got - ref| / bound, row (of `rows` when given), col, got / ref / bound of the worst element,
    bias = the rounding-bias statistic (None unless dt names the operand type of got), n = elements checked)."""
    ref = ref.reshape(ref.shape[0], -1)
    got, bound = d(got).reshape(ref.shape), bound.reshape(ref.shape) + ulp(ref, "fp32")  # (every tap is an fp32 value)
    err = (got - ref).abs()
    r = err / bound
    r = torch.where(torch.isnan(got), torch.full_like(r, float("inf")), r)
    i = int(torch.argmax(r))
    row, col = divmod(i, ref.shape[1])
    bias = None
    if dt is not None:
        u = ulp(ref, dt)
        m = (ref.abs() >= 2.0 ** _EMIN[dt]) & (ref != 0)
        if bool(m.any()):
            bias = float((torch.sign(ref) * (got - ref) / u)[m].mean())
    return dict(ratio=float(r.reshape(-1)[i]), row=int(rows[row]) if rows is not None else row, col=col, got=float(got[row, col]),
                ref=float(ref[row, col]), bound=float(bound[row, col]), bias=bias, n=ref.numel())

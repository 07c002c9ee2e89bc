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
  The KV-cached step (oracle/insitu_kv.py: the same kernel families on the chunk's 1 .. 48 rows, the ring attention over <=
  256 live slots) is judged with these constants unchanged.  tests/test_gpu_insitu_kv.py's summary on an MI355X, worst
  ratio fp16 / bf16 / fp16x3: kv_product 0.495 / 0.499 / 0.078, kv_layernorm 0.479 / 0.497 / 0.004, kv_posconv 0.279 /
  0.166 / 0.039, kv_ring 0.599 / 0.516 / 0.005 (bias of the products and LayerNorms within +-0.008 ulp; the ring
  attention's statistic is reported only: too few independent samples at <= 48 query rows).

  Under key-padding masks (``lens``: ragged batches, judged on the rows of each clip's own length: ``masked_rows``), at the
  two ends of a forward and for the attention kernel alone on lively logits, the constants are the same.  Worst ratio on
  an MI355X (tests/test_gpu_insitu_ragged.py's summary), fp16 / bf16 / fp32 / fp16x3: mhsa_masked 0.409 / 0.415 / 0.022 /
  0.358, mhsa_long (the blocked kernel, uniform and masked; fp16x3: the VALU fallback) 0.357 / 0.363 / 0.034 / 0.017,
  mhsa_few (uniform, 1 .. 3 clips) 0.358 / 0.373 / 0.028 / 0.250, shaw_masked 0.424 / 0.536 / 0.028 / 0.014, dwconv_masked
  0.479 / 0.497 / 0.004 / 0.005, final_ln (both outputs) 0.479 / 0.497 / 0.006 / 0.004, tokens 0.067 / 0.062 / 0.160 /
  0.048, logits 0.015 / 0.015 / 0.013 / 0.013; ``afx.kernels.mhsa`` alone on logits of spread ~9 with planted dominating
  keys, fp16 / bf16 / fp16x3: mhsa_k (one-pass families) 0.457 / 0.612 / 0.234, mhsa_k_long (blocked) 0.457 / 0.623.
  The fp16x3 figures of the short clips and the fp16 figures on lively logits are WITH the absolute-floor terms
  (``F16_FLOOR``, derived at ``_softmax_av``); without them those launches measured 1.3 .. 4.0 and 1.02 .. 1.46.
  The floor terms enter ``mhsa``'s bound for every fp16 and (up to 224 frames) fp16x3 launch, the earlier class "mhsa"
  included: fp16 gains sum_j min(P~_j, 2^-25) |v_j| / sum P~, which for weights above 2^-14 is 2^-14 of the u_op term it
  stands beside (nothing measurable on the earlier shapes, whose logits are flat); fp16x3 gains 2^-24 per element plus
  the q / k term, an absolute addition that matters where |v| is small.  tests/test_cpu_insitu.py shows that an error of
  2^-20 and a dropped key on rows with |v| ~ 2^-10 still fail.
  Bias: the new trunk-attention classes are asserted against the P-rounded reference (``_p_rounded``) and measure within
  +-0.007 ulp (fp16 and bf16, every class above); against the exact reference the same launches read bf16 -0.35 .. +0.17
  ulp at 3 clips and -0.05 at 25, fp16 up to -0.06: P's rounding, shared by the elements of an (utterance, head), not the
  store.  shaw_masked is reported like shaw: +0.014 (fp16), +0.175 (bf16).

The AASIST back-end (``aasist_walk`` and the functions above it) is fp32 throughout, so its bounds carry no operand ulp:

  * products and convs (LL, conv1 / conv2 / downsample as chunked-K products over the padded image, the two 1x1 maps):
    activations exact fp32, weights exact (dtype fp32) or ``Wh + 2^-11 Wl`` rebuilt as ``split_f16_kernel`` builds the
    pair (every other dtype); ``C_ACC["fp32"]`` / ``C_ACC["fp16x3"]`` times ``S``, pushed through the epilogue (bias ->
    residual -> post 1 = BN -> SELU / post 2 = SELU -> BN -> validity mask).  Invalid virtual pixels have reference 0 and
    bound 0, and ``aas_border`` counts every nonzero float in an image's head and at its invalid pixels: it must be 0;
  * VALU kernels (pool_bn_selu, first_block, att_pool, rowlin, gat, readout): ``C_ACC["fp32"]`` times the magnitude sum,
    pushed through the derivative of tanh / softmax / SELU, plus ``C_FN`` fp32 ulps of the OUTPUT of expf / tanhf / the
    sigmoid (for SELU's negative side: lambda alpha C_FN ulp(e^z));
  * GraphPool (``pool_check``) is tie-tolerant and leaves no pool out: each output row is mapped to its nearest
    ``h_j s64_j`` (rows that lie within the bound of several nodes -- exact ties on silence -- are matched to one node
    each), which must be within the product's bound and distinct, and order and membership must agree with the
    fp64 scores up to delta = ``C_ACC["fp32"] (sum |h||w| + |b|) / 4 + C_FN ulps`` of the two scores compared.

  C_FN   2 ulps.  Measured where a device function's output is visible: pool_bn_selu computes u = fmaf(max, sc, sh) and
         lambda alpha (expf(u) - 1), and for e^u in [0.5, 1) the subtraction is exact, so |got - lambda alpha expm1(u)| /
         (lambda alpha ulp32(e^u)) is expf's error plus one rounding of the product: worst 0.780 ulps over the 2 402 such
         elements of five shapes (mean 0.26); twice that, rounded up to a power of two.  tanhf and the sigmoid feed sums
         before anything is stored, so no tap shows them alone; |got - ref| / ulp32(ref) of whole outputs is cancellation
         and accumulation (up to 84 ulps at elements within 1 / 16 of the largest, 1e5 at outputs near 0), not a property
         of the functions.  With C_FN = 0 every launch of the back-end still passes (worst 0.34 of its bound).
         Worst measured ratio per class (fp16 / bf16 / fp32 / fp16x3): aas_conv 0.354 / 0.350 / 0.355 / 0.350, aas_prod
         0.337 / 0.337 / 0.369 / 0.337, aas_valu 0.381 / 0.111 / 0.164 / 0.111, gat 0.139 / 0.080 / 0.126 / 0.080, pool
         0.078 / 0.078 / 0.093 / 0.078, readout 0.091 / 0.034 / 0.042 / 0.034 (fp16 and fp32 ran the larger shapes).

Call audio (``afx.synth.call_waveforms``: silence, a burst cut to silence, DC, a full-scale square wave, one PCM step, a
click, a tone, G.711 steps, comfort noise, "repeat" concealment; tests/test_gpu_insitu_call.py, classes under a ``_call``
suffix) is judged with every constant unchanged.  Its summary on an MI355X, worst ratio fp16 / bf16 / fp32 / fp16x3 (bias
fp16 / bf16): conv0_call 0.483 / 0.497 / 0.088 / 0.088 (-0.0016 / +0.0018), conv_call 0.493 / 0.499 / 0.176 / 0.063 (-0.0017 /
+0.0029), layernorm_call 0.480 / 0.497 / 0.005 / 0.004 (+0.0010 / -0.0013), product_call 0.494 / 0.499 / 0.184 / 0.055
(-0.0013 / -0.0023), posconv_call 0.281 / 0.134 / 0.102 / 0.040, mhsa_few_call 0.417 / 0.405 / 0.014 / 0.023 (-0.0038 /
-0.0013), final_ln_call 0.480 / 0.497 / 0.005 / 0.004 (+0.0007 / +0.0003), tokens_call 0.047 / 0.050 / 0.115 / 0.036,
chain_a_call 0.038 / 0.006 / 0.000 / 0.000, chain_b_call 0.303 / 0.082 / 0.149 / 0.040, chain_c_call 0.010 / 0.004 / 0.000 /
0.000, shaw_call 0.455 / 0.461 / 0.009 / 0.004 (reported: bf16 -0.0039), dwconv_call 0.472 / 0.493 / 0.003 / 0.003 (+0.0015 /
-0.0007), logits_call 0.009 / 0.011 / 0.014 / 0.008; fp16 / fp16x3: mhsa_masked_call 0.416 / 0.105 (+0.0002), kv_product_call
0.494 / 0.067 (+0.0032), kv_layernorm_call 0.479 / 0.004 (+0.0065), kv_posconv_call 0.280 / 0.040, kv_ring_call 0.440 / 0.056;
fp16 / fp32 / fp16x3: aas_conv_call 0.359 / 0.349 / 0.335, aas_prod_call 0.337 / 0.369 / 0.337, aas_valu_call 0.116 / 0.107 /
0.115, gat_call 0.081 / 0.127 / 0.127, pool_call 0.077 / 0.078 / 0.059, readout_call 0.039 / 0.040 / 0.045; the back-end on
400 identical frames (``_call_ties``, fp16 / fp32): aas_valu 0.804 / 0.827, pool 0.061 / 0.062, gat 0.066 / 0.068, readout
0.112 / 0.117, aas_conv 0.325, aas_prod 0.337 / 0.369.  No launch needed a new bound term or a kernel change; what
changed, on the CPU's evidence, is how ``pool_check`` maps rows to tied nodes (``_assign``) and the statistic below.

The bias statistic on such audio: it assumes independent elements whose error is the output store's rounding.  Duplicate
rows repeat one rounding error (a clip that is one click has 1590 copies of one conv-0 row: +0.051 ulp over 281 609
elements is the mean of that row's 177), and an element whose bound BEFORE the store exceeds an output ulp carries the fp32
value's error instead (bf16 has fp32's exponent range: GELU tails of 1e-8 .. 1e-30 are "normal" and wrong by hundreds of
ulps of one sign -- a correct kernel reads -0.39 ulp on conv 1 of a GroupNorm'd burst, and -1.05 once the diluting copies
of the silence row are taken out).  ``check(..., unique_rows=True, rounding_only=True)`` restricts the statistic to the
first of equal rows and to store-dominated elements; both default to off, the call-audio tests pass both and assert from
16 384 remaining elements on (tests/test_cpu_insitu_call.py has the figures and shows a truncating store still fails).

The single-kernel entry points at the edges of their contract (oracle/kernel_edges.py: M around every tile height, ragged
last column blocks, the narrow-store fallback, 1 / 2 / 3 / 5 K-tiles, padded strides, NaN pools around the operands and guard
patterns around the outputs; tests/test_gpu_kernel_edges.py) are judged with every constant unchanged; ``product`` gained
``act="selu"`` from ``selu`` / ``selu_err``.  Its summary on an MI355X, worst ratio fp16 / bf16 / fp16x3: edge_gemm, the lean
epilogue on every tile instance (0, 1, 2, 7, 75, 76, 77, 92) 0.498 / 0.500 / 0.051, non-lean (swish, SELU) 0.499 / 0.500 / 0.219,
narrow-store 0.499 / 0.500 / 0.272, fp32 0.170 / 0.289 / 0.304 for the three forms; edge_conv 0.056 / 0.052, fp32 0.148;
edge_convln (instances 3, 8, 82, 83) 0.485 / 0.498; edge_rownorm 0.494 / 0.499 / 0.021, fp32 0.029, the two-rows-per-wave form
0.494 / 0.499 / 0.022, fp32 0.041.  Bias (fp16 / bf16, asserted per instance and epilogue form, ``rounding_only``): every
edge_gemm class within +-0.0005 ulp over 4.0 M .. 19.5 M elements, edge_convln -0.0006 / +0.0018 (1.17 M / 1.32 M per instance),
edge_rownorm -0.0005 / +0.0009 (526 k / 571 k), two-row form -0.0008 / +0.0005 (1.16 M / 1.25 M).  No launch was found wrong.
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
# "shaw_masked" is the same launch as "shaw" under key-padding masks and shares its open item: measured +0.014 (fp16) and
# +0.175 ulp (bf16) on an MI355X.  The TRUNK attention's new classes (mhsa_masked, mhsa_long, mhsa_few, mhsa_k,
# mhsa_k_long) are asserted, against the reference that rounds P as the kernel does (``mhsa(..., bias_ref=True)``).
BIAS_REPORTED += ("shaw_masked",)
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
    if act == "selu":  # (the device's expf form: C_FN ulps of e^z through ``selu_err``, no polynomial term)
        y, e = alpha * selu(z), alpha * selu_err(z, C_ACC[dt] * s)
    else:
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


def masked_rows(lens, T):
    """The flat rows (utterance b owns rows b T .. b T + T - 1, lens[b] of them valid) a launch of a ragged batch is
    judged on, in the style of the tests' ``check_rows``: valid rows only -- rows at or past a clip's own length are
    unread by contract -- and among them every row of the first and the last utterance, the LAST valid row of every
    utterance, every valid row whose frame index mod 16 is 0 or 15 (so mod 64: 0, 15, 63 as well, the corners of the
    attention's 16-row query tiles and 64-row blocks), every 7th valid row."""
    lens = [int(n) for n in lens]
    B = len(lens)
    t = torch.arange(T)
    out = []
    for b, n in enumerate(lens):
        assert 1 <= n <= T, (n, T)
        m = (t % 16 == 0) | (t % 16 == 15) | (t == n - 1) | ((b * T + t) % 7 == 0)
        if b == 0 or b == B - 1:
            m = m | True
        out.append(b * T + t[m & (t < n)])
    return torch.cat(out)


def valid_rows(lens, T):
    """Every valid flat row of a ragged batch (lens[b] of utterance b's T rows)."""
    return torch.cat([b * T + torch.arange(int(n)) for b, n in enumerate(lens)])


def _key_mask(lens, b_i, keys, add=0):
    """(R, keys) bool: True where key j is past the own length (lens[b] + add) of the row's utterance; None without lens."""
    if lens is None:
        return None
    n = torch.as_tensor([int(v) for v in lens])[b_i] + add
    return torch.arange(keys)[None, :] >= n[:, None]


def posconv(sd, xpad, x, rows, T, dt, groups=16, lens=None):
    """Positional conv launch: x (B T, D) fp32 += GELU(conv(xpad) + bias) for the flat rows `rows`.  xpad: the operand
    copy (B, T + 128, D), frame t of utterance b at padded row t + 64; output frame t reads padded rows t .. t + 127.
    lens (ragged batch): the reference still reads xpad as tapped, whose rows 64 + lens[b] .. of utterance b must be
    exactly 0 (alone, the clip's conv would see zero padding there): asserted here."""
    if lens is not None:
        for b, n in enumerate(lens):
            assert bool((xpad[b, 64 + int(n):] == 0).all()), f"xpad: utterance {b} has nonzero rows past its {int(n)} frames"
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


ATT_CHUNK = 96  # query rows per pass of the attention references (each gathers its own (keys, H, dh) k and v in float64)


def _chunked(fn, rows):
    """fn(rows chunk) -> (ref, bound), over ATT_CHUNK rows at a time (every row's sums are its own: the same numbers)."""
    parts = [fn(rows[i:i + ATT_CHUNK]) for i in range(0, len(rows), ATT_CHUNK)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(len(parts[0])))


def mhsa(qkv, rows, T, dt, heads=16, lens=None, bias_ref=False, blocked=None):
    """Trunk self-attention launch for the flat query rows `rows`: qkv (B T, 3 D) operand values (q unscaled) -> (R, D)
    operand type.  The kernel scales the fp32 logits by dh^-0.5 and rounds P to the operand type before P.V.
    lens (ragged batch: valid frames per utterance): a query row of utterance b attends to keys < lens[b] only; the
    rows past lens[b] may hold anything (NaN included): the reference selects, it never multiplies by a mask.
    bias_ref: -> (ref, bound, pref), pref = the same output with P rounded where the kernel rounds it (``_p_rounded``; the
    reference of the rounding-bias statistic, ``check(..., bias_ref=pref)``); blocked: the kernel is the key-blocked one
    (default: T > 224, the dispatch of launch_mhsa_t; True as well under its mhsa_force_long knob)."""
    if (lens is not None or T > 256) and len(rows) > ATT_CHUNK:  # (the shapes checked before masks existed: one pass, as ever)
        return _chunked(lambda r: mhsa(qkv, r, T, dt, heads, lens, bias_ref, blocked), rows)
    D = qkv.shape[1] // 3
    dh = D // heads
    B = qkv.shape[0] // T
    x = qkv.reshape(B, T, 3, heads, dh)
    b_i, t_i = rows // T, rows % T
    q = x[b_i, t_i, 0]  # (R, H, dh)
    k = x[b_i, :, 1]  # (R, T, H, dh)
    v = x[b_i, :, 2]
    mask = _key_mask(lens, b_i, T)
    if mask is not None:
        k = torch.where(mask[:, :, None, None], torch.zeros_like(k), k)
        v = torch.where(mask[:, :, None, None], torch.zeros_like(v), v)
    s = torch.einsum("rhd,rthd->rht", q, k) * dh ** -0.5
    sa = torch.einsum("rhd,rthd->rht", q.abs(), k.abs()) * dh ** -0.5
    # fp16's absolute floor (F16_FLOOR): fp16 rounds P itself; fp16x3 up to 224 frames is the split-precision kernel, whose
    # q, k, v, P and pair-form output are UNSCALED hi / lo pairs (beyond 224 frames that mode runs the fp32 VALU attention)
    floor = "p" if dt == "fp16" else "pairs" if dt == "fp16x3" and T <= 224 else None
    extra = F16_FLOOR * (q.abs().sum(-1)[..., None] + k.abs().sum(-1).transpose(1, 2)) * dh ** -0.5 if floor == "pairs" else None
    ref, bnd = _softmax_av(s, sa, v, dt, extra=extra, mask=mask, floor=floor)
    if not bias_ref:
        return ref, bnd
    sm = s if mask is None else s.masked_fill(mask[:, None, :], -float("inf"))
    return ref, bnd, _p_rounded(sm, v, dt, 128 if (T > 224 if blocked is None else blocked) else None)


def _p_rounded(s, v, dt, block):
    """The attention output with P rounded to the operand type where the trunk kernels round it, everything else exact:
    sum_j op(P~_j) v_j / sum_j P~_j, the numerator's weights rounded, the row's sum not.  One-pass kernels (block None):
    P~ = exp(s - max over all keys).  The key-blocked kernel (block = 128 keys): P~ = exp(s - running max) per block,
    accumulator and sum rescaled by exp(old max - new max) when the maximum rises.  A correctly rounding output store
    leaves the bias statistic of got against THIS value near 0 whatever the logits: against the exact output the statistic
    also carries P's rounding, which all elements of one (utterance, head) share (bf16 -0.35 .. +0.17 ulp at 3 clips).
    s (R, H, keys) with -inf at masked keys, v (R, keys, H, dh) -> (R, H * dh)."""
    R, H, K = s.shape
    if block is None:
        p = torch.exp(s - s.amax(-1, keepdim=True))
        out = torch.einsum("rht,rthd->rhd", op(p, dt), v) / p.sum(-1)[..., None]
        return out.reshape(R, -1)
    m = torch.full((R, H), -float("inf"), dtype=torch.float64)
    l = torch.zeros(R, H, dtype=torch.float64)
    acc = torch.zeros(R, H, v.shape[-1], dtype=torch.float64)
    for j0 in range(0, K, block):
        sb = s[..., j0:j0 + block]
        mn = torch.maximum(m, sb.amax(-1))
        corr = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - mn))
        p = torch.where(torch.isinf(sb), torch.zeros_like(sb), torch.exp(sb - mn[..., None]))
        l = l * corr + p.sum(-1)
        acc = acc * corr[..., None] + torch.einsum("rht,rthd->rhd", op(p, dt), v[:, j0:j0 + block])
        m = mn
    return (acc / l[..., None]).reshape(R, -1)


# Absolute rounding floor of fp16: below 2^-14 its values are 2^-24 apart, so a rounding there errs by up to 2^-25 however
# small the value (and by at most the value itself, when it rounds to 0).  The relative terms of the attention bound (u_op per
# weight) do not cover it.  Derived from the number format, for the two places the trunk attention meets it (measured
# on lively logits and on short clips: tests/test_gpu_insitu_ragged.py):
#   "p"      fp16 operands: P~ = exp(s - max) is rounded to fp16 before P.V; a weight below 2^-14 errs by min(P~, 2^-25),
#            not by 2^-11 P~.  |d out| <= sum_j min(P~_j, 2^-25) |v_j| / sum P~.  (bf16 has fp32's exponent range.)
#   "pairs"  fp16x3, split-precision kernel: an UNSCALED hi / lo pair x = hi + lo has lo = fp16(x - hi) below 2^-14 whenever
#            |x| < 2^-3, so the pair errs by up to 2^-25 absolutely, not by 2^-22 |x|.  That holds for v (|d out| <= sum_j
#            P_j 2^-25 = 2^-25), for P~ (the term above), for the pair-form output row (2^-25) and for q and k, whose
#            floors move a logit by <= (sum_d |q_d| + sum_d |k_d|) 2^-25 dh^-0.5 (passed as `extra`).
F16_FLOOR = 2.0 ** -25


def _softmax_av(s, sa, v, dt, extra=None, mask=None, floor=None):
    """P = softmax(s) over the last axis, out = P.v (v: (R, keys, H, dh)) -> (R, H * dh) operand type and its bound: P's
    rounding (u_op per weight), the logits' accumulation (C_ACC * sa) moving P, the output's own ulp.  mask (R, keys):
    True = a key past the utterance's own length, P exactly 0 there (its k / v were zeroed by the caller).  floor: the
    absolute-floor terms of F16_FLOOR ("p", "pairs" or None)."""
    if mask is not None:
        s = s.masked_fill(mask[:, None, :], -float("inf"))
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("rht,rthd->rhd", p, v)
    pv = torch.einsum("rht,rthd->rhd", p, v.abs())
    es = C_ACC[dt] * sa + (extra if extra is not None else 0)
    # |d out| <= sum_j P_j |v_j - out| (|ds_j| + max |ds|) <= 2 max |ds| sum_j P_j (|v_j| + |out|)
    ds = es.amax(-1)[..., None]
    e = U_OP[dt] * 1.01 * pv + 2 * ds * (pv + out.abs()) + C_ACC[dt] * 16 * pv
    if floor is not None:  # (P~_j = P_j / max P; sum P~ = 1 / max P)
        e = e + torch.einsum("rht,rthd->rhd", torch.minimum(p, F16_FLOOR * p.amax(-1, keepdim=True)), v.abs())
        if floor == "pairs":
            e = e + 2 * F16_FLOOR
    R = out.shape[0]
    out, e = out.reshape(R, -1), e.reshape(R, -1)
    return out, e + ulp(out, dt)


def shaw(qkv32, rel, rows, N, dt, heads=4, lens=None):
    """Conformer Shaw attention launch for flat query rows `rows`: qkv32 (B N, 3 inner) fp32 -> (R, inner) operand type.
    logits[i, j] = q_i.k_j + q_i.E[clamp(i - j, +-512) + 512] with q scaled by dh^-0.5 before it is rounded (fp16 / bf16),
    k, v and the table rounded to the operand type.  lens (ragged batch: valid FRAMES per utterance): a query row of
    utterance b attends to the tokens < lens[b] + 1 only (the class token and its own frames)."""
    if lens is not None and len(rows) > ATT_CHUNK:
        return _chunked(lambda r: shaw(qkv32, rel, r, N, dt, heads, lens), rows)
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
    k, v = x[b_i, :, 1], x[b_i, :, 2]
    mask = _key_mask(lens, b_i, N, 1)
    if mask is not None:
        k = torch.where(mask[:, :, None, None], torch.zeros_like(k), k)
        v = torch.where(mask[:, :, None, None], torch.zeros_like(v), v)
    k, v = op(k, dt), op(v, dt)
    dist = (t_i[:, None] - torch.arange(N)[None, :]).clamp(-MAX_POS, MAX_POS) + MAX_POS  # (R, N)
    E = op(d(rel), dt)[dist]  # (R, N, dh)
    s = (torch.einsum("rhd,rthd->rht", q, k) + torch.einsum("rhd,rtd->rht", q, E)) * qs
    sa = (torch.einsum("rhd,rthd->rht", q.abs(), k.abs()) + torch.einsum("rhd,rtd->rht", q.abs(), E.abs())) * qs
    if mask is not None:
        sa = sa.masked_fill(mask[:, None, :], 0.0)
    return _softmax_av(s, sa, v, dt, mask=mask)


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


def glu_dwconv(sd, p, glu, B, N, dt, lens=None):
    """GLU -> depthwise conv (same padding) -> BatchNorm (eval) -> swish, glu (B N, 2 C2) fp32 -> (B N, C2) operand type.
    lens (ragged batch: valid FRAMES per utterance): the gated input past lens[b] + 1 tokens is zero (selected, whatever
    the rows hold), as the clip alone would see its zero padding; only the rows < lens[b] + 1 of the result mean anything."""
    a, g = glu.reshape(B, N, -1).chunk(2, dim=-1)
    h = a * torch.sigmoid(g)
    if lens is not None:
        past = torch.arange(N)[None, :] >= (torch.as_tensor([int(v) for v in lens]) + 1)[:, None]  # (B, N)
        h = torch.where(past[:, :, None], torch.zeros_like(h), h)
    h = h.transpose(1, 2)  # (B, C2, N)
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


# ---- the two ends of a forward ----------------------------------------------------------------------------------------
def final_layernorm(x, g, b, dt):
    """The trunk's final LayerNorm: ONE launch, two outputs of the same fp32 value -- the fp32 feature rows (the "ssl" tap)
    and the operand copy the back-end's first product reads ("ssl.op").  x (M, D) the last layer's fp32 rows ->
    ((ref, bound) of the fp32 output, (ref, bound) of the operand output)."""
    return layernorm(x, g, b, dt, out="f32"), layernorm(x, g, b, dt, out="op")


def conf_tokens(sd, ssl_op, B, T, dt):
    """The Conformer's tokens: the LL product (a GEMM launch, fp32 out) -> BatchNorm2d(1) (eval: one scalar scale and
    shift, folded on the host in fp32) -> SELU -> the class token at row 0 of every utterance.  ssl_op (B T, 1024)
    operand values -> (B (T + 1), E) fp32.  Bound: the product's, through one fp32 fma and the device's SELU (C_FN ulps
    of its expf: ``selu_err``); the class-token rows are copies (bound 0)."""
    z, e = product(ssl_op, sd["LL.weight"], sd["LL.bias"], dt)
    sc32 = sd["first_bn.weight"].float() / torch.sqrt(sd["first_bn.running_var"].float() + torch.tensor(BN_EPS, dtype=torch.float32))
    sh32 = sd["first_bn.bias"].float() - sd["first_bn.running_mean"].float() * sc32
    sc, sh = d(sc32).reshape(()), d(sh32).reshape(())  # (the scalars as the engine folds them: fp32)
    u = z * sc + sh
    y, ey = selu(u), selu_err(u, e * sc.abs() + F32 * ((z * sc).abs() + sh.abs()))
    E = z.shape[1]
    cls = d(sd["conformer.class_token"]).reshape(1, 1, E).expand(B, 1, E)
    ref = torch.cat([cls, y.reshape(B, T, E)], 1).reshape(B * (T + 1), E)
    bnd = torch.cat([torch.zeros(B, 1, E, dtype=torch.float64), ey.reshape(B, T, E)], 1).reshape(B * (T + 1), E)
    return ref, bnd


def conf_logits(sd, block, B, N):
    """The Conformer's classifier: fc5 on token 0 of every utterance, an fp32 fma chain per logit (64 lanes, then a wave
    sum).  block (B N, E) the last block's fp32 rows -> (B, 2)."""
    x0 = block.reshape(B, N, -1)[:, 0]
    return aas_product(x0, d(sd["conformer.fc5.weight"]), sd["conformer.fc5.bias"], False)


# ---- AASIST back-end --------------------------------------------------------------------------------------------------
# Everything after the trunk is fp32.  Images are channel-last and zero-padded, tapped whole: wd = T // 3 frames, wp = wd + 2
# pixels per padded row, img = 46 wp pixels per utterance, (B img + wp + 1) pixel rows; a conv computes every "virtual
# pixel" m < M = B img (pix = m % img, h = pix // wp, w = pix % wp, valid iff h < hout and w < wd), reads input pixels
# a_off + m + ch wp + tap and stores row m + wp + 1, zeros where m is invalid: that re-creates the border.
AAS_F, AAS_HP = 42, 46
SELU_L, SELU_A = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
C_FN = 2.0
F32 = C_ACC["fp32"]


def aas_dims(T):
    wd = T // 3
    return wd, wd + 2, AAS_HP * (wd + 2)


def aas_valid(m, T, hout):
    wd, wp, img = aas_dims(T)
    pix = m % img
    return (pix // wp < hout) & (pix % wp < wd)


def aas_rows(B, T, full=8192):
    """Virtual pixels a large image launch is checked on (all of them up to `full`): the first and last 64 of the first
    and the last utterance, every m with m mod 64 in {0, 15, 16, 63} (the corners of the 64-pixel tiles and of their
    16-row fragments), the first valid and the first invalid pixel of every image row, every 61st."""
    wd, wp, img = aas_dims(T)
    M = B * img
    m = torch.arange(M)
    if M <= full:
        return m
    pix = m % img
    k = ((m < img) | (m >= M - img)) & ((pix < 64) | (pix >= img - 64))
    k |= (pix % wp == 0) | (pix % wp == wd) | (m % 61 == 0)
    for r in (0, 15, 16, 63):
        k |= m % 64 == r
    return m[k]


def aas_border(image, B, T, hout, C):
    """Number of nonzero floats where an image must hold exact zeros: its head (the first padded row + 1 pixel) and every
    invalid virtual pixel."""
    wd, wp, img = aas_dims(T)
    x = image.reshape(-1, C)
    M = B * img
    bad = x[:wp + 1] != 0
    inv = ~aas_valid(torch.arange(M), T, hout)
    return int(bad.sum()) + int((x[wp + 1:wp + 1 + M][inv] != 0).sum())


def aas_weight(w, split):
    """The fp32 weights as a launch reads them: exact, or Wh + 2^-11 Wl rebuilt as split_f16_kernel builds the pair."""
    w32 = w.detach().to("cpu", torch.float32)
    if not split:
        return w32.double()
    hi = w32.half()
    lo = ((w32 - hi.float()) * 2048.0).half()
    return hi.double() + lo.double() / 2048.0


def pack_conv(w):
    """(cout, cin, kh, kw) -> tap-major (cout, (dh kw + dw) cin + c), the K order of the chunked products."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def bn_fold(sd, p):
    sc = d(sd[p + "weight"]) / torch.sqrt(d(sd[p + "running_var"]) + BN_EPS)
    return sc, d(sd[p + "bias"]) - d(sd[p + "running_mean"]) * sc


def selu(z):
    return SELU_L * torch.where(z > 0, z, SELU_A * torch.expm1(z))


def selu_err(z, ez):
    """Error of the device's SELU given the error ez of its argument: the derivative (the larger one within ez of the
    kink), C_FN ulps of expf's output e^z <= 1 plus the rounding of the subtraction on the negative side, two roundings
    of the result."""
    dz = SELU_L * torch.where(z > ez, torch.ones_like(z), SELU_A * torch.exp((z + ez).clamp(max=0)))
    fn = torch.where(z > ez, torch.zeros_like(z), SELU_L * SELU_A * ((C_FN + 1) * ulp(torch.exp(z.clamp(max=0)), "fp32")))
    return dz * ez + fn + 2 * ulp(selu(z), "fp32")


def aas_gather(image, C, T, rows, a_off, nch, taps):
    """(R, nch taps C): what virtual pixels `rows` read of the tapped input image (chunk ch = image row + ch)."""
    wd, wp, img = aas_dims(T)
    x = image.reshape(-1, C)
    idx = a_off + rows[:, None, None] + wp * torch.arange(nch)[None, :, None] + torch.arange(taps)[None, None, :]
    idx = idx.clamp(max=x.shape[0] - 1)  # (only invalid pixels read past the tapped rows; their reference is 0)
    return x[idx.reshape(len(rows), -1)].reshape(len(rows), -1)


def aas_product(a, w, bias, split, resid=None, bn=None, post=0, valid=None):
    """One product launch of the back-end: a (R, K) exact fp32 activations, w (N, K) fp32 weights (split: the hi / lo
    pair form), epilogue bias -> residual -> post 1 (BN -> SELU) / post 2 (SELU -> BN) -> validity mask."""
    w = aas_weight(w, split)
    ca = C_ACC["fp16x3" if split else "fp32"]
    z = a @ w.t()
    s = (a.abs().float() @ w.abs().float().t()).double()
    if bias is not None:
        z, s = z + d(bias), s + d(bias).abs()
    if resid is not None:
        z, s = z + resid, s + resid.abs()
    e = ca * s
    if post:
        sc, sh = bn
    if post == 1:
        u = z * sc + sh
        z, e = selu(u), selu_err(u, e * sc.abs() + F32 * ((z * sc).abs() + sh.abs()))
    elif post == 2:
        v, ev = selu(z), selu_err(z, e)
        z, e = v * sc + sh, ev * sc.abs() + F32 * ((v * sc).abs() + sh.abs())
    if valid is not None:
        z, e = z * valid[:, None], e * valid[:, None]
    return z, e


def aas_conv(image, w, bias, split, B, T, rows, kh, a_off, hout, resid=None, bn=None, post=0):
    """A (kh, 3) conv launch over the padded image for the virtual pixels `rows`; compare with out[rows + wp + 1]
    (`resid` is indexed like the output).  w: the reference's (cout, cin, kh, 3) weight."""
    cin = w.shape[1]
    a = aas_gather(image, cin, T, rows, a_off, kh, 3)
    return aas_product(a, pack_conv(d(w)), bias, split, resid, bn, post, aas_valid(rows, T, hout).double())


def pool_bn_selu(sd, ll, B, T):
    """ll (B T, 128) -> the one-channel padded image (B img + 3 wp + 16,): max_pool2d(3, 3) of the (128, T) map -> BN ->
    SELU at (f + 1, t + 1), exact zeros everywhere else."""
    wd, wp, img = aas_dims(T)
    m = F.max_pool2d(ll.reshape(B, T, 128).transpose(1, 2)[:, None], (3, 3))[:, 0]  # (B, 42, wd)
    sc, sh = bn_fold(sd, "first_bn.")
    u = m * sc + sh
    y, e = selu(u), selu_err(u, F32 * ((m * sc).abs() + sh.abs()))
    ref = torch.zeros(B * img + 3 * wp + 16, dtype=torch.float64)
    bnd = torch.zeros_like(ref)
    ref[:B * img].reshape(B, AAS_HP, wp)[:, 1:AAS_F + 1, 1:wd + 1] = y
    bnd[:B * img].reshape(B, AAS_HP, wp)[:, 1:AAS_F + 1, 1:wd + 1] = e
    return ref.reshape(-1, 1), bnd.reshape(-1, 1)


def first_block(sd, x1, B, T, rows):
    """Block 0's VALU kernel on the one-channel image: (Y, D) = (SELU(BN(conv1)), downsample) for virtual pixels `rows`."""
    p = "encoder.0.0."
    a = aas_gather(x1, 1, T, rows, 0, 2, 3)
    y = aas_product(a, pack_conv(d(sd[p + "conv1.weight"])), sd[p + "conv1.bias"], False, bn=bn_fold(sd, p + "bn2."), post=1,
                    valid=aas_valid(rows, T, AAS_F + 1).double())
    dn = aas_product(a[:, 3:], pack_conv(d(sd[p + "conv_downsample.weight"])), sd[p + "conv_downsample.bias"], False,
                     valid=aas_valid(rows, T, AAS_F).double())
    return y, dn


def _softmax_sum(w, x, dim, ew=0.0):
    """sum softmax(w) x over `dim` as the VALU kernels compute it (expf(w - max), a division by the sum) and its bound:
    each weight carries the relative error of expf (C_FN + 1 ulps), of the rounded difference w - max and of the logits'
    own error ew; |d out| <= 2 max(rel) sum p (|x| + |out|)."""
    p = torch.softmax(w, dim)
    out = (p * x).sum(dim, keepdim=True)
    rel = (C_FN + 1) * 2.0 ** -23 + 2.0 ** -24 * (w.amax(dim, keepdim=True) - w.amin(dim, keepdim=True)) + 2 * ew
    mag = (p * x.abs()).sum(dim, keepdim=True)
    return out.squeeze(dim), (2 * rel * (mag + out.abs()) + F32 * mag).squeeze(dim)


def att_pool(sd, x, wm, B, T):
    """x (>= B img, 64) encoder output image, wm (B img, 64) attention logits over the padded pixels ->
    (e_S (B, 42, 64) = softmax over time + pos_S, e_T (B, wd, 64) = softmax over frequency)."""
    wd, wp, img = aas_dims(T)
    v = lambda t: t.reshape(-1, 64)[:B * img].reshape(B, AAS_HP, wp, 64)[:, 1:AAS_F + 1, 1:wd + 1]
    x, wm = v(x), v(wm)
    pos = d(sd["pos_S"]).reshape(1, AAS_F, 64)
    s, es = _softmax_sum(wm, x, 2)
    t, et = _softmax_sum(wm, x, 1)
    return (s + pos, es + F32 * pos.abs()), (t, et)


def rowlin(x, w, b):
    """y = W x + b, fp32 fma chain per output."""
    return aas_product(x, d(w), b, False)


def gat(sd, p, x, n1, temp, master=None, hetero=True):
    """One graph of a gat_kernel launch.  x (B, N, DIN) the (type-projected) nodes, the first n1 of type 1;
    att[i, j] = softmax_j(tanh(W_att (x_i x_j) + b) . v_blk(i, j) / temp) with v11 / v22 inside a type and v12 across;
    y_i = SELU(BN(W1 sum_j att[i, j] x_j + b1 + W2 x_i + b2)).  With `master` ((B or 1, DIN), heterogeneous layers): also
    the master update from the SAME (pre-update) nodes, att_projM / att_weightM, no BN.  -> (y, ey)[, (m, em)]."""
    B, N, DIN = x.shape
    g = lambda k: d(sd[p + k])
    aw, ab = g("att_proj.weight"), g("att_proj.bias")
    if hetero:
        v11, v22, v12 = g("att_weight11")[:, 0], g("att_weight22")[:, 0], g("att_weight12")[:, 0]
    else:
        v11 = v22 = v12 = g("att_weight")[:, 0]
    t1 = torch.arange(N) < n1
    same = t1[:, None] == t1[None, :]
    vsel = torch.where(same[:, :, None], torch.where(t1[:, None, None], v11[None, None], v22[None, None]), v12[None, None])  # (N, N, O)

    def attend(ctr, aw, ab, v, w1, b1, w2, b2):
        """ctr (B, I, DIN) centre vectors, v (I, N, O) -> pre-activation (B, I, O) and its bound."""
        wi = ctr[:, :, None, :] * aw[None, None]  # (B, I, O, D)
        h = torch.einsum("biod,bjd->bijo", wi, x) + ab
        sh = torch.einsum("biod,bjd->bijo", wi.abs().float(), x.abs().float()).double() + ab.abs()
        th = torch.tanh(h)
        sc = (th * v).sum(-1) / temp  # (B, I, N)
        esc = (v.abs() * ((1 - th * th) * F32 * sh + C_FN * ulp(th, "fp32")) + F32 * (th * v).abs()).sum(-1) / temp
        xj = x[:, None]  # (B, 1, N, D)
        agg, ea = _softmax_sum(sc[..., None], xj, 2, esc.amax(-1)[..., None, None])  # (B, I, D)
        pre = agg @ w1.t() + b1 + ctr @ w2.t() + b2
        e = ea @ w1.abs().t() + F32 * (agg.abs() @ w1.abs().t() + b1.abs() + ctr.abs() @ w2.abs().t() + b2.abs())
        return pre, e

    w1, b1, w2, b2 = g("proj_with_att.weight"), g("proj_with_att.bias"), g("proj_without_att.weight"), g("proj_without_att.bias")
    pre, e = [], []
    for i0 in range(0, N, 64):  # (chunks of centre nodes: the (I, N, O, D) products stay small)
        a, b = attend(x[:, i0:i0 + 64], aw, ab, vsel[i0:i0 + 64], w1, b1, w2, b2)
        pre.append(a)
        e.append(b)
    pre, e = torch.cat(pre, 1), torch.cat(e, 1)
    sc, sh = bn_fold(sd, p + "bn.")
    u = pre * sc + sh
    node = (selu(u), selu_err(u, e * sc.abs() + F32 * ((pre * sc).abs() + sh.abs())))
    if master is None:
        return node
    m = master.reshape(-1, 1, DIN).expand(B, 1, DIN)
    vM = g("att_weightM")[:, 0][None, None].expand(1, N, -1)
    mo, em = attend(m, g("att_projM.weight"), g("att_projM.bias"), vM, g("proj_with_attM.weight"), g("proj_with_attM.bias"),
                    g("proj_without_attM.weight"), g("proj_without_attM.bias"))
    return node, (mo[:, 0], em[:, 0])


def _assign(dist, pb):
    """Output rows -> distinct nodes.  dist (keep, N, D) = |out_r - h_j s_j|, pb (N, D) the product's bound.  A row's
    candidates are the nodes it lies within the bound of, nearest first.  Away from ties that is one node and the result
    is the plain nearest-node search.  Silence makes nodes bit-identical (or, one launch later, equal to a few fp32 ulps):
    every copy is then nearest to the same one of them, so the rows are MATCHED to candidates, one node each (augmenting
    paths); which of several indistinguishable nodes a row came from is the kernel's to choose.  A row without a free
    candidate keeps its nearest node: a node returned twice, or a row that is no node's product, still fails."""
    keep, N, _ = dist.shape
    near = dist.amax(-1).argmin(1)
    worst = (dist / pb[None]).amax(-1)  # (keep, N)
    cand = [[j for j in torch.argsort(worst[r]).tolist()[:int((worst[r] <= 1.0).sum())]] for r in range(keep)]
    owner = {}

    def place(r, seen):
        for j in cand[r]:
            if j not in seen:
                seen.add(j)
                if j not in owner or place(owner[j], seen):
                    owner[j] = r
                    return True
        return False

    for r in sorted(range(keep), key=lambda r: len(cand[r])):
        place(r, set())
    out = near.clone()
    for j, r in owner.items():
        out[r] = j
    return out


def pool_check(h, w, b, out, keep):
    """GraphPool launch, tie-tolerant: h (B, N, D) tapped input, out (B, keep, D) tapped output.  s64 = sigmoid(w.h + b);
    delta = the derived error bound of a score.  Every output row is mapped to the node j whose h_j s64_j is nearest
    (among nodes it cannot be told apart from within the bound: to one of them each, ``_assign``);
    required: that distance within the product's bound, distinct j, and order and membership consistent with s64 up to
    the deltas of the two nodes compared.  -> check()-style dict (ratio = the worst of those requirements; margin = the
    smallest fp64 gap that decides order or membership, per launch)."""
    B, N, D = h.shape
    w, b = d(w).reshape(-1), d(b).reshape(-1)
    x = h @ w + b
    s = torch.sigmoid(x)
    delta = F32 * (h.abs() @ w.abs() + b.abs()) / 4 + C_FN * ulp(s, "fp32")  # (B, N)
    prod = h * s[..., None]
    pb = h.abs() * delta[..., None] + ulp(prod, "fp32")
    worst = dict(ratio=0.0, row=0, col=0, got=0.0, ref=0.0, bound=0.0, bias=None, n=out.numel(), margin=float("inf"))

    def note(r, row, col, got, ref, bound):
        if not r <= worst["ratio"]:
            worst.update(ratio=float(r), row=row, col=col, got=float(got), ref=float(ref), bound=float(bound))

    for u in range(B):
        dist = (out[u][:, None, :] - prod[u][None]).abs()  # (keep, N, D)
        j = _assign(dist, pb[u])  # (keep,)
        r = dist[torch.arange(keep), j] / pb[u][j]  # (keep, D)
        k = int(r.argmax())
        note(r.reshape(-1)[k], u * keep + k // D, k % D, out[u].reshape(-1)[k], prod[u][j].reshape(-1)[k], pb[u][j].reshape(-1)[k])
        if len(set(j.tolist())) != keep:
            note(float("inf"), u * keep, 0, 0.0, 0.0, 0.0)
            continue
        sj, dj = s[u][j], delta[u][j]
        if keep > 1:  # order: s64[j_r] >= s64[j_{r+1}] - delta
            r = (sj[1:] - sj[:-1]) / (dj[1:] + dj[:-1])
            k = int(r.argmax())
            note(r[k], u * keep + k, -1, sj[k + 1], sj[k], dj[k] + dj[k + 1])
            worst["margin"] = min(worst["margin"], float((sj[:-1] - sj[1:]).abs().min()))
        drop = torch.ones(N, dtype=torch.bool)
        drop[j] = False
        if bool(drop.any()):  # membership: min kept >= max dropped - delta
            kmin, dmax = int(sj.argmin()), int(torch.where(drop, s[u], torch.full_like(s[u], -1.0)).argmax())
            note((s[u][dmax] - sj[kmin]) / (delta[u][dmax] + dj[kmin]), u * keep + kmin, -2, s[u][dmax], sj[kmin], delta[u][dmax] + dj[kmin])
            worst["margin"] = min(worst["margin"], float((sj[kmin] - s[u][dmax]).abs()))
    return worst


def readout(sd, t1, ta1, s1, m1, ma1, t2, ta2, s2, sa2, m2, ma2, hidden):
    """readout_kernel: the residual adds (branch 1's spectral nodes get the literal + 1, not their second layer), the
    branch maximum, hidden = [max |T|, mean T, max |S|, mean S, master] and the logits, which the kernel computes from
    the hidden vector it stores (`hidden`: the tapped one).  Node inputs (B, n, 32), masters (B, 32)."""
    def pair(a, b, c, e):
        return torch.maximum(a + b, c + e), F32 * torch.maximum(a.abs() + b.abs(), c.abs() + e.abs())

    vt, et = pair(t1, ta1, t2, ta2)
    vs, es = pair(s1, torch.ones_like(s1), s2, sa2)
    vm, em = pair(m1, ma1, m2, ma2)
    hid = torch.cat([vt.abs().amax(1), vt.mean(1), vs.abs().amax(1), vs.mean(1), vm], 1)
    eh = torch.cat([et.amax(1), et.mean(1) + F32 * vt.abs().mean(1), es.amax(1), es.mean(1) + F32 * vs.abs().mean(1), em], 1)
    return (hid, eh), aas_product(hidden, d(sd["out_layer.weight"]), sd["out_layer.bias"], False)


AAS_FILT = [(1, 32), (32, 32), (32, 64), (64, 64), (64, 64), (64, 64)]


def aasist_walk(sd, feats, tap, split):
    """Every launch of ONE back-end forward against its reference, each built from the launch's own tapped inputs.
    feats (B, T, 1024) the forward's input, tap(name) -> the tapped buffer (flat, float64), split: the engine runs the
    split-precision products (every dtype but fp32).  -> (results, zeros): results = [(class, tap name, check() dict)],
    zeros = [(tap name, count of nonzero floats where the image must be exactly 0)].  Pools are never left out."""
    B, T, _ = feats.shape
    wd, wp, img = aas_dims(T)
    M = B * img
    res, zeros = [], []
    rows = aas_rows(B, T)
    o = rows + wp + 1

    def put(cls, name, got, rb, r=None):
        res.append((cls, name, check(got, rb[0], rb[1], None, r)))

    def image(name, C, hout):
        x = tap(name).reshape(-1, C)
        zeros.append((name, aas_border(x, B, T, hout, C)))
        return x

    ll = tap("aa.ll").reshape(B * T, 128)
    put("aas_prod", "aa.ll", ll, aas_product(d(feats).reshape(B * T, 1024), sd["LL.weight"], sd["LL.bias"], split))
    x1 = tap("aa.x1").reshape(-1, 1)
    put("aas_valu", "aa.x1", x1, pool_bn_selu(sd, ll, B, T))
    Y, D = image("aa.b0.y", 32, AAS_F + 1), image("aa.b0.d", 32, AAS_F)
    ry, rd = first_block(sd, x1, B, T, rows)
    put("aas_valu", "aa.b0.y", Y[o], ry, rows)
    put("aas_valu", "aa.b0.d", D[o], rd, rows)
    p = "encoder.0.0."
    X = image("aa.b0", 32, AAS_F)
    put("aas_conv", "aa.b0", X[o], aas_conv(Y, sd[p + "conv2.weight"], sd[p + "conv2.bias"], split, B, T, rows, 2, wp, AAS_F, D[o]), rows)
    for i in range(1, 6):
        p, (cin, cout) = f"encoder.{i}.0.", AAS_FILT[i]
        Y = image(f"aa.b{i}.y", cout, AAS_F + 1)
        put("aas_conv", f"aa.b{i}.y", Y[o], aas_conv(X, sd[p + "conv1.weight"], sd[p + "conv1.bias"], split, B, T, rows, 2, 0, AAS_F + 1,
                                                   bn=bn_fold(sd, p + "bn2."), post=1), rows)
        resid = X[o]
        if cin != cout:
            D = image(f"aa.b{i}.d", cout, AAS_F)
            put("aas_conv", f"aa.b{i}.d", D[o], aas_conv(X, sd[p + "conv_downsample.weight"], sd[p + "conv_downsample.bias"], split, B, T,
                                                       rows, 1, wp, AAS_F), rows)
            resid = D[o]
        Xn = image(f"aa.b{i}", cout, AAS_F)
        last = dict(bn=bn_fold(sd, "first_bn1."), post=1) if i == 5 else {}
        put("aas_conv", f"aa.b{i}", Xn[o], aas_conv(Y, sd[p + "conv2.weight"], sd[p + "conv2.bias"], split, B, T, rows, 2, wp, AAS_F,
                                                  resid, **last), rows)
        X = Xn
    w1, w2 = tap("aa.w1").reshape(M, 128), tap("aa.w2").reshape(M, 64)
    put("aas_prod", "aa.w1", w1[rows], aas_product(X[rows], sd["attention.0.weight"][:, :, 0, 0], sd["attention.0.bias"], split,
                                                   bn=bn_fold(sd, "attention.2."), post=2), rows)
    put("aas_prod", "aa.w2", w2[rows], aas_product(w1[rows], sd["attention.3.weight"][:, :, 0, 0], sd["attention.3.bias"], split), rows)
    eS, eT = tap("e_S").reshape(B, AAS_F, 64), tap("e_T").reshape(B, wd, 64)
    rs, rt = att_pool(sd, X, w2, B, T)
    put("aas_valu", "e_S", eS, rs)
    put("aas_valu", "e_T", eT, rt)
    gS, gT = tap("gat_S").reshape(B, AAS_F, 64), tap("gat_T").reshape(B, wd, 64)
    put("gat", "gat_S", gS, gat(sd, "GAT_layer_S.", eS, AAS_F, 2.0, hetero=False))
    put("gat", "gat_T", gT, gat(sd, "GAT_layer_T.", eT, wd, 2.0, hetero=False))
    nS, nT = AAS_F // 2, max(wd // 2, 1)
    nS1, nT1 = max(nS // 2, 1), max(nT // 2, 1)

    def pool(name, pre, h, keep):
        out = tap(name).reshape(B, keep, h.shape[2])
        res.append(("pool", name, pool_check(h, sd[pre + "proj.weight"], sd[pre + "proj.bias"], out, keep)))
        return out

    oS, oT = pool("out_S", "pool_S.", gS, nS), pool("out_T", "pool_T.", gT, nT)
    br = []
    for k in (1, 2):
        h1, h2 = f"HtrgGAT_layer_ST{k}1.", f"HtrgGAT_layer_ST{k}2."
        n = f"b{k}_"
        xp = tap(n + "xp").reshape(B, nT + nS, 64)
        put("aas_valu", n + "xp.T", xp[:, :nT].reshape(B * nT, 64), rowlin(oT.reshape(B * nT, 64), sd[h1 + "proj_type1.weight"], sd[h1 + "proj_type1.bias"]))
        put("aas_valu", n + "xp.S", xp[:, nT:].reshape(B * nS, 64), rowlin(oS.reshape(B * nS, 64), sd[h1 + "proj_type2.weight"], sd[h1 + "proj_type2.bias"]))
        (y, ey), rm = gat(sd, h1, xp, nT, 100.0, master=d(sd[f"master{k}"]))
        T1, S1, m1 = tap(n + "T1").reshape(B, nT, 32), tap(n + "S1").reshape(B, nS, 32), tap(n + "m1").reshape(B, 32)
        put("gat", n + "T1", T1, (y[:, :nT], ey[:, :nT]))
        put("gat", n + "S1", S1, (y[:, nT:], ey[:, nT:]))
        put("gat", n + "m1", m1, rm)
        S1p, T1p = pool(n + "S1p", f"pool_hS{k}.", S1, nS1), pool(n + "T1p", f"pool_hT{k}.", T1, nT1)
        xp2 = tap(n + "xp2").reshape(B, nT1 + nS1, 32)
        put("aas_valu", n + "xp2.T", xp2[:, :nT1].reshape(B * nT1, 32), rowlin(T1p.reshape(B * nT1, 32), sd[h2 + "proj_type1.weight"], sd[h2 + "proj_type1.bias"]))
        put("aas_valu", n + "xp2.S", xp2[:, nT1:].reshape(B * nS1, 32), rowlin(S1p.reshape(B * nS1, 32), sd[h2 + "proj_type2.weight"], sd[h2 + "proj_type2.bias"]))
        (y, ey), rm = gat(sd, h2, xp2, nT1, 100.0, master=m1)
        Ta, Sa, ma = tap(n + "Ta").reshape(B, nT1, 32), tap(n + "Sa").reshape(B, nS1, 32), tap(n + "ma").reshape(B, 32)
        put("gat", n + "Ta", Ta, (y[:, :nT1], ey[:, :nT1]))
        put("gat", n + "Sa", Sa, (y[:, nT1:], ey[:, nT1:]))
        put("gat", n + "ma", ma, rm)
        br.append((T1p, Ta, S1p, Sa, m1, ma))
    hidden, logits = tap("hidden").reshape(B, 160), tap("logits").reshape(B, 2)
    (a, b) = br
    rh, rl = readout(sd, a[0], a[1], a[2], a[4], a[5], b[0], b[1], b[2], b[3], b[4], b[5], hidden)
    put("readout", "hidden", hidden, rh)
    put("readout", "logits", logits, rl)
    return res, zeros


# ---- the check ---------------------------------------------------------------------------------------------------------
def check(got, ref, bound, dt=None, rows=None, bias_ref=None, unique_rows=False, rounding_only=False):
    """-> dict(ratio = max |got - ref| / bound, row (of `rows` when given), col, got / ref / bound of the worst element,
    bias = the rounding-bias statistic (None unless dt names the operand type of got), n = elements checked).
    bias_ref: the value the output store rounds, where it is known more closely than `ref` (``mhsa(..., bias_ref=True)``):
    the statistic is taken against it; the ratio always against `ref`.
    unique_rows: the statistic is taken over the DISTINCT rows of `ref` only (the first of each set of rows that are equal
    once rounded to fp32: float64 BLAS may sum two identical rows in different orders), and n = the elements of those rows
    that enter it (normal range, nonzero).  The ratio is over every row either way.
    rounding_only: the statistic leaves out the elements whose bound BEFORE the output's own rounding (`bound` minus the
    output ulp it ends with) exceeds that ulp: there the statistic reads the launch's fp32 error, not the store (GELU's
    polynomial is good to C_POLY absolutely, which at a bf16 output of 1e-12 is 1e6 ulps).  n counts what remains."""
    ref = ref.reshape(ref.shape[0], -1)
    got, bound = d(got).reshape(ref.shape), bound.reshape(ref.shape) + ulp(ref, "fp32")  # (every tap is an fp32 value)
    err = (got - ref).abs()
    r = err / bound
    r = torch.where(torch.isnan(got), torch.full_like(r, float("inf")), r)
    i = int(torch.argmax(r))
    row, col = divmod(i, ref.shape[1])
    bias, n = None, ref.numel()
    if dt is not None:
        c = ref if bias_ref is None else bias_ref.reshape(ref.shape)
        u = ulp(c, dt)
        m = (c.abs() >= 2.0 ** _EMIN[dt]) & (c != 0)
        if unique_rows:
            m = m & first_of_equal_rows(ref)[:, None]
        if rounding_only:
            m = m & (bound - ulp(ref, "fp32") <= 2 * ulp(ref, dt))
        if unique_rows or rounding_only:
            n = int(m.sum())
        if bool(m.any()):
            bias = float((torch.sign(c) * (got - c) / u)[m].mean())
    return dict(ratio=float(r.reshape(-1)[i]), row=int(rows[row]) if rows is not None else row, col=col, got=float(got[row, col]),
                ref=float(ref[row, col]), bound=float(bound[row, col]), bias=bias, n=n)


def first_of_equal_rows(x):
    """(R,) bool: True at the first of every set of rows of x (R, C) that are equal once rounded to fp32."""
    _, inv = torch.unique(x.float(), dim=0, return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), x.shape[0], dtype=torch.long).scatter_reduce(0, inv, torch.arange(x.shape[0]), "amin")
    keep = torch.zeros(x.shape[0], dtype=torch.bool)
    keep[first] = True
    return keep

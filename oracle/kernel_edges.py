"""Edge grid, guards and verdicts for the single-kernel entry points (TEST INFRASTRUCTURE, like oracle/insitu.py).

The in-place checks (oracle/insitu.py) judge every launch of a forward, so they only see the shapes a model produces; the
entry points ``afx_k_gemm``, ``afx_k_conv_gemm``, ``afx_k_conv_ln_act`` and ``afx_k_rownorm`` accept far more (any M >= 1,
N % 4 == 0, K % 64 == 0, four independent row strides; any C % 4 == 0 up to 1024).  This module holds what a test of that
wider contract needs and nothing that needs a GPU:

  * the case grid (``gemm_cases``, ``conv_cases``, ``rownorm_cases``) and the knob settings that reach each tile instance
    (``settings``, ``convln_settings``); ``share`` = the part of the grid one setting runs, ``coverage`` = which instance
    the planner really names for each of those launches (a forced tile falls back silently);
  * launches whose operands are views into NaN-filled pools and whose outputs are views into buffers pre-filled with one
    recognisable bit pattern (``gemm_launch``, ``conv_launch``, ``rownorm_launch``): a kernel that reads a column past K, a
    row past M or a frame past the last window turns NaN, one that writes outside its M x N elements changes a guard, one
    that skips an element leaves the pattern in the result;
  * the fp64 references (``insitu.product`` / ``insitu.layernorm`` and compositions of them) and ``judge``, the verdict
    of one output, with a ``Tally`` of the worst ratio and the rounding-bias statistic per class;
  * a simulated correct kernel (fp32 accumulation over 64-wide K-tiles, fp32 epilogue, round-to-nearest-even store) with
    planted defects, for tests/test_cpu_kernel_edges.py: it shows on the CPU that the bounds hold at these shapes and that
    every defect is caught, and by which criterion.

No constant is new: C_ACC, C_POLY, C_FN, BIAS_MAX are oracle/insitu.py's."""
import torch

from . import insitu as I

# ---- the grid ----------------------------------------------------------------------------------------------------------
# M: the edges of every tile height (16-row fragments; 128-row tiles; the 8-phase kernel at 160 / 192 / 224 / 256 rows)
M_EDGES = (1, 15, 16, 17, 127, 128, 129, 159, 160, 161, 191, 192, 193, 223, 224, 225, 255, 256, 257, 300)
# N: ``gemm_is_narrow`` (N <= 64, or 128 < N < 256 with N % 128 != 0) sends these to the 128x64 tile whatever the knob says
N_NARROW = (4, 8, 12, 60, 64, 132, 136, 252)
# the wide-store tiles (N % 8 == 0); 264 leaves a last 256-wide block of 8 columns
N_WIDE = (72, 120, 128, 256, 264, 272, 384, 512, 520)
# N % 8 != 0 on the non-narrow tiles: the narrow-store fallback (68: a second 64-column block of 4 columns where the automatic
# choice or the knob takes the 128x64 tile, a 128-column block of 68 elsewhere)
N_FALLBACK = (68, 260, 508, 516)
K_MAIN = 192            # 3 K-tiles, over the M x N edges
K_CORNERS = (64, 128, 320)  # 1, 2 and 5 K-tiles, on a handful of (M, N) corners
CORNER_M = (1, 17, 129, 161, 225, 257, 300)
CORNER_N = (8, 68, 136, 72, 264, 520, 260)
F32_K_MAIN, F32_K_CORNERS = 48, (16, 64, 192)  # afx_gemm_f32.hip walks K 16 at a time
F32_M = tuple(sorted(set(M_EDGES) | {31, 32, 33}))  # the same M edges, and those of a wave's 32 rows

FORMS = ("plain", "gelu", "swish", "selu", "oh")
LEAN_FORMS = ("plain", "gelu", "oh")
# form -> (bias, act, alpha, resid, out_f, out_h)
FORM_ARGS = {
    "plain": (False, None, 1.0, False, True, True),    # both outputs of one value
    "gelu": (True, "gelu", 0.5, True, True, False),    # bias + gelu, alpha 0.5, resid -> fp32
    "swish": (True, "swish", 1.0, False, False, True),  # bias + swish -> operand type
    "selu": (True, "selu", 1.0, False, True, True),    # bias + selu
    "oh": (True, None, 1.0, False, False, True),       # out_h alone
}
KNOB_DEFAULTS = {"gemm_tile": -1, "gemm_fit": 1, "gemm_ph4": 0, "gemm_map": -1, "gemm_deep": -1}
TILE_COLS = {0: 128, 1: 64, 92: 64, 2: 256, 7: 256, 75: 256, 76: 256, 77: 256, 3: 512, 8: 512, 82: 512, 83: 512}
TILE_ROWS = {0: 128, 1: 128, 92: 128, 2: 256, 7: 256, 75: 160, 76: 192, 77: 224, 3: 128, 8: 128, 82: 64, 83: 96}
INSTANCES = ("0 lean", "0 non-lean", "0 narrow-store", "1 lean", "1 non-lean", "1 narrow-store", "2", "7", "75", "76", "77", "92",
             "3", "8", "82", "83")


def is_narrow(N):
    """``gemm_is_narrow`` of afx_gemm.hip."""
    return N <= 64 or (128 < N < 256 and N % 128 != 0)


def corners():
    """The (M, N) corners the other K values go on: every corner M with two of the corner N."""
    out = []
    for i, M in enumerate(CORNER_M):
        for N in (CORNER_N[i], CORNER_N[(i + 3) % len(CORNER_N)]):
            out.append((M, N))
    return out


def gemm_cases():
    """The (M, N, K) list: K = 192 over the M x N edges, the other K values on the corners."""
    cases = [(M, N, K_MAIN) for M in M_EDGES for N in N_NARROW + N_WIDE + N_FALLBACK]
    cases += [(M, N, K) for K in K_CORNERS for M, N in corners()]
    return cases


def gemm_f32_cases():
    """The fp32 kernel (one 128-row tile family, 64 columns per workgroup at these sizes): K = 48 over the edges."""
    cases = [(M, N, F32_K_MAIN) for M in F32_M for N in N_NARROW + N_WIDE + N_FALLBACK]
    cases += [(M, N, K) for K in F32_K_CORNERS for M, N in corners()]
    return cases


def settings():
    """The knob settings that reach each instance of the plain product.  ``instance``: what a lean, wide-store, non-narrow
    launch runs under the setting; ``n``: the N kinds worth running under it ("narrow" goes to the 128x64 tile under every
    setting, so only the automatic choice and the forced 128x64 tile run it); ``forms``: the epilogue forms (the deep 128x64 tile and the 8-phase kernels
    carry the lean epilogue only -- anything else falls back to instance 0, which its own setting covers);
    ``m``: the M edges of the instance's tile height."""
    m128 = (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 300)
    S = []

    def add(name, instance, n, forms, m, **knobs):
        S.append(dict(name=name, instance=instance, n=n, forms=forms, m=m, knobs=dict(KNOB_DEFAULTS, **knobs)))

    add("auto", 92, ("wide", "fallback"), FORMS, m128, gemm_tile=-1)
    add("auto_narrow", 92, ("narrow",), FORMS, m128, gemm_tile=-1)
    add("tile0", 0, ("wide", "fallback"), FORMS, m128, gemm_tile=0)
    add("tile5", 1, ("wide", "fallback"), FORMS, m128, gemm_tile=5)
    add("tile5_narrow", 1, ("narrow",), FORMS, m128, gemm_tile=5)
    add("tile1", 2, ("wide", "fallback"), FORMS, (1, 15, 16, 17, 255, 256, 257, 300), gemm_tile=1)
    add("tile8", 92, ("wide",), LEAN_FORMS, m128, gemm_tile=8)
    for fit, inst in ((5, 75), (6, 76), (7, 77), (8, 7)):
        h = 32 * fit
        for ph4 in (0, 1, 2):
            add(f"tile3_fit{fit}_ph{ph4}", inst, ("wide",), LEAN_FORMS, (1, 15, 16, 17, h - 1, h, h + 1, 300), gemm_tile=3, gemm_fit=fit, gemm_ph4=ph4)
    for mp in (0, 1, 2):  # a handful of tiles: the XCD remap at its edge
        add(f"tile3_fit8_map{mp}", 7, ("map",), LEAN_FORMS, (1, 257, 300), gemm_tile=3, gemm_fit=8, gemm_map=mp)
        add(f"tile0_map{mp}", 0, ("map",), FORMS, (1, 257, 300), gemm_tile=0, gemm_map=mp)
    return S


F32_SETTING = dict(name="fp32", instance=None, n=("narrow", "wide", "fallback"), forms=FORMS, m=F32_M, knobs=dict(KNOB_DEFAULTS))


def convln_settings():
    """Fused conv + LayerNorm + GELU: ``gemm_deep`` 0 = the 2-stage row-complete tile (instance 3), 2 = the 8-phase one at the
    height ``gemm_fit`` 12 / 13 / 14 forces (82 / 83 / 8), and both ``gemm_ph4`` forms of 8."""
    S = [dict(name="deep0", instance=3, knobs=dict(KNOB_DEFAULTS, gemm_deep=0))]
    for fit, inst in ((12, 82), (13, 83), (14, 8)):
        S.append(dict(name=f"deep2_fit{fit}", instance=inst, knobs=dict(KNOB_DEFAULTS, gemm_deep=2, gemm_fit=fit)))
    S.append(dict(name="deep2_fit14_ph1", instance=8, knobs=dict(KNOB_DEFAULTS, gemm_deep=2, gemm_fit=14, gemm_ph4=1)))
    return S


def n_kind(N):
    return "narrow" if is_narrow(N) else ("wide" if N % 8 == 0 else "fallback")


def share(setting, cases=None):
    """-> [(case, form, packed)]: what one setting runs of the grid.  The corner cases (K != 192) run every form of the
    setting; a K = 192 case runs two forms in rotation (over the M edges every N meets every form, and the reverse); one
    launch in 16 uses packed strides, every other padded ones."""
    cases = gemm_cases() if cases is None else cases
    forms, out, j = setting["forms"], [], 0
    cm = {c[:2] for c in cases if c[2] != K_MAIN and c[2] != F32_K_MAIN}
    for (M, N, K) in cases:
        corner = K not in (K_MAIN, F32_K_MAIN)
        if "map" in setting["n"]:
            if not (M in setting["m"] and N in (264, 512, 520) and not corner):
                continue
        elif n_kind(N) not in setting["n"] or not (corner or M in setting["m"] or (M, N) in cm):
            continue
        i = M_EDGES.index(M) if M in M_EDGES else F32_M.index(M)
        r = i + (N_NARROW + N_WIDE + N_FALLBACK).index(N)
        take = forms if corner else tuple(dict.fromkeys((forms[r % len(forms)], forms[(r + 2) % len(forms)])))
        for f in take:
            out.append(((M, N, K), f, j % 16 == 0))
            j += 1
    return out


def names_instance(case, form):
    """True for the launches that run on the instance a setting names: a lean form with wide stores (everything else may
    fall back to the general tiles)."""
    return case[1] % 8 == 0 and form in LEAN_FORMS


def epilogue_of(form, N, dt="fp16"):
    """The epilogue form a launch takes: narrow-store where N % 8 != 0, else lean (no activation or GELU) or non-lean."""
    if N % 8:
        return "narrow-store"
    return "lean" if FORM_ARGS[form][1] in (None, "gelu") else "non-lean"


def label(tile, form, N):
    """Instance label of a launch (INSTANCES): the two general tiles split by epilogue form."""
    return f"{tile} {epilogue_of(form, N)}" if tile in (0, 1) else str(tile)


def plan_flags(form, dt="fp16", ln=False):
    """The ``flags`` of ``afx_gemm_plan`` for a launch: 1 fused LayerNorm, 2 split precision, 4 a non-lean activation."""
    return (1 if ln else 0) | (2 if dt == "fp16x3" else 0) | (4 if FORM_ARGS.get(form, (0, None))[1] in ("swish", "selu") else 0)


def coverage(plan_fn, dt="fp16"):
    """The table instance label -> [(setting, (M, N, K), form)], every launch counted for the instance the planner NAMES
    under its setting.  plan_fn(knobs, M, N, K, rpb, flags) -> instance (``afx_gemm_plan``'s out[1] with the knobs set)."""
    table = {}
    for s in settings():
        for (M, N, K), form, _packed in share(s):
            tile = plan_fn(s["knobs"], M, N, K, 0, plan_flags(form, dt))
            table.setdefault(label(tile, form, N), []).append((s["name"], (M, N, K), form))
    for s in convln_settings():
        for c in conv_cases(ln=True):
            M, K = c["B"] * c["Tout"], c["k"] * c["Cin"]
            tile = plan_fn(s["knobs"], M, 512, K, c["Tout"], plan_flags("gelu", dt, ln=True))
            table.setdefault(str(tile), []).append((s["name"], (M, 512, K), "convln"))
    return table


def coverage_gaps(table):
    """What the grid lacks, per instance of INSTANCES: a ragged M tail, M smaller than a fragment, a ragged last column block
    (every instance but the row-complete ones admits one), 1, 2, 3 and >= 4 K-tiles.  [] = the condition holds."""
    gaps = []
    for inst in INSTANCES:
        rows = table.get(inst, [])
        tile = int(inst.split()[0])
        ms, ns, ks = {c[0] for _, c, _ in rows}, {c[1] for _, c, _ in rows}, {c[2] // 64 for _, c, _ in rows}
        if not any(M % TILE_ROWS[tile] for M in ms):
            gaps.append((inst, "ragged M tail"))
        if not any(M < 16 for M in ms):
            gaps.append((inst, "M < 16"))
        if TILE_COLS[tile] != 512 and not any(N % TILE_COLS[tile] for N in ns):
            gaps.append((inst, "ragged last column block"))
        for kt in (1, 2, 3):
            if kt not in ks:
                gaps.append((inst, f"{kt} K-tiles"))
        if not any(k >= 4 for k in ks):
            gaps.append((inst, ">= 4 K-tiles"))
    return gaps


CONV_BT = ((1, 1), (5, 1), (3, 43), (2, 64), (7, 37))  # rows per batch < M: tiles straddle batches
CONV_KSC = ((3, 2, 64), (3, 2, 512), (2, 2, 32), (2, 2, 64), (2, 2, 512))  # (k, s, Cin): K = 192, 1536, 64, 128, 1024
CONV_N = (8, 68, 136, 72, 264, 260, 512, 520)


def conv_cases(ln=False):
    """Conv-as-GEMM cases: Tin = s (Tout - 1) + k + 1, so (Tin - k) % s = 1 and every batch ends in a frame no window reads."""
    out, j = [], 0
    for B, Tout in CONV_BT:
        for k, s, Cin in CONV_KSC:
            for N in ((512,) if ln else (CONV_N[j % len(CONV_N)], CONV_N[(j + 3) % len(CONV_N)])):
                out.append(dict(B=B, Tout=Tout, Tin=s * (Tout - 1) + k + 1, k=k, s=s, Cin=Cin, N=N))
            j += 1
    return out


ROWNORM_C = (4, 8, 60, 252, 256, 260, 1020, 1024)
ROWNORM_ROWS = (1, 3, 4, 5, 37)            # one row per wave (four waves per workgroup)
ROWNORM_ROWS2 = (16384, 16385, 16391)      # two rows per wave from 16 384 rows on
ROWNORM_C2 = (8, 260)
ACTS = (None, "gelu", "swish", "selu")


def rownorm_cases():
    return [(r, C) for C in ROWNORM_C for r in ROWNORM_ROWS], [(r, C) for C in ROWNORM_C2 for r in ROWNORM_ROWS2]


def rownorm_rows(rows):
    """The rows a large launch is compared on (all of them up to 4096): both ends and every 61st (the guards and the
    unstored-element check still see the whole buffer)."""
    r = torch.arange(rows)
    return r if rows <= 4096 else r[(r < 64) | (r >= rows - 64) | (r % 61 == 0)]


# ---- pools and guards --------------------------------------------------------------------------------------------------
TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32, "fp16x3": torch.float32}
_INT = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
PATTERN = {torch.float32: 0x7FC5A5A5, torch.float16: 0x7E5A, torch.bfloat16: 0x7FA5}  # NaNs no arithmetic produces
GUARD_ROWS = 2


def pool(data, ld=None, extra=2, device="cpu"):
    """data (R, C) -> (buffer (R + extra, ld) with NaN everywhere else, view [:R, :C])."""
    R, C = data.shape
    ld = C if ld is None else ld
    buf = torch.full((R + extra, ld), float("nan"), dtype=data.dtype)
    buf[:R, :C] = data
    buf = buf.to(device)
    return buf, buf[:R, :C]


class Guarded:
    """An output (R, C) as a view into a (R + 4, ld) buffer pre-filled with PATTERN: two guard rows before and after, guard
    columns C .. ld - 1 of every row; the M x N elements themselves hold the pattern too until the kernel writes them."""

    def __init__(self, R, C, ld, dtype, device="cpu"):
        self.R, self.C, self.ld, self.dtype = R, C, ld, dtype
        b = torch.empty((R + 2 * GUARD_ROWS, ld), dtype=dtype)
        b.view(_INT[dtype]).fill_(PATTERN[dtype])
        self.buf = b.to(device)
        self.view = self.buf[GUARD_ROWS:GUARD_ROWS + R, :C]

    def read(self):
        """-> (result (R, C) on the CPU, elements still holding the pattern, guard elements changed)."""
        b = self.buf.cpu()
        pat = b.view(_INT[self.dtype]) == PATTERN[self.dtype]
        inner = torch.zeros_like(pat)
        inner[GUARD_ROWS:GUARD_ROWS + self.R, :self.C] = True
        return b[GUARD_ROWS:GUARD_ROWS + self.R, :self.C], int((pat & inner).sum()), int((~pat & ~inner).sum())


def round8(n):
    return (n + 7) // 8 * 8


class Launch:
    """One launch: operands (views into NaN pools), outputs (Guarded or None), and the CPU copies the reference reads."""


def gemm_launch(case, form, dt, packed=False, device="cpu", seed=0):
    """Operands and outputs of one ``afx_k_gemm`` launch.  Padded strides differ from the packed value for every one of lda,
    ldw, ldr, ldo_f, ldo_h and keep rows 16-byte aligned (multiples of 8 elements for the half types, of 4 for fp32); the
    fp16x3 test hook demands packed operand rows and gets guards on the outputs only."""
    M, N, K = case
    has_bias, act, alpha, has_r, of, oh = FORM_ARGS[form]
    g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)
    tdt = TORCH_DT[dt]
    A = torch.randn(M, K, generator=g).to(tdt)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(tdt)
    L = Launch()
    L.case, L.form, L.dt, L.packed, L.act, L.alpha = case, form, dt, packed, act, alpha
    half = dt in I.HALF
    q = 8 if half else 4
    pk = packed or dt == "fp16x3"
    L.a64, L.w64 = I.d(A), W.float()
    L.Abuf, L.A = pool(A, K if pk else K + q, 0 if dt == "fp16x3" else 2, device)
    L.Wbuf, L.W = pool(W, K if pk else K + 2 * q, 0 if dt == "fp16x3" else 2, device)
    L.bias = L.resid = L.bias_cpu = L.resid64 = None
    if has_bias:
        L.bias_cpu = torch.randn(N, generator=g)
        L.bias = L.bias_cpu.to(device)
    if has_r:
        r = torch.randn(M, N, generator=g)
        L.resid64 = I.d(r)
        L.Rbuf, L.resid = pool(r, N if packed else N + 12, 2, device)
    L.out_f = Guarded(M, N, N if packed else N + 8, torch.float32, device) if of else None
    L.out_h = Guarded(M, N, N if packed else (round8(N) + 16 if half else N + 16), tdt, device) if oh else None
    return L


def gemm_refs(L):
    """-> {"f": (ref, bound), "h": (ref, bound)} for the outputs the launch has."""
    out = {}
    for key, buf, o in (("f", L.out_f, "f32"), ("h", L.out_h, "op")):
        if buf is not None:
            out[key] = I.product(L.a64, L.w64, L.bias_cpu, L.dt, act=L.act, alpha=L.alpha, resid=L.resid64, out=o)
    return out


def conv_rows(x, k, s, Tout):
    """x (B, Tin, Cin) -> (B Tout, k Cin): the k input frames of every output row, tap-major (K = tap Cin + channel)."""
    B, _Tin, Cin = x.shape
    t = s * torch.arange(Tout)[:, None] + torch.arange(k)[None, :]
    return x[:, t].reshape(B * Tout, k * Cin)


def conv_launch(c, dt, ln=False, device="cpu", seed=0, out_h=True, out_f=True):
    """One ``afx_k_conv_gemm`` (ln False: bias, fp32 out) or ``afx_k_conv_ln_act`` (GELU, both outputs) launch.  The entry
    points take packed tensors, so the guards are the unread last frame of every batch (NaN), NaN rows after the weights,
    and the guard rows around the outputs."""
    B, Tout, Tin, k, s, Cin, N = (c[n] for n in ("B", "Tout", "Tin", "k", "s", "Cin", "N"))
    g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + Tout * 131 + Cin * 7 + k + N)
    tdt = TORCH_DT[dt]
    x = torch.randn(B, Tin, Cin, generator=g).to(tdt)
    assert s * (Tout - 1) + k < Tin
    x[:, s * (Tout - 1) + k:] = float("nan")  # frames no window reads
    W = (torch.randn(N, k * Cin, generator=g) / (k * Cin) ** 0.5).to(tdt)
    L = Launch()
    L.case, L.dt, L.ln, L.c = (B * Tout, N, k * Cin), dt, ln, c
    L.x = x.to(device)
    L.a64 = I.d(conv_rows(x, k, s, Tout))
    L.w64 = W.float()
    L.Wbuf, L.W = pool(W, k * Cin, 2, device)
    L.bias_cpu = torch.randn(N, generator=g)
    L.bias = L.bias_cpu.to(device)
    if ln:
        L.gamma_cpu, L.beta_cpu = 1 + 0.2 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g)
        L.gamma, L.beta = L.gamma_cpu.to(device), L.beta_cpu.to(device)
    L.out_f = Guarded(B * Tout, N, N, torch.float32, device) if out_f else None
    L.out_h = Guarded(B * Tout, N, N, tdt, device) if (ln and out_h) else None
    return L


def convln_ref(a, w, bias, gamma, beta, dt, out):
    """conv + bias -> LayerNorm -> GELU, the composition of ``insitu.conv_layer`` on explicit operands."""
    z, s = I.linear(a, w, bias, dt)
    y, e = I.layernorm(z, gamma, beta, dt, out="f32", acc=I.C_ACC[dt] * s)
    g, e = I.gelu(y), I.dgelu(y) * e + I.C_POLY * (1 + y.abs())
    return (g, e + I.ulp(g, dt)) if out == "op" else (g, e)


def conv_refs(L):
    if not L.ln:
        return {"f": I.product(L.a64, L.w64, L.bias_cpu, L.dt)}
    out = {}
    for key, buf, o in (("f", L.out_f, "f32"), ("h", L.out_h, "op")):
        if buf is not None:
            out[key] = convln_ref(L.a64, L.w64, L.bias_cpu, L.gamma_cpu, L.beta_cpu, L.dt, o)
    return out


def rownorm_launch(rows, C, dt, act, packed=False, device="cpu", seed=0, x=None):
    """One ``afx_k_rownorm`` launch, both outputs: x (rows, C) fp32 in a pool of row stride ldx whose columns C .. ldx - 1
    are NaN; padded ldx / ldo_f / ldo_h all differ from C."""
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 31 + C)
    if x is None:
        x = torch.randn(rows, C, generator=g) * (0.5 + torch.rand(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)
    L = Launch()
    L.case, L.dt, L.act, L.packed = (rows, C), dt, act, packed
    L.x_cpu = x
    L.Xbuf, L.x = pool(x, C if packed else C + 4, 2, device)
    L.gamma_cpu, L.beta_cpu = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    L.gamma, L.beta = L.gamma_cpu.to(device), L.beta_cpu.to(device)
    tdt = TORCH_DT[dt]
    L.out_f = Guarded(rows, C, C if packed else C + 8, torch.float32, device)
    L.out_h = Guarded(rows, C, C if packed else C + (16 if dt in I.HALF else 12), tdt, device)
    return L


def rownorm_ref(x, gamma, beta, dt, act, out):
    """Row LayerNorm + activation: ``insitu.layernorm`` (fp32 out), the activation's derivative and its own error term,
    then the output's ulp."""
    y, e = I.layernorm(I.d(x), gamma, beta, dt, out="f32")
    if act == "gelu":
        y, e = I.gelu(y), I.dgelu(y) * e + I.C_POLY * (1 + y.abs())
    elif act == "swish":
        y, e = I.swish(y), I.dswish(y) * e + I.C_POLY * (1 + y.abs())
    elif act == "selu":
        y, e = I.selu(y), I.selu_err(y, e)
    return (y, e + I.ulp(y, dt)) if out == "op" else (y, e)


def rownorm_refs(L, rows=None):
    x = L.x_cpu if rows is None else L.x_cpu[rows]
    return {"f": rownorm_ref(x, L.gamma_cpu, L.beta_cpu, L.dt, L.act, "f32"),
            "h": rownorm_ref(x, L.gamma_cpu, L.beta_cpu, L.dt, L.act, "op")}


# ---- the verdict -------------------------------------------------------------------------------------------------------
BIAS_MIN_N = 16384  # the rounding-bias statistic is asserted from this many elements on (tests/test_gpu_insitu_call.py's threshold)


def judge(out, ref, bound, dt=None, rows=None):
    """The outcome of one output of one launch.  out: its ``Guarded`` buffer; (ref, bound): the fp64 reference; dt: the
    operand type when the output is a rounded one (then the rounding-bias statistic is taken, over store-dominated
    elements: ``rounding_only``); rows: the row subset the reference covers.  -> dict(verdict, ratio, unstored, overwritten,
    nan, bias, n).  verdict, first that applies: "unstored" the guard pattern shows in the result, "guard" a guard element
    changed, "nan" NaN anywhere in the result, "ratio" |got - ref| > bound somewhere, else "ok"."""
    got, unstored, overwritten = out.read()
    nan = int(torch.isnan(got).sum()) - unstored
    g = got if rows is None else got[rows]
    res = I.check(g, ref, bound, dt if dt in I.HALF else None, rounding_only=True)
    verdict = "unstored" if unstored else "guard" if overwritten else "nan" if nan else "ratio" if not res["ratio"] <= 1.0 else "ok"
    return dict(res, verdict=verdict, unstored=unstored, overwritten=overwritten, nan=nan)


class Tally:
    """Worst ratio, verdicts and the rounding-bias sum per class (instance / launch class, dtype, epilogue form)."""

    def __init__(self):
        self.c = {}

    def add(self, cls, dt, v, what=None):
        t = self.c.setdefault((cls, dt), dict(ratio=0.0, bsum=0.0, n=0, launches=0, bad=[]))
        t["launches"] += 1
        t["ratio"] = max(t["ratio"], v["ratio"]) if v["ratio"] == v["ratio"] else float("inf")
        if v["bias"] is not None:
            t["bsum"] += v["bias"] * v["n"]
            t["n"] += v["n"]
        if v["verdict"] != "ok":
            t["bad"].append((what, v["verdict"], v["ratio"], v["row"], v["col"], v["got"], v["ref"], v["bound"]))

    def merge(self, other):
        for key, o in other.c.items():
            t = self.c.setdefault(key, dict(ratio=0.0, bsum=0.0, n=0, launches=0, bad=[]))
            t["ratio"] = max(t["ratio"], o["ratio"])
            t["bsum"] += o["bsum"]
            t["n"] += o["n"]
            t["launches"] += o["launches"]
            t["bad"] += o["bad"]

    def bias(self, key):
        t = self.c[key]
        return t["bsum"] / t["n"] if t["n"] else None

    def failures(self):
        """Every launch whose verdict is not "ok", and every class of >= BIAS_MIN_N elements whose bias leaves BIAS_MAX."""
        bad = [(key, b) for key, t in self.c.items() for b in t["bad"]]
        for key, t in self.c.items():
            if t["n"] >= BIAS_MIN_N and abs(t["bsum"] / t["n"]) > I.BIAS_MAX:
                bad.append((key, ("bias", t["bsum"] / t["n"], t["n"])))
        return bad

    def lines(self):
        out = []
        for (cls, dt), t in sorted(self.c.items()):
            b = f"  bias {t['bsum'] / t['n']:+.4f} over {t['n']} elements" + ("" if t["n"] >= BIAS_MIN_N else " (reported)") if t["n"] else ""
            out.append(f"  {cls:28s} {dt:7s} ratio {t['ratio']:.3f}  launches {t['launches']}{b}")
        return out


# ---- the simulated kernel and its planted defects ----------------------------------------------------------------------
def truncate(x32, tdt):
    """fp32 -> tdt rounded TOWARD ZERO (the planted truncating store)."""
    h = x32.to(tdt)
    over = h.float().abs() > x32.abs()
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(tdt)


def _act32(v, act):
    if act == "gelu":
        return torch.nn.functional.gelu(v)
    if act == "swish":
        return v * torch.sigmoid(v)
    if act == "selu":
        return torch.nn.functional.selu(v)
    return v


def sim_acc(A, W, defect=None):
    """fp32 accumulation over 64-wide K-tiles of the operand values."""
    M, K = A.shape
    acc = torch.zeros(M, W.shape[0], dtype=torch.float32)
    kend = K - 64 if defect == "drop_k_tile" else K
    for k0 in range(0, kend, 64):
        a = A[:, k0:k0 + 64].float()
        if defect == "drop_k_last" and k0 + 64 == K:
            a = a.clone()
            a[:, -1] = 0
        acc += a @ W[:, k0:k0 + 64].float().t()
    return acc


def _store(out, v, defect, tdt_trunc=False):
    """Write v (M, N) fp32 into a Guarded output, with the store defects."""
    M, N = v.shape
    val = truncate(v, out.dtype) if (defect == "trunc" and out.dtype != torch.float32) else v.to(out.dtype)
    if defect == "skip_last_group":
        out.view[:, :N - 4] = val[:, :N - 4]
        return
    out.view[:] = val
    if defect == "store_past_n":
        out.buf[GUARD_ROWS, N] = 1.0
    if defect == "store_past_m":
        out.buf[GUARD_ROWS + M, 0] = 1.0


def sim_gemm(L, defect=None):
    """The simulated ``afx_k_gemm`` on a CPU launch: correct (defect None) or with one planted defect."""
    M, N, K = L.case
    A = torch.as_strided(L.Abuf, (M, K), (K, 1)) if defect == "lda_as_k" else L.A
    v = sim_acc(A, L.W, defect)
    if L.bias is not None:
        b = L.bias
        if defect == "bias_shift":  # the bias vector shifted by 4 columns in the last 128-column block
            n0 = (N - 1) // 128 * 128
            b = b.clone()
            b[n0 + 4:] = L.bias[n0:N - 4]
        v = v + b
    v = _act32(v, L.act) * torch.tensor(L.alpha, dtype=torch.float32)
    if L.resid is not None:
        v = v + L.resid
    if defect == "row_scale":  # the last row of the ragged tile
        v[M - 1] *= 1 + 2.0 ** -9
    for out in (L.out_f, L.out_h):
        if out is not None:
            _store(out, v, defect)


def sim_conv(L, defect=None, tile=128):
    """The simulated conv launch (plain or fused LayerNorm + GELU).  "batch_off_by_one": a batch that starts inside a row
    tile takes its first row from the batch before."""
    c = L.c
    a = conv_rows(L.x, c["k"], c["s"], c["Tout"])
    if defect == "batch_off_by_one":
        m = torch.arange(a.shape[0])
        wrong = (m % c["Tout"] == 0) & (m % tile != 0)
        a = torch.where(wrong[:, None], a[(m - c["Tout"]).clamp(min=0)], a)
    v = sim_acc(a, L.W, defect) + L.bias
    if L.ln:
        mu = v.mean(1, keepdim=True)
        xc = v - mu
        v = xc * torch.rsqrt((xc * xc).mean(1, keepdim=True) + torch.tensor(1e-5)) * L.gamma + L.beta
        v = torch.nn.functional.gelu(v)
    for out in (L.out_f, L.out_h):
        if out is not None:
            _store(out, v, defect)


def sim_rownorm(L, defect=None):
    """The simulated row LayerNorm.  "stats_1024": the statistics divide by 1024 columns whatever C is."""
    x = L.x.float()
    C = 1024 if defect == "stats_1024" else x.shape[1]
    mu = x.sum(1, keepdim=True) / C
    xc = x - mu
    var = (xc * xc).sum(1, keepdim=True) / C
    v = _act32(xc * torch.rsqrt(var + torch.tensor(1e-5)) * L.gamma + L.beta, L.act)
    for out in (L.out_f, L.out_h):
        _store(out, v, defect)

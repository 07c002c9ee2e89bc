"""CPU-only: the edge grid of the single-kernel entry points (oracle/kernel_edges.py) before it meets a GPU.

  * a simulated correct kernel (fp32 accumulation over 64-wide K-tiles, fp32 epilogue, round-to-nearest-even store) passes
    the whole grid inside the bounds of oracle/insitu.py, with the rounding-bias statistic inside BIAS_MAX, in fp16 and bf16
    and for every epilogue form the GPU tests use: no constant has to move for these shapes;
  * every planted defect fails, by the criterion named beside it -- a truncating store by the bias statistic ALONE (its ratio
    stays below 1: neither the per-element bound nor the older flat tolerances see it);
  * the coverage condition: under the knob settings of the grid, the planner (``afx_gemm_plan``, host arithmetic) names every
    tile instance for a ragged M tail, an M smaller than a fragment, a ragged last column block and 1, 2, 3 and >= 4 K-tiles,
    so that a silent fallback cannot turn a GPU test into a second test of instance 0;
  * the alignment contract of ``afx_k_gemm`` / ``afx_k_rownorm`` (include/afx.h): violations are refused on the host, with
    nothing launched (the refusals return before the first device call, so they run here)."""
import ctypes as C

import pytest
import torch

from oracle import insitu as I
from oracle import kernel_edges as E

HALF = ("fp16", "bf16")


def run_gemm(case, form, dt, defect=None, packed=False):
    L = E.gemm_launch(case, form, dt, packed)
    E.sim_gemm(L, defect)
    refs = E.gemm_refs(L)
    out = {}
    if "f" in refs:
        out["f"] = E.judge(L.out_f, *refs["f"])
    if "h" in refs:
        out["h"] = E.judge(L.out_h, *refs["h"], dt=dt)
    return out


@pytest.mark.parametrize("dt", HALF)
def test_simulated_correct_kernel_passes_the_whole_grid(dt):
    """Every (case, form) any setting runs, once: ratio <= 1, no guard verdict, bias inside BIAS_MAX per epilogue form.
    Measured here: worst ratio 0.498 (fp16) / 0.500 (bf16) -- the output's own half-ulp rounding -- and |bias| < 0.001."""
    todo = {}
    for s in E.settings():
        for case, form, packed in E.share(s):
            todo.setdefault((case, form), packed)
    t = E.Tally()
    for (case, form), packed in todo.items():
        for key, v in run_gemm(case, form, dt, packed=packed).items():
            t.add(f"sim_gemm {E.epilogue_of(form, case[1])} {key}", dt, v, (case, form))
    for c, ln in [(c, False) for c in E.conv_cases()] + [(c, True) for c in E.conv_cases(ln=True)]:
        L = E.conv_launch(c, dt, ln=ln)
        E.sim_conv(L)
        refs = E.conv_refs(L)
        for key in refs:
            t.add("sim_convln" if ln else "sim_conv", dt, E.judge(L.out_f if key == "f" else L.out_h, *refs[key], dt=dt if key == "h" else None), c)
    small, large = E.rownorm_cases()
    for rows, Cc in small + [(16385, 8)]:
        for act in E.ACTS:
            L = E.rownorm_launch(rows, Cc, dt, act)
            E.sim_rownorm(L)
            sub = E.rownorm_rows(rows)
            refs = E.rownorm_refs(L, None if len(sub) == rows else sub)
            for key in refs:
                t.add("sim_rownorm", dt, E.judge(L.out_f if key == "f" else L.out_h, *refs[key], dt=dt if key == "h" else None,
                                                 rows=None if len(sub) == rows else sub), (rows, Cc, act))
    print("\n".join(t.lines()))
    assert not t.failures(), t.failures()[:5]
    worst = max(v["ratio"] for v in t.c.values())
    assert worst <= 0.51, worst  # (the half-ulp rounding of the output itself; the rest is far below)
    asserted = [k for k, v in t.c.items() if v["n"] >= E.BIAS_MIN_N]
    assert {"sim_gemm lean h", "sim_gemm non-lean h", "sim_gemm narrow-store h", "sim_convln", "sim_rownorm"} <= {k[0] for k in asserted}


# (defect, epilogue form, case, the verdict that must catch it); every launch uses padded strides
GEMM_DEFECTS = [
    ("drop_k_last", "plain", (129, 264, 192), "ratio"),
    ("drop_k_tile", "plain", (129, 264, 192), "ratio"),
    ("row_scale", "plain", (129, 264, 192), "ratio"),
    ("bias_shift", "oh", (129, 264, 192), "ratio"),
    ("skip_last_group", "selu", (17, 260, 192), "unstored"),
    ("store_past_n", "plain", (129, 264, 192), "guard"),
    ("store_past_m", "plain", (129, 264, 192), "guard"),
    ("lda_as_k", "plain", (129, 264, 192), "nan"),
]


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("defect,form,case,by", GEMM_DEFECTS)
def test_planted_gemm_defects_fail_by_their_criterion(dt, defect, form, case, by):
    good = run_gemm(case, form, dt)
    assert all(v["verdict"] == "ok" for v in good.values()), good
    bad = run_gemm(case, form, dt, defect)
    verdicts = {v["verdict"] for v in bad.values()}
    assert by in verdicts and verdicts <= {by, "ok"}, (defect, bad)


@pytest.mark.parametrize("dt", HALF)
def test_truncating_store_is_caught_by_the_bias_statistic_alone(dt):
    """The point of the statistic: a store that rounds toward zero stays inside the per-element bound (an ulp) on every
    element of every case, and reads -0.5 ulp of bias against BIAS_MAX = 0.05."""
    t = E.Tally()
    for case in ((129, 264, 192), (17, 260, 192), (300, 520, 64), (257, 68, 320)):
        for form in ("plain", "swish", "oh"):
            v = run_gemm(case, form, dt, "trunc")["h"]
            assert v["verdict"] == "ok" and v["ratio"] < 1.0, v  # no other criterion sees it
            t.add("trunc", dt, v)
    (key, (what, bias, n)), = t.failures()
    assert what == "bias" and n >= E.BIAS_MIN_N and -0.52 < bias < -0.45, (bias, n)


@pytest.mark.parametrize("dt", HALF)
def test_planted_conv_and_layernorm_defects_fail_by_ratio(dt):
    c = dict(B=3, Tout=43, Tin=2 * 42 + 3 + 1, k=3, s=2, Cin=64, N=72)  # batches start at rows 43 and 86: inside the first tile
    for ln in (False, True):
        c = dict(c, N=512) if ln else c
        for defect, want in ((None, "ok"), ("batch_off_by_one", "ratio"), ("drop_k_tile", "ratio")):
            L = E.conv_launch(c, dt, ln=ln)
            E.sim_conv(L, defect)
            v = E.judge(L.out_f, *E.conv_refs(L)["f"])
            assert v["verdict"] == want, (ln, defect, v)
    for defect, want in ((None, "ok"), ("stats_1024", "ratio")):  # statistics over 1024 columns when C = 1020
        L = E.rownorm_launch(5, 1020, dt, None)
        E.sim_rownorm(L, defect)
        refs = E.rownorm_refs(L)
        assert E.judge(L.out_f, *refs["f"])["verdict"] == want and E.judge(L.out_h, *refs["h"], dt=dt)["verdict"] == want


def test_selu_product_reference():
    """``insitu.product(act="selu")``: the value is SELU of the pre-activation, the bound is ``selu_err``'s (C_FN ulps of e^z on
    the negative side) and scales with alpha."""
    g = torch.Generator().manual_seed(3)
    a, w, b = I.d(torch.randn(9, 64, generator=g).half()), torch.randn(8, 64, generator=g) / 8, torch.randn(8, generator=g)
    z, e0 = I.product(a, w, b, "fp16")
    y, e = I.product(a, w, b, "fp16", act="selu")
    assert torch.equal(y, I.selu(z)) and torch.equal(e, I.selu_err(z, e0))
    y2, e2 = I.product(a, w, b, "fp16", act="selu", alpha=0.5)
    assert torch.allclose(y2, 0.5 * y, rtol=0, atol=0) and torch.allclose(e2, 0.5 * e, rtol=1e-15, atol=0)
    pos = z > e0
    assert bool(pos.any()) and bool((e[pos] >= e0[pos] * I.SELU_L).all())  # the linear side: the product's bound times lambda, and more


def test_the_grid_is_the_one_the_kernels_need():
    cases = E.gemm_cases()
    assert len(set(cases)) == len(cases)
    assert {c[0] for c in cases if c[2] == 192} == set(E.M_EDGES) and {c[2] for c in cases} == {64, 128, 192, 320}
    ns = {c[1] for c in cases}
    assert {4, 8, 12, 60, 64, 68, 132, 136, 252, 72, 120, 128, 256, 264, 272, 384, 512, 520, 260, 508, 516} == ns
    assert all(E.is_narrow(n) for n in E.N_NARROW) and not any(E.is_narrow(n) for n in E.N_WIDE + E.N_FALLBACK)
    assert all(n % 8 == 0 for n in E.N_WIDE) and all(n % 8 == 4 for n in E.N_FALLBACK)
    for s in E.settings():  # every setting runs packed strides at least once and padded ones everywhere else
        sh = E.share(s)
        assert 0 < sum(p for _c, _f, p in sh) <= len(sh) // 8 + 1 and len(sh) <= 700, (s["name"], len(sh))
    for c in E.conv_cases() + E.conv_cases(ln=True):
        assert (c["Tin"] - c["k"]) % c["s"] != 0 and (c["k"] * c["Cin"]) % 64 == 0
    L = E.gemm_launch((17, 260, 192), "gelu", "fp16")  # padded: every stride differs from the packed value, rows 16-byte aligned
    for t, packed in ((L.A, 192), (L.W, 192), (L.resid, 260), (L.out_f.view, 260)):
        assert t.stride(0) != packed and (t.stride(0) * t.element_size()) % 16 == 0 and t.data_ptr() % 16 == 0
    L = E.gemm_launch((17, 260, 192), "plain", "bf16")
    assert L.out_h.view.stride(0) % 8 == 0 and L.out_h.view.data_ptr() % 16 == 0 and L.out_h.view.stride(0) != L.out_f.view.stride(0)
    assert bool(torch.isnan(L.Abuf[:17, 192:]).all()) and bool(torch.isnan(L.Abuf[17:]).all()) and not bool(torch.isnan(L.A).any())


# ---- the planner: coverage ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from afx import _lib
    return _lib.lib()


@pytest.fixture()
def plan_fn(lib):
    def fn(knobs, M, N, K, rpb, flags):
        for k, v in knobs.items():
            assert lib.afx_debug_set(k.encode(), v) == 0
        out = (C.c_int * 8)()
        assert lib.afx_gemm_plan(M, N, K, rpb, 0, 1, flags, 0, out) == 0
        assert out[4] == 0  # (no row split at these sizes: one launch, one instance)
        return out[1]
    yield fn
    for k, v in E.KNOB_DEFAULTS.items():
        assert lib.afx_debug_set(k.encode(), v) == 0


def test_every_instance_receives_its_edges(plan_fn):
    table = E.coverage(plan_fn)
    assert set(E.INSTANCES) <= set(table), sorted(set(E.INSTANCES) - set(table))
    assert E.coverage_gaps(table) == []
    # the fallbacks the grid relies on are the planner's: a forced lean-only tile sends everything else to instance 0
    k3 = dict(E.KNOB_DEFAULTS, gemm_tile=3, gemm_fit=5)
    assert plan_fn(k3, 161, 264, 192, 0, 0) == 75 and plan_fn(k3, 161, 264, 192, 0, 4) == 0 and plan_fn(k3, 161, 260, 192, 0, 0) == 0
    k8 = dict(E.KNOB_DEFAULTS, gemm_tile=8)
    assert plan_fn(k8, 161, 264, 192, 0, 0) == 92 and plan_fn(k8, 161, 264, 192, 0, 4) == 0
    assert plan_fn(k3, 161, 136, 192, 0, 0) in (1, 92)  # a narrow N ignores the knob
    # every setting names its instance for the launches that can run on it
    for s in E.settings():
        named = [plan_fn(s["knobs"], *case, 0, E.plan_flags(form)) for case, form, _p in E.share(s)
                 if E.names_instance(case, form)]
        assert named and set(named) == {s["instance"]}, (s["name"], set(named))


# ---- the alignment contract: refused on the host, nothing launched ----------------------------------------------------
def test_misaligned_rows_are_refused_before_any_launch(lib):
    base = 0x7F0000001000  # a 16-byte aligned address nobody dereferences: every call below is refused by the host checks
    P = C.c_void_p
    M, N, K = 32, 264, 192

    def gemm(dt=1, A=base, lda=K, W=base, ldw=K, N=N, bias=None, resid=None, ldr=N, of=base, ldo_f=N, oh=None, ldo_h=N):
        rc = lib.afx_k_gemm(dt, P(A), lda, P(W), ldw, M, N, K, None if bias is None else P(bias), 0, 1.0,
                            None if resid is None else P(resid), ldr, None if of is None else P(of), ldo_f, None if oh is None else P(oh), ldo_h, None)
        return rc, lib.afx_last_error().decode()

    for dt in (0, 1):
        for kw in (dict(A=base + 2), dict(A=base + 8), dict(W=base + 4), dict(lda=K + 4), dict(lda=K + 1), dict(ldw=K + 2),
                   dict(bias=base + 4), dict(resid=base + 8), dict(resid=base, ldr=N + 2), dict(of=base + 4), dict(ldo_f=N + 1),
                   dict(ldo_f=N + 2), dict(oh=base + 8), dict(oh=base, ldo_h=N + 4), dict(oh=base + 4, N=260, ldo_h=260),
                   dict(oh=base, N=260, ldo_h=262)):
            rc, msg = gemm(dt, **kw)
            assert rc != 0 and "gemm:" in msg and ("16-byte" in msg or "boundary" in msg), (kw, rc, msg)
    for kw in (dict(A=base + 4), dict(lda=K + 2), dict(ldw=K + 1), dict(of=base + 8), dict(ldo_f=N + 2), dict(oh=base + 4), dict(oh=base, ldo_h=N + 1),
               dict(resid=base, ldr=N + 3), dict(bias=base + 8)):
        rc, msg = gemm(2, **kw)
        assert rc != 0 and "gemm(fp32)" in msg and "16-byte" in msg, (kw, rc, msg)
    rc, msg = gemm(3, lda=K + 8)  # the split-precision hook: packed rows
    assert rc != 0 and "fp16x3" in msg

    def rownorm(dt=1, x=base, ldx=260, Cc=260, g=base, b=base, of=base, ldo_f=260, oh=None, ldo_h=260):
        rc = lib.afx_k_rownorm(dt, P(x), ldx, 5, Cc, P(g), P(b), 1e-5, 0, None if of is None else P(of), ldo_f, None if oh is None else P(oh), ldo_h, None)
        return rc, lib.afx_last_error().decode()

    for dt in (0, 1, 2, 3):
        for kw in (dict(x=base + 4), dict(ldx=262), dict(g=base + 8), dict(b=base + 4), dict(of=base + 8), dict(ldo_f=261),
                   dict(oh=base + 4), dict(oh=base, ldo_h=262)):
            rc, msg = rownorm(dt, **kw)
            assert rc != 0 and "rownorm:" in msg and ("16-byte" in msg or "boundary" in msg), (dt, kw, rc, msg)
    rc, msg = rownorm(2, oh=base + 8)  # 8-byte alignment is enough for half rows only
    assert rc != 0 and "rownorm:" in msg

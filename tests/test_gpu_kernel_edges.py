"""On a real MI355X: the single-kernel entry points at the edges of their contract, against fp64 references.

``afx_k_gemm`` (fp16 / bf16 / fp16x3 under every knob setting that reaches a tile instance, and fp32), ``afx_k_conv_gemm`` and
``afx_k_conv_ln_act`` (rows per batch < M, tiles straddling batches) and ``afx_k_rownorm`` (both launch forms) on the grid of
oracle/kernel_edges.py: M around every tile height, N with ragged last column blocks and the narrow-store fallback, 1 / 2 / 3 /
5 K-tiles, padded row strides.  Operands are views into NaN pools, outputs views into buffers pre-filled with a guard
pattern; every output is judged by ``kernel_edges.judge``: the bound of oracle/insitu.py (its constants unchanged), no NaN, no
element left unwritten, no guard element touched -- and the rounding-bias statistic per (instance, dtype, epilogue form),
asserted from 16 384 elements on.  Each test reads ``afx_gemm_plan`` under its own knobs first and records the instance that
really runs.  tests/test_cpu_kernel_edges.py shows what each criterion catches.  The last test prints the summary."""
import contextlib
import ctypes as C

import pytest
import torch

from oracle import kernel_edges as E

pytestmark = pytest.mark.gpu

SUMMARY = E.Tally()
HALF = ("fp16", "bf16")


@pytest.fixture(scope="module")
def K():
    from afx import kernels
    return kernels


@pytest.fixture(scope="module")
def lib_():
    from afx._lib import lib
    return lib()


@contextlib.contextmanager
def knobs(lib_, kn):
    from afx._lib import check
    try:
        for k, v in kn.items():
            check(lib_.afx_debug_set(k.encode(), v))
        yield
    finally:
        for k, v in E.KNOB_DEFAULTS.items():
            check(lib_.afx_debug_set(k.encode(), v))


def plan(lib_, M, N, Kk, rpb, flags):
    """The instance launch_gemm takes under the knobs in force (the entry points plan by makespan), one launch at these sizes."""
    out = (C.c_int * 8)()
    assert lib_.afx_gemm_plan(M, N, Kk, rpb, 0, 1, flags, 0, out) == 0 and out[4] == 0
    return out[1]


def finish(tally):
    SUMMARY.merge(tally)
    bad = tally.failures()
    assert not bad, (len(bad), bad[:6])


def outs(L):
    return dict(out_f=L.out_f.view if L.out_f is not None else False, out_h=L.out_h.view if L.out_h is not None else False)


def gemm_params():
    for dt in ("fp16", "bf16", "fp16x3"):
        for s in E.settings():
            # split precision has no 256x256 2-stage instance and one K-loop form of the 8-phase kernel (dispatch_s3)
            if dt == "fp16x3" and (s["knobs"]["gemm_tile"] == 1 or s["knobs"]["gemm_ph4"] != 0):
                continue
            yield pytest.param(dt, s, id=f"{dt}-{s['name']}")


def run_gemm_share(K, lib_, dt, s, share, cls="edge_gemm"):
    tally, named = E.Tally(), []
    for (M, N, Kk), form, packed in share:
        if dt == "fp16x3":
            Kk //= 2  # (K counts fp32 elements: the same number of 64-half K-tiles in pair form)
        tile = plan(lib_, M, N, Kk, 0, E.plan_flags(form, dt)) if dt != "fp32" else "f32"
        if E.names_instance((M, N, Kk), form):
            named.append(tile)
        L = E.gemm_launch((M, N, Kk), form, dt, packed, device="cuda")
        K.gemm(dt, L.A, L.W, bias=L.bias, act=L.act, alpha=L.alpha, resid=L.resid, **outs(L))
        refs = E.gemm_refs(L)
        c = f"{cls} {tile} {E.epilogue_of(form, N)}"
        for key, out in (("f", L.out_f), ("h", L.out_h)):
            if out is not None:
                tally.add(c, dt, E.judge(out, *refs[key], dt=dt if key == "h" else None), ((M, N, Kk), form, key, "packed" if packed else "padded"))
    return tally, named


@pytest.mark.parametrize("dt,s", list(gemm_params()))
def test_gemm_edges(K, lib_, dt, s):
    with knobs(lib_, s["knobs"]):
        tally, named = run_gemm_share(K, lib_, dt, s, E.share(s))
    assert named and set(named) == {s["instance"]}, (s["name"], sorted(set(named)))  # the instance the parametrisation names really ran
    finish(tally)


@pytest.mark.parametrize("kind", ["narrow", "wide", "fallback"])
def test_gemm_fp32_edges(K, lib_, kind):
    s = dict(E.F32_SETTING, n=(kind,))
    tally, _ = run_gemm_share(K, lib_, "fp32", s, E.share(s, E.gemm_f32_cases()))
    assert sum(t["launches"] for t in tally.c.values()) > 100
    finish(tally)


CONV_SETTINGS = ("auto", "tile0", "tile5", "tile1", "tile3_fit5_ph0", "tile3_fit6_ph0", "tile3_fit7_ph0", "tile3_fit8_ph0")


def conv_params():
    by_name = {s["name"]: s for s in E.settings()}
    for dt in HALF:
        for n in CONV_SETTINGS:
            yield pytest.param(dt, by_name[n], id=f"{dt}-{n}")
    yield pytest.param("fp32", E.F32_SETTING, id="fp32")


@pytest.mark.parametrize("dt,s", list(conv_params()))
def test_conv_gemm_edges(K, lib_, dt, s):
    """Rows per batch < M: a tile's rows come from several batches, every batch ends in a NaN frame no window reads."""
    tally, tiles = E.Tally(), set()
    with knobs(lib_, s["knobs"]):
        for c in E.conv_cases():
            M, Kk = c["B"] * c["Tout"], c["k"] * c["Cin"]
            tile = plan(lib_, M, c["N"], Kk, c["Tout"], 0) if dt != "fp32" else "f32"
            tiles.add(tile)
            L = E.conv_launch(c, dt, device="cuda")
            K.conv_gemm(dt, L.x, L.W, c["k"], c["s"], bias=L.bias, out=L.out_f.view.view(c["B"], c["Tout"], c["N"]))
            tally.add(f"edge_conv {tile}", dt, E.judge(L.out_f, *E.conv_refs(L)["f"]), c)
    assert dt == "fp32" or s["instance"] in tiles, (s["name"], tiles)
    finish(tally)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("s", E.convln_settings(), ids=lambda s: s["name"])
def test_conv_ln_act_edges(K, lib_, dt, s):
    """The fused conv + LayerNorm + GELU on the row-complete tiles 3 / 8 / 83 / 82 and both K-loop forms of 8, both outputs."""
    tally = E.Tally()
    with knobs(lib_, s["knobs"]):
        for c in E.conv_cases(ln=True):
            M, Kk = c["B"] * c["Tout"], c["k"] * c["Cin"]
            tile = plan(lib_, M, 512, Kk, c["Tout"], 1)
            assert tile == s["instance"], (s["name"], c, tile)
            L = E.conv_launch(c, dt, ln=True, device="cuda")
            shape = (c["B"], c["Tout"], 512)
            K.conv_ln_act(dt, L.x, L.W, c["k"], c["s"], L.bias, L.gamma, L.beta, act="gelu", out_f=L.out_f.view.view(shape), out_h=L.out_h.view.view(shape))
            refs = E.conv_refs(L)
            for key, out in (("f", L.out_f), ("h", L.out_h)):
                tally.add(f"edge_convln {tile}", dt, E.judge(out, *refs[key], dt=dt if key == "h" else None), (c, key))
    finish(tally)


def run_rownorm(K, dt, cases, tally, cls):
    j = 0
    for rows, Cc in cases:
        x = None
        sub = E.rownorm_rows(rows)
        sub = None if len(sub) == rows else sub
        for act in E.ACTS:
            L = E.rownorm_launch(rows, Cc, dt, act, packed=j % 16 == 0, device="cuda", x=x)
            x = L.x_cpu  # (one input per case: the activations share it)
            j += 1
            K.rownorm(dt, L.x, L.gamma, L.beta, act=act, **outs(L))
            refs = E.rownorm_refs(L, sub)
            for key, out in (("f", L.out_f), ("h", L.out_h)):
                tally.add(cls, dt, E.judge(out, *refs[key], dt=dt if key == "h" else None, rows=sub), (rows, Cc, act, key))


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_rownorm_edges_one_row_per_wave(K, dt):
    tally = E.Tally()
    run_rownorm(K, dt, E.rownorm_cases()[0], tally, "edge_rownorm")
    finish(tally)


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp32", "fp16x3"])
def test_rownorm_edges_two_rows_per_wave(K, dt):
    """From 16 384 rows on a wave takes two rows: an even count, a last wave with one live row, a last workgroup with
    one live wave.  Compared on both ends and every 61st row; the guards cover the whole buffers."""
    tally = E.Tally()
    run_rownorm(K, dt, E.rownorm_cases()[1], tally, "edge_rownorm2")
    finish(tally)


# ---- the module's summary (the last test of the file: it reports what the tests above measured) -----------------------------
def test_summary_of_the_edge_grid(capsys):
    lines = ["edge grid of the single-kernel entry points: worst |got - ref| / bound per class (instance, epilogue form), rounding bias"]
    lines += SUMMARY.lines()
    with capsys.disabled():  # (printed past pytest's output capture)
        print("\n" + "\n".join(lines))
    assert not SUMMARY.failures(), SUMMARY.failures()[:10]

"""GPU: the launch shapes the CU-time objective picks compute the rows of the makespan shapes, bit for bit.

The objective only chooses among forms that already exist (tile heights of the 8-phase GEMM, 4 or 8 waves per workgroup of the
fused Conformer chains); each test first reads through the query entry points that the two objectives really differ on its
shape, then compares outputs with torch.equal."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import afx  # noqa: F401
    from afx import engine, kernels, synth
    from afx._lib import check, lib
    return engine, kernels, synth, check, lib()


def _plan(lib, M, N, K, flags, objective):
    out = (C.c_int * 8)()
    assert lib.afx_gemm_plan(M, N, K, 0, 0, 1, flags, objective, out) == 0
    return list(out)


# M = 3584: 16 x 16 tiles of 224 rows (one round of the 256 CUs exactly) against 14 x 16 of 256 rows; 3579: the same with a
# ragged last tile at both heights; 3589 (5 rows more): a 17th tile row of 224 would start a second round, so
# both objectives take 256 rows there -- asserted as such, and the rows are compared all the same.
@pytest.mark.parametrize("M,differ", [(3584, True), (3579, True), (3589, False)])
@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
@pytest.mark.parametrize("resid", [True, False])
def test_plain_gemm_same_bits_under_both_objectives(mods, M, differ, dt, resid):
    engine, K, synth, check, lib = mods
    N, K_ = 4096, 128
    a, b = _plan(lib, M, N, K_, 2 if dt == "fp16x3" else 0, 0), _plan(lib, M, N, K_, 2 if dt == "fp16x3" else 0, 1)
    assert a[0] == b[0] == 7 and a[4] == b[4] == 0
    assert ((a[2], b[2]) == (224, 256)) if differ else (a[2] == b[2] == 256)
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K_, generator=g)
    W = torch.randn(N, K_, generator=g) / math.sqrt(K_)
    if dt == "fp16":
        A, W = A.half(), W.half()
    A, W = A.cuda(), W.cuda()
    bias = torch.randn(N, generator=g).cuda()
    R = torch.randn(M, N, generator=g).cuda() if resid else None
    outs = []
    try:
        for obj in (0, 1, 0, 1):
            check(lib.afx_debug_set(b"dispatch_objective", obj))
            outs.append(K.gemm(dt, A, W, bias=bias, resid=R, out_f=resid, out_h=True))
    finally:
        check(lib.afx_debug_set(b"dispatch_objective", -1))
    ref = A.float() @ W.float().t() + bias + (R if resid else 0)
    assert (outs[0][1].float() - ref).abs().max().item() < (2e-2 if dt == "fp16" else 1e-4)  # (a product at all: fp16 output rounding / ~22 bits)
    for of, oh in outs[1:]:
        assert torch.equal(oh, outs[0][1])
        if resid:
            assert torch.equal(of, outs[0][0])


@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_conformer_chain_same_bits_with_4_and_8_waves(mods, dt):
    engine, K, synth, check, lib = mods
    B, T = 3, 50  # 3 x (50 + class token) = 153 token rows: no multiple of 64 or 128 (3 workgroups of 4 waves, 2 of 8)
    assert lib.afx_conf_chain_waves(B * (T + 1), 0) == 4 and lib.afx_conf_chain_waves(B * (T + 1), 1) == 8
    head = synth.conformer_head_state_dict(emb_size=144, heads=4, kernel_size=31, n_encoders=2)
    sd = dict(synth.ssl_state_dict(1))
    sd.update(head)
    eng = engine.Engine("conformer", n_layers=1, dtype=dt, conf_blocks=2)
    eng.load_state_dict(sd)
    x = torch.randn(B, T, 144, generator=torch.Generator().manual_seed(5)).cuda()
    got = {}
    try:
        for waves in (4, 8, 4, 8):
            check(lib.afx_debug_set(b"conf_chain_waves", waves))
            out, emb = eng.conformer(x)
            got.setdefault(waves, []).append((out.clone(), emb.clone()))
    finally:
        check(lib.afx_debug_set(b"conf_chain_waves", 0))
    want_out, want_emb = got[4][0]
    assert torch.isfinite(want_out).all() and want_emb.abs().max().item() > 0
    for waves in (4, 8):
        for out, emb in got[waves]:
            assert torch.equal(out, want_out) and torch.equal(emb, want_emb), waves
    # and through the objective itself, not the knob: the concurrent switch picks 8 waves for this call
    check(lib.afx_engine_set(eng._h, b"concurrent", 1))
    try:
        out, emb = eng.conformer(x)
        assert eng.last_objective == 1
    finally:
        check(lib.afx_engine_set(eng._h, b"concurrent", 0))
    assert torch.equal(out, want_out) and torch.equal(emb, want_emb)


def test_engine_lanes_run_under_cu_time_and_forward_does_not(mods):
    engine, K, synth, check, lib = mods
    B, L = 3, 16000
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(synth.model_state_dict("ConformerModel", n_layers=6))
    wave = synth.waveforms(B, L).cuda()
    want = eng.forward(wave).clone()
    assert eng.last_objective == 0
    outs = [eng.forward_lanes(wave) for _ in range(4)]
    assert eng.last_objective == 1  # the lanes' native calls ran with the objective on ...
    eng.join()
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, want)
    v = C.c_int(-1)
    check(lib.afx_engine_get(eng._h, b"concurrent", C.byref(v)))
    assert v.value == 0  # ... and left the switch off
    eng.set_issue("lanes")
    again = eng.forward(wave)
    assert eng.last_objective == 0  # a plain forward after set_issue("lanes"): today's plan
    assert torch.equal(again, want)
    out = (C.c_int * 8)()
    check(lib.afx_gemm_plan(B * 49, 3072, 1024, 0, 0, 1, 0, -1, out))  # a query outside any call: makespan, whatever ran before
    assert out[7] == 0
    outs = [eng.forward_overlapped(wave) for _ in range(2)]  # (issues the lanes form now)
    assert eng.last_objective == 1
    eng.join()
    torch.cuda.synchronize()
    assert all(torch.equal(o, want) for o in outs)


def test_call_state_belongs_to_the_call_and_the_handle(mods):
    """Two engines interleaved on ONE thread share nothing: the objective, the "gemm_small_deep" switch, the profiler and the
    split-precision scratch of a call come from its handle and its workspace, never from what the call before it left behind.

    P (fp16x3, concurrent = 1, profiling on) and Q (fp16, gemm_small_deep = 0) are 1-layer students on 3 clips of 4000 samples
    (12 frames: the trunk's products take the small-M path, where the deep-tile switch and the pair-form scratch decide
    something).  Every interleaved output equals the engine's solo output bit for bit, each handle reports its own objective
    after every call, P's profile counts P's launches only, and a plan query outside any call answers makespan.  The commit
    before the call context satisfied all of these but the last: there the query read the CU-time objective that P's call
    had left in the thread."""
    engine, K, synth, check, lib = mods
    B, L = 3, 4000
    sd = synth.model_state_dict("ConformerModel", n_layers=1)
    P = engine.Engine("conformer", n_layers=1, dtype="fp16x3")
    Q = engine.Engine("conformer", n_layers=1, dtype="fp16")
    P.load_state_dict(sd)
    Q.load_state_dict(sd)
    P.set("concurrent", 1)
    Q.set("gemm_small_deep", 0)
    wave = synth.waveforms(B, L).cuda()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 12, 144, generator=g).cuda()
    feats6 = torch.randn(B, 4, 512, generator=g).cuda()

    def launches(prof):
        return {k: v["launches"] for k, v in prof.items()}

    def solo(call):  # P alone: its output and its launch counts per class
        P.profile_begin()
        out = call()
        return out, launches(P.profile_end())

    (p_fwd, n_fwd), (p_conf, n_conf) = solo(lambda: P.forward(wave)), solo(lambda: P.conformer(x))
    p_step, n_step = solo(lambda: P.kv_state(B).step(feats6))  # (a fresh state: its first chunk)
    q_fwd = Q.forward(wave)
    assert n_fwd["rownorm_kernel"] > 0 and n_conf["conf_chain_kernel"] > 0 and n_step["mhsa_kernel"] > 0
    assert P.last_objective == 1 and Q.last_objective == 0

    def plan_objective():
        out = (C.c_int * 8)()
        check(lib.afx_gemm_plan(B * 12, 3072, 1024, 0, 0, 1, 0, -1, out))
        return out[7]

    kv = P.kv_state(B)
    P.profile_begin()
    for who, call, want in [(P, lambda: P.forward(wave), p_fwd), (Q, lambda: Q.forward(wave), q_fwd),
                            (P, lambda: P.conformer(x), p_conf), (Q, lambda: Q.forward(wave), q_fwd),
                            (P, lambda: kv.step(feats6), p_step), (Q, lambda: Q.forward(wave), q_fwd),
                            (P, lambda: P.forward(wave), p_fwd)]:
        got = call()
        assert P.last_objective == 1 and Q.last_objective == 0
        if who is P:
            assert plan_objective() == 0
        for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            assert torch.equal(a, b)
    mixed = launches(P.profile_end())
    assert mixed == {k: 2 * n_fwd[k] + n_conf[k] + n_step[k] for k in n_fwd}

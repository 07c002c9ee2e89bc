"""Per-launch parity inside the KV-cached streaming step on an MI355X, all three forms (afx_kv_step, afx_kv_step_ragged,
afx_kv_step_active): every tapped launch of every step against its fp64 reference built from the launch's own tapped
inputs, element by element within the bounds of oracle/insitu.py, and the step's bookkeeping against the host-side state
model of oracle/insitu_kv.py (``KvModel``, ``kv_walk``): where the chunk's q | k | v rows land in the ring, that every
other ring row keeps every bit, which slots are live, the left context and the zero rows of the positional conv's
operand, the window buffer and the head's input bit for bit.  Every row of every launch is checked (M <= 48); the rows of
a ragged block past its own n_s are unread by contract and get the zero / not-live statements instead.

Conformer student, two trunk layers, one head block, synthetic weights, S = 3; the steps are driven through
``KVState.step`` / ``reset`` with seeded gelu(randn) frames.  The module's summary line gives the worst |got - ref| /
bound per launch class (kv_product, kv_ring, kv_posconv, kv_layernorm) and dtype, printed by the file's last test."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SUMMARY = {}
S, LAYERS = 3, 2
LAYER_TAPS = ("ln1", "ring", "att", "mid", "ln2", "ff")


_ENG = {}


def _engine(dt, arch="conformer"):
    """One engine per dtype, shared by the tests of this module; -> (engine, the trunk's state dict by oracle names).
    arch "xlsr_aasist": a one-layer teacher (the back-end's bucket loop)."""
    from afx import engine, synth
    from oracle import models as om
    if arch not in _ENG:
        _ENG[arch] = synth.model_state_dict("ConformerModel", n_layers=LAYERS, n_encoders=1) if arch == "conformer" else \
            synth.model_state_dict("XLSR_AASIST", n_layers=1)
    if (arch, dt) not in _ENG:
        kw = dict(n_layers=LAYERS, conf_blocks=1) if arch == "conformer" else dict(n_layers=1)
        _ENG[arch, dt] = engine.Engine(arch, dtype=dt, **kw)
        _ENG[arch, dt].load_state_dict(_ENG[arch])
    return _ENG[arch, dt], om.split(_ENG[arch])[0]


def frames(seed, rows, n):
    """Seeded conv-layer-6 frames (rows, n, 512): gelu(randn), what the conv stack hands the feature LayerNorm."""
    return F.gelu(torch.randn(rows, n, 512, generator=torch.Generator().manual_seed(seed)))


def tap_names(form):
    names = ["kv.feats", "kv.xpad", "kv.proj", "kv.pos"] + [f"kv.l{l}.{t}" for l in range(LAYERS) for t in LAYER_TAPS] + \
            [f"kv.layer{l}" for l in range(LAYERS)] + ["kv.win", "ssl"]
    return names + ([] if form == 1 else ["kv.fl"])


class Walker:
    """A KVState and its KvModel side by side: every step runs with taps on and is walked launch by launch."""

    def __init__(self, dt, n_streams=S, arch="conformer", call=None):
        from oracle import insitu, insitu_kv
        self.I, self.K, self.dt = insitu, insitu_kv, dt
        self.eng, self.sd = _engine(dt, arch)
        self.buckets = arch != "conformer"
        self.kv = self.eng.kv_state(n_streams)
        self.model = insitu_kv.KvModel(n_streams)
        self.prev = [torch.zeros(n_streams, insitu_kv.SLOTS, 3 * 1024, dtype=torch.float64) for _ in range(LAYERS)]
        self.fails, self.steps = [], 0
        # call (tests/test_gpu_insitu_call.py: dict(suffix, summary)): the classes go under the suffix into that module's table
        self.summary, self.suffix = (SUMMARY, "") if call is None else (call["summary"], call["suffix"])
        self.check_kw = None if call is None else dict(unique_rows=True, rounding_only=True)
        self.eng.enable_taps()

    def reset(self, slots):
        self.kv.reset(slots)
        self.model.reset(slots)

    def step(self, f, n_frames=None, slots=None):
        plan = self.model.begin(f.shape[1], n_frames, slots)
        out = self.kv.step(f.cuda(), n_frames, slots).cpu()
        tap = lambda name: self.eng.tap(name).cpu().double()
        res, fails, self.prev = self.K.kv_walk(self.sd, self.dt, tap, self.model, plan, f, self.prev, buckets=self.buckets,
                                                   check_kw=self.check_kw)
        where = f"step {self.steps} (form {plan['form']}, n {[b['n'] for b in plan['blocks']]}, streams {[b['stream'] for b in plan['blocks']]})"
        for cls, name, r, op_dt in res:
            key = (cls + self.suffix, self.dt)
            r0, b0 = self.summary.get(key, (0.0, None))
            # The rounding-bias statistic (oracle/insitu.py) needs thousands of independent samples: BIAS_MAX is 0.05 ulp and
            # one element's rounding error has sigma 0.29 ulp, so a launch is judged from 16384 elements on (sigma 0.002).
            # The ring attention is reported, not asserted: its output error is P's rounding (several output ulps, shared
            # by the 64 columns of a head), so <= 48 query rows give <= 768 independent samples and a standard error above
            # BIAS_MAX; the output store is the dense attention's, whose statistic tests/test_gpu_insitu.py asserts.
            b = r["bias"] if op_dt and self.dt in self.I.HALF and r["n"] >= 16384 and cls != "kv_ring" else None
            self.summary[key] = (max(r0, r["ratio"]), b if b0 is None or (b is not None and abs(b) > abs(b0)) else b0)
            if not r["ratio"] <= 1.0:
                self.fails.append(f"{where} {name} [{self.dt}]: |got - ref| = {r['ratio']:.2f} x bound at row {r['row']}, col {r['col']} "
                                  f"(got {r['got']:.6e}, ref {r['ref']:.6e}, bound {r['bound']:.2e})")
            if b is not None and self.dt in self.I.HALF and abs(b) > self.I.BIAS_MAX:
                self.fails.append(f"{where} {name} [{self.dt}]: rounding bias {b:+.3f} ulp")
        self.fails += [f"{where} {m}" for m in fails]
        assert bool(torch.isfinite(out).all()), where
        self.steps += 1
        return out

    def done(self):
        self.eng.enable_taps(False)
        assert not self.fails, f"{len(self.fails)} failed checks:\n" + "\n".join(self.fails[:40])


# (a) ---- lock-step -------------------------------------------------------------------------------------------------------
# 22 steps: the ring wraps at step 16; group 2 is rewritten 13 -> 12 and group 5 16 -> 1 (stale slots past the new count);
# n = 1 and n = 16 occur; the window holds exactly 200 frames after step 16 and passes 208 at step 17
LOCKSTEP = [12, 12, 13, 12, 1, 16, 16, 7, 12, 13, 12, 12, 13, 12, 12, 13, 12, 12, 12, 12, 5, 1]


@pytest.mark.parametrize("dt", ["fp16", "bf16", "fp16x3"])
def test_lockstep_every_launch_of_22_steps(dt):
    assert sum(LOCKSTEP[:17]) == 200 and sum(LOCKSTEP[:18]) > 208 and LOCKSTEP[2] > LOCKSTEP[18] and LOCKSTEP[5] > LOCKSTEP[21]
    w = Walker(dt)
    for i, n in enumerate(LOCKSTEP):
        w.step(frames(100 + i, S, n))
    assert w.model.hop == 22 and w.model.feat[0].shape[0] == 208
    w.done()


# (b) ---- sessions --------------------------------------------------------------------------------------------------------
def ragged_counts(i):
    n_max = [12, 13, 16, 12, 7, 16][i % 6]
    ns = [n_max, 1 + (5 * i + 3) % n_max, 1 + (7 * i + 1) % n_max]
    return n_max, [16, 1, 9] if i == 2 else ns


def test_sessions_every_launch_with_resets_before_and_after_the_wrap():
    w = Walker("fp16")
    for i in range(22):
        if i == 3:
            w.reset([1])  # before the wrap: base group 3; at steps 16 .. 18 its base is above the current group
        if i == 18:
            w.reset([2])  # after the wrap: base group 2
        if i == 20:
            w.reset([1])  # a stream reset twice
        n_max, ns = ragged_counts(i)
        assert max(ns) <= n_max and min(ns) >= 1
        w.step(frames(200 + i, S, n_max), ns)
    assert w.model.base == [0, 4, 2] and w.model.hop == 22
    w.done()


# (c) ---- active lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_active_lists_every_launch(dt):
    w = Walker(dt)
    for i in range(3):  # lock-step first: the first active step takes over the lock-stepped group
        w.step(frames(300 + i, S, 12))
    lists = [([2, 0, 1], 12, None), ([1], 16, None), ([2, 0], 13, [13, 4])]
    # stream 2 now sits out 18 steps of the two others (their groups wrap past its own), then returns alone
    lists += [([0, 1] if i % 2 else [1, 0], [12, 16, 7][i % 3], [[12, 5], [1, 16], None][i % 3]) for i in range(18)]
    lists += [([2], 1, None), ([1, 2, 0], 16, [3, 16, 9])]
    for j, (slots, n_max, ns) in enumerate(lists):
        if j == 12:
            w.reset([0])  # a reset inside the active state: the stream starts at its own next group
        w.step(frames(400 + j, len(slots), n_max), ns, slots)
    assert w.model.active and len(set(w.model.next)) > 1
    w.done()


def test_aasist_bucket_loop_gathers_each_window_by_length():
    """The AASIST back-end of the per-stream forms scores one uniform batch per window length: every gathered bucket
    (kv.bucket{i}) is the model's windows of that length, in list order; the trunk's launches are checked as above."""
    w = Walker("fp16", arch="xlsr_aasist")
    w.step(frames(350, S, 12), [12, 6, 12])    # windows of 12, 6, 12 frames: two buckets, the shorter one first
    w.step(frames(351, S, 16), [16, 1, 16])
    w.step(frames(352, S, 8), [8, 3, 8], [2, 0, 1])   # 36, 31 and 10 frames: three buckets
    w.reset([0])
    w.step(frames(353, 2, 7), [7, 6], [0, 2])
    w.step(frames(354, 1, 16), None, [1])
    w.done()


# (d) ---- the three forms agree at every tap -------------------------------------------------------------------------------
SEQ = [12, 13, 12, 1, 16, 7, 12, 12, 13, 12, 12, 13, 12, 16, 12, 12, 13, 5, 12]  # 19 chunks of ONE stream: its ring wraps


def _own_taps(eng, block, stream, n, n_max, form):
    """The stream's own rows of the step's taps (block: its row block in the dense buffers)."""
    t = lambda name: eng.tap(name)
    out = {}
    for l in range(LAYERS):
        out[f"l{l}.att"] = t(f"kv.l{l}.att").reshape(-1, 16, 1024)[block, :n].cpu()
        out[f"layer{l}"] = t(f"kv.layer{l}").reshape(-1, n_max, 1024)[block, :n].cpu()
    win = t("kv.win").reshape(-1, 208, 1024)[stream].cpu()
    out["win"] = win
    out["fl"] = win[208 - n:] if form == 1 else t("kv.fl").reshape(-1, n_max, 1024)[block, :n].cpu()
    assert torch.equal(out["fl"], win[208 - n:])
    return out


def _head_rows(eng, block, blocks, th):
    return eng.tap("ssl").reshape(blocks, -1, 1024)[block, :th].cpu()


def test_one_stream_three_forms_bit_identical_at_every_tap():
    eng, _sd = _engine("fp16")
    eng.enable_taps()
    mine = [frames(500 + i, 1, n)[0] for i, n in enumerate(SEQ)]
    runs = {}
    # form 1: lock-step from hop 0, the stream is stream 0
    kv, got, total = eng.kv_state(S), [], 0
    for i, n in enumerate(SEQ):
        f = frames(600 + i, S, n)
        f[0] = mine[i]
        logit = kv.step(f.cuda()).cpu()[0]
        total += n
        t = _own_taps(eng, 0, 0, n, n, 1)
        t["head"], t["logits"] = _head_rows(eng, 0, S, min(total, 200)), logit
        got.append(t)
    runs["lock-step"] = got
    # form 2: a session started at hop 5 on stream 1, beside other traffic of other sizes
    kv, got, total = eng.kv_state(S), [], 0
    for i in range(5):
        kv.step(frames(700 + i, S, 9).cuda(), [9, 4, 7])
    kv.reset([1])
    for i, n in enumerate(SEQ):
        n_max = max(n, [16, 12, 13][i % 3])
        f = frames(720 + i, S, n_max)
        f[1, :n] = mine[i]
        logit = kv.step(f.cuda(), [n_max, n, 1 + i % n_max]).cpu()[1]
        total += n
        t = _own_taps(eng, 1, 1, n, n_max, 2)
        t["head"], t["logits"] = _head_rows(eng, 1, S, min(total, 200)), logit
        got.append(t)
    runs["session"] = got
    # form 3: active lists, the stream is stream 2 at changing positions of lists of changing length
    kv, got, total = eng.kv_state(S), [], 0
    for i, n in enumerate(SEQ):
        slots = [[2], [0, 2], [1, 2, 0], [2, 1]][i % 4]
        n_max = max(n, [12, 16][i % 2]) if len(slots) > 1 else n
        f = frames(740 + i, len(slots), n_max)
        b = slots.index(2)
        f[b, :n] = mine[i]
        ns = [n if s == 2 else 1 + (i + s) % n_max for s in slots]
        logit = kv.step(f.cuda(), ns, slots).cpu()[b]
        total += n
        t = _own_taps(eng, b, 2, n, n_max, 3)
        t["head"], t["logits"] = _head_rows(eng, b, len(slots), min(total, 200)), logit
        got.append(t)
    runs["active"] = got
    eng.enable_taps(False)
    diffs = []
    for name in ("session", "active"):
        for i in range(len(SEQ)):
            for k, v in runs["lock-step"][i].items():
                if not torch.equal(v, runs[name][i][k]):
                    diffs.append(f"chunk {i} (n {SEQ[i]}): {k} of the {name} form differs from the lock-step form's "
                                 f"(max |d| {(v - runs[name][i][k]).abs().max().item():.3e})")
    assert not diffs, "\n".join(diffs[:30])


# (e) ---- taps change nothing; a stale workspace changes nothing -------------------------------------------------------------
def _three_forms(eng, n_streams=S, seed=800, collect=None):
    """A short sequence through all three forms on a fresh state: lock-step x2, a reset and sessions x2, active lists x2.
    -> the logits of every step; collect(form): called after every step (to read taps)."""
    kv, out = eng.kv_state(n_streams), []

    def run(form, f, ns=None, slots=None):
        out.append(kv.step(f.cuda(), ns, slots).cpu())
        if collect:
            collect(form, len(out) - 1)

    run(1, frames(seed, n_streams, 12))
    run(1, frames(seed + 1, n_streams, 7))
    kv.reset([1])
    run(2, frames(seed + 2, n_streams, 13), [13, 5, 1][:n_streams] + [2] * (n_streams - 3))
    run(2, frames(seed + 3, n_streams, 16), [1, 16, 9][:n_streams] + [3] * (n_streams - 3))
    run(3, frames(seed + 4, 2, 12), [12, 3], [2, 0])
    run(3, frames(seed + 5, 1, 5), None, [1])
    return out


@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_taps_do_not_change_the_step(dt):
    eng, _sd = _engine(dt)
    eng.enable_taps(False)
    off = _three_forms(eng)
    eng.enable_taps()
    on = _three_forms(eng)
    eng.enable_taps(False)
    for i, (a, b) in enumerate(zip(off, on)):
        assert torch.equal(a, b), f"[{dt}] step {i}: taps moved the logits by {(a - b).abs().max().item():.3e}"


@pytest.mark.parametrize("dt", ["fp16", "fp16x3"])
def test_stale_workspace_changes_no_tap_of_the_step(dt):
    """The `_stale_vs_fresh` pattern of tests/test_gpu_insitu.py: the sequence after a differently shaped one (5 streams,
    other chunk sizes) equals the same sequence on a zeroed workspace, in the logits and in every tap of every step."""
    eng, _sd = _engine(dt)
    eng.enable_taps(False)
    _three_forms(eng, n_streams=5, seed=900)

    def run():
        taps = {}
        out = _three_forms(eng, collect=lambda form, i: taps.update({(i, n): eng.tap(n).cpu() for n in tap_names(form)}))
        return out, taps

    eng.enable_taps()
    stale_out, stale = run()
    eng._ws = torch.zeros_like(eng._ws)
    fresh_out, fresh = run()
    eng.enable_taps(False)
    for i, (a, b) in enumerate(zip(stale_out, fresh_out)):
        assert torch.equal(a, b), f"step {i}: logits depend on the workspace's earlier contents"
    bad = [f"step {i}: tap {n}" for (i, n) in stale if not torch.equal(stale[(i, n)], fresh[(i, n)])]
    assert not bad, "taps that depend on the workspace's earlier contents: " + ", ".join(bad)


# ---- the module's summary (the last test of the file: it reports what the tests above measured) -----------------------------
def test_summary_of_worst_ratios_per_launch_class(capsys):
    lines = ["KV step, in-place parity: worst |got - ref| / bound, rounding bias (mean signed ulps)"]
    for (cls, dt), (r, b) in sorted(SUMMARY.items()):
        lines.append(f"  {cls:12s} {dt:7s} ratio {r:.3f}" + (f"  bias {b:+.4f}" if b is not None else ""))
    with capsys.disabled():  # (printed past pytest's output capture)
        print("\n" + "\n".join(lines))
    assert all(r <= 1.0 for r, _b in SUMMARY.values()), SUMMARY

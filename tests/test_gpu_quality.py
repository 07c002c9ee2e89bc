"""The input-quality layer on the GPU (afx/quality.py; afx_k_quality).  Every comparison is exact (bits, counts, state bytes):
the kernel against ``QualityPolicy.step_reference`` over consecutive launches that carry the ring, the state and the totals
(the whole device state and the ``meas`` / ``out`` rows after every launch, unnamed rows' bytes included) over hops on both
sides of a thread's four elements, a wave, a tile, with rows that break 16-byte alignment, W = 1, 2, 16, one row, 8192 rows,
no scores and bad rows; ``QualityScorer`` end to end for the three scorer kinds (where ``valid`` holds the score is the bare
scorer's, bit for bit), under the verdict layer, around a cascade, behind the gate, and sessions moved between scorers.

The inputs are constructed: runs that start in one thread's elements and end in another wave's, runs over three hops, a run
that is exactly one hop, clipped samples at the first and the last element, NaN and inf on tile borders.  Before a case
compares anything it asserts ON THE REFERENCE that each of the five flags was set at least once and clear at least once and
that ``valid`` took both values, so an all-clear input cannot hide a dead path.

Tiny engines as in tests/test_gpu_verdict.py: a 1-layer Conformer student scores, a 1-layer XLSR_AASIST teacher verifies,
H = 4000."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
INF, NAN = float("inf"), float("nan")
QNAN = 0x7fc00000
SENT = -77


def fixture_stream():
    g = np.random.default_rng(0)
    x = (0.002 * g.standard_normal(128000)).astype(np.float32)
    t = np.arange(128000) / 16000
    for a, b in [(0.5, 1.3), (2.0, 2.15), (3.0, 5.0), (6.5, 6.52)]:
        m = (t >= a) & (t < b)
        x[m] += (0.2 * np.sin(2 * np.pi * 180 * t[m]) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t[m]))).astype(np.float32)
    x[112000:120000] = 0
    return x


FIX = fixture_stream()


def _clipped(x):
    """The stream through a saturating input stage: 40 dB of gain into a hard limiter."""
    return np.clip(x * np.float32(100), -1, 1).astype(np.float32)


def _ibits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_ibits(a.cpu()), _ibits(b.cpu()))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- 1. the kernel against step_reference --------------------------------------------------------------------------------
class _Mirror:
    """The state of one kernel-level run, on the device and in numpy."""

    def __init__(self, S, W, policy, hop):
        from afx.quality import QualityState
        self.S, self.W, self.p, self.hop = S, W, policy, hop
        self.ref = QualityState(S, W)
        self.d_ring = torch.zeros(S, W, dtype=torch.uint8, device="cuda")
        self.d_st = torch.zeros(S, 3, dtype=torch.int32, device="cuda")
        self.d_tot = torch.zeros(S, 6, dtype=torch.int32, device="cuda")
        self.flags, self.valid = [], []  # what the reference saw, for the coverage condition

    def poison(self, value=31):
        self.ref.ring[:] = value
        self.d_ring[:] = value

    def launch(self, slots, hops, ks, scores=None, layout="dense", what=None):
        """One launch.  layout: "dense" (contiguous, 16-byte aligned), "odd" (the rows one float past alignment at a stride
        of hop + 3 floats), "column" (also the scores as a column of a matrix).  Rows with a slot outside [0, S) are left
        out of the reference; the kernel skips them -> (out, meas) of the reference over all rows."""
        from afx._lib import call_on, lib
        p, hop = self.p, self.hop
        slots, ks, A = np.asarray(slots, dtype=np.int64), np.asarray(ks, dtype=np.int64), len(slots)
        x = np.ascontiguousarray(hops, dtype=np.float32)
        assert x.shape == (A, hop)
        if layout != "odd":
            d_x, stride = torch.from_numpy(x).cuda(), hop
        else:
            stride = hop + 3
            flat = torch.full((A * stride + 1,), 7.0)
            flat[1:].view(A, stride)[:, :hop] = torch.from_numpy(x)
            flat = flat.cuda()
            d_x = flat[1:]
            assert d_x.data_ptr() % 16 == 4
        sc = None if scores is None else np.asarray(scores, dtype=np.float32)
        d_sc, sstride = None, 1
        if sc is not None:
            if layout == "column":
                mat = torch.full((A, 2), 9.0)
                mat[:, 1] = torch.from_numpy(sc)
                d_sc, sstride = mat.cuda()[:, 1], 2
            else:
                d_sc = torch.from_numpy(sc).cuda()
        hdr = torch.from_numpy(np.stack([slots, ks], axis=1).astype(np.int32)).cuda()
        d_meas = torch.full((A, 8), SENT, dtype=torch.int32, device="cuda")
        d_out = torch.full((A,), float(SENT), dtype=torch.float32, device="cuda")
        e_quiet, d = (float(v) for v in p.bounds(hop))
        rc = call_on(self.d_ring, lib().afx_k_quality, _p(d_x), stride, A, hop, _p(hdr), _p(d_sc), sstride, p.clip, p.clip_count,
                     p.flat_run, e_quiet, d, p.mask, p.max_bad, int(p.abstain), _p(self.d_ring), self.W, _p(self.d_st), _p(self.d_tot),
                     self.S, _p(d_meas), _p(d_out) if sc is not None else None)
        torch.cuda.synchronize()
        assert rc == 0, lib().afx_last_error()
        ok = (slots >= 0) & (slots < self.S)
        meas = np.full((A, 8), -1, dtype=np.int32)
        out = None if sc is None else sc.copy()
        o, m = p.step_reference(slots[ok], x[ok], ks[ok], None if sc is None else sc[ok], self.ref)
        meas[ok] = m
        if sc is not None:
            out[ok] = o
        live = m[:, 0] >= 0
        self.flags += m[live, 0].tolist()
        self.valid += (m[live, 7] <= p.max_bad).tolist()
        assert d_meas.cpu().numpy().tobytes() == meas.tobytes(), (what, "meas", d_meas.cpu().numpy()[:4].tolist(), meas[:4].tolist())
        if sc is None:
            assert d_out.cpu().tolist() == [float(SENT)] * A, (what, "out written without scores")
        else:
            assert d_out.cpu().numpy().view(np.int32).tobytes() == out.view(np.int32).tobytes(), (what, "out")
        self.check(what)
        return out, meas

    def check(self, what):
        assert self.d_st.cpu().numpy().tobytes() == self.ref.st.tobytes(), (what, "state")
        assert self.d_ring.cpu().numpy().tobytes() == self.ref.ring.tobytes(), (what, "ring")
        assert self.d_tot.cpu().numpy().tobytes() == self.ref.totals.tobytes(), (what, "totals")

    def covered(self, what):
        """The coverage condition, on the reference's output."""
        for bit in (1, 2, 4, 8, 16):
            assert any(f & bit for f in self.flags) and any(not f & bit for f in self.flags), (what, "flag", bit, sorted(set(self.flags)))
        assert True in self.valid and False in self.valid, (what, "valid")


def _constructed_streams(g, S, hop, T):
    """S >= 6 streams of T hops.  Noise everywhere; then, at the level of the STREAM so that runs cross hop borders:
    slot 0: one value from the middle of hop 0 into hop 2 (a run over three hops, a whole hop inside it);
    slot 1: hop 1 is one value, its neighbours differ (a run that is exactly one hop);
    slot 2: clipped samples at the first and the last element of hop 1, and one more hop with a single one;
    slot 3: NaN / inf on the borders of a thread's elements, of a wave and of a tile, two equal-bit NaNs side by side;
    slot 4: a run from element 250 to 262 of hop 2 (thread 62 of wave 0 to thread 65 of wave 1), -0.0 beside +0.0, a denormal;
    slot 5: a gap of zeros over hops 2-3, a DC offset in hop 4.
    Positions past a short hop fold back into it."""
    L = T * hop
    x = (0.2 * g.standard_normal((S, L))).astype(np.float32)
    x[np.abs(x) >= 0.9] = 0.5
    at = lambda k, j: k * hop + min(j, hop - 1)  # noqa: E731
    x[0, hop // 2:2 * hop + (7 * hop) // 10 + 1] = 0.25
    x[1, hop:2 * hop] = 0.125
    x[2, hop], x[2, 2 * hop - 1] = 0.95, -0.97
    x[2, at(3, 5)] = 0.99
    nan_a = np.array([0x7fc00055], dtype=np.uint32).view(np.float32)[0]
    for k, j, v in ((1, 3, NAN), (1, 4, INF), (2, 255, -INF), (2, 256, NAN), (3, 1023, NAN), (3, 1024, INF), (4, 2047, nan_a), (4, 2048, nan_a)):
        x[3, at(k, j)] = v
    x[4, at(2, 250):at(2, 262) + 1] = -0.375
    x[4, at(3, 8):at(3, 8) + 2] = (0.0, -0.0) if hop > 1 else (0.0,)
    x[4, at(1, 2)] = 1e-40  # (a denormal sample: kept in the sum, its square underflows)
    x[5, 2 * hop - 3:4 * hop + 3] = 0.0
    x[5, 4 * hop + 3:5 * hop] += np.float32(0.6)
    return x


def _issue_policy(hop, W):
    from afx.quality import QualityPolicy
    return QualityPolicy(clip=0.9, clip_count=1 if hop == 1 else 2, flat_run=max(2, min(hop, 13)), quiet=1e-3, dc=0.5,
                         max_bad=0 if W == 1 else 1)


@pytest.mark.parametrize("layout", ["dense", "odd"])
@pytest.mark.parametrize("hop", [1, 3, 255, 256, 257, 1023, 1024, 1025, 4000, 4001])
def test_kernel_equals_the_reference_launch_by_launch(hop, layout):
    """Both sides of a thread's elements, of a wave's 256, of the 1024-sample tile, and the product's hop; rows aligned and
    one float past alignment at a stride that is no multiple of four.  S = 7 slots, six of them named in a new random
    subset and order at every launch until each has had its T = 6 hops; slot 6 is never named.  Every third launch carries
    no scores, the others as a vector or as a column of a matrix."""
    S, T = 7, 6
    W = [1, 2, 16][(hop + (layout == "odd")) % 3]
    g = np.random.default_rng(hop)
    streams = _constructed_streams(g, 6, hop, T)
    mir = _Mirror(S, W, _issue_policy(hop, W), hop)
    mir.poison(31)  # (a ring a previous session left)
    pos, n = [0] * 6, 0
    while min(pos) < T:
        named = [int(s) for s in g.permutation(6)[:g.integers(1, 7)] if pos[s] < T]
        if not named:
            continue
        x = np.stack([streams[s][pos[s] * hop:(pos[s] + 1) * hop] for s in named])
        sc = None if n % 3 == 2 else g.standard_normal(len(named)).astype(np.float32)
        if sc is not None and len(named) > 2:
            sc[1] = NAN
        mir.launch(named, x, [pos[s] + 1 for s in named], sc, layout="column" if layout == "dense" and n % 3 == 1 else layout, what=(hop, layout, n))
        for s in named:
            pos[s] += 1
        n += 1
    assert mir.ref.st[6].tolist() == [0, 0, 0] and mir.ref.ring[6].tolist() == [31] * W
    mir.covered((hop, layout))


@pytest.mark.parametrize("W", [1, 2, 16])
def test_the_window_on_the_device_a_reset_and_a_poisoned_ring(W):
    """k <= W and beyond; mid-stream the slot is reset the way ``Quality.reset`` does it, with the ring poisoned."""
    from afx.quality import QualityPolicy
    hop, S = 64, 3
    p = QualityPolicy(clip=0.9, clip_count=2, flat_run=8, quiet=1e-3, dc=0.5, mask=2 | 4, max_bad=0)
    g = np.random.default_rng(W)
    mir = _Mirror(S, W, p, hop)

    def hop_of(kind):
        x = (0.2 * g.standard_normal(hop)).astype(np.float32).clip(-0.8, 0.8)
        if kind == 1:
            x[[0, hop - 1]] = 0.95
        if kind == 2:
            x[10:30] = x[10]
        return x

    for session in range(2):
        for k in range(1, 2 * W + 4):
            kinds = g.choice([0, 0, 1, 2], S)
            slots = g.permutation(S)
            mir.launch(slots, np.stack([hop_of(kinds[i]) for i in range(S)]), np.full(S, k), g.standard_normal(S).astype(np.float32), what=(W, session, k))
        mir.poison(31)
        mir.ref.reset([0, 2])
        mir.d_st[[0, 2]] = 0
        mir.d_tot[[0, 2]] = 0
    assert True in mir.valid and False in mir.valid


def test_one_row_no_scores_and_bad_rows():
    from afx._lib import lib
    from afx.quality import QualityPolicy
    hop = 160
    p = QualityPolicy(clip=0.9, clip_count=2, flat_run=8, quiet=1e-3, dc=0.5)
    g = np.random.default_rng(5)
    # A = 1, S = 1, with and without scores
    mir = _Mirror(1, 2, p, hop)
    for k in range(1, 5):
        x = (0.3 * g.standard_normal((1, hop))).astype(np.float32).clip(-0.8, 0.8)
        if k == 2:
            x[0, :3] = 0.95
        mir.launch([0], x, [k], None if k % 2 else [1.5], layout="odd" if k > 2 else "dense", what=("A=1", k))
    assert [v for v in mir.valid] == [True, False, False, True]
    # bad rows sit among good ones: slot -1, slot S, a far slot, and k = 0 / k < 0 for a good slot -- skipped whole
    S = 5
    mir = _Mirror(S, 2, p, hop)
    slots = np.array([2, -1, 0, S, 4, 1 << 20, 1, 3])
    ks = np.array([1, 1, 1, 1, 1, 1, 0, -5])
    x = (0.3 * g.standard_normal((slots.size, hop))).astype(np.float32).clip(-0.8, 0.8)
    x[:, :4] = 0.95  # every row would be flagged
    sc = np.arange(slots.size, dtype=np.float32) + 0.5
    out, meas = mir.launch(slots, x, ks, sc, what="bad rows")
    assert (meas[[1, 3, 5, 6, 7]] == -1).all() and out[[1, 3, 5, 6, 7]].tolist() == sc[[1, 3, 5, 6, 7]].tolist()
    assert (meas[[0, 2, 4], 0] == 2).all() and np.isnan(out[[0, 2, 4]]).all()
    assert mir.ref.st[[1, 3]].tolist() == [[0, 0, 0]] * 2 and mir.ref.totals[:, 0].tolist() == [1, 0, 1, 0, 1]
    # bad arguments: an error, nothing launched, no byte of the state changed
    l = lib()
    A = 4
    d_x = torch.zeros(A, hop, device="cuda")
    hdr = torch.tensor([[0, 1], [1, 1], [2, 1], [3, 1]], dtype=torch.int32, device="cuda")
    d_sc, d_out = torch.zeros(A, device="cuda"), torch.zeros(A, device="cuda")
    d_meas = torch.zeros(A, 8, dtype=torch.int32, device="cuda")
    good = [d_x, hop, A, hop, hdr, d_sc, 1, 0.9, 2, 8, 0.16, 80.0, 31, 0, 1, mir.d_ring, 2, mir.d_st, mir.d_tot, S, d_meas, d_out]
    cases = [(0, None), (4, None), (15, None), (17, None), (18, None), (20, None), (21, None), (6, 0), (2, 0), (2, 8193), (3, 0), (1, hop - 1),
             (19, 0), (16, 0), (16, 1025), (7, 0.0), (7, NAN), (8, 0), (9, 1), (10, -1.0), (10, NAN), (11, -1.0), (11, NAN), (12, 32), (12, -1),
             (13, -1), (14, 2)]
    for i, val in cases:
        args = list(good)
        args[i] = val
        rc = l.afx_k_quality(*[_p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], None)
        torch.cuda.synchronize()
        assert rc != 0 and b"quality" in l.afx_last_error(), (i, val)
    mir.check("bad arguments")
    assert d_meas.abs().sum().item() == 0


def test_the_most_rows_one_launch_takes():
    """A = S = 8192 at hop 160, W = 2, three launches in three slot orders; a sixth of the rows flagged each way."""
    from afx.quality import QualityPolicy
    S, hop = 8192, 160
    p = QualityPolicy(clip=0.9, clip_count=2, flat_run=20, quiet=1e-3, dc=0.5, max_bad=0)
    g = np.random.default_rng(8192)
    mir = _Mirror(S, 2, p, hop)
    for k in range(1, 4):
        slots = g.permutation(S)
        x = (0.2 * g.standard_normal((S, hop))).astype(np.float32).clip(-0.8, 0.8)
        kind = g.integers(0, 12, S)
        x[kind == 0, :2] = 0.95
        x[kind == 1, 40:70] = 0.3
        x[kind == 2] = 0.0
        x[kind == 3] += np.float32(0.7)
        x[kind == 4, 159] = NAN
        sc = g.standard_normal(S).astype(np.float32)
        mir.launch(slots, x, np.full(S, k), sc, layout="column" if k == 2 else "dense", what=("8192", k))
    mir.covered("8192 rows")


def test_update_reads_a_view_in_place_and_flags_valid_and_stats_follow():
    """``Quality.update`` on a chunk that is a column block of a wider matrix (row stride 3 hops) and on an expanded row."""
    from afx.quality import Quality, QualityPolicy, QualityState
    hop, S = 256, 4
    p = QualityPolicy(clip=0.9, clip_count=2, flat_run=300, quiet=1e-3, dc=0.2)
    q = Quality(S, p, hop, 4 * hop, "cuda")
    ref = QualityState(S, 4)
    g = np.random.default_rng(2)
    wide = (0.2 * g.standard_normal((3, 3 * hop))).astype(np.float32).clip(-0.8, 0.8)
    wide[1, hop:hop + 2] = 0.95
    d_wide = torch.from_numpy(wide).cuda()
    view = d_wide[:, hop:2 * hop]
    assert view.stride(0) == 3 * hop and not view.is_contiguous()
    sc = torch.tensor([0.5, -0.5, 1.5], device="cuda")
    out, meas = q.update(view, [3, 0, 2], hop_index=1, scores=sc)
    want_out, want = p.step_reference([3, 0, 2], wide[:, hop:2 * hop], 1, sc.cpu().numpy(), ref)
    assert meas.cpu().numpy().tobytes() == want.tobytes() and out.cpu().numpy().view(np.int32).tobytes() == want_out.view(np.int32).tobytes()
    one = torch.full((1, hop), 0.25, device="cuda")
    out, meas = q.update(one.expand(2, hop), [1, 3], hop_index=[1, 2])  # (two rows of one row in memory: made contiguous)
    _, want = p.step_reference([1, 3], np.full((2, hop), 0.25, np.float32), [1, 2], None, ref)
    assert out is None and meas.cpu().numpy().tobytes() == want.tobytes()
    assert q.st.cpu().numpy().tobytes() == ref.st.tobytes() and q.ring.cpu().numpy().tobytes() == ref.ring.tobytes()
    assert q.valid.cpu().tolist() == (ref.st[:, 2] <= 0).tolist() == [False, False, True, False]
    assert q.flags_at([1, 1, 1, 2]).cpu().tolist() == [2, 16, 0, 16] and q.flags_at([0, 0, 0, 1]).cpu().tolist() == [0, 0, 0, 0]
    assert {k: v.tolist() for k, v in q.stats().items()} == dict(hops=[1, 1, 1, 2], nonfinite=[0] * 4, clipped=[1, 0, 0, 0], flat=[0] * 4,
                                                                  quiet=[0] * 4, dc=[0, 1, 0, 1])


def test_measure_offline_equals_run_reference():
    from afx.quality import QualityPolicy
    p = QualityPolicy()
    loud = _clipped(FIX[8000:8000 + 5 * H + 123])
    clips = [torch.from_numpy(FIX[:3 * H].copy()), torch.from_numpy(loud), torch.from_numpy(FIX[108000:108000 + 3 * H].copy()), torch.zeros(100)]
    got = p.measure(clips, H, 16000)
    assert [m.shape for m in got] == [(3, 8), (5, 8), (3, 8), (0, 8)]
    for c, m in zip(clips, got):
        assert m.tobytes() == p.run_reference(c.numpy(), H, 16000)[0].tobytes()
    assert any(m[:, 0].any() for m in got) and not got[0][:, 0].any()
    same = p.measure(torch.stack([clips[0], clips[2]]), H, 16000)
    assert same[0].tobytes() == got[0].tobytes() and same[1].tobytes() == got[2].tobytes()


# ---- engines and scorers -----------------------------------------------------------------------------------------------------
_ENGINES = {}
KINDS = ["sliding", "incremental", "kv"]


def _student(dtype="fp16"):
    if dtype not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES[dtype] = (eng, sd)
    return _ENGINES[dtype]


def _teacher():
    if "teacher" not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype="fp16")
        eng.load_state_dict(sd)
        _ENGINES["teacher"] = (eng, sd)
    return _ENGINES["teacher"]


def _screen(kind, S):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    eng, sd = _student()
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _window(kind):
    return 64000 if kind == "kv" else 16000


def _three_streams(ticks):
    """Slot 0 clean; slot 1 through a saturating stage for hops 3-5; slot 2 a dead leg (one stuck value) over hops 2-3."""
    a = FIX[:ticks * H].copy()
    b = np.roll(FIX, -30057)[:ticks * H].copy()
    b[2 * H:5 * H] = _clipped(b[2 * H:5 * H])
    c = np.roll(FIX, -44000)[:ticks * H].copy()
    c[H + 700:3 * H - 900] = c[H + 699]
    return [a, b, c]


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_where_valid_holds_the_score_is_the_bare_scorers_bit_for_bit(kind):
    """Named subsets in changing orders.  ``out`` is the bare scorer's score where the reference says valid and the quiet NaN
    where it does not; ``last_meas``, ``valid``, ``flags`` and the state follow ``run_reference`` per slot."""
    from afx.quality import QualityPolicy, QualityScorer
    S, ticks = 3, 12
    p = QualityPolicy()
    streams = _three_streams(ticks)
    orders = [None, [2, 0, 1], [1, 2, 0]]

    def run(front, each=None):
        out = []
        for t in range(ticks):
            named = orders[t % 3]
            order = list(range(S)) if named is None else named
            chunk = torch.from_numpy(np.stack([streams[s][t * H:(t + 1) * H] for s in order])).cuda()
            sc = front.push(chunk) if named is None else front.push(chunk, named)
            out.append((order, None if sc is None else sc.clone()))
            if each is not None:
                each(t, order)
        return out

    dry = run(_screen(kind, S))
    want = [p.run_reference(streams[s], H, _window(kind)) for s in range(S)]
    valid_ref = np.stack([v for _, v in want], axis=1)  # (ticks, S)
    assert valid_ref[:, 0].all() and not valid_ref[:, 1].all() and not valid_ref[:, 2].all() and valid_ref[0].all(), "the fixture"
    assert (want[1][0][:, 0] & 2).any() and (want[2][0][:, 0] & 4).any() and not want[0][0][:, 0].any(), "the fixture"
    qs = QualityScorer(_screen(kind, S), p)

    def each(t, order):
        assert qs.last_meas.cpu().numpy().tobytes() == np.stack([want[s][0][t] for s in order]).tobytes(), (kind, t)
        assert qs.valid.cpu().tolist() == valid_ref[t].tolist() and qs.flags.cpu().tolist() == [int(want[s][0][t, 0]) for s in range(S)], (kind, t)

    got = run(qs, each)
    withheld = 0
    for t, ((o1, a), (o2, b)) in enumerate(zip(got, dry)):
        assert o1 == o2 and (a is None) == (b is None), (kind, t)
        if a is None:
            continue
        ok = torch.from_numpy(valid_ref[t, o1])
        expect = _ibits(b.to(torch.float32).cpu()).clone()
        expect[~ok] = QNAN
        assert torch.equal(_ibits(a.cpu()), expect), (kind, t)
        withheld += int((~ok).sum())
    assert withheld >= 3
    st = qs.stats()
    assert st["hops"].tolist() == [ticks] * S and st["clipped"].tolist() == [int((m[:, 0] & 2 != 0).sum()) for m, _ in want]
    assert qs.samples_seen.tolist() == [ticks * H] * S


def test_under_the_verdict_layer_no_alarm_while_clipped_and_one_after_w_clean_hops():
    """enter = +inf: every score the verdict layer is given sits under it, so a slot raises at the first score it is GIVEN.
    Slot 0 is clean and raises at hop 1.  Slot 1 is clipped over hops 1-5 (W = 4): its scores are withheld through hop 8 and
    it raises at hop 9, after W clean hops.  Events and state are ``VerdictPolicy.step_reference``'s fed the bare scorer's
    scores with NaN where ``run_reference`` says not valid."""
    from afx.quality import QualityPolicy, QualityScorer
    from afx.verdict import VerdictPolicy, VerdictScorer, new_state
    S, ticks = 2, 11
    qp, vp = QualityPolicy(), VerdictPolicy(INF, INF, latch=True)
    streams = [FIX[:ticks * H].copy(), FIX[48000:48000 + ticks * H].copy()]  # (slot 1: 8 hops of the tone, then noise)
    streams[1][:5 * H] = _clipped(streams[1][:5 * H])
    hops = lambda t: torch.from_numpy(np.stack([s[t * H:(t + 1) * H] for s in streams])).cuda()  # noqa: E731
    bare = _screen("sliding", S)
    dry = [bare.push(hops(t)).clone().cpu().numpy() for t in range(ticks)]
    ref = [qp.run_reference(s, H, 16000) for s in streams]
    assert [bool(m[0] & 2) for m in ref[1][0]] == [True] * 5 + [False] * 6 and not ref[0][0][:, 0].any(), "the fixture"
    assert ref[1][1].tolist() == [False] * 8 + [True] * 3
    vs = VerdictScorer(QualityScorer(_screen("sliding", S), qp), vp)
    state, want = new_state(S), []
    for t in range(ticks):
        sc = vs.push(hops(t))
        fed = dry[t].copy()
        fed[[not ref[s][1][t] for s in range(S)]] = NAN
        assert sc.cpu().numpy().view(np.int32).tobytes() == fed.view(np.int32).tobytes(), t
        want += vp.step_reference([0, 1], fed, t + 1, *state)
        assert vs.alarm.cpu().tolist() == [True, t + 1 >= 9], t
    slot, kind, k, sm = vs.take_events()
    assert list(zip(slot.tolist(), kind.tolist(), k.tolist(), sm.view(np.int32).tolist())) == want
    assert [(e[0], e[1], e[2]) for e in want] == [(0, 1, 1), (1, 1, 9)]
    assert vs.verdicts.st.cpu().numpy().tobytes() == state[1].tobytes() and _same_bits(vs.smoothed, torch.from_numpy(state[0]))
    assert vs.verdicts.st[1].tolist() == [3, 0, 1, 9]  # the withheld scores were not taken: n counts hops 9, 10, 11


def test_around_a_cascade_an_invalid_slots_verifier_score_does_not_raise():
    """Every slot is verified at every hop from 2 H on (threshold +inf, budget S).  enter = -inf: the smoothed score never
    raises; verifier_enter = +inf: any verifier score raises.  Slot 1 is clipped throughout: it is verified like the others
    and must not raise.  Without the quality layer the same chain raises it."""
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.quality import QualityPolicy, QualityScorer
    from afx.verdict import VerdictPolicy, VerdictScorer, new_state
    S, ticks = 3, 5
    teacher, tsd = _teacher()
    cpol, qp = CascadePolicy(INF, S, 0, 2 * H), QualityPolicy()
    vp = VerdictPolicy(-INF, INF, verifier_enter=INF, latch=True)
    streams = [np.roll(FIX, -o)[:ticks * H].copy() for o in (0, 30057, 44000)]
    streams[1] = _clipped(streams[1])
    hops = lambda t: torch.from_numpy(np.stack([s[t * H:(t + 1) * H] for s in streams])).cuda()  # noqa: E731
    ref_valid = np.stack([qp.run_reference(s, H, 64000)[1] for s in streams], axis=1)
    assert ref_valid[:, [0, 2]].all() and not ref_valid[:, 1].any(), "the fixture"

    def run(front, cascade):
        rows = []
        for t in range(ticks):
            sc = front.push(hops(t)).clone()
            v = np.full(S, NAN, np.float32)
            for slots, _at, _s, vsc in cascade.take_events():
                v[slots.tolist()] = vsc.cpu().numpy()
            rows.append((sc.cpu().numpy(), v))
        return rows

    plain_c = CascadeScorer(_screen("kv", S), teacher, cpol, state_dict=tsd)
    plain = VerdictScorer(plain_c, vp)
    dry = run(plain, plain_c)
    assert sorted(plain.take_events()[0].tolist()) == [0, 1, 2]  # without the quality layer slot 1 is raised by its verifier score
    cs = CascadeScorer(_screen("kv", S), teacher, cpol, state_dict=tsd)
    qs = QualityScorer(cs, qp)
    vs = VerdictScorer(qs, vp)
    assert vs._verified
    got = run(vs, qs)  # (take_events is the cascade's, forwarded: the verifier scores as the verifier gave them)
    state, want = new_state(S), []
    for t, ((sc, v), (sc0, v0)) in enumerate(zip(got, dry)):
        assert v.tobytes() == v0.tobytes() and (t < 1 or not np.isnan(v).any()), t
        fed = sc0.copy()
        fed[~ref_valid[t]] = NAN
        assert sc.view(np.int32).tobytes() == fed.view(np.int32).tobytes(), t
        want += vp.step_reference([0, 1, 2], fed, t + 1, *state, np.where(ref_valid[t], v, np.float32(NAN)).astype(np.float32))
    slot, kind, k, sm = vs.take_events()
    assert list(zip(slot.tolist(), kind.tolist(), k.tolist(), sm.view(np.int32).tolist())) == want
    assert sorted(slot.tolist()) == [0, 2] and set(kind.tolist()) == {2} and vs.alarm.cpu().tolist() == [True, False, True]
    assert not torch.isnan(qs.verified).any()  # slot 1 WAS verified
    chosen, v = qs.last_verified()
    v = v.cpu()
    assert torch.isnan(v[chosen == 1]).all() and not torch.isnan(v[chosen != 1]).any()


def test_behind_the_gate_the_hops_measured_are_the_gated_streams():
    """``GatedScorer(QualityScorer(screen))``: the quality layer sees the hops of the kept samples.  Its meas rows, in the
    order the inner session completed hops, are ``run_reference`` over ``gate_reference``'s kept samples."""
    from afx.quality import QualityPolicy, QualityScorer
    from afx.vad import GatedScorer, SpeechGate
    S, ticks = 2, 20
    qp, gate = QualityPolicy(), SpeechGate()
    streams = [FIX[:ticks * H].copy(), np.roll(FIX, -30057)[:ticks * H].copy()]
    streams[1][8 * H:12 * H] = _clipped(streams[1][8 * H:12 * H])
    qs = QualityScorer(_screen("kv", S), qp)
    front = GatedScorer(qs, gate)
    bare = GatedScorer(_screen("kv", S), gate)
    rows, outs, plain = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for t in range(ticks):
        chunk = torch.from_numpy(np.stack([s[t * H:(t + 1) * H] for s in streams])).cuda()
        before = qs.samples_seen.clone()
        sc, sc0 = front.push(chunk).cpu(), bare.push(chunk).cpu()
        done = ((qs.samples_seen - before) > 0).tolist()
        meas = qs.last_meas.cpu().numpy()
        at = 0
        for s in range(S):
            if done[s]:
                rows[s].append(meas[at].tolist())
                outs[s].append(sc[s:s + 1].clone())
                plain[s].append(sc0[s:s + 1].clone())
                at += 1
            else:
                assert bool(torch.isnan(sc[s])) and bool(torch.isnan(sc0[s]))  # the gate's own NaN: no hop completed
    withheld = 0
    for s in range(S):
        kept = gate.gate_reference(streams[s])[1]
        want, valid = qp.run_reference(kept, H, 64000)
        assert len(rows[s]) == kept.size // H >= 4 and rows[s] == want.tolist(), s
        for j, ok in enumerate(valid.tolist()):
            assert _same_bits(outs[s][j], plain[s][j]) if ok else int(_ibits(outs[s][j])) == QNAN, (s, j)
            withheld += not ok
    assert withheld >= 1


# ---- 3. sessions ---------------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_moved_sessions_continue_bit_for_bit_with_a_run_in_progress(kind):
    """Two sessions move after tick 4 into other slots of a scorer in use, under another clip and mask.  Session 1 has a
    stuck value from the middle of hop 3 to the middle of hop 6: the run is in progress at the move."""
    from afx.quality import QualityPolicy, QualityScorer
    from afx.streaming import StreamState
    t0, ticks = 4, 8
    p = QualityPolicy()
    streams = [np.roll(FIX, -2000)[:ticks * H].copy(), np.roll(FIX, -50000)[:ticks * H].copy()]
    streams[0][H:2 * H] = _clipped(streams[0][H:2 * H])
    streams[1][3 * H + 1500:6 * H + 2000] = streams[1][3 * H + 1499]
    hopsof = lambda t, rows: torch.from_numpy(np.stack([streams[i][t * H:(t + 1) * H] for i in rows])).cuda()  # noqa: E731
    step = lambda front, t, s0, s1: (front.push(hopsof(t, [1, 0]), [s1, s0]).clone(), front.last_meas.clone())  # noqa: E731

    never = QualityScorer(_screen(kind, 3), p)
    ref = [step(never, t, 0, 2) for t in range(ticks)]
    a = QualityScorer(_screen(kind, 3), p)
    for t in range(t0):
        sc, meas = step(a, t, 0, 2)
        assert _same_bits(sc, ref[t][0]) and torch.equal(meas, ref[t][1])
    st = a.export_slots([0, 2])
    assert int(st.tensors["quality_state"][1, 1]) == H - 1500 + 1 and st.tensors["quality_state"][1, 2] >= 1  # mid-run, and flagged
    b = QualityScorer(_screen(kind, 4), p)
    b.push(torch.from_numpy(np.stack([FIX[8000:12000], FIX[48000:52000]])).cuda(), [3, 0])  # the destination is in use
    snap = lambda c: (c.quality.ring.clone(), c.quality.st.clone(), c.quality.totals.clone(), c.samples_seen)  # noqa: E731
    before = snap(b)
    moved = _move(st)
    t = moved.tensors
    W = b.quality.W
    refused = [a.scorer.export_slots([0, 2]),                                                                # no quality part
               StreamState(dict(moved.meta, quality=2), moved.seen, t),                                      # a foreign format
               StreamState(dict(moved.meta, quality_window=dict(W=W + 1, hop=H)), moved.seen, t),            # a wrong W
               StreamState(moved.meta, moved.seen, dict(t, quality_state=torch.tensor([[0, -1, 0], [0, 5, 0]]))),      # a negative run
               StreamState(moved.meta, moved.seen, dict(t, quality_state=torch.tensor([[0, 1, W + 1], [0, 5, 0]])))]  # bad > W
    for i, state in enumerate(refused):
        with pytest.raises(ValueError):
            b.import_slots([3, 1], state)
        assert all(torch.equal(u, v) for u, v in zip(before, snap(b))), i
    with pytest.raises(ValueError):
        b.scorer.import_slots([3, 1], moved)  # a bare scorer refuses a quality state
    b.import_slots([3, 1], moved)
    assert torch.equal(b.quality.st[[0, 2]], before[1][[0, 2]]) and torch.equal(b.quality.ring[[0, 2]], before[0][[0, 2]])
    for t_ in range(t0, ticks):
        sc, meas = step(b, t_, 3, 1)
        assert _same_bits(sc, ref[t_][0]) and torch.equal(meas, ref[t_][1]), t_
    assert torch.equal(b.quality.st[[3, 1]], never.quality.st[[0, 2]]) and torch.equal(b.quality.totals[[3, 1]], never.quality.totals[[0, 2]])
    assert torch.equal(b.quality.ring[[3, 1]], never.quality.ring[[0, 2]])
    # the run that crossed the move was measured whole: its longest value is the stream's
    longest = max(int(m[1][0, 3]) for m in ref)
    assert longest == 3 * H + 500 + 1

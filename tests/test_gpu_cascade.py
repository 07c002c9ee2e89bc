"""The cascade on the GPU (afx/cascade.py; afx_k_cascade_store / _select / _windows).  Every comparison is exact: the select
kernel against ``CascadePolicy.select_reference`` over consecutive launches that carry ``wait``; the store and windows
kernels against a numpy mirror of a ring pre-filled with random values; ``CascadeScorer`` end to end for the four screen
kinds (its scores against a dry run of the bare screen, its events against the reference applied to those scores, every
verifier score against ``verifier.forward`` on a window built in numpy from the pushed audio); behind the gate and the packet
front; and sessions moved between scorers.

Tiny engines as in tests/test_gpu_vad.py: a 1-layer Conformer student screens, a 1-layer XLSR_AASIST teacher verifies,
H = 4000.  The exact screens run a 1-s window, the KV-cached screen its 4-s window."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
INF, NAN = float("inf"), float("nan")


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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- 1. the select kernel against select_reference -------------------------------------------------------------------------
_VALUES = np.array([-INF, -2.0, -0.5, -0.0, 0.0, 0.25, 0.25, 0.5, 1.0, 3.0, INF, NAN], dtype=np.float32)


def _select(scores, stride, hdr, A, wait, counts, S, thr, budget, cooldown, sel):
    from afx._lib import call_on, lib
    rc = call_on(wait, lib().afx_k_cascade_select, _p(scores), stride, _p(hdr), A, _p(wait), _p(counts), S, thr, budget, cooldown, _p(sel))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("A", [1, 5, 64, 65, 257, 1000, 2500, 8192])
def test_select_kernel_equals_the_reference_launch_by_launch(A):
    """A above 1024: a thread owns several rows (2500: not a multiple; 8192: the most one launch takes)."""
    from afx.cascade import CascadePolicy
    S, SENT = A + 3, -77
    g = np.random.default_rng(A)
    for budget in (sorted({1, 3, 64, min(A, 1024)}) if A <= 2500 else [3, 1024]):
        cooldown = int(g.integers(0, 4))
        m_wait = (g.integers(1, 4, S) * (g.random(S) < 0.3)).astype(np.int32)  # (some slots begin in cooldown)
        m_counts = np.zeros((S, 2), dtype=np.int32)
        wait, counts = torch.from_numpy(m_wait.copy()).cuda(), torch.zeros(S, 2, dtype=torch.int32, device="cuda")
        seen_all = seen_none = seen_bound = False
        for launch in range(6):
            slots = g.permutation(S)[:A]
            elig = g.random(A) < 0.85
            sc = _VALUES[g.integers(0, _VALUES.size, A)].copy()
            thr = [0.5, INF, 0.25, -3.0e38, 0.0, 1.5][launch]
            if launch == 1:  # every row a candidate: eligible, out of cooldown, a finite or -inf score under threshold = +inf
                elig[:] = True
                sc = np.where(np.isnan(sc) | (sc == INF), np.float32(0.25), sc)
                m_wait[:] = 0
                wait.zero_()
            if launch == 3:  # no candidate: nothing is below the lowest finite threshold but -inf
                sc = np.where(sc == -INF, np.float32(-2.0), sc)
            policy = CascadePolicy(thr, budget, cooldown)
            with np.errstate(invalid="ignore"):
                cand = elig & (m_wait[slots] == 0) & (sc < np.float32(thr))
            want_sel, want_wait = policy.select_reference(slots, sc, elig, m_wait)
            chosen = np.zeros(A, dtype=bool)
            chosen[want_sel] = True
            m_counts[slots, 0] += cand
            m_counts[slots, 1] += cand & ~chosen
            strided = launch % 2 == 1  # (a column of a logits matrix, read in place)
            mat = torch.full((A, 2), 9.0)
            mat[:, 1] = torch.from_numpy(sc)
            d_sc = mat.cuda()[:, 1] if strided else torch.from_numpy(sc).cuda()
            hdr = torch.from_numpy(np.stack([slots, elig], axis=1).astype(np.int32)).cuda()
            sel = torch.full((1 + budget,), SENT, dtype=torch.int32, device="cuda")
            assert _select(d_sc, 2 if strided else 1, hdr, A, wait, counts, S, float(thr), budget, cooldown, sel) == 0
            got = sel.cpu().numpy()
            n = len(want_sel)
            assert got[0] == n and got[1:1 + n].tolist() == want_sel, (A, budget, launch)
            assert (got[1 + n:] == SENT).all(), (A, budget, launch)  # entries past the count are not written
            m_wait = want_wait.astype(np.int32)
            assert wait.cpu().numpy().tobytes() == m_wait.tobytes(), (A, budget, launch)  # (unnamed slots' wait included)
            assert counts.cpu().numpy().tobytes() == m_counts.tobytes(), (A, budget, launch)
            seen_all |= bool(cand.all())
            seen_none |= not cand.any()
            seen_bound |= int(cand.sum()) > budget
        assert seen_all and seen_none and (seen_bound or budget >= A), (A, budget)


def test_select_skips_bad_rows_and_refuses_bad_arguments():
    from afx._lib import lib
    from afx.cascade import CascadePolicy
    S, A, budget = 4, 5, 3
    slots = [2, -1, 0, 4, 3]  # rows 1 and 3 name no slot of the state: skipped whole
    sc = torch.tensor([0.1, -5.0, 0.2, -6.0, 0.3], device="cuda")
    hdr = torch.tensor([[s, 1] for s in slots], dtype=torch.int32, device="cuda")
    wait = torch.zeros(S, dtype=torch.int32, device="cuda")
    counts = torch.zeros(S, 2, dtype=torch.int32, device="cuda")
    sel = torch.full((1 + budget,), -77, dtype=torch.int32, device="cuda")
    assert _select(sc, 1, hdr, A, wait, counts, S, 1.0, budget, 2, sel) == 0
    want, w = CascadePolicy(1.0, budget, 2).select_reference([2, 0, 3], np.array([0.1, 0.2, 0.3], np.float32), [1, 1, 1], [0] * S)
    assert sel.tolist() == [3, 0, 2, 4] and [[0, 2, 4][i] for i in want] == [0, 2, 4] and wait.tolist() == w.tolist() == [2, 0, 2, 2]
    assert counts.tolist() == [[1, 0], [0, 0], [1, 0], [1, 0]]
    # counts is optional
    wait.zero_()
    assert _select(sc, 1, hdr, A, wait, None, S, 1.0, 1, 2, sel) == 0 and sel.tolist()[:2] == [1, 0] and wait.tolist() == [0, 0, 2, 0]
    # bad arguments: an error, nothing launched (A above 8192 included)
    before = (wait.clone(), sel.clone())
    big = torch.zeros(8193, device="cuda")
    bhdr = torch.zeros(8193, 2, dtype=torch.int32, device="cuda")
    for args in ((big, 1, bhdr, 8193, wait, None, S, 1.0, 1, 0, sel), (sc, 1, hdr, 0, wait, None, S, 1.0, 1, 0, sel),
                 (sc, 1, hdr, A, wait, None, 0, 1.0, 1, 0, sel), (sc, 1, hdr, A, wait, None, S, 1.0, 0, 0, sel),
                 (sc, 1, hdr, A, wait, None, S, 1.0, 1, -1, sel), (sc, 0, hdr, A, wait, None, S, 1.0, 1, 0, sel),
                 (sc, 1, hdr, A, wait, None, S, NAN, 1, 0, sel), (None, 1, hdr, A, wait, None, S, 1.0, 1, 0, sel),
                 (sc, 1, None, A, wait, None, S, 1.0, 1, 0, sel), (sc, 1, hdr, A, None, None, S, 1.0, 1, 0, sel),
                 (sc, 1, hdr, A, wait, None, S, 1.0, 1, 0, None)):
        rc = lib().afx_k_cascade_select(*[_p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], None)
        torch.cuda.synchronize()
        assert rc != 0 and b"cascade_select" in lib().afx_last_error(), args[3:]
    assert torch.equal(before[0], wait) and torch.equal(before[1], sel)


# ---- 2. the store and windows kernels against a numpy mirror -------------------------------------------------------------
@pytest.mark.parametrize("hop,window", [(800, 3200), (250, 1750), (4000, 64000)])
def test_store_and_windows_kernels_equal_a_numpy_mirror(hop, window):
    from afx._lib import call_on, lib
    S, budget, SENT = 6, 8, -123.0
    g = torch.Generator().manual_seed(hop)
    mirror = torch.randn(S, window, generator=g).numpy().copy()  # (not zeros: a stray write shows)
    ring = torch.from_numpy(mirror).cuda()
    rng = np.random.default_rng(window)

    def store(slots, wpos):
        x = rng.standard_normal((len(slots), hop)).astype(np.float32)
        hdr = torch.tensor(list(zip(slots, wpos)), dtype=torch.int32, device="cuda")
        dx = torch.from_numpy(x).cuda()
        rc = call_on(ring, lib().afx_k_cascade_store, _p(dx), len(slots), hop, _p(hdr), _p(ring), S, window)
        torch.cuda.synchronize()
        assert rc == 0
        for i, (s, w) in enumerate(zip(slots, wpos)):
            if 0 <= s < S and 0 <= w < window:
                mirror[s, (w + np.arange(hop)) % window] = x[i]
        assert ring.cpu().numpy().tobytes() == mirror.tobytes(), (slots, wpos)

    store([0, 1, 2, 3, 4, 5], [0, hop, window - hop, window - hop // 2, 1, window - 1])  # aligned, to the end, wrapping, odd, last column
    store([5, 3], [window - hop + 4, 3 * hop + 3])  # a subset, in another order: the other slots' rows are untouched
    store([2, -1, 0, S, 4, 1], [7, 0, window, 0, -1, 2 * hop])  # bad slots and bad wpos: those rows are skipped whole
    store([4], [window - 3])

    def windows(rows, sel_list, count=None, A=None):
        """rows: (slot, n, start) per header row; sel_list: the row positions sel names."""
        A = len(rows) if A is None else A
        hdr = torch.tensor(rows, dtype=torch.int32, device="cuda")
        count = len(sel_list) if count is None else count
        sel = torch.tensor([count] + list(sel_list) + [0] * (budget - len(sel_list)), dtype=torch.int32, device="cuda")
        out = torch.full((budget, window), SENT, device="cuda")
        rc = call_on(ring, lib().afx_k_cascade_windows, _p(ring), S, window, _p(hdr), A, _p(sel), budget, _p(out))
        torch.cuda.synchronize()
        assert rc == 0
        want = np.full((budget, window), SENT, dtype=np.float32)
        for r, i in enumerate(sel_list[:min(count, budget)]):
            if not 0 <= i < A:
                continue
            s, n, st = rows[i]
            if 0 <= s < S and 1 <= n <= window and 0 <= st < n:
                want[r] = mirror[s, (st + np.arange(window)) % n]
        assert out.cpu().numpy().tobytes() == want.tobytes(), (rows, sel_list, count)
        assert ring.cpu().numpy().tobytes() == mirror.tobytes()  # (the ring is only read)
        return want

    odd_n = 401 if window >= 401 else hop + 1
    rows = [(0, hop, 0), (1, 3 * hop, 0), (2, odd_n, 0), (3, window, 0), (4, window, 4 * (window // 8)), (5, window, 1),
            (0, window, window - 1), (1, window, hop + 3)]
    # warm (n = hop, 3 hop, 401), steady (start 0, a multiple of 4, odd, the last column); 5 rows for a budget of 8
    w = windows(rows, [2, 0, 4, 6, 1])
    assert (w[5:] == SENT).all() and (w[:5] != SENT).all()
    assert np.array_equal(w[1][:hop], mirror[0, :hop]) and np.array_equal(w[1][hop:2 * hop], mirror[0, :hop])  # tiled
    windows(rows, [7, 6, 5, 4, 3, 2, 1, 0])  # a full budget
    windows(rows, [])  # nothing chosen: nothing written
    windows(rows, [3, 1, 5, 2, 0, 4, 6, 7], count=budget + 3)  # a count beyond the budget reads budget entries
    windows(rows, [3, 5, 1], count=2)  # entries past the count are not read
    # bad headers and bad sel entries: those rows of out are skipped whole
    bad = [(S, hop, 0), (-1, hop, 0), (0, 0, 0), (1, window + 1, 0), (2, hop, hop), (3, window, -1), (4, window, window), (5, hop, 0)]
    w = windows(bad, [0, 1, 2, 3, 4, 5, 6, 7])
    assert (w[:7] == SENT).all() and (w[7] != SENT).all()
    w = windows(rows, [-1, 8, 3], A=8)
    assert (w[:2] == SENT).all() and (w[2] != SENT).all()
    w = windows(rows, [7, 3], A=7)  # (row 7 is outside a table of 7 rows)
    assert (w[0] == SENT).all() and (w[1] != SENT).all()
    # bad arguments: an error, nothing launched
    l = lib()
    x, hdr = torch.zeros(1, hop, device="cuda"), torch.zeros(1, 3, dtype=torch.int32, device="cuda")
    sel, out = torch.zeros(1 + budget, dtype=torch.int32, device="cuda"), torch.full((budget, window), SENT, device="cuda")
    for args in ((None, 1, hop, _p(hdr), _p(ring), S, window), (_p(x), 0, hop, _p(hdr), _p(ring), S, window),
                 (_p(x), 1, 0, _p(hdr), _p(ring), S, window), (_p(x), 1, window + 1, _p(hdr), _p(ring), S, window),
                 (_p(x), 1, hop, _p(hdr), _p(ring), 0, window), (_p(x), 1, hop, None, _p(ring), S, window)):
        assert l.afx_k_cascade_store(*args, None) != 0 and b"cascade_store" in l.afx_last_error(), args[1:3]
    for args in ((None, S, window, _p(hdr), 1, _p(sel), budget, _p(out)), (_p(ring), 0, window, _p(hdr), 1, _p(sel), budget, _p(out)),
                 (_p(ring), S, 0, _p(hdr), 1, _p(sel), budget, _p(out)), (_p(ring), S, window, _p(hdr), 0, _p(sel), budget, _p(out)),
                 (_p(ring), S, window, _p(hdr), 1, _p(sel), 0, _p(out)), (_p(ring), S, window, _p(hdr), 1, None, budget, _p(out)),
                 (_p(ring), S, window, _p(hdr), 1, _p(sel), budget, None)):
        assert l.afx_k_cascade_windows(*args, None) != 0 and b"cascade_windows" in l.afx_last_error(), args[1:5]
    torch.cuda.synchronize()
    assert ring.cpu().numpy().tobytes() == mirror.tobytes() and bool((out == SENT).all())


# ---- engines and screens -----------------------------------------------------------------------------------------------------
_ENGINES = {}


def _student(dtype):
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
    eng, sd = _student("fp16x3" if kind == "kv-fp16x3" else "fp16")
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _cascade(kind, S, policy):
    from afx.cascade import CascadeScorer
    teacher, tsd = _teacher()
    return CascadeScorer(_screen(kind, S), teacher, policy, state_dict=tsd)


def _window_of(history, window):
    """history: the hops a session was pushed since its reset (numpy rows) -> its window as the module docstring defines it."""
    h = np.concatenate(history)
    h = h[-min(h.size, window):]
    return h[np.arange(window) % h.size]


def _verify_alone(W):
    teacher, _ = _teacher()
    return teacher.forward(torch.from_numpy(np.ascontiguousarray(W)[None]).cuda())[0, 1]


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------
_TICKS, _RESET_AT = 22, 9


def _schedule(t):
    """None: the lock-stepped push; else the named slots, in the order named (slot 1 sits out one tick in four)."""
    return [None, [2, 0, 1], [1, 2, 0], [0, 2]][t % 4]


def _run(front, streams, S, on_tick=None):
    """Pushes the schedule into ``front`` (a bare screen or a cascade), slot 1 reset before tick _RESET_AT -> per tick
    (slots in the order of the returned scores, the scores on the host)."""
    pos, out = [0] * S, []
    for t in range(_TICKS):
        if t == _RESET_AT:
            front.reset([1])
        named = _schedule(t)
        order = list(range(S)) if named is None else named
        chunk = torch.from_numpy(np.stack([streams[s][pos[s]:pos[s] + H] for s in order])).cuda()
        sc = front.push(chunk) if named is None else front.push(chunk, named)
        assert sc.shape == (len(order),) and sc.dtype == torch.float32 and sc.is_cuda
        out.append((order, sc.clone()))
        if on_tick is not None:
            on_tick(t, order, [streams[s][pos[s]:pos[s] + H] for s in order])
        for s in order:
            pos[s] += H
    return out


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv", "kv-fp16x3"])
def test_cascade_end_to_end_equals_the_screen_the_reference_and_the_verifier_alone(kind):
    from afx.cascade import CascadePolicy
    S, budget, cooldown, min_samples = 3, 1, 2, 2 * H
    streams = [np.roll(FIX, -o)[:_TICKS * H].copy() for o in (0, 30000 + 57, 44000)]
    dry = _run(_screen(kind, S), streams, S)
    thr = float(np.median(torch.cat([sc for _, sc in dry]).cpu().numpy()))
    policy = CascadePolicy(thr, budget, cooldown, min_samples)
    cs = _cascade(kind, S, policy)
    window = cs.window
    assert (cs.hist is None) == (kind in ("sliding", "incremental"))  # only the KV-cached screen pays for a second ring

    history = [[] for _ in range(S)]
    wait = np.zeros(S, dtype=np.int64)
    seen = np.zeros(S, dtype=np.int64)
    want_events, cover = [], dict(bound=0, none=0, suppressed=0, warm=0, steady=0)
    want_stats = {k: np.zeros(S, dtype=np.int64) for k in ("screened", "candidates", "verified", "passed_over")}
    want_verified_at = np.full(S, -1, dtype=np.int64)
    want_verified = [None] * S
    tick_events = []

    def on_tick(t, order, hops):
        nonlocal wait
        if t == _RESET_AT:  # (the reset came before this tick's push)
            history[1].clear()
            wait[1], seen[1], want_verified_at[1], want_verified[1] = 0, 0, -1, None
        for s, hop in zip(order, hops):
            history[s].append(hop)
            seen[s] += H
        sc = dry[t][1].cpu().numpy()
        elig = seen[order] >= min_samples
        below = elig & (sc < np.float32(thr))
        cand = below & (wait[order] == 0)
        sel, new_wait = policy.select_reference(order, sc, elig, wait)
        cover["bound"] += int(cand.sum()) >= 2 and len(sel) == budget
        cover["none"] += not cand.any()
        cover["suppressed"] += bool((below & (wait[order] > 0)).any())
        for k, v in (("screened", 1), ("candidates", cand), ("passed_over", cand & ~np.isin(np.arange(len(order)), sel))):
            want_stats[k][order] += v
        wait = new_wait
        ev = cs.take_events()
        tick_events.append(len(ev))
        if not sel:
            assert ev == [], t
            return
        assert len(ev) == 1, t
        slots, at, s_scores, v_scores = ev[0]
        assert slots.dtype == at.dtype == torch.int64 and not slots.is_cuda and s_scores.is_cuda and v_scores.is_cuda
        assert slots.tolist() == [order[i] for i in sel] and at.tolist() == [int(seen[order[i]]) for i in sel], t
        assert _same_bits(s_scores, dry[t][1][sel]), t
        for r, i in enumerate(sel):
            s = order[i]
            alone = _verify_alone(_window_of(history[s], window))
            assert _same_bits(v_scores[r:r + 1], alone.reshape(1)), (kind, t, s)
            cover["warm" if seen[s] < window else "steady"] += 1
            want_stats["verified"][s] += 1
            want_verified_at[s], want_verified[s] = seen[s], v_scores[r].clone()
        want_events.append((t, slots.tolist()))

    got = _run(cs, streams, S, on_tick)
    for t, ((o1, a), (o2, b)) in enumerate(zip(got, dry)):
        assert o1 == o2 and _same_bits(a, b), (kind, t)  # (a) the cascade never changes a screen score
    # (d) verified, verified_at and stats() agree with the events
    assert cs.verified_at.tolist() == want_verified_at.tolist()
    for s in range(S):
        if want_verified[s] is None:
            assert bool(torch.isnan(cs.verified[s]))
        else:
            assert _same_bits(cs.verified[s:s + 1], want_verified[s].reshape(1))
    st = cs.stats()
    assert {k: v.tolist() for k, v in st.items()} == {k: v.tolist() for k, v in want_stats.items()}
    assert cs.samples_seen.tolist() == seen.tolist()
    print(f"cascade end to end [{kind}]: threshold {thr!r}, coverage {cover}, events per tick {tick_events}")
    # the run did something: the budget bound, a tick had no candidate, a cooldown suppressed a candidate, warm and steady windows
    assert cover["bound"] >= 1 and cover["none"] >= 1 and cover["suppressed"] >= 1 and cover["warm"] >= 1 and cover["steady"] >= 1, cover


# ---- 4. behind the gate and a front ------------------------------------------------------------------------------------------------
def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the reference decodes the same bytes)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def test_cascade_behind_the_gate_and_the_packet_front():
    from afx.cascade import CascadePolicy
    from afx.ingest import PacketScorer, decode
    from afx.resample import Resampler
    from afx.vad import GatedScorer, SpeechGate
    S, kind, gate, cooldown, min_samples = 3, "kv", SpeechGate(), 3, 2 * H
    cs = _cascade(kind, S, CascadePolicy(INF, S, cooldown, min_samples))
    ps = PacketScorer(GatedScorer(cs, gate), 8000, "mulaw")
    codes = [_mulaw_encode(np.roll(FIX, -o)[:96000:2]) for o in (0, 30000 + 57, 44000)]  # 8 kHz by plain slicing, 6 s each
    events = []
    for k in range(0, codes[0].size, 160):  # 20-ms packets
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        ps.feed([codes[s][k:k + 160].tobytes() for s in named], named)
        events += cs.take_events()
    # the gated stream of each slot, offline: what both models saw
    G = []
    for c in codes:
        g = gate.gate([Resampler(8000)(decode(c, "mulaw")[None])[0]])[0]
        G.append(g[:g.numel() // H * H].reshape(-1, H).cpu().numpy())
    assert cs.samples_seen.tolist() == [g.shape[0] * H for g in G]
    at_of = [[] for _ in range(S)]
    for slots, at, s_scores, v_scores in events:
        for r, (s, a) in enumerate(zip(slots.tolist(), at.tolist())):
            at_of[s].append(a)
            alone = _verify_alone(_window_of(list(G[s][:a // H]), cs.window))  # the window of the slot's gated stream at that hop
            assert _same_bits(v_scores[r:r + 1], alone.reshape(1)), (s, a)
    # threshold = +inf, cooldown 3: one verification per 4 gated hops per slot from min_samples on
    for s in range(S):
        assert at_of[s] == list(range(min_samples, G[s].shape[0] * H + 1, (cooldown + 1) * H)), (s, at_of[s], G[s].shape[0])
    assert sum(len(a) for a in at_of) >= 4 and min(len(a) for a in at_of) >= 1, at_of
    assert cs.stats()["verified"].tolist() == [len(a) for a in at_of] and cs.stats()["passed_over"].tolist() == [0] * S


# ---- 5. sessions ---------------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def _snap(cs):
    st = cs.export_slots(list(range(cs.S)))
    return [st.seen, cs.wait.clone(), cs.verified_at.clone()] + [st.tensors[k].clone() for k in sorted(st.tensors)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and (_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x.cpu(), y.cpu()))
                                    for x, y in zip(a, b))


def _events_as(ev, names):
    """An event log with the slots renamed by ``names`` (a scorer's slot -> the session's number), tensors on the host."""
    return [([names[s] for s in slots.tolist()], at.tolist(), _bits(a.cpu()).tolist(), _bits(b.cpu()).tolist()) for slots, at, a, b in ev]


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_moved_sessions_continue_bit_for_bit(kind):
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.vad import GatedScorer
    t0, ticks, cooldown = 3, 12, 2
    policy = CascadePolicy(INF, 1, cooldown, 2 * H)  # every eligible slot out of cooldown is a candidate; the scores rank them
    streams = [np.roll(FIX, -2000)[:ticks * H], np.roll(FIX, -50000)[:ticks * H]]
    hopsof = lambda t, rows: torch.from_numpy(np.stack([streams[i][t * H:(t + 1) * H] for i in rows])).cuda()  # noqa: E731
    never = _cascade(kind, 3, policy)
    ref = torch.stack([never.push(hopsof(t, [0, 1]), [0, 2]).clone() for t in range(ticks)])  # (ticks, 2)
    ref_events = _events_as(never.take_events(), {0: 0, 2: 1})
    # budget 1 and two slots that cool down for 2 hops: from 2 H on, one verification at two ticks out of three
    assert len(ref_events) == len([t for t in range(1, ticks) if t % 3]) and all(len(e[0]) == 1 for e in ref_events)

    a = _cascade(kind, 3, policy)
    for t in range(t0):
        assert _same_bits(a.push(hopsof(t, [1, 0]), [2, 0]), ref[t].flip(0))
    ev = _events_as(a.take_events(), {0: 0, 2: 1})
    st = a.export_slots([0, 2])
    # one session was verified by the last push (wait = cooldown), the other is in the middle of its cooldown
    assert sorted(st.tensors["cascade_wait"].tolist()) == [1, cooldown] and (st.tensors["cascade_verified_at"] >= 0).all()
    assert ("cascade_samples" in st.tensors) == (kind == "kv")
    teacher, tsd = _teacher()
    b = _cascade(kind, 4, policy)
    b.push(torch.from_numpy(np.stack([FIX[8000:12000], FIX[48000:52000]])).cuda(), [3, 0])  # the destination is in use
    # refusals, each with the destination unchanged
    other_weights = {k: (v + 1 if torch.is_tensor(v) and v.dtype.is_floating_point else v) for k, v in tsd.items()}
    for dest, state in ((CascadeScorer(_screen(kind, 4), teacher, CascadePolicy(INF, 1, cooldown + 1, 2 * H), state_dict=tsd), _move(st)),
                        (CascadeScorer(_screen(kind, 4), teacher, policy, state_dict=other_weights), _move(st)),
                        (b, a.screen.export_slots([0, 2])),                          # no cascade part
                        (b, GatedScorer(_screen(kind, 3)).export_slots([0, 2]))):    # a GatedScorer state
        before = _snap(dest)
        with pytest.raises(ValueError):
            dest.import_slots([3, 1], state)
        assert _same(before, _snap(dest))
    with pytest.raises(ValueError):
        b.screen.import_slots([3, 1], _move(st))  # a bare screen refuses a cascade state
    others = b.export_slots([0, 2])
    b.import_slots([3, 1], _move(st))
    after = b.export_slots([0, 2])
    assert _same([others.seen] + [others.tensors[k] for k in sorted(others.tensors)],
                 [after.seen] + [after.tensors[k] for k in sorted(after.tensors)])  # the destination's other slots are untouched
    assert b.take_events() == []
    for t in range(t0, ticks):
        assert _same_bits(b.push(hopsof(t, [1, 0]), [1, 3]), ref[t].flip(0)), t
    ev += _events_as(b.take_events(), {3: 0, 1: 1})
    assert ev == ref_events  # the selections, the screen scores and the verifier scores of a scorer that never moved
    assert b.samples_seen.tolist() == [H, ticks * H, 0, ticks * H]
    assert _same_bits(b.verified[[3, 1]], never.verified[[0, 2]]) and b.verified_at[[3, 1]].tolist() == never.verified_at[[0, 2]].tolist()


# ---- 6. ValueErrors ------------------------------------------------------------------------------------------------------------------
def test_what_the_cascade_refuses():
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.ingest import PacketScorer
    from afx.vad import GatedScorer
    teacher, tsd = _teacher()
    pol = CascadePolicy(0.0, 2)
    for front in (PacketScorer(_screen("sliding", 2), 8000, "mulaw"), GatedScorer(_screen("sliding", 2)), _cascade("sliding", 2, pol)):
        with pytest.raises(ValueError):
            CascadeScorer(front, teacher, pol)
    with pytest.raises(ValueError):
        CascadeScorer(_screen("sliding", 1), teacher, pol)  # a budget above S
    with pytest.raises(ValueError):
        CascadeScorer(_screen("sliding", 2), torch.nn.Linear(16000, 2), pol)  # a verifier on another device (the host)
    cs = _cascade("kv", 2, pol)
    for chunk, slots in ((torch.zeros(2, H - 1, device="cuda"), None), (torch.zeros(1, H, device="cuda"), None),
                         (torch.zeros(2, H, device="cuda"), [1]), (torch.zeros(2, H), None),
                         (torch.zeros(2, H, dtype=torch.float64, device="cuda"), None), (torch.zeros(1, H, device="cuda"), [2])):
        with pytest.raises(ValueError):
            cs.push(chunk, slots)
    assert cs.samples_seen.tolist() == [0, 0] and cs.take_events() == []  # nothing moved
    # around it the gate and the fronts are accepted
    PacketScorer(GatedScorer(cs), 8000, "mulaw")

"""The tone gate on the GPU (afx/vad.py ToneGate, afx_k_gate_tone).  Every comparison is exact -- bits of fp32, and integers:
the kernel against the numpy restatement after every launch (``nf``, ``h``, ``tone_state``, the whole ring, ``kept``,
``ntone``, ``mask`` and ``tsum``), ``GatedScorer(inner, ToneGate())`` streamed against the offline ``ToneGate.gate`` and the
reference, its scores against a fresh inner scorer pushed the reference's gated stream for the three scorer kinds, the same
behind the packet and jitter fronts, and sessions moved in the middle of a tone and of a hold.

Before a case compares kernel and reference it asserts, on the reference alone (``_exercised``), that its input did what it
claims: ``tonal``, ``tone`` and ``keep`` each took both values, a run was confirmed and a hold expired."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
f32 = np.float32
DTMF = [(697, 1209), (770, 1336), (852, 1477), (941, 1633)]


def _sin(n, *freqs, amp=0.25, start=0):
    t = (start + np.arange(n)) / 16000
    return sum((amp * np.sin(2 * np.pi * f * t)).astype(f32) for f in freqs)


def _noise(n, std, seed):
    return (std * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def _voice(n, seed):
    t = np.arange(n) / 16000
    return (0.2 * np.sin(2 * np.pi * 180 * t) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t))).astype(f32) + _noise(n, 0.002, seed)


def call_stream(seed, n=12 * H, shift=0):
    """A call: ringback (440 + 480 Hz) for 0.75 s, a pause, then talk with a DTMF digit string in it, over line noise;
    ``shift`` moves everything off the frame grid."""
    x = _noise(n + shift, 0.002, seed)
    x[:12000] += _sin(12000, 440, 480, amp=0.15)
    x[16000:] += _voice(n + shift - 16000, seed + 1)
    for d, (lo, hi) in enumerate(DTMF):
        a = 26000 + d * 2400
        x[a:a + 1280] = _sin(1280, lo, hi) + _noise(1280, 0.002, seed + 2 + d)
    return x[shift:].copy()


def _exercised(flags):
    """flags: per stream (tonal, tone, keep) bool arrays of the reference -> the asserts every case makes before the GPU
    is compared: each flag took both values, a run was confirmed, and a hold expired (a tone frame followed by one that is not;
    every gate here has hold > 0)."""
    tonal, tone, keep = (np.concatenate([f[i] for f in flags]) for i in range(3))
    for name, v in (("tonal", tonal), ("tone", tone), ("keep", keep)):
        assert v.any() and not v.all(), name
    assert any((f[1] & f[0]).any() for f in flags), "no run was confirmed"
    assert any((f[1][:-1] & ~f[1][1:]).any() for f in flags), "no hold expired"  # (hold > 0: a tone ends only when its hold runs out)


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------
FILL_KEPT, FILL_NTONE, FILL_MASK, FILL_TSUM = -5, -7, 0x99, -3.0


class _Mirror:
    """The host side of afx_k_gate_tone: ring, nf, h and tone_state advanced by the reference, row by row."""

    def __init__(self, gate, S, ring_len, seed):
        self.gate, self.S, self.ring_len = gate, S, ring_len
        self.ring = torch.randn(S, ring_len, generator=torch.Generator().manual_seed(seed)).numpy().copy()  # (a stray write shows)
        self.state = [gate.new_state() for _ in range(S)]
        self.wpos = [0] * S
        self.flags = [[] for _ in range(S)]
        self.wrapped = False

    def step(self, rows, slots, wpos=None):
        """One launch -> what it must leave: kept, ntone, mask, tsum (rows of skipped rows keep their fill) and the state."""
        g, A, frames = self.gate, len(slots), rows.shape[1] // self.gate.frame
        kept, ntone = [0] * A, [0] * A
        mask = np.full((A, frames), FILL_MASK, dtype=np.uint8)
        tsum = np.full((A, frames), FILL_TSUM, dtype=f32)
        for i, s in enumerate(slots):
            w = self.wpos[s] if wpos is None else wpos[i]
            if not (0 <= s < self.S and 0 <= w < self.ring_len and rows.shape[1] <= self.ring_len):
                continue
            T, tonal, tone, keep = g.decide_reference(rows[i], self.state[s])
            m, k, self.state[s] = g.gate_reference(rows[i], self.state[s])
            assert m.tolist() == keep.tolist()
            self.ring[s, (w + np.arange(k.size)) % self.ring_len] = k
            self.wrapped |= w + k.size > self.ring_len
            if wpos is None:
                self.wpos[s] = (w + k.size) % self.ring_len
            kept[i], ntone[i] = k.size, int(tone.sum())
            mask[i] = keep.astype(np.uint8) | (tone.astype(np.uint8) << 1) | (tonal.astype(np.uint8) << 2)
            tsum[i] = T
            self.flags[s].append((tonal, tone, keep))
        return dict(kept=kept, ntone=ntone, mask=mask, tsum=tsum, ring=self.ring.copy(),
                    nf=np.array([st["nf"] for st in self.state], dtype=f32), h=[st["h"] for st in self.state],
                    ts=[[st["r"], st["q"], st["tones"]] for st in self.state], slots=list(slots), rows=rows)

    def exercised(self):
        _exercised([tuple(np.concatenate([f[i] for f in fl]) for i in range(3)) for fl in self.flags if fl])


def _expected(gate, S, ring_len, seed, plan):
    """plan: [(rows (A, n), slots, wpos or None)] -> (the mirror, what every launch must leave).  The write positions of
    a launch are those BEFORE it, so they are recorded first."""
    mir, out = _Mirror(gate, S, ring_len, seed), []
    for rows, slots, wpos in plan:
        before = [mir.wpos[s] if 0 <= s < S else 0 for s in slots] if wpos is None else list(wpos)
        e = mir.step(rows, slots, wpos)
        e["wpos"] = before
        out.append(e)
    return mir, out


class _Device:
    def __init__(self, gate, S, ring_len, seed):
        self.gate, self.S, self.ring_len = gate, S, ring_len
        self.ring = torch.randn(S, ring_len, generator=torch.Generator().manual_seed(seed)).cuda()
        self.nf = torch.full((S,), float("inf"), device="cuda")
        self.h = torch.zeros(S, dtype=torch.int32, device="cuda")
        self.ts = torch.zeros(S, 3, dtype=torch.int32, device="cuda")
        self.coef = torch.from_numpy(gate.coef.copy()).cuda()

    def launch(self, rows, slots, wpos, outputs=True):
        from afx._lib import call_on, lib, ptr
        g = self.gate
        x = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        A, n = x.shape
        hdr = torch.tensor(list(zip(slots, wpos)), dtype=torch.int32).cuda()
        kept = torch.full((A,), FILL_KEPT, dtype=torch.int32, device="cuda")
        ntone = torch.full((A,), FILL_NTONE, dtype=torch.int32, device="cuda") if outputs else None
        mask = torch.full((A, n // g.frame), FILL_MASK, dtype=torch.uint8, device="cuda") if outputs else None
        tsum = torch.full((A, n // g.frame), FILL_TSUM, dtype=torch.float32, device="cuda") if outputs else None
        rc = call_on(x, lib().afx_k_gate_tone, ptr(x), A, n, ptr(hdr), g.frame, float(g.E_floor), float(g.ratio32),
                     float(g.rise32), g.hang, ptr(self.coef), self.coef.numel(), float(g.thr), g.confirm, g.hold, ptr(self.nf),
                     ptr(self.h), ptr(self.ts), ptr(self.ring), self.S, self.ring_len, ptr(kept), ptr(ntone), ptr(mask), ptr(tsum))
        torch.cuda.synchronize()
        return rc, kept, ntone, mask, tsum

    def check(self, e, what):
        assert self.ring.cpu().numpy().tobytes() == e["ring"].tobytes(), what
        assert self.nf.cpu().numpy().tobytes() == e["nf"].tobytes(), (what, self.nf.tolist(), e["nf"].tolist())
        assert self.h.tolist() == e["h"], what
        assert self.ts.tolist() == e["ts"], (what, self.ts.tolist(), e["ts"])

    def run(self, expected, outputs=lambda it: True):
        for it, e in enumerate(expected):
            rc, kept, ntone, mask, tsum = self.launch(e["rows"], e["slots"], e["wpos"], outputs(it))
            assert rc == 0, it
            assert kept.tolist() == e["kept"], (it, e["slots"])
            if ntone is not None:
                assert ntone.tolist() == e["ntone"], (it, e["slots"])
                assert np.array_equal(mask.cpu().numpy(), e["mask"]), it
                assert tsum.cpu().numpy().tobytes() == e["tsum"].tobytes(), it
            self.check(e, (it, e["slots"]))  # (the whole ring and state: the named slots' AND the unnamed slots' bytes)


def _pattern(frame, K, seed, hang, confirm, hold):
    """A stream in whole frames that walks the state machine: speech with its hangover, a confirmed tone burst, a hold that
    expires, a burst of confirm - 1, a hold bridged by a new run, a tone inside a hangover."""
    freqs = (697,) if K <= 2 else (697, 1209)
    segs = [("Q", 3), ("S", 5), ("Q", hang + 3), ("T", confirm + 3), ("Q", hold + 2), ("T", confirm - 1), ("Q", hang + 2),
            ("T", confirm + 1), ("S", 1), ("T", confirm), ("Q", hold + 3), ("S", 3), ("Q", 1), ("T", confirm + 2), ("Q", hold + hang)]
    n = sum(m for _, m in segs) * frame
    src = {"Q": _noise(n, 0.0003, seed), "S": _noise(n, 0.1, seed + 1), "T": _sin(n, *freqs) + _noise(n, 0.001, seed + 2)}
    out, pos = [], 0
    for kind, m in segs:
        out.append(src[kind][pos:pos + m * frame])
        pos += m * frame
    return np.concatenate(out)


def _subset_plan(streams, n, S, seed):
    """Launches of n samples over random permuted subsets of the slots (every slot in the first, one alone in the second),
    until every stream is used up; a stream shorter than the others is padded with zeros."""
    rng = np.random.default_rng(seed)
    total = max(len(x) for x in streams)
    total += -total % n
    streams = [np.concatenate([x, np.zeros(total - len(x), dtype=f32)]) for x in streams]
    pos, plan = [0] * S, []
    while min(pos) < total:
        live = [s for s in range(S) if pos[s] < total]
        slots = live if not plan else [live[-1]] if len(plan) == 1 else rng.permutation(live)[:min(len(live), 3 if len(live) > 3 else rng.integers(1, len(live) + 1))].tolist()
        plan.append((np.stack([streams[s][pos[s]:pos[s] + n] for s in slots]), slots, None))
        for s in slots:
            pos[s] += n
    return plan


def _case(frame, n, K):
    from afx.vad import TELEPHONY_TONES, ToneGate
    S = 5
    if n == H:  # the default gate on call audio, every stream at another offset from the frame grid
        gate = ToneGate()
        streams = [call_stream(3 * s, shift=37 * s) for s in range(S)]
    else:
        gate = ToneGate(frame=frame, freqs=TELEPHONY_TONES[:K], hang=3, confirm=3, hold=3)
        base = _pattern(frame, K, 10 * frame + K, 3, 3, 3)
        streams = [np.roll(base, -s * 4 * frame) for s in range(S)]
    return gate, S, n + 3, _subset_plan(streams, n, S, frame + n + K)


CASES = [(160, 160, 16), (160, 320, 2), (160, H, 16), (64, 192, 1), (65, 195, 16), (1, 5, 2)]


@pytest.mark.parametrize("frame,n,K", CASES)
def test_kernel_equals_the_reference_launch_by_launch(frame, n, K):
    gate, S, ring_len, plan = _case(frame, n, K)
    mir, expected = _expected(gate, S, ring_len, frame + K, plan)
    mir.exercised()
    assert mir.wrapped and any(len(p[1]) == 3 and p[1] != sorted(p[1]) for p in plan)  # a wrapped write; A = 3 permuted of S = 5
    assert len(plan[0][1]) == S and len(plan[1][1]) == 1                                 # A = S, and A = 1
    _Device(gate, S, ring_len, frame + K).run(expected, outputs=lambda it: it % 3 != 1)  # (every third launch: no optional outputs)


def _special_streams():
    """Six streams of six hops, one per kind of input the kernel must get right."""
    n = 6 * H
    bursts = _noise(n + 37, 0.002, 1)
    for a, m in ((1600, 480), (4800, 800), (6400, 3200)):  # 30, 50 and 200 ms; the last crosses the border of pushes 1 and 2
        bursts[a:a + m] += _sin(m, 770, 1336)
    ringback = _noise(n, 0.002, 2)
    ringback[800:16800] += _sin(16000, 440, 480, amp=0.15)
    ramp = _sin(n, 1004, amp=0.1) + (np.linspace(0.01, 0.06, n) * np.random.default_rng(3).standard_normal(n)).astype(f32)
    tiny = np.concatenate([_sin(n // 2, 697, 1209, amp=1.0) * f32(1e-20), _sin(n // 2, 697, 1209, amp=1.0) * f32(1e-22)]).astype(f32)
    broken = _sin(n, 852, 1477) + _noise(n, 0.002, 4)
    broken[1607], broken[1765], broken[3300], broken[3301] = np.nan, np.inf, np.inf, np.nan
    broken[8000:] = _noise(n - 8000, 0.002, 5)
    return [bursts[:n].copy(), bursts[37:].copy(), ringback, ramp, tiny, broken]


def test_the_inputs_a_telephone_line_brings():
    from afx.vad import ToneGate
    gate = ToneGate()
    streams = _special_streams()
    S = len(streams)
    plan = [(np.stack([x[t * H:(t + 1) * H] for x in streams]), list(range(S)), None) for t in range(6)]
    mir, expected = _expected(gate, S, 2 * H, 7, plan)
    mir.exercised()
    fl = [tuple(np.concatenate([f[i] for f in mir.flags[s]]) for i in range(3)) for s in range(S)]
    T = [np.concatenate([e["tsum"][s] for e in expected]) for s in range(S)]
    # 30 ms aligned: three tonal frames, never a tone; 50 ms: tone from its 4th frame; 200 ms: a tone across the push border at frame 50
    assert fl[0][0][10:13].all() and not fl[0][1][8:20].any() and fl[0][1][33:38].all() and not fl[0][1][30:33].any()
    assert fl[0][1][43:63].all() and fl[1][1][45:62].all() and not fl[1][1][8:20].any()
    # ringback for 1 s: its first confirm - 1 frames pass as speech, then it is rejected throughout, and the hangover with it
    assert fl[2][2][5:8].all() and fl[2][1][8:108].all() and not fl[2][2][8:].any()
    # a tone in rising noise: frames on both sides of thr * e, some within 5 % of it
    e_ramp = np.array([float(np.sum(streams[3][f * 160:(f + 1) * 160].astype(np.float64) ** 2)) for f in range(150)])
    ratio = T[3] / (float(gate.thr) * e_ramp)
    assert fl[3][0].any() and not fl[3][0].all() and ((ratio > 0.95) & (ratio < 1.0)).any() and ((ratio >= 1.0) & (ratio < 1.05)).any()
    # amplitudes where squares and products underflow: powers in the denormal range, never tonal
    assert ((T[4] > 0) & (T[4] < 1e-38)).any() and (T[4] > 0).all() and not fl[4][0].any()
    # NaN and +inf inside a confirmed tone: not tonal, the run breaks, the hold carries it
    assert fl[5][1][10:12].all() and not fl[5][0][10] and not fl[5][0][11] and not fl[5][0][20] and fl[5][0][12:20].all()
    _Device(gate, S, 2 * H, 7).run(expected)


def test_every_slot_of_a_large_scorer_in_one_launch():
    from afx.vad import ToneGate
    gate, S = ToneGate(), 2048
    bank = []
    for s in range(16):  # one hop each: quiet, talk, a digit (at another offset from the frame grid in every row), quiet, talk
        x = _noise(H, 0.002, 100 + s)
        x[480:1600] += _voice(1120, 200 + s)
        x[1600 + 40 * s:2880 + 40 * s] = _sin(1280, *DTMF[s % 4])
        x[3700:] += _voice(300, 300 + s)
        bank.append(x)
    bank = np.stack(bank)
    refs = []
    for row in bank:
        T, tonal, tone, keep = gate.decide_reference(row)
        m, k, st = gate.gate_reference(row)
        refs.append((T, tonal, tone, keep, k, st))
    _exercised([r[1:4] for r in refs])
    which = np.random.default_rng(0).integers(0, 16, S)
    slots = np.random.default_rng(1).permutation(S)
    dev = _Device(gate, S, 2 * H, 11)
    ring0 = dev.ring.cpu().numpy()
    rc, kept, ntone, mask, tsum = dev.launch(bank[which], slots.tolist(), [5] * S)
    assert rc == 0
    want = [refs[w] for w in which]
    assert kept.tolist() == [r[4].size for r in want] and ntone.tolist() == [int(r[2].sum()) for r in want]
    assert np.array_equal(mask.cpu().numpy(), np.stack([r[3].astype(np.uint8) | (r[2].astype(np.uint8) << 1) | (r[1].astype(np.uint8) << 2) for r in want]))
    assert tsum.cpu().numpy().tobytes() == np.stack([r[0] for r in want]).tobytes()
    ring = ring0.copy()
    for i, r in enumerate(want):
        ring[slots[i], 5:5 + r[4].size] = r[4]
    assert dev.ring.cpu().numpy().tobytes() == ring.tobytes()
    order = np.argsort(slots)  # row of each slot
    assert dev.nf.cpu().numpy().tobytes() == np.array([want[i][5]["nf"] for i in order], dtype=f32).tobytes()
    assert dev.h.tolist() == [want[i][5]["h"] for i in order]
    assert dev.ts.tolist() == [[want[i][5][k] for k in ("r", "q", "tones")] for i in order]


def test_a_row_of_two_launches_carries_a_tone_run_across_the_split():
    from afx.vad import MAX_FRAMES, ToneGate
    gate = ToneGate()
    frames = MAX_FRAMES + 1
    n = frames * 160
    a = call_stream(21, n=n)
    a[(MAX_FRAMES - 3) * 160:] = _sin(4 * 160, 941, 1633)  # tonal from frame 509: the 4th frame of the run is frame 512
    b = call_stream(22, n=n)
    b[(MAX_FRAMES - 12) * 160:] = _sin(13 * 160, 350, 440)  # confirmed before the split, still a tone after it
    c = call_stream(23, n=n)
    c[(MAX_FRAMES - 2) * 160:] = _noise(3 * 160, 0.1, 24)    # speech on both sides: kept accumulates
    plan = [(np.stack([a, b, c]), [2, 0, 1], [n - 320, 5, 0])]
    mir, expected = _expected(gate, 3, n + 160, 9, plan)
    mir.exercised()
    fa, fb, fc = (mir.flags[s][0] for s in (2, 0, 1))
    assert fa[1][MAX_FRAMES] and not fa[1][MAX_FRAMES - 4:MAX_FRAMES].any() and fa[0][MAX_FRAMES - 3:].all()
    assert fb[1][MAX_FRAMES - 9:].all() and fc[2][MAX_FRAMES - 2:].all() and fc[2][:MAX_FRAMES - 2].any()
    assert expected[0]["ts"][2][:2] == [4, gate.hold] and mir.wrapped
    _Device(gate, 3, n + 160, 9).run(expected)


def test_bad_rows_are_skipped_whole_and_bad_arguments_launch_nothing():
    from afx._lib import lib
    from afx.vad import ToneGate
    gate = ToneGate()
    n, S, ring_len = 1600, 3, 3200
    row = np.concatenate([_noise(320, 0.002, 1), _sin(1280, 697, 1209)])  # quiet, then a digit: three frames kept, then tone
    rows = np.stack([row] * 5)
    # bad rows between good ones: slot 3 and slot -1 are outside the state, wpos 3200 is outside the ring; rows 0 and 2 are gated
    plan = [(rows, [0, 3, 1, -1, 2], [0, 0, 7, 0, ring_len])]
    mir, expected = _expected(gate, S, ring_len, 5, plan)
    e = expected[0]
    assert e["kept"] == [480, 0, 480, 0, 0] and e["ntone"] == [5, 0, 5, 0, 0] and e["ts"] == [[8, 3, 5], [8, 3, 5], [0, 0, 0]]
    assert (e["mask"][[1, 3, 4]] == FILL_MASK).all() and set(e["mask"][0].tolist()) == set(e["mask"][2].tolist()) == {0, 4 | 1, 4 | 2}
    dev = _Device(gate, S, ring_len, 5)
    dev.run(expected)
    # a row longer than the ring: every row is skipped
    small = _Device(gate, 2, n - 160, 6)
    _, exp_small = _expected(gate, 2, n - 160, 6, [(rows[:2], [0, 1], [0, 0])])
    assert exp_small[0]["kept"] == [0, 0]
    small.run(exp_small)
    # scalar arguments and NULL pointers: an error, nothing launched, nothing changed
    x = torch.from_numpy(rows[:1].copy()).cuda()
    hdr = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    kept = torch.full((1,), FILL_KEPT, dtype=torch.int32, device="cuda")
    ntone = torch.full((1,), FILL_NTONE, dtype=torch.int32, device="cuda")
    mask = torch.full((1, 10), FILL_MASK, dtype=torch.uint8, device="cuda")
    tsum = torch.full((1, 10), FILL_TSUM, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = dict(x=p(x), A=1, n=n, hdr=p(hdr), frame=160, floor=float(gate.E_floor), ratio=8.0, rise=1.01, hang=20, coef=p(dev.coef),
                K=16, thr=float(gate.thr), confirm=4, hold=3, nf=p(dev.nf), h=p(dev.h), ts=p(dev.ts), ring=p(dev.ring), S=S,
                ring_len=ring_len, kept=p(kept), ntone=p(ntone), mask=p(mask), tsum=p(tsum))
    bads = [dict(n=n + 1), dict(frame=0), dict(A=0), dict(A=65536), dict(S=0), dict(ring_len=0), dict(hang=-1), dict(ratio=1.0),
            dict(floor=0.0), dict(rise=0.5), dict(K=0), dict(K=17), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("inf")),
            dict(thr=float("nan")), dict(confirm=0), dict(hold=-1)] + [{k: None} for k in ("x", "hdr", "coef", "nf", "h", "ts", "ring", "kept")]
    for bad in bads:
        a = dict(good, **bad)
        rc = lib().afx_k_gate_tone(*[a[k] for k in good], None)
        torch.cuda.synchronize()
        assert rc != 0 and b"gate_tone" in lib().afx_last_error(), bad
        assert kept.tolist() == [FILL_KEPT] and ntone.tolist() == [FILL_NTONE] and (mask == FILL_MASK).all() and (tsum == FILL_TSUM).all()
        dev.check(e, bad)
    after = mir.step(rows[:1], [0], [0])  # (and the good arguments are good: slot 0 takes the row again, mid-tone this time)
    assert lib().afx_k_gate_tone(*good.values(), None) == 0
    torch.cuda.synchronize()
    assert kept.tolist() == after["kept"] == [320] and ntone.tolist() == after["ntone"] == [8]
    assert np.array_equal(mask.cpu().numpy(), after["mask"]) and tsum.cpu().numpy().tobytes() == after["tsum"].tobytes()
    dev.check(after, "good arguments")


def test_the_three_forms_share_one_decision_on_the_device():
    """afx_k_gate, afx_k_gate_la (pre 5) and afx_k_gate_tone (the default bank) over the same audio, 40 launches of 10
    frames for 3 slots: where no frame is tonal the three kernels leave the same ``nf`` bits and ``h`` after every launch,
    and the tone form keeps, copies and masks exactly what the plain form does.  The audio is that of
    tests/test_cpu_vad_tone.py::test_without_a_tonal_frame_it_is_the_plain_gate, and the noise bursts once more with an
    onset frame made +inf and another made NaN (each then not speech: the plain decision changes at exactly those two)."""
    import test_cpu_vad_tone as host
    from test_gpu_vad import _Raw as Plain
    from test_gpu_vad_lookahead import _Raw as Lookahead
    from afx.vad import LookaheadGate, SpeechGate, ToneGate
    S, n, total, L = 3, 1600, 64000, 3200
    noise = (0.002 * np.random.default_rng(9).standard_normal(total)).astype(f32)
    bursts = host._noise_bursts(total, 3) + noise
    voice = host._voice(total, 4) * np.repeat((np.arange(total // 8000) % 2).astype(f32), 8000) + noise
    broken = bursts.copy()
    broken[19 * 160 + 17], broken[161 * 160 + 5] = np.inf, np.nan  # frames 19 and 161: the first two onsets of the bursts
    streams = [bursts, voice, broken]
    gate = ToneGate()
    keeps = []
    for x in streams:  # on the reference, before the GPU is touched: no frame is tonal, and keep takes both values
        _, tonal, is_tone, keep = gate.decide_reference(x)
        assert not tonal.any() and not is_tone.any() and keep.any() and not keep.all()
        keeps.append(keep)
    assert np.flatnonzero(keeps[2] != keeps[0]).tolist() == [19, 161]
    plain, la, tone = Plain(SpeechGate(), S, L, seed=4), Lookahead(LookaheadGate(pre=5), S, L, seed=4), _Device(gate, S, L, 4)
    assert tone.ring.cpu().numpy().tobytes() == plain.m_ring.tobytes()  # (the same bytes to begin with)
    slots, w, w_la = list(range(S)), [0] * S, [0] * S
    for t in range(total // n):
        rows = np.stack([x[t * n:(t + 1) * n] for x in streams])
        rc_p, kept_p, mask_p = plain.launch(rows, slots, wpos=w, mask=True)
        rc_l, kept_l, _ = la.launch(rows, slots, wpos=w_la, F=[t * 10] * S)
        rc_t, kept_t, _, mask_t, _ = tone.launch(rows, slots, w)
        assert rc_p == rc_l == rc_t == 0, t
        nf = plain.nf.cpu().numpy().tobytes()
        assert la.nf.cpu().numpy().tobytes() == nf and tone.nf.cpu().numpy().tobytes() == nf, t
        assert plain.h.tolist() == la.h.tolist() == tone.h.tolist(), t
        assert kept_t.tolist() == kept_p and tone.ring.cpu().numpy().tobytes() == plain.ring.cpu().numpy().tobytes(), t
        assert np.array_equal(mask_t.cpu().numpy() & 1, mask_p) and mask_p.tolist() == [k[t * 10:(t + 1) * 10].tolist() for k in keeps], t
        assert tone.ts.tolist() == [[0, 0, 0]] * S, t
        w = [(a + k) % L for a, k in zip(w, kept_p)]
        w_la = [(a + k) % L for a, k in zip(w_la, kept_l)]


# ---- 2. streamed equals offline ----------------------------------------------------------------------------------------------------
def _tap(S, hop):
    from afx.streaming import SlidingWindowScorer

    class Tap(SlidingWindowScorer):
        def __init__(self):
            super().__init__(None, S, window=4 * hop, hop=hop, device="cuda")
            self.got = [[] for _ in range(S)]

        def push(self, chunk, slots=None):
            idx = self._slot_list(slots, ordered=True)
            assert chunk.is_cuda and chunk.dtype == torch.float32 and chunk.shape == (len(idx), hop)
            for i, s in enumerate(idx):
                self.got[s].append(chunk[i].clone())
            self._seen[idx] += hop
            return torch.tensor([float(10 * s + 1) for s in idx], device=chunk.device)

    return Tap()


def _reference_streams(gate, streams):
    """-> per stream (kept samples, tone frames per hop), with the asserts that the streams exercised the gate."""
    out, flags = [], []
    for x in streams:
        _, tonal, tone, keep = gate.decide_reference(x)
        out.append((gate.gate_reference(x)[1], tone.reshape(-1, H // gate.frame).sum(axis=1)))
        flags.append((tonal, tone, keep))
    _exercised(flags)
    return out


def test_streamed_gate_equals_the_offline_gate_and_the_reference():
    from afx.vad import GatedScorer, SpeechGate, ToneGate
    S, ticks = 4, 12
    gate = ToneGate()
    streams = [call_stream(40 + s, shift=53 * s) for s in range(S)]
    ref = _reference_streams(gate, streams)
    tap = _tap(S, H)
    gs = GatedScorer(tap, gate)
    assert gs.last_tone_frames is None and gs.tone_frames.tolist() == [0] * S
    pos, kept_n, tones, state = [0] * S, [0] * S, [0] * S, [gate.new_state() for _ in range(S)]
    for t in range(ticks):
        named = [[0, 1, 2, 3], [3, 1, 0, 2], [2, 0, 3]][t % 3]  # (slot 1 is not named every third tick: its stream lags)
        out = gs.push(torch.from_numpy(np.stack([streams[s][pos[s]:pos[s] + H] for s in named])).cuda(), named)
        want, last = [], []
        for s in named:
            hop = streams[s][pos[s]:pos[s] + H]
            last.append(int(gate.decide_reference(hop, state[s])[2].sum()))
            _, k, state[s] = gate.gate_reference(hop, state[s])
            want.append((kept_n[s] + k.size) // H > kept_n[s] // H)
            kept_n[s], pos[s], tones[s] = kept_n[s] + k.size, pos[s] + H, tones[s] + last[-1]
        assert gs.emitted(out).tolist() == want, t
        assert gs.last_tone_frames.dtype == torch.int32 and gs.last_tone_frames.is_cuda
        assert gs.last_tone_frames.tolist() == last, t
        assert gs.tone_frames.tolist() == tones and gs.tone_frames.dtype == torch.int32 and gs.tone_frames.is_cuda, t
    assert pos == [ticks * H, (ticks - ticks // 3) * H, ticks * H, ticks * H] and sum(tones) == sum(int(r[1][:p // H].sum()) for r, p in zip(ref, pos))
    return_of = gate.gate([torch.from_numpy(x.copy()).cuda() for x in streams], return_mask=True, return_tones=True)
    for s, (off, m, tn) in enumerate(zip(*return_of)):
        mask, kept, _ = gate.gate_reference(streams[s])
        assert off.cpu().numpy().tobytes() == kept.tobytes() and m.cpu().numpy().tolist() == mask.tolist()
        assert tn.dtype == torch.bool and tn.cpu().numpy().tolist() == gate.decide_reference(streams[s])[2].tolist()
    for s in range(S):  # what the inner scorer was pushed: the whole hops of the reference's gated stream of what the slot saw
        seen = ticks * H if s != 1 else (ticks - ticks // 3) * H
        kept = gate.gate_reference(streams[s][:seen])[1]
        whole = kept.size // H
        assert len(tap.got[s]) == whole and whole >= 2, (s, whole)
        assert torch.cat(tap.got[s]).cpu().numpy().tobytes() == kept[:whole * H].tobytes(), s
        assert int(gs.samples_seen[s]) == seen and int(gs.pending[s]) == kept.size - whole * H
    # fewer hops than the plain gate passes on: the ringback and the digits are gone
    assert all(len(tap.got[s]) < SpeechGate().gate_reference(streams[s])[1].size // H for s in (0, 2, 3))
    # the offline form: a (B, n) tensor, trailing samples dropped, an empty clip
    two = torch.from_numpy(np.stack([streams[0][:8000 + 77], streams[1][:8000 + 77]])).cuda()
    for row, o in zip(two.cpu().numpy(), gate.gate(two)):
        assert o.cpu().numpy().tobytes() == gate.gate_reference(row[:8000])[1].tobytes()
    assert gate.gate([torch.zeros(100, device="cuda")])[0].numel() == 0
    gs.reset([1])
    assert gs.tone_frames.tolist() == [tones[0], 0, tones[2], tones[3]] and gs.tone_state[1].tolist() == [0, 0, 0]


# ---- 3. scores -----------------------------------------------------------------------------------------------------------------
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES[dtype] = (eng, sd)
    return _ENGINES[dtype]


def _inner(kind, S):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    eng, sd = _engine("fp16")
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _gated_reference(gate, R):
    """R: (n,) fp32 (numpy, or a CUDA tensor) -> the whole hops of the REFERENCE's gated stream, (hops, H) on the GPU."""
    x = R.cpu().numpy() if isinstance(R, torch.Tensor) else R
    g = gate.gate_reference(x[:x.size // gate.frame * gate.frame])[1]
    return torch.from_numpy(g[:g.size // H * H].reshape(-1, H).copy()).cuda()


def _check_scores(kind, got, G):
    """got[s]: the non-NaN scores slot s emitted, in order; G[s]: (hops, H) gated stream -> equal to a fresh inner scorer."""
    S = len(G)
    fresh = _inner(kind, S)
    for s in range(S):
        assert len(got[s]) == G[s].shape[0], (s, len(got[s]), G[s].shape[0])
        for j in range(G[s].shape[0]):
            ref = fresh.push(G[s][j:j + 1].contiguous(), [s])
            assert torch.equal(got[s][j].reshape(1), ref), (kind, s, j)


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_scores_equal_a_fresh_inner_scorer_pushed_the_reference_gated_stream(kind):
    from afx.vad import GatedScorer, ToneGate
    S, hops = 3, 12
    gate = ToneGate()
    gs = GatedScorer(_inner(kind, S), gate)
    streams = [call_stream(60 + s, shift=57 * s) for s in range(S)]  # ringback, then talk with a DTMF string in it
    ref = _reference_streams(gate, streams)
    dev = [torch.from_numpy(x).cuda() for x in streams]
    got = [[] for _ in range(S)]
    for t in range(hops):
        named = [[0, 1, 2], [2, 1, 0], [1, 2, 0]][t % 3]
        out = gs.push(torch.stack([dev[s][t * H:(t + 1) * H] for s in named]), named)
        assert gs.last_tone_frames.tolist() == [int(ref[s][1][t]) for s in named]
        for s, v, e in zip(named, out, gs.emitted(out).tolist()):
            if e:
                got[s].append(v.clone())
    G = [_gated_reference(gate, x) for x in streams]
    assert min(g.shape[0] for g in G) >= 2 and all(g.shape[0] < hops for g in G)
    _check_scores(kind, got, G)
    assert torch.equal(gs.scorer.samples_seen, torch.tensor([g.shape[0] * H for g in G]))
    assert gs.tone_frames.tolist() == [int(r[1].sum()) for r in ref]


# ---- 4. behind the fronts --------------------------------------------------------------------------------------------------------
def _mulaw_encode(x):
    """G.711 mu-law of fp32 samples in [-1, 1) -> uint8 (any encoder serves: the reference decodes the same bytes)."""
    s = np.clip(np.round(x.astype(np.float64) * 32768), -32635, 32635).astype(np.int64)
    sign, mag = s < 0, np.abs(s) + 132
    exp = np.floor(np.log2(mag)).astype(np.int64) - 7
    mant = (mag >> (exp + 3)) & 15
    return (~((sign.astype(np.int64) << 7) | (exp << 4) | mant) & 0xFF).astype(np.uint8)


def _collect(got, res, named):
    from afx.vad import emitted
    for s, part in zip(named, res.split()):
        got[s] += [v.clone() for v in part[emitted(part)]]


@pytest.mark.parametrize("front", ["packet", "jitter"])
def test_tone_gate_behind_the_fronts(front):
    from afx.ingest import PacketScorer, decode
    from afx.jitter import JitterScorer
    from afx.resample import Resampler
    from afx.vad import GatedScorer, ToneGate
    S, gate = 3, ToneGate()
    kind = "kv" if front == "packet" else "incremental"
    gs = GatedScorer(_inner(kind, S), gate)
    fs = PacketScorer(gs, 8000, "mulaw") if front == "packet" else JitterScorer(gs, 8000, "mulaw", depth=480, conceal="zero")
    codes = [_mulaw_encode(call_stream(80 + s, shift=57 * s)[::2]) for s in range(S)]  # 8 kHz by plain slicing, 3 s each
    got = [[] for _ in range(S)]
    for k in range(0, codes[0].size, 160):  # 20-ms packets
        named = [[0, 1, 2], [2, 0, 1]][(k // 160) % 2]
        packets = [codes[s][k:k + 160].tobytes() for s in named]
        _collect(got, fs.feed(packets, named) if front == "packet" else fs.feed(packets, named, [k] * len(named)), named)
    if front == "jitter":
        _collect(got, fs.flush(), list(range(S)))
    R = [Resampler(8000)(decode(c, "mulaw")[None])[0].cpu().numpy() for c in codes]  # the stream the front's contract defines
    seen = [int(v) for v in gs.samples_seen]
    assert min(seen) >= 10 * H
    flags = [gate.decide_reference(r[:n])[1:] for r, n in zip(R, seen)]
    _exercised(flags)
    G = [_gated_reference(gate, r[:n]) for r, n in zip(R, seen)]
    assert min(g.shape[0] for g in G) >= 2
    _check_scores(kind, got, G)
    assert gs.tone_frames.tolist() == [int(f[1].sum()) for f in flags]


# ---- 5. moving sessions ------------------------------------------------------------------------------------------------------------
def _move(st):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _snap(gs):
    st = gs.export_slots(list(range(gs.S)))
    return [st.seen] + [st.tensors[k].clone() for k in sorted(st.tensors)]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and _same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x.cpu(), y.cpu())
                                    for x, y in zip(a, b))


def _cut_streams(t0, ticks):
    """Stream 0 is cut (after t0 hops) in the middle of a confirmed tone, stream 1 in the middle of a hold."""
    n, cut = ticks * H, t0 * H
    a = _voice(n, 1)
    a[cut - 8 * 160:cut + 9 * 160] = _sin(17 * 160, 852, 1336)
    b = _voice(n, 2)
    b[cut - 12 * 160:cut - 2 * 160] = _sin(10 * 160, 941, 1209)
    b[cut - 2 * 160:cut + 320] = _noise(640, 0.002, 3)  # the burst ended two frames before the cut; quiet across it
    return [a, b]


@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_sessions_moved_inside_a_tone_and_inside_a_hold_continue_bit_for_bit(kind):
    from afx.vad import GatedScorer, LookaheadGate, SpeechGate, ToneGate
    gate, t0, ticks = ToneGate(), 5, 12
    streams = _cut_streams(t0, ticks)
    flags = [gate.decide_reference(x)[1:] for x in streams]
    _exercised(flags)
    states = [gate.gate_reference(x[:t0 * H])[2] for x in streams]
    assert states[0]["r"] >= gate.confirm and states[0]["q"] == gate.hold and states[1]["r"] == 0 and 0 < states[1]["q"] < gate.hold
    hopsof = lambda t, rows: torch.from_numpy(np.stack([streams[i][t * H:(t + 1) * H] for i in rows])).cuda()  # noqa: E731
    never = GatedScorer(_inner(kind, 3), gate)
    ref = torch.stack([never.push(hopsof(t, [0, 1]), [0, 2]).clone() for t in range(ticks)])  # (ticks, 2)
    assert never.emitted(ref[t0:, 0]).any() and never.emitted(ref[t0:, 1]).any() and never.emitted(ref[:t0]).any()

    a = GatedScorer(_inner(kind, 3), gate)
    for t in range(t0):
        assert _same_bits(a.push(hopsof(t, [1, 0]), [2, 0]), ref[t].flip(0))
    st = a.export_slots([0, 2])
    assert st.tensors["gate_tone"].tolist() == [[s["r"], s["q"], s["tones"]] for s in states]
    b = GatedScorer(_inner(kind, 4), gate)
    b.push(hopsof(2, [0, 1]), [3, 0])  # the destination is in use
    # a plain-gated, a look-ahead and a differently tuned tone-gated scorer refuse the state; a tone-gated one refuses a plain state
    for other in (GatedScorer(_inner(kind, 4), SpeechGate()), GatedScorer(_inner(kind, 4), LookaheadGate()),
                  GatedScorer(_inner(kind, 4), ToneGate(hold=4))):
        before = _snap(other)
        with pytest.raises(ValueError):
            other.import_slots([3, 1], _move(st))
        assert _same(before, _snap(other))
    plain = GatedScorer(_inner(kind, 4), SpeechGate())
    plain.push(hopsof(2, [0, 1]), [3, 0])
    before = _snap(b)
    with pytest.raises(ValueError):
        b.import_slots([3, 1], _move(plain.export_slots([3, 0])))
    spoiled = _move(st)
    spoiled.tensors["gate_tone"][0, 1] = gate.hold - 1  # inside a confirmed tone without the full hold
    with pytest.raises(ValueError):
        b.import_slots([3, 1], spoiled)
    assert _same(before, _snap(b))
    b.import_slots([3, 1], _move(st))
    assert b.tone_frames[[3, 1]].tolist() == [s["tones"] for s in states]
    for t in range(t0, ticks):
        assert _same_bits(b.push(hopsof(t, [1, 0]), [1, 3]), ref[t].flip(0)), t
    assert b.tone_frames[[3, 1]].tolist() == never.tone_frames[[0, 2]].tolist() == [int(f[1].sum()) for f in flags]

"""The one numpy reference of the jitter buffer (afx/jitter.py, afx/rtp.py).  TEST INFRASTRUCTURE ONLY, like the rest of this
package: the CPU and the GPU jitter tests are all held against what stands here.

``RefSlot`` is the definition of one slot's played-out stream E, per sample: first arrival wins, late samples are dropped, the
playout point is ``hi - depth``, a run of missing samples is comfort noise from its latest silence mark on and the loss
concealment of the scorer's mode before it, and the concealment recurs over E itself.  ``NumpyDevice`` runs the launches a
scorer plans (place / noise / pitch / conceal / release / pop) on the scorer's own numpy ring as include/afx.h states them and
checks what the host promises about a plan.  ``Schedule`` is the seeded lossy traffic the tests drive both with, ``dtx_events``
the traffic of a call with silence suppression.  The decode tables are computed here from the G.711 formulas, independently
of afx/codecs.py; the pitch rule, the gain table and the noise samples are the library's own numpy statements
(``pitch_reference``, ``gain_table``, ``ComfortNoise.samples``), which have known-answer tests of their own.

A new jitter feature extends this module, not a test file."""
import random
import struct

import numpy as np

ENCODINGS = ("pcm_f32le", "pcm_s16le", "mulaw", "alaw")  # (the number a mixed place row carries is the index here)
BPS = {"pcm_f32le": 4, "pcm_s16le": 2, "mulaw": 1, "alaw": 1}


# ---- decoding ------------------------------------------------------------------------------------------------------------------
def _mulaw_table():
    t = []
    for c in range(256):
        u = ~c & 0xFF
        v = ((((u & 15) << 3) + 132) << ((u >> 4) & 7)) - 132
        t.append(-v if u & 0x80 else v)
    return np.array(t, dtype=np.float32) / np.float32(32768)


def _alaw_table():
    t = []
    for c in range(256):
        a = c ^ 0x55
        e, m = (a >> 4) & 7, a & 15
        v = ((m << 4) + 264) << (e - 1) if e else (m << 4) + 8
        t.append(v if a & 0x80 else -v)
    return np.array(t, dtype=np.float32) / np.float32(32768)


TABLES = {"mulaw": _mulaw_table(), "alaw": _alaw_table()}  # fp32 values / 32768, as ``decode`` gives them


def decode_ref(raw, encoding):
    """The bytes of a payload -> its fp32 samples."""
    if encoding in TABLES:
        return TABLES[encoding][np.frombuffer(raw, dtype=np.uint8)]
    if encoding == "pcm_s16le":
        return np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768)
    assert encoding == "pcm_f32le"
    return np.frombuffer(raw, dtype="<f4").astype(np.float32)


# ---- payloads ------------------------------------------------------------------------------------------------------------------
def packet(encoding, n, g, amp=0.1, div=8, quiet=False):
    """n random samples as ``encoding``, drawn from the numpy generator ``g`` -> (the bytes, their decoded fp32 values).
    ``amp``: the level of fp32 noise; ``div``: 16-bit samples are full scale // div; ``quiet``: G.711 codes of low level."""
    if encoding == "pcm_f32le":
        raw = (amp * g.standard_normal(n)).astype("<f4").tobytes()
    elif encoding == "pcm_s16le":
        raw = (g.integers(-32768, 32768, n) // div).astype("<i2").tobytes()
    else:
        raw = (g.integers(96, 160, n) if quiet else g.integers(0, 256, n)).astype(np.uint8).tobytes()
    return raw, decode_ref(raw, encoding)


def voiced(rate, f0, n, seed, t0=0):
    """The signal the pitch rule was prototyped on: seven harmonics of f0 and a little noise, fp32."""
    t = (t0 + np.arange(n)) / rate
    x = 0.1 * sum(np.sin(2 * np.pi * f0 * k * t + k) / k for k in range(1, 8))
    return (x + 0.003 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def coded(encoding, n, seed, f0=None, rate=8000):
    """n samples of a signal (noise, or ``voiced`` at f0) rounded to ``encoding`` -> (the bytes, their decoded fp32 values)."""
    x = (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32) if f0 is None else voiced(rate, f0, n, seed)
    if encoding == "pcm_f32le":
        return x.astype("<f4").tobytes(), x
    if encoding == "pcm_s16le":
        raw = np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
        return raw, decode_ref(raw, encoding)
    table = TABLES["mulaw"] * np.float32(32768)
    order = np.argsort(table, kind="stable")  # the nearest mu-law code of every sample
    levels = table[order]
    k = np.clip(np.searchsorted(levels, x * 32768.0), 1, 255)
    raw = order[np.where(np.abs(levels[k] - x * 32768.0) < np.abs(levels[k - 1] - x * 32768.0), k, k - 1)].astype(np.uint8).tobytes()
    return raw, decode_ref(raw, encoding)


def _cut(raw, x, encoding, sizes):
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return [(raw[a * BPS[encoding]:b * BPS[encoding]], x[a:b]) for a, b in zip(offs, offs[1:])]


def whole_stream(rate, encs, sizes, seed):
    """A Schedule's payloads: one stream of random samples in the first encoding, cut into the packets."""
    return _cut(*packet(encs[0], sum(sizes), np.random.default_rng(seed)), encs[0], sizes)


def per_packet(**kw):
    """A Schedule's payloads: every packet drawn on its own, in its own encoding (``kw``: ``packet``'s)."""
    def make(rate, encs, sizes, seed):
        g = np.random.default_rng(seed)
        return [packet(e, n, g, **kw) for e, n in zip(encs, sizes)]
    return make


def voiced_stream(f0):
    """A Schedule's payloads: ``coded`` (noise, or the voiced signal at f0) in the first encoding, cut into the packets."""
    def make(rate, encs, sizes, seed):
        return _cut(*coded(encs[0], sum(sizes), seed, f0, rate), encs[0], sizes)
    return make


# ---- traffic -------------------------------------------------------------------------------------------------------------------
class Schedule:
    """One slot's traffic: 20-ms packets, packet k in encodings[k % len(encodings)], packet 11 of ``short`` samples between two
    lost ones (two gaps close to each other in one release), packets 25..28 lost (80 ms), a forward ``jump`` at packet 44,
    5 % other loss, duplicates and shuffles within the depth of ``depth_pk`` packets, grouped into ticks (the packets one
    ``feed`` delivers).  ``lossy`` = False: no loss and no short packet.  ``payload``: ``whole_stream``, ``per_packet(...)`` or
    ``voiced_stream(f0)``."""

    def __init__(self, rate, encodings, seed, jump=0, short=1, lossy=True, n_pk=72, origin=None, depth_pk=3, payload=whole_stream):
        encodings = (encodings,) if isinstance(encodings, str) else tuple(encodings)
        rng = random.Random(seed)
        n = rate // 50
        sizes = [n] * n_pk
        sizes[11] = short if lossy else n
        offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        self.enc = [encodings[k % len(encodings)] for k in range(n_pk)]
        self.pk = payload(rate, self.enc, sizes, seed)
        self.raw, self.x = b"".join(p[0] for p in self.pk), np.concatenate([p[1] for p in self.pk])
        self.origin = rng.randrange(1 << 32) if origin is None else origin
        self.start = [offs[k] + (jump if k >= 44 else 0) for k in range(n_pk)]  # packet 44 begins `jump` samples late
        self.size, self.cap = sizes, offs[-1] + jump + 8
        forced = {10, 12, 25, 26, 27, 28} if lossy else set()
        calm = set(range(6, 34)) if lossy else set()  # delivered in order around the forced gaps
        self.lost = set(forced)
        ticks, k = [], 0
        while k < n_pk:
            if lossy and k == 11:  # the short packet and four more in one feed: both gaps fall in its release
                ticks.append([11, 13, 14, 15, 16])
                k = 17
                continue
            if k in calm:
                if k not in forced:
                    ticks.append([k])
                k += 1
                continue
            blk = [q for q in range(k, min(k + depth_pk, n_pk)) if q not in calm]
            k = blk[-1] + 1
            if lossy:
                for q in list(blk):
                    if q and rng.random() < 0.05:
                        blk.remove(q)
                        self.lost.add(q)
            blk += [q for q in blk if rng.random() < 0.15]  # duplicates
            rng.shuffle(blk)  # within depth_pk packets = the depth: every packet is on time
            if 0 in blk:  # the first packet accepted is the session's origin: index 0 here
                blk.remove(0)
                blk.insert(0, 0)
            while blk:
                m = rng.randint(1, 3)
                ticks.append(blk[:m])
                blk = blk[m:]
        self.ticks, self.at = ticks, 0

    def done(self):
        return self.at >= len(self.ticks)

    def tick(self):
        """-> [(timestamp, relative index, bytes, decoded, encoding)] of the next tick."""
        ks = self.ticks[self.at]
        self.at += 1
        return [((self.origin + self.start[k]) % (1 << 32), self.start[k], self.pk[k][0], self.pk[k][1], self.enc[k]) for k in ks]


def dtx_events(rate, seed, n_spurts=6):
    """One slot's traffic as a list of ("pkt", t, fp32 samples) / ("cn", t, level): talk spurts of 20-ms packets, a CN at the
    end of each spurt and every 200 ms of silence with a new level; every third spurt loses its last speech packet, every
    fourth its first CN, 5 % other loss; duplicate marks; some level updates arrive late; arrival shuffled within blocks of
    three."""
    rng, g = random.Random(seed), np.random.default_rng(seed)
    n = rate // 50
    t, ev, late = 0, [], []
    for k in range(n_spurts):
        length = rng.randint(3, 8)
        for q in range(length):
            x = (0.1 * g.standard_normal(n)).astype("<f4")
            lost = k % 3 == 1 if q == length - 1 else (k or q) and rng.random() < 0.05
            if not lost:
                ev.append(("pkt", t, x))
            t += n
        level = rng.randrange(30, 80)
        for q in range(rng.randint(12, 24) if k % 4 == 3 or k % 3 == 2 else rng.randint(4, 24)):
            if q % 10 == 0:
                level = rng.randrange(30, 80) if q else level
                if q or k % 4 != 3:  # (else: a lost CN)
                    ev.append(("cn", t, level))
                    if q and k % 3 == 2:
                        late.append(ev[-1])
                    if rng.random() < 0.3:
                        ev.append(("cn", t, (level + 5) % 128))  # a second mark at the same t: the first arrival wins
            t += n
    out = ev[:1]
    for i in range(1, len(ev), 3):
        blk = ev[i:i + 3]
        rng.shuffle(blk)
        out += blk
    for e in late:  # late marks: they arrive well behind the playout point
        i = next(i for i, v in enumerate(out) if v is e)
        out.insert(min(len(out), i + 9), out.pop(i))
    return out


def rtp(seq, ts, pt=0, ssrc=0x11223344, payload=b"", marker=False, csrc=(), ext=None, pad=0, version=2):
    """A hand-built RTP datagram (RFC 3550)."""
    b0 = (version << 6) | (0x20 if pad else 0) | (0x10 if ext is not None else 0) | len(csrc)
    out = struct.pack("!BBHII", b0, (0x80 if marker else 0) | pt, seq, ts, ssrc)
    out += b"".join(struct.pack("!I", c) for c in csrc)
    if ext is not None:
        out += struct.pack("!HH", 0xBEDE, len(ext) // 4) + ext
    out += payload
    if pad:
        out += bytes(pad - 1) + bytes([pad])
    return out


def sizing(rate, mode="repeat", depth_ms=60, hop=4000):
    """(depth, P, F, lookback, W, J) of a rate at the default period and fade, from the Resampler's L, M, T alone."""
    from afx.resample import Resampler
    rs = Resampler(rate, "cpu")
    depth = depth_ms * rate // 1000
    P, F = (rate // 100, 3 * (rate // 100)) if mode == "repeat" else (0, 0)
    lookback = max(0 if rs.identity else rs.T - 1, P + F)
    W = depth + -(-hop * rs.M // rs.L) + 1
    return depth, P, F, lookback, W, lookback + W


# ---- the noise function, restated with Python integers -------------------------------------------------------------------------
def k_ref(seed, i):
    m = 0xFFFFFFFF
    x = ((i & m) * 0x9E3779B9 + (i >> 32) * 0x85EBCA6B + seed) & m
    x ^= x >> 16
    x = x * 0x7FEB352D & m
    x ^= x >> 15
    x = x * 0x846CA68B & m
    x ^= x >> 16
    return (x - (1 << 32) if x & 0x80000000 else x) >> 8


def amp_ref(level):
    return np.float32(np.sqrt(3.0) * 10.0 ** (-level / 20.0) / 2.0 ** 23)


def noise_ref(seed, i, level):
    return np.float32(amp_ref(level) * np.float32(k_ref(seed, i)))


# ---- the reference: one slot's played-out stream, per sample ------------------------------------------------------------------
class RefSlot:
    """One slot's played-out stream E.  ``mode`` "repeat": period ``P``, fade ``F``; "pitch_sync": ``rate``, ``hold`` and
    ``fade`` (defaults: the scorer's, 10 ms and 50 ms; ``P`` is the search's fallback, default 10 ms); "zero": neither.
    ``noise``: a ``ComfortNoise`` or its seed, for a slot that takes silence marks.

    Recorded: ``E``, ``next``, ``hi``, ``got`` (the samples held back), ``marks``, ``stats`` (the keys of the scorer's
    ``stats()``), ``kinds`` ("r" received / "n" noise / "l" loss per released index), ``releases`` (per release the runs of
    missing samples [i, j) it wrote), and per run of missing samples of E, pieces released by several calls joined: ``spans``
    ([origin, end)), ``calls`` (the releases that wrote it) and, for "pitch_sync", ``periods``.  ``gap`` / ``level`` / ``p``: the
    origin, the noise level in force (-1: none) and the period of the run the playout point stands in."""

    FAST = True  # (False: ``packet`` takes every packet sample by sample, which is the definition)

    def __init__(self, depth, mode, P=0, F=0, rate=None, hold=None, fade=None, noise=None):
        assert mode in ("zero", "repeat", "pitch_sync")
        self.depth, self.mode, self.rate = depth, mode, rate
        if mode == "pitch_sync":
            from afx.jitter import gain_table, pitch_lags
            self.Pmin, self.Pmax, self.Wc = pitch_lags(rate)
            self.P0, self.Hd, self.F = P or rate // 100, rate // 100 if hold is None else hold, rate // 20 if fade is None else fade
            self.G, self.Lh, self.gain = self.Hd + self.F, self.Pmax + self.Wc, gain_table(self.Hd, self.F)
        else:
            self.P, self.F, self.G = P, F, F if mode == "repeat" else 0
            self.gain = (1.0 - np.arange(max(F, 1), dtype=np.float64) / max(F, 1)).astype(np.float32)
        if noise is not None and not hasattr(noise, "samples"):
            from afx.jitter import ComfortNoise
            noise = ComfortNoise(noise)
        self.cn = noise
        self.got, self.marks, self.E = {}, {}, []
        self.next = self.hi = 0
        self.started = False
        self.gap, self.level, self.p = None, -1, P if mode == "repeat" else None
        self.max_start, self._run = None, (0, -1, ())
        self.stats = dict(received=0, late=0, duplicate=0, concealed=0, out_of_order=0)
        if noise is not None:
            self.stats.update(comfort=0, marks=0, marks_late=0)
        self.kinds, self.releases, self.spans, self.calls, self.periods = [], [], [], [], []

    def mark(self, t, level):
        """A silence mark: noise at ``level`` from t on, to the end of the run of missing samples t stands in."""
        assert self.cn is not None, "a slot that takes marks has a ComfortNoise"
        if not self.started or t < self.next:
            self.stats["marks_late"] += 1
        elif t not in self.marks:
            self.marks[t] = level
            self.stats["marks"] += 1

    def packet(self, t, values, by_seq=False):
        """``by_seq``: the caller orders packets by sequence number, so a timestamp behind an earlier one counts nothing."""
        self.started = True
        if not by_seq and self.max_start is not None and t < self.max_start:
            self.stats["out_of_order"] += 1
        self.max_start = t if self.max_start is None else max(self.max_start, t)
        if self.FAST and t >= self.next and len(values) and self.got.keys().isdisjoint(range(t, t + len(values))):
            self.got.update(zip(range(t, t + len(values)), values))  # the common case at once: all on time, none held
            self.stats["received"] += len(values)
            self.hi = max(self.hi, t + len(values))
            return
        for k, v in enumerate(values):
            i = t + k
            if i < self.next:
                self.stats["late"] += 1
            elif i in self.got:
                self.stats["duplicate"] += 1
            else:
                self.got[i] = v
                self.stats["received"] += 1
                self.hi = max(self.hi, i + 1)

    def release(self, upto):
        gaps = []
        for i in range(self.next, upto):
            if i in self.got:
                v, self.gap, self.level = self.got.pop(i), None, -1
                self.kinds.append("r")
            else:
                if self.gap is None:
                    self.gap = i
                    self.spans.append([i, i])
                    self.calls.append(0)
                    if self.mode == "pitch_sync":
                        from afx.jitter import pitch_reference
                        self.p = pitch_reference(np.array(self.E[-self.Lh:], dtype=np.float32), self.rate, self.P0)
                        self.periods.append(self.p)
                if not gaps or gaps[-1][1] != i:
                    gaps.append([i, i])
                    self.calls[-1] += 1
                gaps[-1][1] = self.spans[-1][1] = i + 1
                self.level = self.marks.get(i, self.level)
                if self.level >= 0:
                    v = self._noise(i, upto)
                    self.stats["comfort"] += 1
                    self.kinds.append("n")
                else:
                    d, v = i - self.gap, np.float32(0)
                    if d < self.G:
                        j = self.gap - self.p + d % self.p
                        v = np.float32(self.gain[d] * (self.E[j] if j >= 0 else np.float32(0)))
                    self.stats["concealed"] += 1
                    self.kinds.append("l")
            self.E.append(np.float32(v))
        if upto > self.next:
            self.releases.append(gaps)
        self.next = max(self.next, upto)
        self.hi = max(self.hi, self.next)
        self.marks = {t: l for t, l in self.marks.items() if t >= self.next}

    def after_feed(self):
        self.release(max(self.next, self.hi - self.depth))

    def _noise(self, i, upto):
        """The noise sample of index i at the level in force.  ``samples`` is a function of (index, level) alone, so it is
        evaluated once for [i, upto) and read from there while the level stays."""
        i0, level, v = self._run
        if level != self.level or not i0 <= i < i0 + len(v):
            i0, level, v = self._run = i, self.level, self.cn.samples(i, upto - i, self.level)
        return v[i - i0]


# ---- the kernels restated on a numpy ring --------------------------------------------------------------------------------------
class NumpyDevice:
    """Runs a Plan's launches as include/afx.h states them, on the host-only scorer's own (CPU) ring, for a one-rate or a
    rated scorer (a row's last int is then its rate index) of one encoding or several (a place row then carries its
    encoding), validates every row against ITS rate as the device does, checks what the host promises about a plan and
    collects what each slot releases in ``out``; ``N`` is each slot's playout counter.  A rate's J, P, F, L, M come from the
    host table the launches take.  ``count_pops``: the inner session counts the hops a pop would have pushed it."""

    WIDTH = dict(place=4, noise=6, pitch=2, conceal=4, release=8)

    def __init__(self, js, count_pops=False):
        self.js, self.count_pops, self.pitch = js, count_pops, js.conceal == "pitch_sync"
        self.ring = js.jring.numpy()  # export_slots / import_slots see what is placed here
        self.period = js.jperiod.numpy() if self.pitch else None
        self.rate = [dict(J=t.J, P=t.P, F=t.F, L=t.L, M=t.M, T=t.T, fade=js._fades[i].numpy()) for i, t in enumerate(js._table)]
        assert js._rated or len(self.rate) == 1
        if self.pitch:
            for i, r in enumerate(self.rate):
                r.update(Pmin=int(js._rPmin[i]), Pmax=int(js._rPmax[i]), Wc=int(js._rWc[i]), G=int(js._rG[i]), hz=js._rates[i])
        else:
            assert all(r["fade"].size == max(r["F"], 1) for r in self.rate)
        self.Js = self.ring.shape[1]
        self.out = [[] for _ in range(js.S)]
        self.N = [0] * js.S
        self.launches, self.rounds, self.noise_rows = [], [], 0

    def reset(self, s):
        self.ring[s] = 0
        self.out[s], self.N[s] = [], 0

    def _rate_of_row(self, row):
        ri = row[-1] if self.js._rated else 0
        assert 0 <= ri < len(self.rate) and ri == int(self.js._rate_of[row[0]])  # a row carries its slot's rate
        return self.rate[ri]

    def run(self, plan, pay):
        from afx.ingest import layout, plan as ingest_plan
        js = self.js
        offs, total = layout([len(p) for p in pay])
        stage = bytearray(total)
        for o, p in zip(offs, pay):
            stage[o:o + len(p)] = bytes(p)
        kinds = [op[0] for op in plan.ops]
        self.rounds.append(kinds)
        for a, b in zip(kinds, kinds[1:]):  # the order of a round: place, ONE noise, the conceal ranks, release, pop
            assert not (a == "noise" and b in ("noise", "place")) and not (a in ("pitch", "conceal") and b in ("noise", "place"))
        for op in plan.ops:
            self.launches.append(op[0])
            if op[0] == "pop":
                if self.count_pops:
                    js.scorer._seen[op[2]] += js.hop
                continue
            rows = op[1]
            assert rows.dtype == np.int32 and len(rows) >= 1
            assert rows.shape[1] == self.WIDTH[op[0]] + (js._rated and op[0] != "release") + (js._mixed and op[0] == "place")
            if op[0] in ("pitch", "conceal", "release"):
                assert len(set(rows[:, 0].tolist())) == len(rows)  # one gap per slot and launch: gaps of a slot are ordered
            written = set()  # the rows of a place or noise launch write disjoint ranges
            for row in rows.tolist():
                s, r = row[0], self._rate_of_row(row)
                J, P, F = r["J"], r["P"], r["F"]
                if op[0] == "place":
                    off, n, col = row[1:4]
                    enc = ENCODINGS[row[4]] if js._mixed else js.encoding
                    assert 0 < n <= op[2] <= (self.Js if js._rated else js.W) and n <= J and 0 <= col < J
                    assert off % BPS[enc] == 0 and off + n * BPS[enc] <= total
                    cols = {(s, (col + k) % J) for k in range(n)}
                    assert not (cols & written)
                    written |= cols
                    self.ring[s, (col + np.arange(n)) % J] = decode_ref(bytes(stage[off:off + n * BPS[enc]]), enc)
                elif op[0] == "noise":
                    col, n, lo, hi, level = row[1:6]
                    i0 = (hi << 32) | (lo & 0xFFFFFFFF)
                    assert 0 < n <= min(op[2], J) and op[2] <= self.Js and col == i0 % J and hi >= 0 and 0 <= level <= 127
                    assert self.N[s] <= i0 and i0 + n <= self.N[s] + J  # inside the released range of this round
                    cols = {(s, (col + k) % J) for k in range(n)}
                    assert not (cols & written)
                    written |= cols
                    self.ring[s, (col + np.arange(n)) % J] = js.cn.samples(i0, n, level)
                    self.noise_rows += 1
                elif op[0] == "pitch":
                    from afx.jitter import pitch_reference
                    ac, Lh = row[1], r["Pmax"] + r["Wc"]
                    assert 0 <= ac < J and Lh <= J and op[2] >= Lh
                    self.period[s] = pitch_reference(self.ring[s, (ac - Lh + np.arange(Lh)) % J], r["hz"], P)
                elif op[0] == "conceal":
                    ac, lo, hi = row[1:4]
                    # the source of a gap's samples is never overwritten by them: it lies P (the longest lag, for a period
                    # that is searched) behind the origin, and the gap's rows end that much before the ring comes round
                    assert 0 <= ac < J and 0 <= lo < hi and hi - lo <= op[2] and hi + (r["Pmax"] if self.pitch else P) <= J
                    if self.pitch:
                        p, G = int(self.period[s]) if r["Pmin"] <= self.period[s] <= r["Pmax"] else P, r["G"]
                    else:
                        p, G = P, F if js.conceal == "repeat" else 0
                    for d in range(lo, hi):
                        self.ring[s, (ac + d) % J] = r["fade"][d] * self.ring[s, (ac - p + d % p) % J] if d < G else np.float32(0)
                else:
                    col, n_in, n_out, p0, d0, wpos, ri = row[1:]
                    assert js._rated or ri == 0  # (the one-rate entry point does not read the eighth int)
                    assert (n_out, p0, d0) == ingest_plan(self.N[s], n_in, r["L"], r["M"]) and col == self.N[s] % J and p0 < r["L"]
                    assert 0 < n_in <= (J if js._rated else js.W) and n_out <= op[2] <= js.ring_len and 0 <= wpos < js.ring_len
                    self.out[s].extend(self.ring[s, (col + np.arange(n_in)) % J].tolist())
                    self.N[s] += n_in

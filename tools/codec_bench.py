"""The expand verb (afx_k_payload_expand) and a jitter front in DVI4, measured.

  expand  the launch alone, over a staging buffer that is already on the device: 2 048 DVI4 rows of 20 ms at 8 kHz (84-byte
          packets, one wave each, three 64-code steps), and one 1-s block (8 000 codes: 125 steps on one wave).  --launches
          launches back to back between two device events, the time per launch; the median of --reps such runs.  The
          wave-per-block form is the only one built.
  feed    a ``JitterScorer`` over --streams slots at 8 kHz, depth 60 ms, fed one 20-ms packet per slot and tick, in order: once
          in dvi4, once the same audio in mulaw (the reference: no expand launch, a quarter of the staging bytes per sample),
          in one process.  The inner scorer only sums what it is pushed, so the front alone is timed.  The expectation to confirm
          or refute: the feed stays bound by the host planner, and the expand launch is a small fraction of it.

    python tools/codec_bench.py [--streams 2048] [--ticks 30] [--reps 5] [--launches 200] [--out profiles/codec_expand.txt]

A pass of the feed part is --ticks ticks back to back, wall clock around it, ending in a device synchronise; after a warm-up
pass of each way the two alternate for --reps passes each; the median per-feed time is reported with min and max, and the
host time inside the feed calls beside it.  The expand launch's output is compared with ``afx.codecs.reference`` once.
Nothing is asserted about a time.  The summary is printed and written to --out, stamped with afx_build_id()."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx import codecs  # noqa: E402
from afx._lib import call_on, check, lib  # noqa: E402
from afx.ingest import _at, layout, pack  # noqa: E402
from afx.jitter import JitterScorer  # noqa: E402
from afx.streaming import SlidingWindowScorer  # noqa: E402

H = 4000
RATE, PACKET = 8000, 160  # 20 ms
POOL = 16  # distinct streams, encoded once on the host and dealt to the slots in turn


class Summing(SlidingWindowScorer):
    """A streaming scorer that only adds up what it is pushed, per slot, on the device."""

    def __init__(self, S):
        super().__init__(None, S, window=4 * H, hop=H, device="cuda")
        self.acc = torch.zeros(S, dtype=torch.int64, device="cuda")

    def push(self, chunk, slots=None):
        idx = self._slot_list(slots, ordered=True)
        rows = torch.tensor(idx, dtype=torch.long, device=chunk.device)
        self.acc.index_add_(0, rows, chunk.view(torch.int32).to(torch.int64).sum(1))
        self._seen[idx] += H
        return torch.zeros(len(idx), device=chunk.device)


def speech(n, g):
    t = np.arange(n)
    x = 5000.0 * np.sin(2 * np.pi * t * g.uniform(0.01, 0.06)) * (1 + 0.5 * np.sin(t / 900.0)) + 300.0 * g.standard_normal(n)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def mulaw_encode(x):
    """int16 -> G.711 mu-law codes (the usual biased segment search, in numpy)."""
    v = x.astype(np.int32)
    mag = np.minimum(np.abs(v), 32635) + 132
    seg = np.clip(np.floor(np.log2(mag)).astype(np.int32) - 7, 0, 7)
    code = ((v < 0).astype(np.int32) << 7) | (seg << 4) | ((mag >> (seg + 3)) & 15)
    return (~code & 0xFF).astype(np.uint8)


def time_expand(blocks, launches, reps):
    """blocks: DVI4 packets -> (median seconds per launch of one expand call over all of them, min, max, output exact)."""
    offs, front = layout([len(b) for b in blocks])
    n = [codecs.samples(len(b), "dvi4") for b in blocks]
    zoffs, zone = layout([4 * k for k in n])
    (_, th), up = layout([front, 4 * codecs.EXPAND_HDR * len(blocks)])
    hdr = np.array([[o, len(b), up + z, 0] for o, z, b in zip(offs, zoffs, blocks)], dtype=np.int32)
    buf, _, _ = pack(blocks, [hdr])
    d = torch.zeros(up + zone, dtype=torch.uint8, device="cuda")
    d[:up] = buf.cuda()
    launch = lambda: check(call_on(d, lib().afx_k_payload_expand, _at(d, 0), d.numel(), _at(d, th), len(blocks), max(n)))
    launch()
    got = d.cpu().numpy()
    exact = all(got[up + z:up + z + 4 * k].tobytes() == codecs.reference(b, "dvi4").tobytes()
                for z, k, b in list(zip(zoffs, n, blocks))[:: max(1, len(blocks) // 32)])
    times = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3 / launches)
    t = sorted(times[1:])  # (the first run is the warm-up)
    return t[len(t) // 2], t[0], t[-1], exact


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--ticks", type=int, default=30, help="ticks (feeds of every slot) per pass")
    ap.add_argument("--reps", type=int, default=5, help="timed passes per way, and timed runs per expand shape")
    ap.add_argument("--launches", type=int, default=200, help="expand launches per timed run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_expand.txt"))
    args = ap.parse_args()
    S = args.streams
    if S <= 0 or args.ticks <= 0 or args.reps <= 0 or args.launches <= 0:
        raise SystemExit("--streams, --ticks, --reps, --launches: positive")
    if not torch.cuda.is_available():
        raise SystemExit("codec_bench measures on the GPU; there is no CPU fallback")
    torch.cuda.set_device(0)
    g = np.random.default_rng(31)
    passes = 1 + args.reps
    n_pk = passes * args.ticks
    # the pool: per stream its packets in dvi4 (the encoder's state runs on from packet to packet) and in mulaw
    dvi4, mulaw = [], []
    for _ in range(POOL):
        x, state = speech(n_pk * PACKET, g), None
        row = []
        for k in range(n_pk):
            blk, state = codecs.dvi4_encode(x[k * PACKET:(k + 1) * PACKET], state)
            row.append(blk)
        dvi4.append(row)
        mulaw.append([mulaw_encode(x[k * PACKET:(k + 1) * PACKET]).tobytes() for k in range(n_pk)])
    second, _ = codecs.dvi4_encode(speech(RATE, g))
    shapes = [(f"{S} rows of 20 ms at 8 kHz ({len(dvi4[0][0])}-byte packets)", [dvi4[s % POOL][s // POOL % n_pk] for s in range(S)]),
              (f"one 1-s block ({len(second)} bytes, {RATE} codes)", [second])]
    lines = [f"codec_bench: build {lib().afx_build_id().decode()}; afx_k_payload_expand, wave-per-block form (the only form built); "
             f"{args.launches} launches back to back between device events per run, median of {args.reps} runs after a warm-up run"]
    expand_s, exact = None, True
    for what, blocks in shapes:
        med, lo, hi, ok = time_expand(blocks, args.launches, args.reps)
        exact = exact and ok
        expand_s = med if expand_s is None else expand_s
        lines.append(f"  expand  {med * 1e6:9.2f} us per launch (min {lo * 1e6:.2f}, max {hi * 1e6:.2f})   [{what}]; output equals the reference: {ok}")
    scorers = {"dvi4": JitterScorer(Summing(S), RATE, "dvi4", 480), "mulaw": JitterScorer(Summing(S), RATE, "mulaw", 480)}
    pool = {"dvi4": dvi4, "mulaw": mulaw}
    slots = list(range(S))
    times, host = {w: [] for w in scorers}, {w: [] for w in scorers}
    for rep in range(passes):
        prepared = {w: [([pool[w][s % POOL][rep * args.ticks + t] for s in slots], [(rep * args.ticks + t) * PACKET] * S)
                        for t in range(args.ticks)] for w in scorers}
        for way in (("dvi4", "mulaw") if rep % 2 == 0 else ("mulaw", "dvi4")):
            torch.cuda.synchronize()
            t_host, t0 = 0.0, time.perf_counter()
            for pk, ts in prepared[way]:
                a = time.perf_counter()
                scorers[way].feed(pk, slots, ts)
                t_host += time.perf_counter() - a
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep > 0:
                times[way].append(dt / args.ticks)
                host[way].append(t_host / args.ticks)
    fed = all(int(sc.samples_seen.min()) >= H and int(sc.stats()["concealed"].sum()) == 0 for sc in scorers.values())
    lines.append(f"  feed: JitterScorer, {S} slots at {RATE} Hz, depth 60 ms, one 20-ms packet per slot and tick, in order, no loss; a summing "
                 f"inner scorer (the front alone); {args.ticks} ticks per pass, {args.reps} timed passes per way after a warm-up pass of each, "
                 f"the ways alternating; wall clock around a pass that ends in a device synchronise; every slot scored and nothing concealed: {fed}")
    med = {}
    for way in ("dvi4", "mulaw"):
        t, h = sorted(times[way]), sorted(host[way])
        med[way] = t[len(t) // 2]
        lines.append(f"  {way:6s} {med[way] * 1e3:8.3f} ms per feed of all {S} slots (min {t[0] * 1e3:.3f}, max {t[-1] * 1e3:.3f}); host time "
                     f"inside the feed calls {h[len(h) // 2] * 1e3:.3f} ms")
    t = sorted(times["mulaw"])
    lines.append(f"  dvi4 / mulaw {med['dvi4'] / med['mulaw']:.2f}x (spread of mulaw: {(t[-1] - t[0]) / med['mulaw'] * 100:.1f} % of its median); "
                 f"the expand launch of {S} rows is {expand_s / med['dvi4'] * 100:.2f} % of a dvi4 feed")
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    if not (exact and fed):
        raise SystemExit(1)


if __name__ == "__main__":
    main()

"""The jitter buffer over several clock rates at once, measured: S live calls in four groups (8 kHz mu-law, 8 kHz A-law -- a
second encoding at the same rate --, 16 kHz pcm_s16le, 48 kHz pcm_s16le; S / 4 slots each) deliver --packet-ms packets over a
network that loses --loss of them and shuffles the rest within the playout depth.  The inner scorer only sums what it is
pushed, so the front alone is timed.  Two ways over the same packets, in one process:

  mixed   one afx.jitter.MixedJitterScorer over all S slots: per tick one ``feed`` = one upload, and per round one
          afx_k_jitter_place_rates, one afx_k_jitter_conceal_rates per gap rank, one afx_k_jitter_release_rates and one pop;
  split   what a service runs without it: one afx.jitter.JitterScorer per rate (8 kHz with both encodings over S / 2 slots,
          16 kHz and 48 kHz over S / 4 each), per tick one ``feed`` each = three uploads and three times the launches.

    python tools/jitter_mixed_bench.py [--streams 2048] [--packet-ms 20] [--depth-ms 60] [--loss 0.02] [--ticks 30] [--reps 5]
                                       [--out profiles/jitter_mixed.txt]

A pass is --ticks ticks back to back, wall clock around it, ending in a device synchronise; the per-feed time of a pass is
its time over its ticks (a tick of the split way is its three feeds).  After a warm-up pass of each way (results compared:
every slot's pushed sums, pending, playout point, buffered span and the five counters must agree exactly) the two ways
alternate for --reps passes each, over new packets of the same streams; the median per-feed time is reported with min and
max, and the host time inside the feed calls (launches are asynchronous) beside it.  Nothing is asserted about a time.  The
summary is printed and written to --out, stamped with afx_build_id()."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx._lib import lib  # noqa: E402
from afx.jitter import JitterScorer, MixedJitterScorer  # noqa: E402
from afx.streaming import SlidingWindowScorer  # noqa: E402

H = 4000
GROUPS = [(8000, "mulaw"), (8000, "alaw"), (16000, "pcm_s16le"), (48000, "pcm_s16le")]
RATES = [(8000, ("mulaw", "alaw")), (16000, ("pcm_s16le",)), (48000, ("pcm_s16le",))]  # the split way's scorers
DTYPE = {"mulaw": np.uint8, "alaw": np.uint8, "pcm_s16le": np.dtype("<i2")}
BLOCK = 3  # packets shuffled among themselves: the depth in packets


class Summing(SlidingWindowScorer):
    """A streaming scorer that only adds up what it is pushed, per slot, on the device: the bit patterns of the samples as
    integers, so the sum is exact whatever the order and the batch, and equal sums mean the front made the same samples."""

    def __init__(self, S):
        super().__init__(None, S, window=4 * H, hop=H, device="cuda")
        self.acc = torch.zeros(S, dtype=torch.int64, device="cuda")

    def push(self, chunk, slots=None):
        idx = self._slot_list(slots, ordered=True)
        rows = torch.tensor(idx, dtype=torch.long, device=chunk.device)
        self.acc.index_add_(0, rows, chunk.view(torch.int32).to(torch.int64).sum(1))
        self._seen[idx] += H
        return torch.zeros(len(idx), device=chunk.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--packet-ms", type=int, default=20)
    ap.add_argument("--depth-ms", type=int, default=60)
    ap.add_argument("--loss", type=float, default=0.02)
    ap.add_argument("--ticks", type=int, default=30, help="ticks (feeds of every slot) per pass, a multiple of 3")
    ap.add_argument("--reps", type=int, default=5, help="timed passes per way")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jitter_mixed.txt"))
    args = ap.parse_args()
    S, ng = args.streams, len(GROUPS)
    if S % ng or S <= 0:
        raise SystemExit(f"--streams: a positive multiple of {ng}")
    if args.ticks % BLOCK or args.ticks <= 0 or args.depth_ms < BLOCK * args.packet_ms:
        raise SystemExit(f"--ticks: a positive multiple of {BLOCK}; --depth-ms: at least {BLOCK} packets")
    if not torch.cuda.is_available():
        raise SystemExit("jitter_mixed_bench measures on the GPU; there is no CPU fallback")
    torch.cuda.set_device(0)
    per = S // ng
    passes = 1 + args.reps
    g = np.random.default_rng(29)
    pk = [r * args.packet_ms // 1000 for r, _ in GROUPS]  # samples per packet, per group
    n_pk = passes * args.ticks
    data, origin = [], []
    for (r, e), p in zip(GROUPS, pk):
        v = g.integers(0, 256, (per, n_pk * p), dtype=np.uint8) if e != "pcm_s16le" else g.integers(-4000, 4000, (per, n_pk * p), dtype=np.int16)
        data.append(v.astype(DTYPE[e], copy=False))
        origin.append(g.integers(0, 1 << 32, per))
    # mixed slot f + ng * i <-> slot i of group f; the split way's 8 kHz scorer holds group 0 in its slots [0, per), group 1 after
    mixed = MixedJitterScorer(Summing(S), GROUPS, args.depth_ms)
    mixed.reset(list(range(S)), [GROUPS[s % ng][0] for s in range(S)])
    split = [JitterScorer(Summing(per * len(encs)), r, encs, args.depth_ms * r // 1000) for r, encs in RATES]
    home = [(0, 0), (0, per), (1, 0), (2, 0)]  # group -> (the split way's scorer, its first slot there)

    def tick_rows(t):
        """The rows of tick t (packet index within a block shuffled per stream, some lost) -> (mixed feed args, split feed args)."""
        base = t - t % BLOCK
        m = ([], [], [], [])
        sp = [([], [], [], []) for _ in RATES]
        for f, ((r, e), p) in enumerate(zip(GROUPS, pk)):
            ks = base + perm[f][:, t % BLOCK]
            keep = np.flatnonzero(~lost[f][np.arange(per), ks])
            sc, first = home[f]
            for i, k in zip(keep.tolist(), ks[keep].tolist()):
                raw, ts = data[f][i, k * p:(k + 1) * p].tobytes(), int((origin[f][i] + k * p) % (1 << 32))
                for dst, slot in ((m, f + ng * i), (sp[sc], first + i)):
                    dst[0].append(raw)
                    dst[1].append(slot)
                    dst[2].append(ts)
                    dst[3].append(e)
        return m, sp

    def feed(way, rows):
        if way == "mixed":
            mixed.feed(rows[0], rows[1], rows[2], encodings=rows[3])
        else:
            for sc, r in zip(split, rows):
                if r[1]:
                    sc.feed(r[0], r[1], r[2], encodings=r[3])

    def gathered(fn):
        """A per-slot quantity of the split way's scorers in the mixed scorer's slot order."""
        parts = [fn(sc) for sc in split]
        by_group = [parts[sc][first:first + per] for sc, first in home]
        return torch.stack(by_group, dim=1).reshape(-1)

    times, host = {"mixed": [], "split": []}, {"mixed": [], "split": []}
    same = None
    for rep in range(passes):
        lost = [g.random((per, n_pk)) < args.loss for _ in GROUPS]
        for f in range(ng):
            lost[f][:, 0] = False  # (the first packet is the session's origin)
        perm = [np.argsort(g.random((per, BLOCK)), axis=1) for _ in GROUPS]
        prepared = [tick_rows(rep * args.ticks + t) for t in range(args.ticks)]
        for way in (("mixed", "split") if rep % 2 == 0 else ("split", "mixed")):  # the two ways alternate, over the same packets
            torch.cuda.synchronize()
            t_host, t0 = 0.0, time.perf_counter()
            for m, sp in prepared:
                a = time.perf_counter()
                feed(way, m if way == "mixed" else sp)
                t_host += time.perf_counter() - a
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep > 0:
                times[way].append(dt / args.ticks)
                host[way].append(t_host / args.ticks)
        if rep == 0:  # the warm-up pass: both ways must have done the same thing
            same = torch.equal(mixed.scorer.acc, gathered(lambda sc: sc.scorer.acc))
            for q in ("pending", "samples_in", "buffered", "samples_seen"):
                same = same and torch.equal(getattr(mixed, q), gathered(lambda sc: getattr(sc, q)))
            for k, v in mixed.stats().items():
                same = same and torch.equal(v, gathered(lambda sc: sc.stats()[k]))
            same = bool(same and int(mixed.samples_seen.min()) >= H and int(mixed.stats()["concealed"].sum()) > 0)
    lines = [f"jitter_mixed_bench: build {lib().afx_build_id().decode()}; {S} slots, {per} each of " +
             ", ".join(f"{r} Hz {e}" for r, e in GROUPS) + f"; {args.packet_ms}-ms packets, depth {args.depth_ms} ms, "
             f"{args.loss * 100:g} % lost, the rest shuffled within {BLOCK} packets; a summing inner scorer (the front alone); "
             f"{args.ticks} ticks per pass, {args.reps} timed passes per way after a warm-up pass of each, the ways alternating over "
             "the same packets; wall clock around a pass that ends in a device synchronise",
             f"  results identical on the warm-up pass (pushed sums, pending, playout point, buffered span, scored counts and the "
             f"five counters of all {S} slots): {same}"]
    med = {}
    for way, what in (("mixed", "one MixedJitterScorer: 1 upload, 1 place_rates + 1 release_rates call per round"),
                      ("split", f"{len(RATES)} JitterScorers: {len(RATES)} uploads, {len(RATES)} place + release calls per round")):
        t, h = sorted(times[way]), sorted(host[way])
        med[way] = t[len(t) // 2]
        lines.append(f"  {way:6s} {med[way] * 1e3:8.3f} ms per feed of all {S} slots (min {t[0] * 1e3:.3f}, max {t[-1] * 1e3:.3f}); host time "
                     f"inside the feed calls {h[len(h) // 2] * 1e3:.3f} ms   [{what}]")
    t = sorted(times["split"])
    lines.append(f"  mixed / split {med['mixed'] / med['split']:.2f}x (spread of split: {(t[-1] - t[0]) / med['split'] * 100:.1f} % of its median)")
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

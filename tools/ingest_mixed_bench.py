"""The packet front over several formats at once, measured: S live calls in four formats (8 kHz mu-law, 8 kHz A-law, 16 kHz
pcm_s16le, 48 kHz pcm_s16le; S / 4 slots each) deliver --packet-ms packets, random phase per stream against the 250-ms hop.
The inner scorer only sums what it is pushed, so the front alone is timed.  Two ways over the same bytes, in one process:

  mixed   one afx.ingest.MixedPacketScorer over all S slots: per tick one ``feed`` = one upload, one afx_k_ingest_mixed call
          (one ingest launch and one history launch) and one pop per round;
  split   what a service runs without it: one afx.ingest.PacketScorer of S / 4 slots per format, per tick one ``feed`` each =
          four uploads, one afx_k_ingest launch pair per format and four pops per round.

    python tools/ingest_mixed_bench.py [--streams 2048] [--packet-ms 20] [--ticks 50] [--reps 5] [--out profiles/ingest_mixed.txt]

A pass is --ticks ticks back to back, wall clock around it, ending in a device synchronise; the per-feed time of a pass is
its time over its ticks (a tick of the split way is its four feeds).  After a warm-up pass of each way (every launch shape
of the timed passes; results compared: every slot's pushed sums, pending and input counts must agree exactly) the two ways
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
from afx.ingest import MixedPacketScorer, PacketScorer  # noqa: E402
from afx.streaming import SlidingWindowScorer  # noqa: E402

H = 4000
FORMATS = [(8000, "mulaw"), (8000, "alaw"), (16000, "pcm_s16le"), (48000, "pcm_s16le")]
DTYPE = {"mulaw": np.uint8, "alaw": np.uint8, "pcm_s16le": np.dtype("<i2")}


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
    ap.add_argument("--ticks", type=int, default=50, help="ticks (feeds of every slot) per pass")
    ap.add_argument("--reps", type=int, default=5, help="timed passes per way")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_mixed.txt"))
    args = ap.parse_args()
    S, nf = args.streams, len(FORMATS)
    if S % nf or S <= 0:
        raise SystemExit(f"--streams: a positive multiple of {nf}")
    if not torch.cuda.is_available():
        raise SystemExit("ingest_mixed_bench measures on the GPU; there is no CPU fallback")
    torch.cuda.set_device(0)
    per = S // nf
    passes = 1 + args.reps
    g = np.random.default_rng(23)
    pk = [r * args.packet_ms // 1000 for r, _ in FORMATS]  # samples per packet, per format
    n_total = [(1 + passes * args.ticks) * p for p in pk]
    data, phase = [], []
    for (r, e), p, n in zip(FORMATS, pk, n_total):
        v = g.integers(0, 256, (per, n), dtype=np.uint8) if e != "pcm_s16le" else g.integers(-4000, 4000, (per, n), dtype=np.int16)
        data.append(v.astype(DTYPE[e], copy=False))
        phase.append(g.integers(0, p, per))  # the first packet of each stream is cut short
    # mixed slot f + nf * i <-> slot i of the split way's scorer f
    mixed = MixedPacketScorer(Summing(S), FORMATS)
    mixed.reset(list(range(S)), [s % nf for s in range(S)])
    split = [PacketScorer(Summing(per), r, e) for r, e in FORMATS]
    all_slots, sub_slots = list(range(S)), list(range(per))

    def cut(pos, first=False):
        """The next packet of every stream -> per format the list of its slots' packets; pos moves on."""
        out = []
        for f in range(nf):
            n = phase[f] if first else np.full(per, pk[f])
            out.append([data[f][i, pos[f][i]:pos[f][i] + n[i]].tobytes() for i in range(per)])
            pos[f] += n
        return out

    def interleave(by_format):
        return [by_format[s % nf][s // nf] for s in range(S)]

    def feed(way, tick):
        if way == "mixed":
            mixed.feed(tick, all_slots)
        else:
            for f in range(nf):
                split[f].feed(tick[f], sub_slots)

    pos = [np.zeros(per, dtype=np.int64) for _ in range(nf)]
    first = cut(pos, first=True)
    feed("mixed", interleave(first))
    feed("split", first)
    times, host = {"mixed": [], "split": []}, {"mixed": [], "split": []}
    same = None
    for rep in range(passes):
        ticks = [cut(pos) for _ in range(args.ticks)]
        prepared = {"mixed": [interleave(t) for t in ticks], "split": ticks}
        for way in (("mixed", "split") if rep % 2 == 0 else ("split", "mixed")):  # the two ways alternate, over the same packets
            torch.cuda.synchronize()
            t_host, t0 = 0.0, time.perf_counter()
            for tick in prepared[way]:
                a = time.perf_counter()
                feed(way, tick)
                t_host += time.perf_counter() - a
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep > 0:
                times[way].append(dt / args.ticks)
                host[way].append(t_host / args.ticks)
        if rep == 0:  # the warm-up pass: both ways must have done the same thing
            acc = torch.stack([sc.scorer.acc for sc in split], dim=1).reshape(-1)  # (per, nf) -> mixed slot order
            pend = torch.stack([sc.pending for sc in split], dim=1).reshape(-1)
            nin = torch.stack([sc.samples_in for sc in split], dim=1).reshape(-1)
            seen = torch.stack([sc.samples_seen for sc in split], dim=1).reshape(-1)
            same = (torch.equal(mixed.scorer.acc, acc) and torch.equal(mixed.pending, pend) and torch.equal(mixed.samples_in, nin)
                    and torch.equal(mixed.samples_seen, seen) and int(seen.min()) >= H)
    lines = [f"ingest_mixed_bench: build {lib().afx_build_id().decode()}; {S} slots, {per} each of " +
             ", ".join(f"{r} Hz {e}" for r, e in FORMATS) + f"; {args.packet_ms}-ms packets, random phase per stream; a summing inner "
             f"scorer (the front alone); {args.ticks} ticks per pass, {args.reps} timed passes per way after a warm-up pass of each, "
             "the ways alternating over the same packets; wall clock around a pass that ends in a device synchronise",
             f"  results identical on the warm-up pass (pushed sums, pending, input and scored counts of all {S} slots): {same}"]
    med = {}
    for way, what in (("mixed", "one MixedPacketScorer: 1 upload, 1 afx_k_ingest_mixed call per round"),
                      ("split", f"{nf} PacketScorers: {nf} uploads, {nf} afx_k_ingest launch pairs per round")):
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

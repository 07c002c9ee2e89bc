"""Three ways to produce the same per-hop timeline of one long recording, timed (student fp16, full 6-layer trunk,
4-s window, 250-ms hop):

  timeline     afx.timeline.score_timeline: conv layers 0-5 once over the recording, the tail on batches of windows
  unfold       the recording unfolded into windows (tiled history for the first ones), Engine.forward at batch 64
  incremental  a one-slot IncrementalScorer pushed hop by hop

    python tools/timeline_bench.py [--seconds 600] [--reps 3] [--batch 64]

The three score vectors must be identical (torch.equal); windows/s per method is the median over --reps timed passes after
one warm-up pass (min and max given as the spread).  Stamped with afx_build_id()."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx import engine, harness, synth  # noqa: E402
from afx._lib import lib  # noqa: E402
from afx.streaming import IncrementalScorer  # noqa: E402
from afx.timeline import score_timeline  # noqa: E402

W, H = 64000, 4000


def by_timeline(eng, sd, x, B):
    return score_timeline(eng, [x], window=W, hop=H, batch_windows=B, state_dict=sd)[0].scores


def by_unfold(eng, sd, x, B):
    n = x.numel() // H
    warm = [(j + 1) * H for j in range(n) if (j + 1) * H < W]
    out = []
    for i in range(0, len(warm), B):
        out.append(eng.forward(harness.batch_adjust_duration([x[:e] for e in warm[i:i + B]], W))[:, 1])
    wins = x[(len(warm) + 1) * H - W:n * H].unfold(0, W, H)  # (steady windows: a view)
    for i in range(0, wins.shape[0], B):
        out.append(eng.forward(wins[i:i + B].contiguous())[:, 1])
    return torch.cat(out).cpu()


def by_incremental(eng, sd, x, B):
    sc = IncrementalScorer(eng, sd, 1, window=W, hop=H)
    out = torch.empty(x.numel() // H, dtype=torch.float32, device=x.device)
    for j in range(out.numel()):
        out[j:j + 1] = sc.push(x[None, j * H:(j + 1) * H])
    return out.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    sd = synth.model_state_dict("ConformerModel", n_layers=6)
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(sd)
    x = synth.waveforms(1, int(16000 * args.seconds), batch_idx=9001)[0].cuda()
    n = x.numel() // H
    print(f"timeline_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), recording {args.seconds:g} s, "
          f"window {W}, hop {H}: {n} windows, batch {args.batch}, {args.reps} timed passes per method", flush=True)
    results = {}
    for name, fn in (("timeline", by_timeline), ("unfold", by_unfold), ("incremental", by_incremental)):
        results[name] = fn(eng, sd, x, args.batch)  # warm-up pass (its scores are compared)
        rates = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = fn(eng, sd, x, args.batch)
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
            if not torch.equal(s, results[name]):
                raise SystemExit(f"{name}: scores differ between passes")
        rates.sort()
        results[name + "_rate"] = rates
        print(f"  {name:12s} {rates[len(rates) // 2]:10.1f} windows/s  (min {rates[0]:.1f}, max {rates[-1]:.1f})", flush=True)
    same = torch.equal(results["timeline"], results["unfold"]) and torch.equal(results["timeline"], results["incremental"])
    med = {k: results[k + "_rate"][len(results[k + "_rate"]) // 2] for k in ("timeline", "unfold", "incremental")}
    print(f"  scores identical across the three methods: {same}; timeline / unfold {med['timeline'] / med['unfold']:.2f}x, "
          f"timeline / incremental {med['timeline'] / med['incremental']:.1f}x", flush=True)
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

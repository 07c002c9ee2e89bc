"""The two launches of conceal="pitch_sync" alone (afx_k_jitter_pitch, afx_k_jitter_conceal_period), beside the launch they
stand in for (afx_k_jitter_conceal, "repeat"): device events around --iters back-to-back launches, the median of --passes
passes, the variants alternating inside each pass.  Rings hold the voiced test signal of tests/test_gpu_jitter_pitch.py.

    python tools/jitter_pitch_bench.py [--rows 2048] [--iters 200] [--passes 7] [--out profiles/jitter_pitch.txt]

Prints, stamped with afx_build_id(): the estimate for --rows gaps at 8 kHz and for one gap at 48 kHz, the synthesis and the
"repeat" conceal for --rows rows of 20 ms at 8 kHz, and the ring memory per slot of both modes at a 60-ms depth."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx._lib import call_on, check, lib, ptr  # noqa: E402
from afx.jitter import JitterScorer, gain_table, pitch_lags  # noqa: E402
from afx.streaming import SlidingWindowScorer  # noqa: E402


def ring_of(rate, S, J, f0=125):
    t = np.arange(J) / rate
    x = 0.1 * sum(np.sin(2 * np.pi * f0 * k * t + k) / k for k in range(1, 8))
    g = np.random.default_rng(rate)
    return torch.from_numpy((x[None, :] + 0.003 * g.standard_normal((S, J))).astype(np.float32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the printed lines to this file")
    args = ap.parse_args()
    l, S = lib(), args.rows
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    variants = {}
    # 8 kHz: --rows gaps, each slot its own; 20 ms rows for the synthesis and for "repeat"
    Pmin, Pmax, Wc = pitch_lags(8000)
    P0, Hd, F, J = 80, 80, 400, 3081
    ring8 = ring_of(8000, S, J)
    written = ring8.clone()  # (the ring the two conceal launches write: the estimate's stays the signal)
    g = np.random.default_rng(1)
    cols = g.integers(0, J, S)
    hdr2 = torch.from_numpy(np.stack([np.arange(S), cols], axis=1).astype(np.int32)).cuda()
    hdr4 = torch.from_numpy(np.stack([np.arange(S), cols, np.zeros(S), np.full(S, 160)], axis=1).astype(np.int32)).cuda()
    period8 = torch.zeros(S, dtype=torch.int32).cuda()
    gain, fade = torch.from_numpy(gain_table(Hd, F)).cuda(), torch.from_numpy((1.0 - np.arange(240) / 240).astype(np.float32)).cuda()
    variants[f"estimate, {S} rows at 8 kHz"] = lambda: check(call_on(ring8, l.afx_k_jitter_pitch, ptr(ring8), S, J, ptr(hdr2), S, Pmin,
                                                                     Pmax, Wc, P0, ptr(period8)))
    variants[f"synthesis, {S} rows of 20 ms at 8 kHz"] = lambda: check(call_on(
        written, l.afx_k_jitter_conceal_period, ptr(written), S, J, ptr(hdr4), S, 160, ptr(gain), ptr(period8), Pmin, Pmax, P0, Hd, F))
    variants[f"repeat conceal, {S} rows of 20 ms at 8 kHz"] = lambda: check(call_on(
        written, l.afx_k_jitter_conceal, ptr(written), S, J, ptr(hdr4), S, 160, ptr(fade), 80, 240, 1))
    # 48 kHz: one gap
    q = pitch_lags(48000)
    J48 = 18481
    ring48 = ring_of(48000, 1, J48)
    hdr48, period48 = torch.tensor([[0, 7000]], dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    variants["estimate, 1 row at 48 kHz"] = lambda: check(call_on(ring48, l.afx_k_jitter_pitch, ptr(ring48), 1, J48, ptr(hdr48), 1, *q, 480,
                                                                  ptr(period48)))
    for fn in variants.values():  # warm-up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    names = list(variants)
    for p in range(args.passes):
        for name in names[p % len(names):] + names[:p % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                variants[name]()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
    say(f"jitter_pitch_bench: build {l.afx_build_id().decode()}; {torch.cuda.get_device_name(0)}; device events around {args.iters} "
        f"back-to-back launches, median of {args.passes} passes (min, max), variants alternating inside a pass")
    for name, t in times.items():
        t.sort()
        say(f"  {name:44s} {t[len(t) // 2]:8.2f} us per launch (min {t[0]:.2f}, max {t[-1]:.2f})")
    say(f"  periods found: 8 kHz {sorted(set(period8.tolist()))[:6]} (rate / f0 = 64), 48 kHz {period48.tolist()} (384)")
    inner = SlidingWindowScorer(None, 1, window=16000, hop=4000, device="cpu")
    for rate in (8000, 16000, 48000):
        old, new = (JitterScorer(inner, rate, "mulaw", 60 * rate // 1000, conceal=m) for m in ("repeat", "pitch_sync"))
        say(f"  ring per slot at {rate} Hz, depth 60 ms: lookback {old.lookback} -> {new.lookback} columns, J {old.J} -> {new.J} "
            f"({4 * old.J} -> {4 * new.J} bytes)")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

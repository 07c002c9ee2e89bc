"""Offline resampling to 16 kHz (afx/resample.py, afx_k_resample): time of one batch of 4-s clips at each input rate,
achieved bytes/s against the 8 TB/s HBM bound, and its share of the fp16 Conformer student's batch forward at 16 kHz.

    python tools/resample_bench.py [--batch 64] [--seconds 4] [--rates 48000 44100 8000 96000] [--reps 50] [--no-forward]

Times are device-event medians over --reps calls after a warm-up.  Bytes = fp32 input + fp32 output + the tap table (the
least a pass must move).  For kernel times run it under ``rocprofv3 --kernel-trace --stats`` (resample_kernel rows)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx import engine, synth  # noqa: E402
from afx.resample import Resampler  # noqa: E402

HBM = 8.0e12


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--rates", type=int, nargs="*", default=[48000, 44100, 8000, 96000])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-forward", action="store_true", help="skip the student forward (the share column)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    B = args.batch
    fwd_ms = None
    if not args.no_forward:
        sd = synth.model_state_dict("ConformerModel", n_layers=6)
        eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
        eng.load_state_dict(sd)
        wave = synth.waveforms(B, int(16000 * args.seconds)).cuda()
        fwd_ms = _median_ms(lambda: eng.forward(wave), max(10, args.reps // 5))
        print(f"student fp16 forward, batch {B} x {args.seconds:g} s at 16 kHz: {fwd_ms:.3f} ms", flush=True)
    for r in args.rates:
        rs = Resampler(r)
        N = int(r * args.seconds)
        x = (0.1 * torch.randn(B, N, generator=torch.Generator().manual_seed(r))).cuda()
        ms = _median_ms(lambda: rs(x), args.reps)
        nbytes = 4 * (B * N + B * rs.n_out(N) + rs.taps.numel())
        line = (f"resample {r:6d} Hz -> 16 kHz, batch {B} x {args.seconds:g} s (L {rs.L}, M {rs.M}, T {rs.T}): {ms * 1e3:8.1f} us  "
                f"{nbytes / 1e6:6.1f} MB  {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s ({100 * nbytes / (ms * 1e-3) / HBM:4.1f} % of 8 TB/s)")
        if fwd_ms:
            line += f"  {100 * ms / fwd_ms:5.2f} % of the student forward"
        print(line, flush=True)


if __name__ == "__main__":
    main()

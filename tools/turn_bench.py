"""What scoring per talk spurt costs beside the speech gate, on the same build: S live streams of seeded synthetic talk-spurt
audio (tools/gate_bench.py's ``talk_spurts``) pushed hop by hop (250 ms) two ways, over the same stand-in for a model (the
sum of the window: the layers are measured, not a model):

  turns   afx.turns.TurnScorer around SlidingWindowScorer(sum, S, 64000, 64000): per push the gate's launch, afx_k_turn, the
          read-back of ``done``, and -- where a row closed a turn -- afx_k_turn_collect and one inner push of whole clips;
  gated   afx.vad.GatedScorer around SlidingWindowScorer(sum, S, 64000, 4000): the gate's launch, the read-back of ``kept``,
          one pop and one inner push of hops.

    python tools/turn_bench.py [--streams 2048] [--activity 0.4] [--hops 16] [--reps 3]

The two paths score different things by design (one score per utterance against one per 250 ms of kept audio), so their
scores are not compared; the contracts are pinned by tests/test_gpu_turns.py and tests/test_gpu_vad.py.  The paths
alternate pass by pass in one process; times are the median over --reps timed passes after one warm-up pass (min and max
given), wall clock around a pass that ends in a device synchronise.  On an MI355X the report is written to
profiles/turn_stream.txt, stamped with afx_build_id().  Nothing asserts a time."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd"), os.path.join(ROOT, "tools")]
from afx._lib import lib  # noqa: E402
from afx.streaming import SlidingWindowScorer  # noqa: E402
from afx.turns import TurnPolicy, TurnScorer  # noqa: E402
from afx.vad import GatedScorer, SpeechGate, emitted  # noqa: E402
from gate_bench import talk_spurts  # noqa: E402

W, H = 64000, 4000


class Summing:
    """The stand-in for a model: (A, window) -> (A, 2), column 1 the sum of the window."""

    def forward(self, batch):
        s = batch.sum(dim=1)
        return torch.stack([-s, s], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=16, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    S, hops = args.streams, args.hops
    torch.cuda.set_device(0)
    warm = W // H + 2
    n_hops = warm + args.reps * hops
    g = np.random.default_rng(11)
    bank_hops = 4 * n_hops
    bank = torch.from_numpy(np.stack([talk_spurts(bank_hops * H, args.activity, g) for _ in range(args.bank)])).cuda()
    bank = bank.reshape(args.bank, bank_hops, H)
    which = torch.from_numpy(g.integers(0, args.bank, S)).cuda()
    start = torch.from_numpy(g.integers(0, bank_hops, S)).cuda()
    policy = TurnPolicy()
    paths = {"turns": TurnScorer(SlidingWindowScorer(Summing(), S, W, W), SpeechGate(), policy, hop=H),
             "gated": GatedScorer(SlidingWindowScorer(Summing(), S, W, H), SpeechGate())}
    scores = dict.fromkeys(paths, 0)
    times = {name: [] for name in paths}

    def run(name, t0, n):
        chunks = [bank[which, (start + t) % bank_hops].contiguous() for t in range(t0, t0 + n)]
        outs = []
        torch.cuda.synchronize()
        begin = time.perf_counter()
        for c in chunks:
            outs.append(paths[name].push(c))
        torch.cuda.synchronize()
        dt = time.perf_counter() - begin
        scores[name] += int(sum(emitted(o).sum() for o in outs))
        return dt / n

    for name in paths:
        run(name, 0, warm)
    for rep in range(args.reps):
        for name in paths:  # the two paths alternate, pass by pass
            times[name].append(run(name, warm + rep * hops, hops))
    report = [f"turn_bench: build {lib().afx_build_id().decode()}; {S} streams of synthetic talk spurts ({args.activity:.0%} talk), a "
              f"summing stand-in for the model, window {W}, hop {H}, gate {SpeechGate().params()}, min_frames {policy.min_frames}; "
              f"{hops} hops per pass, the median of {args.reps} timed passes per path (alternating) after a warm-up pass of {warm} hops"]
    med = {}
    for name, ts in times.items():
        ts = sorted(ts)
        med[name] = ts[len(ts) // 2]
        pushes = n_hops * S
        report.append(f"  {name:6s} {med[name] * 1e3:8.2f} ms per hop (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}); RTF "
                      f"{med[name] / 0.25:.3f}; {scores[name]} scores from {pushes} slot-pushes ({scores[name] / pushes:.2%})")
    st = paths["turns"].stats()
    report.append(f"  turns: {int(st['scored'].sum())} scored ({int(st['cut'].sum())} of them cut at the window), {int(st['short'].sum())} "
                  f"dropped as short, {int(st['kept_frames'].sum())} frames kept")
    report.append(f"  turns / gated {med['turns'] / med['gated']:.2f}x")
    print("\n".join(report), flush=True)
    if torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"):
        path = os.path.join(ROOT, "profiles", "turn_stream.txt")
        with open(path, "w") as f:
            f.write(f"tools/turn_bench.py {' '.join(sys.argv[1:])} on one MI355X: TurnScorer and GatedScorer over the same summing "
                    "stand-in scorer, alternating pass by pass in one process, on the same audio.  One run on one machine; the "
                    "kernels were not profiled separately.\n\n" + "\n".join(report) + "\n")
        print(f"  written to {path}", flush=True)


if __name__ == "__main__":
    main()

"""The verdict layer measured against the bare scorer on the same build, in the same process: S live streams of seeded
synthetic talk-spurt audio (tools/gate_bench.py's), the student scores them in KV-cached mode.  Two ways, timed per 250-ms hop:

  verdict   afx.verdict.VerdictScorer around the KV-cached scorer: every hop one ``push`` of all S slots, then one pinned
            upload of the (S x 2 int32) header (16 KB at 2048 streams) and one ``afx_k_verdict`` launch, no synchronisation;
  bare      the KV-cached scorer alone pushed the same hops.

    python tools/verdict_bench.py [--streams 2048] [--hops 8] [--reps 3] [--out profiles/verdict_stream.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/verdict_bench.py --profile   (verdict path only, 4 hops: kernel times,
                                                                                       a run of its own; writes no report)

The scores of the two paths are the same tensors bit for bit (tests/test_gpu_verdict.py pins that); printed with the times:
the events the pass logged and the slots in alarm at its end.  The policy's thresholds are the lower quartile (enter) and the
median (exit) of the warm-up pass's scores, so that alarms are raised and cleared during the timed passes.  Times are the median
over --reps timed passes after one warm-up pass (min and max given), wall clock around a pass that ends in a device
synchronise.  Nothing here asserts a time.  Stamped with afx_build_id()."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd"), os.path.join(ROOT, "tools")]
from afx import engine, synth  # noqa: E402
from afx._lib import lib  # noqa: E402
from afx.streaming import KVCachedScorer  # noqa: E402
from afx.verdict import VerdictPolicy, VerdictScorer  # noqa: E402
from gate_bench import talk_spurts  # noqa: E402

W, H = 64000, 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=8, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="the verdict path only, a short pass (for a rocprofv3 run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verdict_stream.txt"), help="the report is also written here")
    args = ap.parse_args()
    S = args.streams
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.cuda.set_device(0)
    sd = synth.model_state_dict("ConformerModel", n_layers=6)
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(sd)
    passes = 1 if args.profile else 1 + args.reps
    hops = 4 if args.profile else args.hops
    warm = W // H + 2
    n_hops = warm + passes * hops
    g = np.random.default_rng(11)
    bank_hops = 4 * n_hops
    bank = torch.from_numpy(np.stack([talk_spurts(bank_hops * H, args.activity, g) for _ in range(args.bank)])).cuda()
    bank = bank.reshape(args.bank, bank_hops, H)
    which = torch.from_numpy(g.integers(0, args.bank, S)).cuda()
    start = torch.from_numpy(g.integers(0, bank_hops, S)).cuda()

    def hop(t):
        return bank[which, (start + t) % bank_hops].contiguous()

    say(f"verdict_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams of synthetic talk "
        f"spurts; {hops} hops per pass, {args.reps} timed passes per path after a warm-up pass of {warm} hops")
    # the thresholds: from the bare scorer's own warm-up scores (a pass that is not timed)
    inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
    sc = torch.cat([inner.push(hop(t)).clone() for t in range(warm)]).cpu().numpy()
    sc = np.sort(sc[~np.isnan(sc)])
    policy = VerdictPolicy(float(sc[sc.size // 4]), float(sc[sc.size // 2]), alpha=0.3, confirm=2, release=2, min_scores=2)
    say(f"  policy {policy.params()}")
    del inner
    results = {}
    for name in (["verdict"] if args.profile else ["verdict", "bare"]):
        inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
        front = VerdictScorer(inner, policy) if name == "verdict" else inner

        def run(t0, n):
            chunks = [hop(t) for t in range(t0, t0 + n)]
            torch.cuda.synchronize()
            begin = time.perf_counter()
            for c in chunks:
                front.push(c)
            torch.cuda.synchronize()
            return time.perf_counter() - begin

        run(0, warm)
        times = []
        for rep in range(passes):
            dt = run(warm + rep * hops, hops)
            if rep > 0 or args.profile:
                times.append(dt / hops)
        times.sort()
        med = times[len(times) // 2]
        results[name] = (med, times)
        extra = ""
        if name == "verdict":
            kinds = front.take_events()[1]
            extra = (f"; {kinds.size} events (raised {int((kinds == 1).sum())}, cleared {int((kinds == 3).sum())}), "
                     f"{int(front.alarm.sum())} of {S} slots in alarm at the end")
        say(f"  {name:7s} {med * 1e3:8.2f} ms per hop (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); RTF {med / 0.25:.3f}{extra}")
        del front, inner
        torch.cuda.empty_cache()
    if not args.profile:
        (mv, tv), (mb, tb) = results["verdict"], results["bare"]
        say(f"  verdict / bare {mv / mb:.3f}x, {(mv - mb) * 1e6:+.0f} us per hop (spread of bare: {(tb[-1] - tb[0]) / mb * 100:.1f} % of its "
            f"median, of verdict: {(tv[-1] - tv[0]) / mv * 100:.1f} %)")
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The input-quality layer measured against the bare scorer on the same build, in the same process: S live streams of seeded
synthetic talk-spurt audio (tools/gate_bench.py's), an eighth of them through a saturating input stage, the student scores
them in KV-cached mode.  Two ways, timed per 250-ms hop:

  quality   afx.quality.QualityScorer around the KV-cached scorer: every hop one ``push`` of all S slots, then one pinned
            upload of the (S x 2 int32) header (16 KB at 2048 streams) and one ``afx_k_quality`` launch of S workgroups
            that read the chunk once (32 MB at 2048 streams of 4000 samples), no synchronisation;
  bare      the KV-cached scorer alone pushed the same hops.

    python tools/quality_bench.py [--streams 2048] [--hops 8] [--reps 3] [--out profiles/quality_stream.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/quality_bench.py --profile   (quality path only, 4 hops: kernel times,
                                                                                       a run of its own; writes no report)

Where a slot is valid the scores of the two paths are the same bit for bit (tests/test_gpu_quality.py pins that); printed
with the times: the hops each flag was set on and the slots whose score is withheld at the end.  The policy is the default
one.  Times are the median over --reps timed passes after one warm-up pass (min and max given), wall clock around a pass
that ends in a device synchronise.  Nothing here asserts a time.  Stamped with afx_build_id()."""
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
from afx.quality import FLAG_NAMES, QualityPolicy, QualityScorer  # noqa: E402
from afx.streaming import KVCachedScorer  # noqa: E402
from gate_bench import talk_spurts  # noqa: E402

W, H = 64000, 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=8, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="the quality path only, a short pass (for a rocprofv3 run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_stream.txt"), help="the report is also written here")
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
    streams = np.stack([talk_spurts(bank_hops * H, args.activity, g) for _ in range(args.bank)])
    streams[::8] = np.clip(streams[::8] * np.float32(30), -1, 1)  # every eighth stream of the bank: gain into a hard limiter
    bank = torch.from_numpy(streams).cuda().reshape(args.bank, bank_hops, H)
    which = torch.from_numpy(g.integers(0, args.bank, S)).cuda()
    start = torch.from_numpy(g.integers(0, bank_hops, S)).cuda()

    def hop(t):
        return bank[which, (start + t) % bank_hops].contiguous()

    policy = QualityPolicy()
    say(f"quality_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams of synthetic talk "
        f"spurts; {hops} hops per pass, {args.reps} timed passes per path after a warm-up pass of {warm} hops")
    say(f"  policy {policy.params()}")
    results = {}
    for name in (["quality"] if args.profile else ["quality", "bare"]):
        inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
        front = QualityScorer(inner, policy) if name == "quality" else inner

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
        if name == "quality":
            st = front.stats()
            extra = ("; hops flagged " + ", ".join(f"{k} {int(st[k].sum())}" for k in FLAG_NAMES)
                     + f" of {int(st['hops'].sum())}; {S - int(front.valid.sum())} of {S} scores withheld at the end")
        say(f"  {name:7s} {med * 1e3:8.2f} ms per hop (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); RTF {med / 0.25:.3f}{extra}")
        del front, inner
        torch.cuda.empty_cache()
    if not args.profile:
        (mq, tq), (mb, tb) = results["quality"], results["bare"]
        say(f"  quality / bare {mq / mb:.3f}x, {(mq - mb) * 1e6:+.0f} us per hop (spread of bare: {(tb[-1] - tb[0]) / mb * 100:.1f} % of its "
            f"median, of quality: {(tq[-1] - tq[0]) / mq * 100:.1f} %)")
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

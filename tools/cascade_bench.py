"""The cascade measured against the bare screen on the same build: S live streams of seeded synthetic talk-spurt audio
(tools/gate_bench.py's), the student screens them in KV-cached mode, the 24-layer teacher verifies.  Timed per 250-ms hop:

  bare      the KV-cached scorer alone, pushed lock-stepped: what the parent of the cascade could do;
  cascade   afx.cascade.CascadeScorer around a scorer of the same kind pushed the same hops, at a threshold below every
            score (nothing verified: the cost of a tick that only stores, selects and reads back (1 + budget) int32), and at
            thresholds that verify about 1 % and about 10 % of the slot-hops (taken from the bare run's own score quantiles;
            cooldown 0 and budget S, so that the share verified is the share of scores under the threshold);
  teacher   ``verifier.forward`` alone on batches of the sizes the cascade gave it, for the cost of the verified windows.

    python tools/cascade_bench.py [--streams 2048 256] [--hops 8] [--reps 3] [--out profiles/cascade_stream.txt]

The cascade never changes a screen score (tests/test_gpu_cascade.py), so nothing is compared here.  Times are the median
over --reps timed passes after a warm-up pass that fills the 4-s window (min and max given), wall clock around a pass that
ends in a device synchronise.  Stamped with afx_build_id()."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx import engine, synth  # noqa: E402
from afx._lib import lib  # noqa: E402
from afx.cascade import CascadePolicy, CascadeScorer  # noqa: E402
from afx.streaming import KVCachedScorer  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gate_bench import talk_spurts  # noqa: E402

W, H = 64000, 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[2048, 256])
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=8, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--teacher-layers", type=int, default=24)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = synth.model_state_dict("ConformerModel", n_layers=6)
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(sd)
    tsd = synth.model_state_dict("XLSR_AASIST", n_layers=args.teacher_layers)
    teacher = engine.Engine("xlsr_aasist", n_layers=args.teacher_layers, dtype="fp16")
    teacher.load_state_dict(tsd)
    passes, hops, warm = 1 + args.reps, args.hops, W // H + 2
    n_hops = warm + passes * hops
    g = np.random.default_rng(11)
    bank_hops = 4 * n_hops
    bank = torch.from_numpy(np.stack([talk_spurts(bank_hops * H, args.activity, g) for _ in range(args.bank)])).cuda()
    bank = bank.reshape(args.bank, bank_hops, H)
    say(f"cascade_bench: build {lib().afx_build_id().decode()}; screen: student fp16 (6 layers), KV-cached; verifier: XLSR_AASIST "
        f"fp16 ({args.teacher_layers} layers) on the 4-s window; synthetic talk spurts ({args.activity:.0%} talk); {hops} hops per "
        f"pass, {args.reps} timed passes per path after a warm-up pass of {warm} hops")
    for S in args.streams:
        which = torch.from_numpy(g.integers(0, args.bank, S)).cuda()
        start = torch.from_numpy(g.integers(0, bank_hops, S)).cuda()

        def hop(t):
            return bank[which, (start + t) % bank_hops].contiguous()

        def measure(front, keep=None, mark=None):
            """-> (median s per hop, sorted times); keep: a list that takes the timed passes' scores; mark: called once
            before the first timed pass."""
            def run(t0, n, timed):
                chunks = [hop(t) for t in range(t0, t0 + n)]
                torch.cuda.synchronize()
                begin = time.perf_counter()
                outs = [front.push(c) for c in chunks]
                torch.cuda.synchronize()
                dt = time.perf_counter() - begin
                if timed and keep is not None:
                    keep.extend(o.clone() for o in outs)
                return dt
            run(0, warm, False)
            times = []
            for rep in range(passes):
                if rep == 1 and mark is not None:
                    mark()
                dt = run(warm + rep * hops, hops, rep > 0)
                if rep > 0:
                    times.append(dt / hops)
            times.sort()
            return times[len(times) // 2], times

        say(f" S = {S}")
        scores = []
        bare, tb = measure(KVCachedScorer(eng, sd, S, window=W, hop=H), scores)
        say(f"  bare               {bare * 1e3:8.2f} ms per hop (min {tb[0] * 1e3:.2f}, max {tb[-1] * 1e3:.2f}); RTF {bare / 0.25:.3f}")
        torch.cuda.empty_cache()
        allsc = torch.cat(scores).float().cpu().numpy()
        batches = set()
        for name, thr in (("nothing verified", -3.0e38), ("about 1 % verified", float(np.quantile(allsc, 0.01))),
                          ("about 10 % verified", float(np.quantile(allsc, 0.10)))):
            cs = CascadeScorer(KVCachedScorer(eng, sd, S, window=W, hop=H), teacher, CascadePolicy(thr, min(S, 1024)), state_dict=tsd)
            base = {}

            def mark():
                cs.take_events()
                base.update({k: int(v.sum()) for k, v in cs.stats().items()})

            med, tc = measure(cs, mark=mark)
            ev = cs.take_events()
            st = {k: int(v.sum()) - base[k] for k, v in cs.stats().items()}  # (the timed passes only)
            share = st["verified"] / max(st["screened"], 1)
            sizes = [int(e[0].numel()) for e in ev]
            per_push = float(np.mean(sizes)) if sizes else 0.0
            if sizes:
                batches.add(int(round(per_push)))
            say(f"  cascade, {name:20s} {med * 1e3:8.2f} ms per hop (min {tc[0] * 1e3:.2f}, max {tc[-1] * 1e3:.2f}); RTF {med / 0.25:.3f}; "
                f"{med / bare:.3f}x bare, +{(med - bare) * 1e3:.2f} ms; threshold {thr:.6g}: {share:.2%} of the slot-hops verified, "
                f"{per_push:.1f} windows per verifying push, {st['passed_over']} candidates passed over")
            del cs
            torch.cuda.empty_cache()
        for B in sorted(b for b in batches if b > 0):
            x = hop(0)[:1].repeat(1, W // H).expand(B, W).contiguous()
            teacher.forward(x)
            torch.cuda.synchronize()
            times = []
            for _ in range(max(args.reps, 3)):
                begin = time.perf_counter()
                teacher.forward(x)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - begin)
            times.sort()
            say(f"  teacher alone, batch {B:4d}   {times[len(times) // 2] * 1e3:8.2f} ms per forward (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

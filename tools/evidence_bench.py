"""The evidence recorder measured against the verdict layer alone on the same build, in the same process: S live streams of
seeded synthetic talk-spurt audio (tools/gate_bench.py's), the student scores them in KV-cached mode.  Two ways, timed per
250-ms hop:

  evidence  afx.evidence.EvidenceScorer(VerdictScorer(KV-cached scorer)): every hop one ``push`` of all S slots, then one pinned
            upload of the (S x 2 int32) header and the ``afx_k_evidence_mark`` and ``afx_k_evidence_copy`` launches, no
            synchronisation;
  verdict   the same VerdictScorer alone pushed the same hops.

    python tools/evidence_bench.py [--streams 2048] [--raising 0.05] [--hops 8] [--reps 3] [--out profiles/evidence_stream.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/evidence_bench.py --profile   (evidence path only, 4 hops: kernel times,
                                                                                        a run of its own; writes no report)

``--raising``: the share of slots whose alarm is raised during a timed pass.  The verdict policy's ``enter`` is that quantile of
the warm-up pass's scores and ``exit`` is +inf with ``release`` 1, ``confirm`` 1: a slot whose score falls below ``enter``
raises and stays in alarm, so the share is approximate and the report prints what was counted (raised, recorded, dropped,
merged).  After the timed passes ``take_clips()`` is timed for a full pool: a fresh scorer under ``enter = +inf`` raises every
slot at its first score, the first ``--clips`` rows take the pool's entries, and a window and the post-roll are pushed; the time
is the wall clock of the one ``take_clips()`` that returns them, with the bytes read back.  Times are the
median over --reps timed passes after one warm-up pass (min and max given), wall clock around a pass that ends in a device
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
from afx.evidence import EvidencePolicy, EvidenceScorer  # noqa: E402
from afx.streaming import KVCachedScorer  # noqa: E402
from afx.verdict import VerdictPolicy, VerdictScorer  # noqa: E402
from gate_bench import talk_spurts  # noqa: E402

W, H = 64000, 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--raising", type=float, default=0.05, help="share of slots raising during a timed pass (approximate)")
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=8, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--post", type=int, default=8)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--encoding", default="fp32", choices=["fp32", "pcm16"])
    ap.add_argument("--profile", action="store_true", help="the evidence path only, a short pass (for a rocprofv3 run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence_stream.txt"), help="the report is also written here")
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

    epol = EvidencePolicy(post=args.post, clips=args.clips, encoding=args.encoding)
    say(f"evidence_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams of synthetic talk "
        f"spurts; {hops} hops per pass, {args.reps} timed passes per path after a warm-up pass of {warm} hops; evidence {epol.params()} "
        f"(pre = window // hop - 1 = {W // H - 1})")
    # the threshold: a quantile of the bare scorer's own warm-up scores (a pass that is not timed)
    inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
    sc = torch.cat([inner.push(hop(t)).clone() for t in range(warm)]).cpu().numpy()
    sc = np.sort(sc[~np.isnan(sc)])
    # (a slot raises when any of a pass's scores falls below enter: the per-score quantile that gives about the asked share)
    q = 1.0 - (1.0 - min(max(args.raising, 0.0), 1.0)) ** (1.0 / (warm + passes * hops))
    vpol = VerdictPolicy(float(sc[min(int(q * sc.size), sc.size - 1)]), float("inf"))
    say(f"  verdict policy {vpol.params()}")
    del inner
    results = {}
    for name in (["evidence"] if args.profile else ["evidence", "verdict"]):
        vs = VerdictScorer(KVCachedScorer(eng, sd, S, window=W, hop=H), vpol)
        front = EvidenceScorer(vs, epol) if name == "evidence" else vs

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
        extra = f"; {int(vs.alarm.sum())} of {S} slots in alarm at the end"
        if name == "evidence":
            extra += f"; {front.stats()}"
        say(f"  {name:8s} {med * 1e3:8.2f} ms per hop (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); RTF {med / 0.25:.3f}{extra}")
        del front, vs
        torch.cuda.empty_cache()
    if not args.profile:
        (me, te), (mv, tv) = results["evidence"], results["verdict"]
        say(f"  evidence / verdict {me / mv:.3f}x, {(me - mv) * 1e6:+.0f} us per hop (spread of verdict: {(tv[-1] - tv[0]) / mv * 100:.1f} % of its "
            f"median, of evidence: {(te[-1] - te[0]) / me * 100:.1f} %)")
        # take_clips() for a full pool: every entry COMPLETE with L hops
        es = EvidenceScorer(VerdictScorer(KVCachedScorer(eng, sd, S, window=W, hop=H), VerdictPolicy(float("inf"), float("inf"))), epol)
        for t in range(W // H + args.post + 1):
            es.push(hop(t))
        torch.cuda.synchronize()
        st = es.stats()
        begin = time.perf_counter()
        clips = es.take_clips()
        dt = time.perf_counter() - begin
        nbytes = sum(c.audio.nbytes + c.scores.nbytes for c in clips)
        say(f"  take_clips() of a full pool: {len(clips)} clips ({sum(c.complete for c in clips)} complete, {nbytes / 2**20:.1f} MiB, "
            f"longest {max(c.hops for c in clips)} hops) in {dt * 1e3:.2f} ms; before it {st}")
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

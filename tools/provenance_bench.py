"""What the provenance lane costs a jitter front (afx/provenance.py): S live calls send --packet-ms packets through a lossy
network (--loss never arrive, --reorder arrive one or two packets late, inside the playout depth) into a JitterScorer over
a summing stand-in for the model, as in tools/turn_bench.py, so that the front, not a model, is what is timed.  Two chains
of this build in one process, on the same arrivals:

  plain       JitterScorer(SlidingWindowScorer(stand-in)): no provenance layer below, so no lane -- the chain the parent
              commit had;
  provenance  JitterScorer(ProvenanceScorer(SlidingWindowScorer(stand-in))): the byte ring, one "spans" op per round, one
              afx_k_prov_frames launch per pop, one afx_k_provenance launch per push;
  --gate      both chains with a GatedScorer (plain SpeechGate) under the front: then also the mask, afx_k_prov_compact per
              gate launch and afx_k_prov_take per pop;
  --chain lookahead   both chains with a GatedScorer(LookaheadGate()) under the front, the layer's policy through="all": the
              mask, afx_k_prov_compact_la per gate launch (the delayed frames' counts in gline), afx_k_prov_take per pop;
  --chain turns       both chains with a TurnScorer (default gate and policy, pushes of one hop, a 4-s window) under the
              front, the layer around a scorer with hop == window, through="all": afx_k_prov_turn before every afx_k_turn, and
              per push that scores a turn afx_k_prov_turn_sum beside the collect.  The stand-in traffic is loud throughout, so
              every turn is a cut one of 400 frames: one scored turn per slot every 16 hops.

Every tick one ``feed(packets, slots, timestamps, score=False)`` with whatever arrived, one ``drain()`` per hop.  Both chains are
warmed up, then the timed passes alternate between them.  Reported per 250 ms of audio: wall clock around a pass that ends in
a device synchronise (median, min, max over --reps passes), the host time inside the feed / drain calls and the part of it
spent in the planner (``_plan``: where the spans rows are made).

  --parent DIR  instead: the chain without the layer against the parent commit.  DIR is a checkout of the parent commit with
              its own library built.  tools/jitter_bench.py --reps 5 (the student, KV-cached, behind a JitterScorer: a chain
              without the layer) is run as a child process from this tree and from DIR, --parent-runs times each, the two
              alternating, and the tool's "jitter" line of every run is reported with the build it measured.  The path is
              untouched by the lane, so this tree's figures should sit inside the parent's own run-to-run spread.

On an MI355X every invocation APPENDS its report, with its command line, to profiles/provenance_stream.txt (--chain turns
and --chain lookahead: to profiles/provenance_turns.txt), stamped with afx_build_id() (delete the file for a fresh one; what follows a "Reading" heading there is written by hand).  Nothing
asserts a time.

    python tools/provenance_bench.py [--streams 2048] [--packet-ms 20] [--loss 0.02] [--reorder 0.1] [--hops 8] [--reps 5] [--gate]
    python tools/provenance_bench.py --chain turns | --chain lookahead [the same options]
    python tools/provenance_bench.py --parent DIR [--parent-runs 2]
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx._lib import lib  # noqa: E402
from afx.jitter import JitterScorer  # noqa: E402
from afx.provenance import ProvenancePolicy, ProvenanceScorer  # noqa: E402
from afx.streaming import SlidingWindowScorer  # noqa: E402
from afx.turns import TurnScorer  # noqa: E402
from afx.vad import GatedScorer, LookaheadGate  # noqa: E402

W, H = 64000, 4000


class Summing:
    """The stand-in for a model: (A, window) -> (A, 2), column 1 the sum of the window."""

    def forward(self, batch):
        s = batch.sum(dim=1)
        return torch.stack([-s, s], dim=1)


HEADER = ("tools/provenance_bench.py on one MI355X: a jitter front over a summing stand-in scorer with and without the provenance "
          "layer below it, alternating pass by pass in one process, on the same arrivals; and (--parent) tools/jitter_bench.py of "
          "this tree and of a checkout of the parent commit.  Every section is one invocation, appended by the tool with its "
          "command line; the kernels were not profiled separately; nothing here is a gate.\n")


HEADER_TURNS = ("tools/provenance_bench.py --chain turns / --chain lookahead on one MI355X: a jitter front over a TurnScorer / a "
                "look-ahead gate and a summing stand-in scorer, with and without the provenance layer (through=\"all\") below it, "
                "alternating pass by pass in one process, on the same arrivals.  Every section is one invocation, appended by the tool "
                "with its command line; nothing here is a gate.\n")


def record(report, name="provenance_stream.txt", header=HEADER):
    """Print the report; on an MI355X append it, with the command line, to profiles/<name>."""
    print("\n".join(report), flush=True)
    if torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"):
        path = os.path.join(ROOT, "profiles", name)
        fresh = not os.path.exists(path)
        with open(path, "a") as f:
            f.write((header if fresh else "") + f"\n(tools/provenance_bench.py {' '.join(sys.argv[1:])})\n" + "\n".join(report) + "\n")
        print(f"  appended to {path}", flush=True)


def against_parent(args):
    """The --parent measurement (module docstring): child processes only, this process opens the GPU afterwards, to record."""
    trees = [("this tree", ROOT), ("parent", os.path.abspath(args.parent))]
    report = [f"provenance_bench --parent: tools/jitter_bench.py --reps 5 as a child process from each tree, {args.parent_runs} runs each, "
              "alternating; the tool's \"jitter\" line (a JitterScorer over the KV-cached student: a chain without the layer)"]
    med = {name: [] for name, _ in trees}
    for run in range(args.parent_runs):
        for name, tree in trees:
            out = subprocess.run([sys.executable, os.path.join("tools", "jitter_bench.py"), "--reps", "5"], cwd=tree, capture_output=True,
                                 text=True, timeout=600)
            if out.returncode:
                raise SystemExit(f"tools/jitter_bench.py failed in {tree}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            build = re.search(r"jitter_bench: build (\w+)", out.stdout).group(1)
            line = next(l for l in out.stdout.splitlines() if l.startswith("  jitter  "))
            med[name].append(float(re.search(r"([0-9.]+) ms per 250 ms", line).group(1)))
            report.append(f"  {name:9s} run {run + 1}, build {build}: {';'.join(line.strip().split(';')[:2])}")
    (a, b) = (med["this tree"], med["parent"])
    report.append(f"  this tree {min(a):.2f} to {max(a):.2f} ms, parent {min(b):.2f} to {max(b):.2f} ms per 250 ms of audio")
    record(report)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--packet-ms", type=int, default=20)
    ap.add_argument("--depth-ms", type=int, default=60)
    ap.add_argument("--loss", type=float, default=0.02)
    ap.add_argument("--reorder", type=float, default=0.1)
    ap.add_argument("--hops", type=int, default=8, help="hops of audio per timed pass")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gate", action="store_true", help="a GatedScorer under the front in both chains")
    ap.add_argument("--chain", choices=["default", "turns", "lookahead"], default="default",
                    help="turns: a TurnScorer under the front; lookahead: a GatedScorer(LookaheadGate()); the layer's policy is then through=\"all\"")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: measure "
                    "tools/jitter_bench.py of both trees instead")
    ap.add_argument("--parent-runs", type=int, default=2)
    args = ap.parse_args()
    if args.parent:
        return against_parent(args)
    S, rate = args.streams, args.rate
    pk, depth = rate * args.packet_ms // 1000, rate * args.depth_ms // 1000
    late_max = min(2, depth // pk)
    hop_in = -(-H * rate // 16000)
    ticks = args.hops * hop_in // pk
    warm_ticks = (W // H + 2) * hop_in // pk
    n_ticks = warm_ticks + (1 + args.reps) * ticks
    torch.cuda.set_device(0)
    g = np.random.default_rng(11)
    audio = [g.integers(0, 256, n_ticks * pk).astype(np.uint8) for _ in range(S)]
    origin = g.integers(0, 1 << 32, S)
    lost = g.random((S, n_ticks)) < args.loss
    lost[:, 0] = False  # (the first packet sets the origin)
    delay = np.where(g.random((S, n_ticks)) < args.reorder, g.integers(1, late_max + 1, (S, n_ticks)) if late_max else 0, 0)
    delay[:, 0] = 0
    arrivals = [[] for _ in range(n_ticks + late_max + 1)]
    for k in range(n_ticks):
        for s in np.flatnonzero(~lost[:, k]).tolist():
            arrivals[k + int(delay[s, k])].append((s, k))

    def tick_args(t):
        rows = arrivals[t]
        return ([audio[s][k * pk:(k + 1) * pk].tobytes() for s, k in rows], [s for s, _ in rows],
                np.array([(int(origin[s]) + k * pk) % (1 << 32) for s, k in rows], dtype=np.int64))

    if args.gate and args.chain != "default":
        raise SystemExit("--gate goes with the default chain")

    def chain(layer):
        s = SlidingWindowScorer(Summing(), S, W, W if args.chain == "turns" else H)
        s = ProvenanceScorer(s, ProvenancePolicy(through="plain" if args.chain == "default" else "all")) if layer else s
        if args.chain == "turns":
            s = TurnScorer(s, hop=H)
        elif args.chain == "lookahead":
            s = GatedScorer(s, LookaheadGate())
        return JitterScorer(GatedScorer(s) if args.gate else s, rate, "mulaw", depth)

    under = {"default": ", a plain SpeechGate under the front" if args.gate else "", "turns": ", a TurnScorer (pushes of one hop) under the front",
             "lookahead": ", a GatedScorer(LookaheadGate()) under the front"}[args.chain]

    names = ["plain", "provenance"]
    fronts = {"plain": chain(False), "provenance": chain(True)}
    planning = dict.fromkeys(names, 0.0)
    spans = [0, 0]  # the spans ops planned and their rows, over all passes
    for name, front in fronts.items():  # the planner's share of the host time: a timer around _plan
        def timed_plan(*a, _inner=front._plan, _name=name, **kw):
            begin = time.perf_counter()
            plan = _inner(*a, **kw)
            planning[_name] += time.perf_counter() - begin
            for op in plan.ops:
                if op[0] == "spans":
                    spans[0] += 1
                    spans[1] += len(op[1])
            return plan
        front._plan = timed_plan
    timed = {n: ([], [], []) for n in names}

    def run(name, t0, n):
        front = fronts[name]
        calls = [tick_args(t) for t in range(t0, t0 + n)]
        torch.cuda.synchronize()
        planning[name] = 0.0
        t_host, start = 0.0, time.perf_counter()
        for i, c in enumerate(calls):
            a = time.perf_counter()
            front.feed(*c, score=False)
            if ((t0 + i + 1) * pk) // hop_in > ((t0 + i) * pk) // hop_in:  # a hop's worth of audio has gone by: score
                front.drain()
            t_host += time.perf_counter() - a
        torch.cuda.synchronize()
        return time.perf_counter() - start, t_host, planning[name]

    for rep in range(-1, 1 + args.reps):
        for name in names[rep % 2:] + names[:rep % 2]:
            if rep < 0:
                run(name, 0, warm_ticks)
                continue
            dt, th, tp = run(name, warm_ticks + rep * ticks, ticks)
            if rep > 0:
                for lst, v in zip(timed[name], (dt, th, tp)):
                    lst.append(v / args.hops)
    report = [f"provenance_bench: build {lib().afx_build_id().decode()}; {torch.cuda.get_device_properties(0).name}; {S} streams, {rate} Hz "
              f"mulaw, {args.packet_ms}-ms packets, depth {args.depth_ms} ms, loss {args.loss:.3f}, reordered {args.reorder:.3f}; a summing "
              f"stand-in for the model, window {W}, hop {H}{under}; {args.hops} hops "
              f"({ticks} ticks) per pass, the median of {args.reps} timed passes per chain (alternating) after a warm-up pass"]
    med = {}
    for name in names:
        wall, host, plan = (sorted(v) for v in timed[name])
        med[name] = wall[len(wall) // 2], host[len(host) // 2], plan[len(plan) // 2]
        report.append(f"  {name:10s} {med[name][0] * 1e3:8.2f} ms per 250 ms of audio (min {wall[0] * 1e3:.2f}, max {wall[-1] * 1e3:.2f}; spread "
                      f"{(wall[-1] - wall[0]) / med[name][0] * 100:.1f} % of the median); host time inside feed / drain calls "
                      f"{med[name][1] * 1e3:.2f} ms, of it in the planner {med[name][2] * 1e3:.2f} ms (min {plan[0] * 1e3:.2f}, max {plan[-1] * 1e3:.2f})")
    st = fronts["provenance"].stats()
    layer = fronts["provenance"].scorer.scorer if args.gate or args.chain != "default" else fronts["provenance"].scorer
    ps = layer.stats()
    report.append(f"  provenance / plain {med['provenance'][0] / med['plain'][0]:.3f}x wall, planner +{(med['provenance'][2] - med['plain'][2]) * 1e3:.2f} ms "
                  f"per 250 ms of audio; all passes planned {spans[0]} spans ops with {spans[1]} rows")
    report.append(f"  over all streams: {int(st['concealed'].sum())} concealed input samples; the layer saw {int(ps['hops'].sum())} hops, "
                  f"{int(ps['synthetic'].sum())} synthetic 16 kHz samples, withheld {int(ps['withheld'].sum())} scores")
    if args.chain == "default":
        record(report)
    else:
        record(report, "provenance_turns.txt", HEADER_TURNS)


if __name__ == "__main__":
    main()

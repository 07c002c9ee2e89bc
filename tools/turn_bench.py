"""What scoring per talk spurt costs beside the speech gate, on the same build: S live streams of seeded synthetic talk-spurt
audio (tools/gate_bench.py's ``talk_spurts``) pushed hop by hop (250 ms) two ways, over the same stand-in for a model (the
sum of the window: the layers are measured, not a model):

  turns   afx.turns.TurnScorer around SlidingWindowScorer(sum, S, 64000, 64000): per push the gate's launch, afx_k_turn, the
          read-back of ``done``, and -- where a row closed a turn -- afx_k_turn_collect and one inner push of whole clips;
  gated   afx.vad.GatedScorer around SlidingWindowScorer(sum, S, 64000, 4000): the gate's launch, the read-back of ``kept``,
          one pop and one inner push of hops.

    python tools/turn_bench.py [--streams 2048] [--activity 0.4] [--hops 16] [--reps 3]

With --offline the tool measures the offline form instead (see ``offline`` below):

    python tools/turn_bench.py --offline [--recordings 16] [--seconds 120] [--reps 3]

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


def offline(args):
    """``afx.turns.score_turns`` over --recordings seeded synthetic recordings (``talk_spurts``, 0.5 to 1.5 times --seconds
    each, whole hops), scored with the student (fp16, 6 layers), against the way a caller had before it: per recording a
    one-slot ``TurnScorer`` pushed hop by hop (250 ms), then flushed.  Both run in this process, alternating pass by pass,
    and must give the same bits.  Times are wall clock around a pass that ends in a device synchronise, per hour of audio,
    the median of --reps passes after a warm-up pass; the split of the offline form is event-timed at the stage marks of
    ``score_turns`` (gate: the gate's offline launch and its kept-audio copy; scan: packing the masks, afx_k_turn_scan and
    the read-back of the count; clips: afx_k_turn_clips; forward: the engine).  On an MI355X the report is written to
    profiles/turn_offline.txt, stamped with afx_build_id().  Nothing asserts a time."""
    from afx import engine, synth, turns
    torch.cuda.set_device(0)
    sd = synth.model_state_dict("ConformerModel", n_layers=6)
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(sd)
    g = np.random.default_rng(11)
    hops = [max(1, int(args.seconds * 4 * (0.5 + i / max(args.recordings - 1, 1)))) for i in range(args.recordings)]
    recs = [torch.from_numpy(talk_spurts(n * H, args.activity, g)).cuda() for n in hops]
    hours = sum(hops) * H / 16000 / 3600
    gate, policy = SpeechGate(), TurnPolicy()
    ts = TurnScorer(SlidingWindowScorer(eng, 1, W, W, state_dict=sd), gate, policy, hop=H)

    def by_score_turns():
        marks = []

        def stage(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((name, e))

        turns._stage = stage
        try:
            torch.cuda.synchronize()
            begin = time.perf_counter()
            res = turns.score_turns(eng, recs, gate, policy, window=W)
            torch.cuda.synchronize()
            dt = time.perf_counter() - begin
        finally:
            turns._stage = None
        split = dict.fromkeys(("gate", "scan", "clips", "forward"), 0.0)
        for (name, a), (_, b) in zip(marks, marks[1:]):
            split[name] += a.elapsed_time(b) * 1e-3
        return [t.scores for t in res], dt, split, res

    def by_stream():
        torch.cuda.synchronize()
        begin = time.perf_counter()
        out = []
        for x in recs:
            ts.reset([0])
            got = [ts.push(x[None, t * H:(t + 1) * H]) for t in range(x.numel() // H)] + [ts.flush()]
            out.append(torch.cat(got))
        torch.cuda.synchronize()
        dt = time.perf_counter() - begin
        return [o[emitted(o)].cpu() for o in out], dt

    times = {"score_turns": [], "stream": []}
    splits = []
    for rep in range(1 + args.reps):  # (the first pass warms both up)
        a, dt_a, split, res = by_score_turns()
        b, dt_b = by_stream()
        assert len(a) == len(b) and all(u.shape == v.shape and torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b)), \
            "score_turns and the streamed, flushed TurnScorer differ"
        if rep:
            times["score_turns"].append(dt_a), times["stream"].append(dt_b), splits.append(split)
    n_turns = sum(len(t) for t in res)
    report = [f"turn_bench --offline: build {lib().afx_build_id().decode()}; {len(recs)} recordings of synthetic talk spurts "
              f"({args.activity:.0%} talk), {hours * 60:.1f} min of audio in all ({min(hops) // 4} to {max(hops) // 4} s each); student fp16 "
              f"(6 layers), window {W}, gate {gate.params()}, min_frames {policy.min_frames}; {n_turns} scored turns "
              f"({sum(int(t.cut.sum()) for t in res)} cut, {sum(int(t.at_end.sum()) for t in res)} closed by the end), "
              f"{sum(t.totals['short'] for t in res)} dropped as short; the median of {args.reps} timed passes per path (alternating) "
              "after a warm-up pass; the scores of the two paths are the same bits"]
    med = {}
    for name, tt in times.items():
        tt = sorted(tt)
        med[name] = tt[len(tt) // 2]
        report.append(f"  {name:11s} {med[name] / hours:8.2f} s per hour of audio (min {tt[0] / hours:.2f}, max {tt[-1] / hours:.2f}); "
                      f"{med[name] * 1e3:.1f} ms a pass")
    split = splits[sorted(range(len(splits)), key=lambda i: times["score_turns"][i])[len(splits) // 2]]
    total = sum(split.values())
    report.append("  score_turns on the device (events, the median pass): " + ", ".join(
        f"{k} {v * 1e3:.2f} ms ({v / total:.1%})" for k, v in split.items()) + f"; {total * 1e3:.2f} ms of {med['score_turns'] * 1e3:.1f} ms")
    report.append(f"  stream / score_turns {med['stream'] / med['score_turns']:.1f}x; the scan is {split['scan'] / total:.1%} of the device time")
    print("\n".join(report), flush=True)
    if torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"):
        path = os.path.join(ROOT, "profiles", "turn_offline.txt")
        with open(path, "w") as f:
            f.write(f"tools/turn_bench.py {' '.join(sys.argv[1:])} on one MI355X: afx.turns.score_turns against a one-slot TurnScorer "
                    "pushed hop by hop and flushed, alternating pass by pass in one process, on the same audio.  One run on one "
                    "machine; the kernels were not profiled separately.\n\n" + "\n".join(report) + "\n")
        print(f"  written to {path}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--offline", action="store_true", help="measure afx.turns.score_turns against a streamed one-slot TurnScorer")
    ap.add_argument("--recordings", type=int, default=16, help="--offline: recordings")
    ap.add_argument("--seconds", type=float, default=120.0, help="--offline: the middle recording length")
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=16, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.offline:
        return offline(args)
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

"""The speech gate measured against the bare scorer on the same build: S live streams of seeded synthetic talk-spurt audio
(alternating exponential talk / silence spells, --activity of the time in talk on average; talk = a 180 Hz tone under a 4 Hz
tremolo at -14 dBFS, silence = noise at -54 dBFS), the student scores them in KV-cached mode.  Two ways, timed per 250-ms hop:

  gated     afx.vad.GatedScorer around the KV-cached scorer: every hop one ``push`` of all S slots (one afx_k_gate launch,
            one read-back of S int32, one pop and one inner push over the slots that completed a hop of kept audio);
  bare      the KV-cached scorer alone pushed the same hops lock-stepped: every slot scored every hop, what the parent of
            the gate could do;
  lookahead (with --pre N) the gated path with ``LookaheadGate(pre=N)``: ``afx_k_gate_la`` in place of ``afx_k_gate`` (one
            more read and write of N frames per slot and the source indices), timed in the same process.  It keeps N more
            frames per onset, so it scores slightly more hops: read its time beside its own share of slot-pushes.
  tone      (with --tones) the gated path with ``ToneGate()``: ``afx_k_gate_tone`` in place of ``afx_k_gate`` (a Goertzel bank
            of 16 frequencies per frame), timed in the same process on the same audio.  With --tones every bank stream
            begins with 2 s of ringback (440 + 480 Hz) and carries a string of five DTMF digits inside its first talk spell
            after it; the slots meet them wherever their offsets put them.  The tone gate drops those frames, so it
            scores fewer hops: read its time beside its own share of slot-pushes and the tone frames it rejected.  On an
            MI355X the report is also written to profiles/gate_tone.txt.

    python tools/gate_bench.py [--streams 2048] [--activity 0.4] [--hops 8] [--reps 3] [--pre 5] [--tones]
    rocprofv3 --kernel-trace --stats ... -- python tools/gate_bench.py --profile   (gated path only, 4 hops: kernel times)

The two paths score different audio by design (the gate drops frames), so their scores are not compared; the gate's own
contract is pinned by tests/test_gpu_vad.py.  Printed with the times: the share of slot-pushes that emitted a score and the
share of samples kept.  Times are the median over --reps timed passes after one warm-up pass (min and max given), wall
clock around a pass that ends in a device synchronise.  The streams come from a bank of --bank distinct seeded streams, each
slot reading one of them from its own whole-hop offset.  Stamped with afx_build_id()."""
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
from afx.streaming import KVCachedScorer  # noqa: E402
from afx.vad import GatedScorer, LookaheadGate, SpeechGate, ToneGate, emitted  # noqa: E402

W, H = 64000, 4000


DTMF = [(697, 1209), (770, 1336), (852, 1477), (941, 1633), (697, 1336)]  # the digits 1, 5, 9, D, 2


def talk_spurts(n, activity, g, talk_s=1.0, tones=False):
    """n samples at 16 kHz: alternating talk / silence spells with exponential lengths (mean talk_s seconds of talk).
    tones: the stream begins with 2 s of ringback (440 + 480 Hz at -19 dBFS each) in place of its first spells, and the first
    talk spell after it lasts at least 1 s and carries five DTMF digits (80 ms on, 80 ms off, -15 dBFS per tone)."""
    x = (0.002 * g.standard_normal(n)).astype(np.float32)
    t = np.arange(n) / 16000
    voice = (0.2 * np.sin(2 * np.pi * 180 * t) * (1 + 0.5 * np.sin(2 * np.pi * 4 * t))).astype(np.float32)
    quiet_s = talk_s * (1 - activity) / activity
    pos, talking, digits = 0, g.random() < activity, tones
    if tones:
        x[:32000] += (0.15 * (np.sin(2 * np.pi * 440 * t[:32000]) + np.sin(2 * np.pi * 480 * t[:32000]))).astype(np.float32)
        pos = 32000
    while pos < n:
        m = int(16000 * g.exponential(talk_s if talking else quiet_s)) + 160
        if talking:
            if digits:
                m, digits = max(m, 16000), False
                for d, (lo, hi) in enumerate(DTMF):
                    a = pos + 1600 + d * 2560
                    if a + 1280 <= n:
                        x[a:a + 1280] += (0.25 * (np.sin(2 * np.pi * lo * t[:1280]) + np.sin(2 * np.pi * hi * t[:1280]))).astype(np.float32) \
                            - voice[a:a + 1280]
            x[pos:pos + m] += voice[pos:pos + m]
        pos, talking = pos + m, not talking
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--activity", type=float, default=0.4)
    ap.add_argument("--bank", type=int, default=64, help="distinct synthetic streams the slots draw from")
    ap.add_argument("--hops", type=int, default=8, help="hops per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pre", type=int, default=0, help="also time the look-ahead gate with this many frames of pre-roll")
    ap.add_argument("--tones", action="store_true", help="ringback and DTMF in the bank; also time the tone gate (ToneGate())")
    ap.add_argument("--profile", action="store_true", help="the gated path only, a short pass (for a rocprofv3 run)")
    args = ap.parse_args()
    S = args.streams
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
    bank = torch.from_numpy(np.stack([talk_spurts(bank_hops * H, args.activity, g, tones=args.tones) for _ in range(args.bank)])).cuda()
    bank = bank.reshape(args.bank, bank_hops, H)
    which = torch.from_numpy(g.integers(0, args.bank, S)).cuda()
    start = torch.from_numpy(g.integers(0, bank_hops, S)).cuda()

    def hop(t):
        return bank[which, (start + t) % bank_hops].contiguous()

    report = []

    def say(line):
        report.append(line)
        print(line, flush=True)

    say(f"gate_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams of synthetic "
        f"talk spurts ({args.activity:.0%} talk{', every bank stream begins with 2 s of ringback and has five DTMF digits in its first talk spell' if args.tones else ''}), "
        f"gate {SpeechGate().params()}; {hops} hops per pass, {args.reps} timed passes "
        f"per path after a warm-up pass of {warm} hops")
    if args.tones:
        tp = ToneGate().params()
        say(f"  tone gate: {len(tp['freqs'])} frequencies, frac {tp['frac']}, confirm {tp['confirm']}, hold {tp['hold']}")
    results = {}
    look = (["lookahead"] if args.pre else []) + (["tone"] if args.tones else [])
    for name in (["gated"] + look if args.profile else ["gated"] + look + ["bare"]):
        inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
        front = {"gated": GatedScorer, "lookahead": lambda sc: GatedScorer(sc, LookaheadGate(pre=args.pre)),
                 "tone": lambda sc: GatedScorer(sc, ToneGate()), "bare": lambda sc: sc}[name](inner)
        pushes = scores = 0

        def run(t0, n):
            nonlocal pushes, scores
            chunks = [hop(t) for t in range(t0, t0 + n)]
            outs = []
            torch.cuda.synchronize()
            begin = time.perf_counter()
            for c in chunks:
                outs.append(front.push(c))
            torch.cuda.synchronize()
            dt = time.perf_counter() - begin
            if name != "bare":
                pushes += n * S
                scores += int(sum(emitted(o).sum() for o in outs))
            return dt

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
        if name != "bare":
            kept = float(front.samples_kept.sum()) / float(front.samples_seen.sum())
            extra = f"; {scores / pushes:.1%} of {pushes} slot-pushes emitted a score, {kept:.1%} of the samples kept"
            if name == "tone":
                frames = int(front.samples_seen.sum()) // front.gate.frame
                extra += f", {int(front.tone_frames.sum())} of {frames} frames rejected as tone"
        say(f"  {name:9s} {med * 1e3:8.2f} ms per hop (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); RTF {med / 0.25:.3f}{extra}")
        del front, inner
        torch.cuda.empty_cache()
    if not args.profile:
        (mg, tg), (mb, tb) = results["gated"], results["bare"]
        say(f"  gated / bare {mg / mb:.2f}x (spread of bare: {(tb[-1] - tb[0]) / mb * 100:.1f} % of its median, of gated: "
            f"{(tg[-1] - tg[0]) / mg * 100:.1f} %)")
        if args.pre:
            ml, tl = results["lookahead"]
            say(f"  lookahead (pre {args.pre}) / gated {ml / mg:.2f}x (spread of lookahead: {(tl[-1] - tl[0]) / ml * 100:.1f} % of its "
                f"median)")
        if args.tones:
            mt, tt = results["tone"]
            say(f"  tone / gated {mt / mg:.2f}x (spread of tone: {(tt[-1] - tt[0]) / mt * 100:.1f} % of its median)")
            if torch.cuda.get_device_properties(0).gcnArchName.startswith("gfx950"):
                path = os.path.join(ROOT, "profiles", "gate_tone.txt")
                with open(path, "w") as f:
                    f.write(f"tools/gate_bench.py {' '.join(sys.argv[1:])} on one MI355X: the plain gate, the tone "
                            f"gate and the bare scorer, one after the other in the same process, on the same audio.  One run on one "
                            f"machine; the kernels were not profiled separately.\n\n" + "\n".join(report) + "\n")
                print(f"  written to {path}", flush=True)


if __name__ == "__main__":
    main()

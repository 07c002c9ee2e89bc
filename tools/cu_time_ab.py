"""A/B of the CU-time dispatch objective in the two-lanes form (whole forwards of consecutive batches on alternating streams:
Engine.forward_lanes), one process, interleaved.  For student (B = 64) and teacher (B = 16), 4-s clips, each precision given:
every decision the objective may take over ("dispatch_cu_mask" bits: 1 height of the 256-wide GEMM tile, 2 waves per workgroup
of the fused Conformer chains, 4 height of the row-complete conv tile, 8 the two row splits) alone, all together, and off
(mask 0 = the makespan shapes on both lanes), ROUNDS rounds of NB batches each, logits checked against the one-stream forward.
A switch counts as a win only if its median beats EVERY off run.
    python tools/cu_time_ab.py [fp16 fp16x3 ...] [--rounds 7] [--out FILE] [--masks 0,1,2,4,8,3,11,15]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx import engine, synth  # noqa: E402
from afx._lib import LIB_PATH, check, lib  # noqa: E402

NAMES = {0: "off (makespan shapes)", 1: "gemm 256-wide height", 2: "chain 8 waves", 4: "conv tile height", 8: "row splits", 3: "1 + 2 (shipped)",
         11: "1 + 2 + 8", 15: "all four"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dtypes", nargs="*", default=["fp16"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--masks", default="0,1,2,4,8,3,11,15")
    ap.add_argument("--models", default="student,teacher")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    masks = [int(m) for m in args.masks.split(",")]
    l = lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    stamp = os.path.join(os.path.dirname(LIB_PATH), "build_stamp.json")
    say(f"# build {json.load(open(stamp)) if os.path.exists(stamp) else l.afx_build_id().decode()}  {torch.cuda.get_device_name(0)}")
    say(f"# two-lanes form, {args.rounds} rounds x {args.batches} batches per configuration, interleaved; ms per batch")
    models = {"student": ("conformer", "ConformerModel", 6, 64), "teacher": ("xlsr_aasist", "XLSR_AASIST", 24, 16)}
    for dtype in args.dtypes:
        for name in args.models.split(","):
            arch, oname, nl, B = models[name]
            eng = engine.Engine(arch, n_layers=nl, dtype=dtype)
            eng.load_state_dict(synth.model_state_dict(oname, n_layers=nl, **({"head_scale": 1.5} if arch == "xlsr_aasist" else {})))
            L, NB = 64000, args.batches
            waves = [synth.waveforms(B, L, batch_idx=40 + i).cuda() for i in range(4)]
            want = [eng.forward(w).clone() for w in waves]

            def timed(fn, join):
                for i in range(4):
                    fn(i)
                join()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs = [fn(i) for i in range(NB)]
                join()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / NB, all(torch.equal(o, want[i % 4]) for i, o in enumerate(outs))

            one = [timed(lambda i: eng.forward(waves[i % 4]), lambda: None)[0] for _ in range(3)]
            say(f"{name} {dtype} B {B}: one stream {min(one):.3f} .. {max(one):.3f}")
            times = {m: [] for m in masks}
            same = True
            for _ in range(args.rounds):
                for m in masks:
                    check(l.afx_debug_set(b"dispatch_cu_mask", m))
                    ms, ok = timed(lambda i: eng.forward_lanes(waves[i % 4]), eng.join)
                    times[m].append(ms)
                    same = same and ok
            check(l.afx_debug_set(b"dispatch_cu_mask", 3))  # (the shipped default)
            off = times.get(0, [])
            for m in masks:
                t = times[m]
                verdict = ""
                if m and off:
                    verdict = "  WIN (median below every off run)" if statistics.median(t) < min(off) else "  no win"
                say(f"{name} {dtype} B {B}: mask {m:2d} {NAMES.get(m, 'combination'):24s} median {statistics.median(t):.3f}  min {min(t):.3f}  max {max(t):.3f}"
                    f"  runs {' '.join(f'{x:.3f}' for x in t)}{verdict}")
            say(f"{name} {dtype} B {B}: every batch of every run equals the one-stream logits bit for bit: {same}")
            del eng
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

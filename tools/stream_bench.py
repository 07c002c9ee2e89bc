"""Real-time factor of the streaming mode (BASELINE config 5): S concurrent streams per GPU, 250 ms hops, every hop
emits each stream's score of its last 4 s.  Two scorers with bit-identical outputs (afx/streaming.py), reference-exact:
  sliding      the whole model on the window every hop (round 1);
  incremental  conv layers 0-5 cached per absolute frame, only the new 800/400/.../25 frames computed per hop;
and the labelled NON-reference mode config 5 names (a different, block-causal function: oracle/streaming.py):
  kv-cached    cached keys / values of the last 16 chunks, only the chunk's 12-13 new frames through the trunk.

    python tools/stream_bench.py [--workload conformer_student|xlsr_aasist] [--streams 1 64 512 2048]
    python tools/stream_bench.py --staggered [--session-hops 120] --modes incremental ...

--staggered measures every mode twice: lockstep (all streams started together, as above) and with per-slot sessions --
before every hop, warm-up included, each slot restarts (``scorer.reset``) with probability 1 / session-hops, seeded, so
that slots warming up and slots in the steady state share the ticks as they do on a server scoring live calls (the warm-up
runs session-hops more ticks, so the timed hops see the stationary mix: ~1 - (1 - 1/120)^16 = 12.5 % of the slots still
younger than the window at the default).
--active-frac F [F ...] measures non-paced streams (``push(chunk, slots)``): after the warm-up (every slot pushed until its
window is full), before each timed hop each slot has audio with probability F, seeded, and only those slots are pushed.
Reported per F: ms per hop, the RTF of the active streams (hop time / hop duration) and scores/s (active slots per second).
    python tools/stream_bench.py --active-frac 0.25 0.5 1.0 --streams 2048 ...
--migrate measures moving sessions (``export_slots`` / ``import_slots``) instead, per mode (kv-cached, incremental): export
and import of 1 / 64 / 512 steady sessions (--streams) device to device and through pinned host memory (ms, GB/s of state,
bytes per session), then the hop time of a --migrate-hop-streams scorer that imports 64 sessions between every two hops
against one that does not.
    python tools/stream_bench.py --migrate [--workload xlsr_aasist] [--streams 1 64 512] ...
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/stream_bench.py --gpus N ...
--input-rate R feeds every scorer audio at R Hz through ``ResamplingScorer`` (hops of 4000 * R / 16000 samples resampled to
16 kHz on the GPU with per-slot filter history); the hop time then includes the resampling.
    python tools/stream_bench.py --input-rate 48000 --modes kv-cached --streams 2048 ...

With --gpus N every rank pins its own S streams to its GPU (state lives there; nothing is exchanged on the data path);
the hop time reported is the max over ranks (one RCCL all-reduce of a scalar, outside the timed hops), the stream
count the sum."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]
from afx import engine, synth  # noqa: E402
from afx.streaming import IncrementalScorer, KVCachedScorer, ResamplingScorer, SlidingWindowScorer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--workload", default="conformer_student", choices=["conformer_student", "xlsr_aasist"])
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 64, 512, 2048])
    ap.add_argument("--hops", type=int, default=10)
    ap.add_argument("--modes", nargs="*", default=["sliding", "incremental", "kv-cached"])
    ap.add_argument("--staggered", action="store_true", help="also time per-slot sessions restarting at random ticks")
    ap.add_argument("--session-hops", type=int, default=120, help="--staggered: mean session length in hops (120 = 30 s)")
    ap.add_argument("--active-frac", type=float, nargs="*", default=[],
                    help="also time non-paced streams: each slot has audio on a tick with this probability (seeded)")
    ap.add_argument("--migrate", action="store_true", help="time export_slots / import_slots instead of the hop (see above)")
    ap.add_argument("--migrate-hop-streams", type=int, default=2048, help="--migrate: streams of the scorer timed while it imports")
    ap.add_argument("--input-rate", type=int, default=16000, help="audio rate fed to the scorers (resampled to 16 kHz on the GPU)")
    args = ap.parse_args()
    rank, local, world = (int(os.environ.get(k, d)) for k, d in (("RANK", 0), ("LOCAL_RANK", 0), ("WORLD_SIZE", 1)))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    arch, oname, nl = ("conformer", "ConformerModel", 6) if args.workload == "conformer_student" else ("xlsr_aasist", "XLSR_AASIST", 24)
    sd = synth.model_state_dict(oname, n_layers=nl)
    eng = engine.Engine(arch, n_layers=nl, dtype="fp16")
    eng.load_state_dict(sd)
    W, H = 64000, 4000
    H_in = H * args.input_rate // 16000
    if args.migrate:
        return migrate(args, eng, sd, W, H)
    for S in args.streams:
        line = f"{args.workload}, {world} GPU(s) x {S} streams" + (f" at {args.input_rate} Hz" if args.input_rate != 16000 else "") + ":"
        for name in args.modes:
            for staggered, frac in [(False, None)] + ([(True, None)] if args.staggered else []) + [(False, f) for f in args.active_frac]:
                label = name + (" staggered" if staggered else "") + (f" active {frac:.2f}" if frac is not None else "")
                try:
                    sc = {"sliding": lambda: SlidingWindowScorer(eng, S, window=W, hop=H), "incremental": lambda: IncrementalScorer(eng, sd, S, window=W, hop=H),
                          "kv-cached": lambda: KVCachedScorer(eng, sd, S, window=W, hop=H)}[name]()
                    if args.input_rate != 16000:
                        sc = ResamplingScorer(sc, args.input_rate)
                    if staggered:
                        sc.reset([0])  # (a no-op on a fresh scorer; a mode without sessions refuses it here)
                except Exception as exc:  # (the K / V rings of 24 layers are 38 MB per stream: 2 048 streams of the teacher do not fit beside the rest)
                    line += f"  {label} n/a ({str(exc)[:60]})"
                    continue
                chunk = (0.1 * torch.randn(S, H_in, generator=torch.Generator().manual_seed(rank))).cuda()
                gen = torch.Generator().manual_seed(1000 + rank)

                n_active = []

                def tick(warm=False):
                    if staggered:
                        sc.reset(torch.rand(S, generator=gen) < 1.0 / args.session_hops)
                    if frac is None:
                        sc.push(chunk)
                    elif warm:
                        sc.push(chunk, slots=range(S))
                    else:
                        on = (torch.rand(S, generator=gen) < frac).nonzero().flatten()
                        n_active.append(on.numel())
                        sc.push(chunk[on.cuda()], slots=on)
                for _ in range(W // H + 2 + (args.session_hops if staggered else 0)):  # fill the window, reach the steady state
                    tick(warm=True)
                torch.cuda.synchronize()
                if dist:
                    dist.barrier()
                t0 = time.perf_counter()
                for _ in range(args.hops):
                    tick()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / args.hops
                if dist:
                    t = torch.tensor([dt], dtype=torch.float64, device="cuda")
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    dt = t.item()
                per_hop = world * (sum(n_active) / len(n_active) if n_active else S)  # scores per hop
                line += f"  {label} {dt * 1e3:8.2f} ms/hop RTF {dt / 0.25:6.3f} ({per_hop / dt:8.0f} scores/s)"
                if n_active:
                    line += f" [{per_hop:.0f} active]"
                del sc
        if rank == 0:
            print(line, flush=True)
    if dist:
        dist.destroy_process_group()


def _state_bytes(st):
    return sum(t.numel() * t.element_size() for t in st.tensors.values())


def _timed(fn, reps=3):
    """Median wall time of fn() (device-synchronised before and after) over reps calls -> (seconds, last result)."""
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sorted(times)[len(times) // 2], out


def migrate(args, eng, sd, W, H):
    """Export / import times of steady sessions, device to device and through pinned host memory, and the hop time of a
    scorer importing 64 sessions between hops."""
    stamp = os.path.join(ROOT, "real-time-deepfake-speech-detection_amd", "lib", "build_stamp.json")
    if os.path.exists(stamp):
        print("# build", open(stamp).read().strip(), flush=True)
    make = {"incremental": lambda S: IncrementalScorer(eng, sd, S, window=W, hop=H), "kv-cached": lambda S: KVCachedScorer(eng, sd, S, window=W, hop=H)}
    modes = [m for m in args.modes if m in make]
    n_max = max(args.streams)
    for name in modes:
        gen = torch.Generator().manual_seed(7)
        try:
            src, dst = make[name](n_max), make[name](n_max)
            for sc in (src, dst):  # steady sessions: the window full, the KV ring wrapped
                for _ in range(W // H + 2):
                    sc.push((0.1 * torch.randn(n_max, H, generator=gen)).cuda())
                sc.state_meta()  # (the weights fingerprint: once per scorer, outside the timing)
        except RuntimeError as exc:
            print(f"{args.workload} {name} {n_max} sessions: n/a ({str(exc)[:80]})", flush=True)
            src = dst = None
            torch.cuda.empty_cache()
            continue
        for n in args.streams:
            idx = list(range(n))
            te, st = _timed(lambda: src.export_slots(idx))
            ti, _ = _timed(lambda: dst.import_slots(idx, st))
            nb = _state_bytes(st)
            line = f"{args.workload} {name:11s} {n:4d} sessions, {nb / n / 1e6:7.2f} MB each:  device export {te * 1e3:8.2f} ms ({nb / te / 1e9:6.1f} GB/s)  import {ti * 1e3:8.2f} ms ({nb / ti / 1e9:6.1f} GB/s)"
            try:
                host = st.to("cpu", pin_memory=True)  # (the pinned buffers once, outside the timing)

                def to_host():
                    st2 = src.export_slots(idx)
                    for k, t in st2.tensors.items():
                        host.tensors[k].copy_(t, non_blocking=True)
                    return host
                th, _ = _timed(to_host)
                tr, _ = _timed(lambda: dst.import_slots(idx, host))
                line += f"  | pinned host: export + D2H {th * 1e3:8.2f} ms ({nb / th / 1e9:6.1f} GB/s)  H2D + import {tr * 1e3:8.2f} ms ({nb / tr / 1e9:6.1f} GB/s)"
                del host
            except RuntimeError as exc:
                line += f"  | pinned host n/a ({str(exc)[:60]})"
            print(line, flush=True)
            del st
        del src, dst
        torch.cuda.empty_cache()
    # hop time of a large scorer that takes 64 sessions between every two hops, against one that does not
    S, n_imp = args.migrate_hop_streams, 64
    for name in modes if S >= 4 * n_imp else []:
        try:
            sc = make[name](S)
        except Exception as exc:
            print(f"{args.workload} {name} {S} streams: n/a ({str(exc)[:60]})", flush=True)
            continue
        chunk = (0.1 * torch.randn(S, H, generator=torch.Generator().manual_seed(3))).cuda()
        for _ in range(W // H + 2):
            sc.push(chunk)
        st = sc.export_slots(list(range(S - n_imp, S)))
        sc.import_slots(list(range(n_imp)), st)  # (both timings then run the per-slot path an import puts the scorer on)
        sc.push(chunk)
        res = {}
        for imp in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for h in range(args.hops):
                if imp:
                    sc.import_slots(list(range(n_imp * (h % 4), n_imp * (h % 4 + 1))), st)
                sc.push(chunk)
            torch.cuda.synchronize()
            res[imp] = (time.perf_counter() - t0) / args.hops
        print(f"{args.workload} {name} {S} streams: hop {res[False] * 1e3:.2f} ms; hop + import of {n_imp} sessions {res[True] * 1e3:.2f} ms "
              f"(+{(res[True] - res[False]) * 1e3:.2f} ms)", flush=True)
        del sc, st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""The jitter front measured against the packet front on the same build: S live calls send --packet-ms packets (per-stream
random phase against the 250-ms hop), the student scores them in KV-cached mode.  Two ways, timed per 250 ms of audio:

  jitter    afx.jitter.JitterScorer behind a lossy network: --loss of the packets never arrive, --reorder of them arrive one
            or two packets late (inside the --depth-ms playout depth, so they are on time); every tick one
            ``feed(packets, slots, timestamps, score=False)`` with whatever arrived (a slot 0 to 3 times), one ``drain()`` per hop;
  packets   afx.ingest.PacketScorer fed the same streams losslessly and in order, one packet per slot and tick: what the
            parent of the jitter front could do.
  --conceal {zero,repeat,pitch_sync}: the jitter path's concealment mode; --against MODE: a second jitter path in that mode on
            the same arrivals.  Every path is warmed up first and the timed passes alternate between the paths.

  --dtx     silence suppression instead: talk-spurt traffic (about 40 % activity; spurts and pauses of geometric length, mean
            1 s and 1.5 s), a CN mark (RFC 3389) at each spurt end and every 200 ms of silence, --loss of all datagrams lost, in
            order.  Three scorers of this build in one process, the same inner scorer and call pattern as above:
            every tick ``feed(..., score=False)`` with what arrived, then ``advance`` of all streams to the playout clock (a silent
            stream sends nothing to release it), one ``drain()`` per hop:
              dtx       a JitterScorer with comfort_noise: ``silence`` with the tick's marks before the ``feed``;
              filtered  the same traffic with the CN datagrams removed, a JitterScorer without comfort_noise: every pause is a
                        loss gap (what a caller could do before);
              plain     ordinary traffic (every stream talks all the time), a JitterScorer without comfort_noise, for scale.
            Whether ordinary traffic through a scorer without comfort_noise costs what it cost before is the default mode's
            "jitter" line of this tree against the parent commit's on the same box.
            --out FILE appends what was printed to FILE (profiles/jitter_dtx.txt).

    python tools/jitter_bench.py [--streams 2048] [--rate 8000] [--encoding mulaw] [--packet-ms 20] [--depth-ms 60]
                                 [--loss 0.02] [--reorder 0.1] [--hops 8] [--reps 3] [--conceal repeat] [--against MODE]
    rocprofv3 --kernel-trace --stats ... -- python tools/jitter_bench.py --profile   (jitter path only, 4 hops: kernel times)

The two paths score different audio where packets were lost (concealed samples instead of the sent ones), so their scores are
not compared; with --loss 0 the jitter path's scores must equal the packet path's delayed by the depth, which is checked
on the warm-up pass for the hops both have emitted.  Times are the median over --reps timed passes after one warm-up pass
(min and max given), wall clock around a pass that ends in a device synchronise; the host time spent inside feed / drain
calls (planning, packing, launching; launches are asynchronous) is listed beside it.  Stamped with afx_build_id()."""
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
from afx.ingest import ENCODINGS, PacketScorer  # noqa: E402
from afx.jitter import CONCEAL, ComfortNoise, JitterScorer  # noqa: E402
from afx.streaming import KVCachedScorer  # noqa: E402

W, H = 64000, 4000


def dtx(args, eng, sd):
    """The --dtx measurement (module docstring)."""
    S, rate, enc = args.streams, args.rate, args.encoding
    bps = {"pcm_f32le": 4, "pcm_s16le": 2}.get(enc, 1)
    pk = rate * args.packet_ms // 1000
    depth = rate * args.depth_ms // 1000
    hop_in = -(-H * rate // 16000)
    ticks = args.hops * hop_in // pk
    warm_ticks = (W // H + 2) * hop_in // pk
    n_ticks = warm_ticks + (1 + args.reps) * ticks
    g = np.random.default_rng(13)
    data = {"pcm_f32le": lambda n: (0.1 * g.standard_normal(n)).astype("<f4"), "pcm_s16le": lambda n: g.integers(-4000, 4000, n).astype("<i2")
            }.get(enc, lambda n: g.integers(0, 256, n).astype(np.uint8))
    audio = [data(n_ticks * pk) for _ in range(S)]
    origin = g.integers(0, 1 << 32, S)
    # the senders: talking[s, k]; a two-state chain with mean spurt 1 s and mean pause 1.5 s (40 % activity)
    p_stop, p_start = args.packet_ms / 1000.0, args.packet_ms / 1500.0
    talking = np.ones((S, n_ticks), dtype=bool)
    u = g.random((S, n_ticks))
    for k in range(1, n_ticks):
        talking[:, k] = np.where(talking[:, k - 1], u[:, k] >= p_stop, u[:, k] < p_start)
    run_len = np.zeros(S, dtype=np.int64)  # ticks of silence so far
    cn_at = np.zeros((S, n_ticks), dtype=bool)  # a CN at the spurt end and every 200 ms of silence
    every = max(1, 200 // args.packet_ms)
    for k in range(n_ticks):
        run_len = np.where(talking[:, k], 0, run_len + 1)
        cn_at[:, k] = ~talking[:, k] & ((run_len - 1) % every == 0)
    level = g.integers(30, 71, (S, n_ticks))
    lost = g.random((S, n_ticks)) < args.loss
    lost[:, 0] = False  # (the first packet sets the origin)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"jitter_bench --dtx: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams, {rate} Hz {enc}, "
        f"{args.packet_ms}-ms packets ({pk * bps} bytes), depth {args.depth_ms} ms, loss {args.loss:.3f}, in order; activity "
        f"{talking.mean():.3f}, {int(cn_at.sum())} CN datagrams; {args.hops} hops ({ticks} ticks) per pass, {args.reps} timed passes per "
        f"path after a warm-up pass")
    ts_of = lambda s, k: (int(origin[s]) + k * pk) % (1 << 32)
    results = {}
    for name in ("dtx", "filtered", "plain"):
        inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
        front = JitterScorer(inner, rate, enc, depth, comfort_noise=ComfortNoise(1) if name == "dtx" else None)
        calls = []
        for k in range(n_ticks):
            sent = ~lost[:, k] if name == "plain" else talking[:, k] & ~lost[:, k]
            ss = np.flatnonzero(sent).tolist()
            feed = ([audio[s][k * pk:(k + 1) * pk].tobytes() for s in ss], ss, np.array([ts_of(s, k) for s in ss], dtype=np.int64))
            ms = np.flatnonzero(cn_at[:, k] & ~lost[:, k]).tolist() if name == "dtx" else []
            calls.append((feed, (ms, np.array([ts_of(s, k) for s in ms], dtype=np.int64), level[ms, k].tolist()) if ms else None))

        def run(t0, n):
            torch.cuda.synchronize()
            t_host, start = 0.0, time.perf_counter()
            for t in range(t0, t0 + n):
                feed, marks = calls[t]
                a = time.perf_counter()
                if marks is not None:
                    front.silence(*marks)
                front.feed(*feed, score=False)
                front.advance(everyone, max(0, (t + 1) * pk - depth), score=False)  # the playout clock: a silent stream sends nothing
                if ((t + 1) * pk) // hop_in > (t * pk) // hop_in:  # a hop's worth of audio has gone by: score
                    front.drain()
                t_host += time.perf_counter() - a
            torch.cuda.synchronize()
            return time.perf_counter() - start, t_host

        everyone = list(range(S))
        run(0, warm_ticks)
        times, host = [], []
        for r in range(1 + args.reps):
            dt, th = run(warm_ticks + r * ticks, ticks)
            if r > 0:
                times.append(dt / args.hops)
                host.append(th / args.hops)
        times.sort()
        host.sort()
        med = results[name] = times[len(times) // 2]
        st = {k: int(v.sum()) for k, v in front.stats().items()}
        say(f"  {name:8s} {med * 1e3:8.2f} ms per 250 ms of audio (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); host time inside "
            f"silence / feed / drain calls {host[len(host) // 2] * 1e3:.2f} ms; RTF {med / 0.25:.3f}; stats over all streams {st}")
        del front, inner
        torch.cuda.empty_cache()
    say(f"  dtx / filtered {results['dtx'] / results['filtered']:.2f}x, dtx / plain {results['dtx'] / results['plain']:.2f}x")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--encoding", default="mulaw", choices=ENCODINGS)
    ap.add_argument("--packet-ms", type=int, default=20)
    ap.add_argument("--depth-ms", type=int, default=60)
    ap.add_argument("--loss", type=float, default=0.02)
    ap.add_argument("--reorder", type=float, default=0.1, help="fraction of packets that arrive one or two packets late")
    ap.add_argument("--hops", type=int, default=8, help="hops of audio per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--conceal", default="repeat", choices=CONCEAL, help="the jitter path's concealment mode")
    ap.add_argument("--against", default=None, choices=CONCEAL, help="a second jitter path in this mode, its passes alternating with the first's")
    ap.add_argument("--profile", action="store_true", help="the jitter path only, a short pass (for a rocprofv3 run)")
    ap.add_argument("--dtx", action="store_true", help="silence-suppression traffic through a comfort-noise scorer (see above)")
    ap.add_argument("--out", default=None, help="--dtx: append the printed lines to this file")
    args = ap.parse_args()
    S, rate, enc = args.streams, args.rate, args.encoding
    bps = {"pcm_f32le": 4, "pcm_s16le": 2}.get(enc, 1)
    pk = rate * args.packet_ms // 1000
    depth = rate * args.depth_ms // 1000
    late_max = min(2, depth // pk)  # packets a reordered packet may fall behind and still be on time
    hop_in = -(-H * rate // 16000)
    torch.cuda.set_device(0)
    sd = synth.model_state_dict("ConformerModel", n_layers=6)
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(sd)
    if args.dtx:
        return dtx(args, eng, sd)
    passes = 1 if args.profile else 1 + args.reps
    hops = 4 if args.profile else args.hops
    ticks = hops * hop_in // pk
    warm_ticks = (W // H + 2) * hop_in // pk
    n_ticks = warm_ticks + passes * ticks
    g = np.random.default_rng(11)
    phase = g.integers(1, pk + 1, S)  # the first packet of each stream is cut short: hop boundaries fall anywhere in later packets
    data = {"pcm_f32le": lambda n: (0.1 * g.standard_normal(n)).astype("<f4"), "pcm_s16le": lambda n: g.integers(-4000, 4000, n).astype("<i2")
            }.get(enc, lambda n: g.integers(0, 256, n).astype(np.uint8))
    n_total = pk + n_ticks * pk
    audio = [data(n_total) for _ in range(S)]
    origin = g.integers(0, 1 << 32, S)

    def packet(s, k):
        """Packet k of stream s -> (timestamp, bytes): packet 0 holds phase[s] samples, the others pk."""
        a = 0 if k == 0 else int(phase[s]) + (k - 1) * pk
        b = int(phase[s]) + k * pk
        return (int(origin[s]) + a) % (1 << 32), audio[s][a:b].tobytes()

    # the network: arrival tick of every packet (or never)
    lost = g.random((S, n_ticks)) < args.loss
    lost[:, 0] = False  # (the first packet sets the origin)
    delay = np.where(g.random((S, n_ticks)) < args.reorder, g.integers(1, late_max + 1, (S, n_ticks)) if late_max else 0, 0)
    delay[:, 0] = 0
    arrivals = [[] for _ in range(n_ticks + late_max + 1)]
    for k in range(n_ticks):
        for s in np.flatnonzero(~lost[:, k]).tolist():
            arrivals[k + int(delay[s, k])].append((s, k))
    print(f"jitter_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams, {rate} Hz {enc}, "
          f"{args.packet_ms}-ms packets ({pk * bps} bytes), depth {args.depth_ms} ms, loss {args.loss:.3f}, reordered {args.reorder:.3f}; "
          f"{hops} hops ({ticks} ticks) per pass, {args.reps} timed passes per path after a warm-up pass", flush=True)
    results = {}
    names = ["jitter"] + ([f"jitter ({args.against})"] if args.against else []) + ([] if args.profile else ["packets"])
    slots = list(range(S))
    fronts, kept, timed = {}, {n: [[] for _ in range(S)] for n in names}, {n: ([], []) for n in names}
    for name in names:
        inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
        mode = args.against if name.endswith(")") else args.conceal
        fronts[name] = PacketScorer(inner, rate, enc) if name == "packets" else JitterScorer(inner, rate, enc, depth, conceal=mode)

    def tick_args(name, t):
        if name == "packets":
            return ([packet(s, t)[1] for s in slots], slots)
        rows = arrivals[t]
        pt = [packet(s, k) for s, k in rows]
        return ([p[1] for p in pt], [s for s, _ in rows], np.array([p[0] for p in pt], dtype=np.int64))

    # every path warms up, then the timed passes alternate between the paths (pass r of each before pass r + 1 of any, the
    # order rotating), so a drift of the box falls on all of them
    for rep in range(-1, passes):
        for name in names[rep % len(names):] + names[:rep % len(names)]:
            front, scores = fronts[name], kept[name]

            def run(t0, n, keep):
                """Ticks t0 .. t0 + n - 1 -> (wall seconds, host seconds inside the calls)."""
                calls = [tick_args(name, t) for t in range(t0, t0 + n)]
                torch.cuda.synchronize()
                t_host, start, fed = 0.0, time.perf_counter(), 0
                for i, c in enumerate(calls):
                    a = time.perf_counter()
                    front.feed(*c, score=False)
                    res = None
                    if ((t0 + i + 1) * pk) // hop_in > ((t0 + i) * pk) // hop_in:  # a hop's worth of audio has gone by: score
                        res = front.drain()
                    t_host += time.perf_counter() - a
                    if keep and res is not None:
                        for s, v in zip(np.repeat(np.arange(S), res.counts.numpy()).tolist(), res.scores.tolist()):
                            scores[s].append(v)
                torch.cuda.synchronize()
                return time.perf_counter() - start, t_host

            if rep < 0:
                run(0, warm_ticks, True)
                continue
            dt, th = run(warm_ticks + rep * ticks, ticks, False)
            if rep > 0 or args.profile:
                timed[name][0].append(dt / hops)
                timed[name][1].append(th / hops)
    for name in names:
        times, host = sorted(timed[name][0]), sorted(timed[name][1])
        med = times[len(times) // 2]
        results[name] = (med, times, kept[name])
        extra = ""
        if name != "packets":
            st = {k: int(v.sum()) for k, v in fronts[name].stats().items()}
            extra = f"; conceal {fronts[name].conceal}; stats over all streams {st}"
        print(f"  {name:8s} {med * 1e3:8.2f} ms per 250 ms of audio (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); "
              f"host time inside feed / drain calls {host[len(host) // 2] * 1e3:.2f} ms; RTF {med / 0.25:.3f}{extra}", flush=True)
    if args.against:
        (ma, ta, _), (mb, tb, _) = results["jitter"], results[names[1]]
        print(f"  {args.conceal} / {args.against} {ma / mb:.3f}x (spread of {args.against}: {(tb[-1] - tb[0]) / mb * 100:.1f} % of its median, "
              f"of {args.conceal}: {(ta[-1] - ta[0]) / ma * 100:.1f} %)", flush=True)
    if not args.profile:
        (mj, tj, a), (mp, tp, b) = results["jitter"], results["packets"]
        print(f"  jitter / packets {mj / mp:.2f}x (spread of packets: {(tp[-1] - tp[0]) / mp * 100:.1f} % of its median, of jitter: "
              f"{(tj[-1] - tj[0]) / mj * 100:.1f} %)", flush=True)
        if args.loss == 0:
            n = [min(len(x), len(y)) for x, y in zip(a, b)]
            same = all(x[:k] == y[:k] for x, y, k in zip(a, b, n)) and min(n) >= 1
            print(f"  lossless: scores identical on the warm-up pass ({sum(n)} scores, >= {min(n)} per stream): {same}", flush=True)
            if not same:
                raise SystemExit(1)


if __name__ == "__main__":
    main()

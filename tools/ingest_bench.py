"""The packet front measured: S live calls deliver encoded packets of --packet-ms each (per-stream random phase against the
250-ms hop), the student scores them in KV-cached mode.  Two ways over the same bytes, timed per 250 ms of audio:

  packets   afx.ingest.PacketScorer: every tick one ``feed(packets, slots, score=False)`` (one upload; decode, resampling and
            per-slot assembly on the GPU), one ``drain()`` per hop;
  host      the path without the packet front: every tick the packets are decoded and appended to per-slot buffers on the
            host (numpy, vectorised over the streams), and once per hop the slots that hold a whole hop are uploaded and
            pushed through ``ResamplingScorer(KVCachedScorer, rate)`` (rates whose hop is a whole number of samples only).

    python tools/ingest_bench.py [--streams 2048] [--rate 8000] [--encoding mulaw] [--packet-ms 20] [--hops 8] [--reps 3]
    rocprofv3 --kernel-trace --stats ... -- python tools/ingest_bench.py --profile     (packets path only, 4 hops: kernel times)

Both paths must emit the same scores (checked on the warm-up pass: per slot, bit for bit).  Times are the median over --reps
timed passes after one warm-up pass (min and max given), wall clock around a pass that ends in a device synchronise; the
host time spent inside feed / drain calls (launches are asynchronous) is listed beside it.  Stamped with afx_build_id()."""
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
from afx.streaming import KVCachedScorer, ResamplingScorer  # noqa: E402

W, H = 64000, 4000


def g711_tables():
    mu, al = [], []
    for c in range(256):
        u = ~c & 0xFF
        v = ((((u & 15) << 3) + 132) << ((u >> 4) & 7)) - 132
        mu.append(-v if u & 0x80 else v)
        a = c ^ 0x55
        e, m = (a >> 4) & 7, a & 15
        v = ((m << 4) + 264) << (e - 1) if e else (m << 4) + 8
        al.append(v if a & 0x80 else -v)
    return {"mulaw": np.array(mu, dtype=np.float32) / np.float32(32768), "alaw": np.array(al, dtype=np.float32) / np.float32(32768)}


class HostFront:
    """Decode and per-slot hop assembly on the host (what a user of the bare scorers writes), then ResamplingScorer.push."""

    def __init__(self, scorer, rate, encoding):
        self.sc, self.enc, self.hop_in = ResamplingScorer(scorer, rate), encoding, H * rate // 16000
        self.S, self.cap = scorer.S, 4 * self.hop_in
        self.buf = np.zeros((self.S, self.cap), dtype=np.float32)
        self.head, self.fill = np.zeros(self.S, dtype=np.int64), np.zeros(self.S, dtype=np.int64)
        self.table = g711_tables().get(encoding)
        self.stage = torch.empty(self.S, self.hop_in, dtype=torch.float32, pin_memory=True)

    def _decode(self, data):
        raw = np.frombuffer(data, dtype=np.uint8)
        if self.table is not None:
            return self.table[raw]
        if self.enc == "pcm_s16le":
            return raw.view("<i2").astype(np.float32) / np.float32(32768)
        return raw.view("<f4")

    def feed(self, packets, n):
        """packets: one packet of n samples per slot (all slots, slot order)."""
        if n:
            x = self._decode(b"".join(packets)).reshape(self.S, n)
            cols = ((self.head + self.fill)[:, None] + np.arange(n)) % self.cap
            self.buf[np.arange(self.S)[:, None], cols] = x
            self.fill += n

    def drain(self):
        idx = np.flatnonzero(self.fill >= self.hop_in)
        if not idx.size:
            return idx, None
        cols = (self.head[idx][:, None] + np.arange(self.hop_in)) % self.cap
        st = self.stage[: idx.size]
        st.numpy()[:] = self.buf[idx[:, None], cols]
        self.head[idx] = (self.head[idx] + self.hop_in) % self.cap
        self.fill[idx] -= self.hop_in
        return idx, self.sc.push(st.cuda(non_blocking=True), idx.tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--rate", type=int, default=8000)
    ap.add_argument("--encoding", default="mulaw", choices=ENCODINGS)
    ap.add_argument("--packet-ms", type=int, default=20)
    ap.add_argument("--hops", type=int, default=8, help="hops of audio per timed pass")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="the packets path only, a short pass (for a rocprofv3 run)")
    args = ap.parse_args()
    S, rate, enc = args.streams, args.rate, args.encoding
    bps = {"pcm_f32le": 4, "pcm_s16le": 2}.get(enc, 1)
    pk = rate * args.packet_ms // 1000
    hop_in = H * rate // 16000
    if (H * rate) % 16000:
        raise SystemExit("the host path needs a rate whose hop is a whole number of samples")
    torch.cuda.set_device(0)
    sd = synth.model_state_dict("ConformerModel", n_layers=6)
    eng = engine.Engine("conformer", n_layers=6, dtype="fp16")
    eng.load_state_dict(sd)
    slots = list(range(S))
    passes = 1 if args.profile else 1 + args.reps
    hops = 4 if args.profile else args.hops
    ticks = hops * hop_in // pk
    warm_hops = W // H + 2
    g = np.random.default_rng(11)
    phase = g.integers(0, pk, S)  # the first packet of each stream is cut short: hop boundaries fall anywhere in later packets
    n_total = int(phase.max()) + warm_hops * hop_in + passes * ticks * pk

    def audio():
        if enc == "pcm_f32le":
            return (0.1 * g.standard_normal((S, n_total))).astype("<f4")
        if enc == "pcm_s16le":
            return g.integers(-4000, 4000, (S, n_total)).astype("<i2")
        return g.integers(0, 256, (S, n_total)).astype(np.uint8)
    data = audio()

    def cut(pos, n):
        """The next n samples of every stream from its own position pos[s] -> list of bytes."""
        return [data[s, pos[s]:pos[s] + n].tobytes() for s in range(S)]

    print(f"ingest_bench: build {lib().afx_build_id().decode()}; student fp16 (6 layers), KV-cached, {S} streams, {rate} Hz {enc}, "
          f"{args.packet_ms}-ms packets ({pk * bps} bytes), random phase per stream; {hops} hops ({ticks} ticks) per pass, "
          f"{args.reps} timed passes per path after a warm-up pass", flush=True)
    results = {}
    for name in (["packets"] if args.profile else ["packets", "host"]):
        inner = KVCachedScorer(eng, sd, S, window=W, hop=H)
        front = PacketScorer(inner, rate, enc) if name == "packets" else HostFront(inner, rate, enc)
        pos = np.zeros(S, dtype=np.int64)
        scores = [[] for _ in range(S)]

        def keep(idx, sc):
            if sc is not None and len(idx):
                for s, v in zip(idx, sc.tolist()):
                    scores[s].append(v)

        # the cut-short first packets, then whole hops until the K / V rings have wrapped
        first = [data[s, :phase[s]].tobytes() for s in range(S)]
        if name == "packets":
            front.feed(first, slots, score=False)
        else:
            for s in range(S):  # (ragged: slot by slot, outside every timing)
                x = front._decode(first[s])
                front.buf[s, :x.size] = x
                front.fill[s] = x.size
        pos += phase
        for _ in range(warm_hops):
            p = cut(pos, hop_in)
            pos += hop_in
            if name == "packets":
                front.feed(p, slots, score=True)
            else:
                front.feed(p, hop_in)
                front.drain()
        torch.cuda.synchronize()
        times, host = [], []
        for rep in range(passes):
            packets = []
            for t in range(ticks):
                packets.append(cut(pos, pk))
                pos += pk
            torch.cuda.synchronize()
            t_host = 0.0
            t0 = time.perf_counter()
            for t in range(ticks):
                a = time.perf_counter()
                if name == "packets":
                    front.feed(packets[t], slots, score=False)
                else:
                    front.feed(packets[t], pk)
                res = None
                if ((t + 1) * pk) // hop_in > (t * pk) // hop_in:  # a hop's worth of audio has gone by: score
                    res = front.drain()
                t_host += time.perf_counter() - a
                if rep == 0 and res is not None:  # the warm-up pass keeps its scores for the comparison
                    if name == "packets":
                        c = np.repeat(np.arange(S), res.counts.numpy())
                        keep(c.tolist(), res.scores)
                    else:
                        keep(res[0].tolist(), res[1])
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / hops
            if rep > 0 or args.profile:
                times.append(dt)
                host.append(t_host / hops)
        times.sort()
        host.sort()
        med = times[len(times) // 2]
        results[name] = (med, times, scores)
        print(f"  {name:8s} {med * 1e3:8.2f} ms per 250 ms of audio (min {times[0] * 1e3:.2f}, max {times[-1] * 1e3:.2f}); "
              f"host time inside feed / drain calls {host[len(host) // 2] * 1e3:.2f} ms; RTF {med / 0.25:.3f}", flush=True)
        del front, inner
        torch.cuda.empty_cache()
    if not args.profile:
        a, b = results["packets"][2], results["host"][2]
        n = [min(len(x), len(y)) for x, y in zip(a, b)]
        same = all(x[:k] == y[:k] for x, y, k in zip(a, b, n)) and min(n) >= 1
        (mb, tb, _), (mc, tc, _) = results["packets"], results["host"]
        print(f"  scores identical on the warm-up pass ({sum(n)} scores, >= {min(n)} per stream): {same}; packets / host "
              f"{mb / mc:.2f}x (spread of host: {(tc[-1] - tc[0]) / mc * 100:.1f} % of its median)", flush=True)
        if not same:
            raise SystemExit(1)


if __name__ == "__main__":
    main()

"""Offline timelines: the score of every window of a long recording, one per hop, as the streaming scorers would emit it.

Contract (window ``w``, hop ``h``, a recording ``x`` of N samples at 16 kHz): score j, for j = 0 .. N // h - 1, equals bit for
bit the j-th score of a fresh one-slot ``SlidingWindowScorer(model, 1, window=w, hop=h)`` fed x[j*h:(j+1)*h] in order: while
(j+1)*h < w the tiled history x[:(j+1)*h] (the reference's pad policy), after that ``model(x[(j+1)*h - w:(j+1)*h])``.
``warmup=False`` drops the tiled windows; ``cover_end=True`` adds one score for the window that ends at the last sample
(``model(x[-w:])``, or the tiled whole recording when N < w).  At another input rate r the recording is resampled once
(``afx.resample.Resampler``, bit-identical to hop-by-hop resampling) and the timeline equals what
``ResamplingScorer(SlidingWindowScorer(...), r)`` emits fed hops of h*r/16000 input samples.

Fast path (fp16 / bf16 engine, layer-norm extractor, no engine-side pre-emphasis, h % 160 == 0 and w % 160 == 0): every
steady window starts on a layer-5 frame of the recording's own frame sequence (frame f reads samples 160 f .. 160 f + 239),
so conv layers 0-5 run ONCE over the recording instead of once per window.  The recording is cut into chunk rows of
160 m + 80 samples that start at multiples of 160 m; layers 0-5 turn a row into exactly m layer-5 frames (32m+15, 16m+7,
8m+3, 4m+1, 2m, m), so the rows laid end to end ARE the frame sequence.  They run through the kernels ``IncrementalScorer``
uses (afx_k_conv0_packed, afx_k_conv_ln_act), whose frames are the engine's own bit for bit; frames that read the zero
padding past the recording's end are dropped.  Rows go in blocks of ``block_rows``; a shared buffer keeps only the frames
later windows still need, and ``afx_tail_forward_windows`` runs the tail (conv layer 6 on) on windows of many recordings
at once, at their offsets in that buffer.  Device memory is bounded by the block, buffer and batch sizes, not by N.

Everything else (fp32 / fp16x3 engines, the group-norm extractor, engine pre-emphasis, a hop or window that is not a
multiple of 160, the tiled warm-up windows, a ``cover_end`` window off the frame grid) runs through ``Engine.forward`` on
window rows built on the device -- the same scores, without the conv reuse."""
import torch

from . import harness
from . import kernels as K
from .engine import Engine, torch_dtype
from .streaming import CONV_KS, _frames5

FRAME = 160           # samples between two layer-5 frames (the cumulative stride of conv layers 0-5)
SPAN5 = 240           # samples one layer-5 frame reads
ROW_EXTRA = SPAN5 - FRAME  # a chunk row of m frames reads 160 m + 80 samples
CHUNK_FRAMES = 100    # m: layer-5 frames per chunk row (160 m + 80 samples; 1.005x the recording's samples)
BLOCK_ROWS = 64       # chunk rows per conv launch (64 s of audio at m = 100)
MIN_SAMPLES = 400     # one SSL frame (forward_ragged's rule)


class Timeline:
    """The timeline of one recording: ``scores`` (n,) fp32 CPU, bonafide scores (class 1: low means spoof);
    ``starts`` / ``ends`` (n,) float64 window bounds in input-rate samples (the resampler's delay taken out at other rates;
    a tiled warm-up window starts at 0); ``sample_rate`` the input rate."""

    def __init__(self, scores, starts, ends, sample_rate=16000):
        self.scores = torch.as_tensor(scores, dtype=torch.float32).cpu().reshape(-1)
        self.starts = torch.as_tensor(starts, dtype=torch.float64).cpu().reshape(-1)
        self.ends = torch.as_tensor(ends, dtype=torch.float64).cpu().reshape(-1)
        self.sample_rate = int(sample_rate)
        if not self.scores.numel() == self.starts.numel() == self.ends.numel():
            raise ValueError("scores, starts and ends differ in length")

    def __len__(self):
        return int(self.scores.numel())

    def times(self):
        """(n, 2) float64: each window's (start, end) in seconds."""
        return torch.stack([self.starts, self.ends], dim=1) / self.sample_rate

    def segments(self, threshold, min_windows=1):
        """Merged (start_s, end_s) intervals of runs of at least ``min_windows`` consecutive windows scoring below
        ``threshold``."""
        t = self.times().tolist()
        low = (self.scores < threshold).tolist()
        out, i = [], 0
        while i < len(low):
            if not low[i]:
                i += 1
                continue
            j = i
            while j + 1 < len(low) and low[j + 1]:
                j += 1
            if j - i + 1 >= min_windows:
                out.append((t[i][0], max(e for _, e in t[i:j + 1])))
            i = j + 1
        return out

    def alarms(self, policy):
        """The alarms a ``VerdictPolicy`` raises over this timeline (``policy.run_reference`` over ``scores``: what a one-slot
        ``afx.verdict.VerdictScorer`` logs when pushed the recording hop by hop): a list of ``(raised_s, cleared_s or None,
        kind)`` -- the ends, in seconds, of the windows at which the alarm was raised and cleared (None: still on at the
        end), and the raise's kind (1: by the smoothed score)."""
        events, _ = policy.run_reference(self.scores.numpy(), hop_index=range(len(self)))
        ends = (self.ends / self.sample_rate).tolist()
        out = []
        for _slot, kind, j, _bits in events:
            if kind == 3:
                out[-1] = (out[-1][0], ends[j], out[-1][2])
            else:
                out.append((ends[j], None, kind))
        return out

    def summary(self, threshold):
        """min, mean and the fraction of windows scoring below ``threshold`` (flagged as spoof)."""
        n = len(self)
        if n == 0:
            return {"windows": 0, "min": float("nan"), "mean": float("nan"), "flagged": 0.0}
        return {"windows": n, "min": float(self.scores.min()), "mean": float(self.scores.double().mean()),
                "flagged": float((self.scores < threshold).double().mean())}


# ---- plans (pure host arithmetic) -------------------------------------------------------------------------------
def plan_windows(n, window, hop, warmup=True, cover_end=False):
    """Windows of an n-sample (16 kHz) recording, in timeline order: a list of (start, end, warm) in samples.  Tick j ends
    at (j+1)*hop; ``warm`` = the window is the tiled history x[:end] (end < window; start is reported as 0); else it is
    x[end - window:end].  ``cover_end`` adds the window that ends at n."""
    out = []
    for j in range(n // hop):
        e = (j + 1) * hop
        if e < window and not warmup:
            continue
        out.append((max(e - window, 0), e, e < window))
    if cover_end:
        out.append((max(n - window, 0), n, n < window))
    return out


def chunk_rows(n, m=CHUNK_FRAMES):
    """-> (F, R): the layer-5 frames of an n-sample recording and the chunk rows of 160 m + 80 samples (row r starts at
    sample 160 m r and yields frames m r .. m r + m - 1) that produce them; the last row may read zero padding."""
    f = _frames5(n)
    return f, -(-f // m)


def row_blocks(n, m=CHUNK_FRAMES, block_rows=BLOCK_ROWS):
    """The blocks of chunk rows the fast path launches: (first row, rows, first frame, frames kept).  The frames kept are
    those whose 240-sample span lies inside the recording; together they are frames 0 .. F - 1, each once."""
    f, r = chunk_rows(n, m)
    out = []
    for r0 in range(0, r, block_rows):
        nb = min(block_rows, r - r0)
        out.append((r0, nb, r0 * m, min(nb * m, f - r0 * m)))
    return out


def fast_path_ok(engine, window, hop, state_dict=None):
    """Whether the conv stack can run once over the recording: an engine whose conv frames ``IncrementalScorer`` reproduces
    (fp16 / bf16, layer-norm extractor, no engine-side pre-emphasis), the conv weights at hand, and windows that start on
    the layer-5 frame grid (hop and window multiples of 160)."""
    return (getattr(engine, "dtype", None) in ("fp16", "bf16")
            and getattr(engine, "extractor_mode", "layer_norm") == "layer_norm"
            and not getattr(engine, "pre_emphasis", False)
            and getattr(engine, "arch", None) in ("conformer", "xlsr_aasist")
            and state_dict is not None and hop % FRAME == 0 and window % FRAME == 0 and _frames5(window) >= 2)


def input_hop(hop, rate):
    """The hop in input-rate samples (``ResamplingScorer``'s rule and message): hop * rate / 16000, refused when not whole."""
    from .resample import TARGET_RATE, _rate
    r = _rate(rate)
    if (hop * r) % TARGET_RATE:
        raise ValueError(f"a hop of {hop} samples at 16 kHz is {hop * r / TARGET_RATE} samples at {r} Hz: not a whole number")
    return hop * r // TARGET_RATE


def default_batch(engine):
    """BASELINE.json: batch 64 for the Conformer student, 16 for the XLS-R + AASIST teacher."""
    return 64 if getattr(engine, "arch", None) == "conformer" else 16


# ---- the driver ---------------------------------------------------------------------------------------------------
def _resolve(model, state_dict):
    """-> (engine, state_dict or None): an afx Engine with the weights it was loaded from, or a drop-in ``models.*`` module
    (its engine and its own weights)."""
    if isinstance(model, Engine):
        return model, state_dict
    if hasattr(model, "_afx_engine"):
        if model.training:
            raise RuntimeError("the MI355X-native path is inference-only: call model.eval() first")
        return model._afx_engine(), (state_dict if state_dict is not None else model.state_dict())
    raise ValueError("model: an afx Engine (with state_dict=) or a drop-in models.* module")


class _ConvStack:
    """Conv layers 0-5 on chunk rows, with IncrementalScorer's kernels and operand blocks."""

    def __init__(self, engine, state_dict):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        pre = "ssl_model.model.feature_extractor.conv_layers."
        dev = engine.device
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.dt = engine.dtype
        self.w0 = f32(sd[pre + "0.0.weight"])
        self.pack0 = K.conv0_pack(self.w0, f32(sd[pre + "0.0.bias"]))
        self.cw = [None] + [K.pack_conv(self.dt, f32(sd[f"{pre}{i}.0.weight"])) for i in range(1, 6)]
        self.cb = [f32(sd[f"{pre}{i}.0.bias"]) for i in range(6)]
        self.lg = [f32(sd[f"{pre}{i}.2.1.weight"]) for i in range(6)]
        self.lb = [f32(sd[f"{pre}{i}.2.1.bias"]) for i in range(6)]

    def __call__(self, rows):
        """rows (R, 160 m + 80) fp32 -> (R, m, 512) layer-5 frames in the operand type: one launch per layer."""
        y = K.conv0_packed(self.dt, rows, self.pack0, self.w0, self.cb[0], self.lg[0], self.lb[0])
        for i in range(1, 6):
            k, s = CONV_KS[i]
            _, y = K.conv_ln_act(self.dt, y, self.cw[i], k, s, self.cb[i], self.lg[i], self.lb[i])
        return y


class _Run:
    """One score_timeline call: the queues of windows waiting for a batch and the shared layer-5 buffer."""

    def __init__(self, eng, window, batch, n_windows, conv=None, T5=0, cap=0):
        self.eng, self.window, self.batch, self.dev = eng, window, batch, eng.device
        self.scores = torch.empty(n_windows, dtype=torch.float32, device=self.dev)
        self.full = []  # (window id, recording, start, end, warm): Engine.forward on rows built here
        self.tail = []  # (window id, element offset into self.pool)
        self.conv, self.T5 = conv, T5
        self.pool = torch.empty(cap, 512, dtype=torch_dtype(eng.dtype), device=self.dev) if conv is not None else None
        self.pool_end = 0  # pool rows in use (the last recording's frames end there)

    def add_full(self, item):
        self.full.append(item)
        if len(self.full) >= self.batch:
            self.flush_full()

    def flush_full(self):
        if not self.full:
            return
        items, self.full = self.full, []
        B, w = len(items), self.window
        rows = torch.empty(B, w, dtype=torch.float32, device=self.dev)
        warm = [i for i, it in enumerate(items) if it[4]]
        steady = [i for i, it in enumerate(items) if not it[4]]
        if warm:  # the tiled history, as the streaming scorers build it
            rows[warm] = harness.batch_adjust_duration([items[i][1][:items[i][3]].to(self.dev) for i in warm], w, device=self.dev)
        if steady:  # one copy of the batch's windows
            rows[steady] = torch.stack([items[i][1][items[i][2]:items[i][3]].to(self.dev, torch.float32) for i in steady])
        self.scores[torch.tensor([it[0] for it in items], device=self.dev)] = self.eng.forward(rows)[:, 1]

    def add_tail(self, wid, off):
        self.tail.append((wid, off))
        if len(self.tail) >= self.batch:
            self.flush_tail()

    def flush_tail(self):
        if not self.tail:
            return
        items, self.tail = self.tail, []
        out = self.eng.tail_windows(self.pool, [o for _, o in items], self.T5)
        self.scores[torch.tensor([i for i, _ in items], device=self.dev)] = out[:, 1]

    def recording(self, x, plan, wid0, m, block_rows):
        """Queue the windows of one 16 kHz recording x; fast path: run its conv stack block by block into the pool."""
        if self.conv is None:
            for k, (s, e, warm) in enumerate(plan):
                self.add_full((wid0 + k, x, s, e, warm))
            return
        n = x.numel()
        tails = []
        for k, (s, e, warm) in enumerate(plan):
            if not warm and s % FRAME == 0:
                tails.append((s // FRAME, wid0 + k))
            else:
                self.add_full((wid0 + k, x, s, e, warm))
        if not tails:
            return
        tails.sort()
        pos = self.pool_end  # pool row of the recording's frame `base`
        base, nxt, L = 0, 0, FRAME * m + ROW_EXTRA
        done = 0  # frames of this recording produced so far
        for r0, nb, f0, keep in row_blocks(n, m, block_rows):
            if f0 >= tails[-1][0] + self.T5:
                break  # no window needs the frames from here on
            a, b = FRAME * m * r0, FRAME * m * (r0 + nb) + ROW_EXTRA
            seg = torch.zeros(b - a, dtype=torch.float32, device=self.dev)
            seg[:min(b, n) - a] = x[a:min(b, n)].to(self.dev, torch.float32)
            y = self.conv(seg.as_strided((nb, L), (FRAME * m, 1)).contiguous()).reshape(-1, 512)[:keep]
            if pos + (f0 + keep - base) > self.pool.shape[0]:  # full: run the queued windows, keep what later ones need
                self.flush_tail()
                k0 = min(tails[nxt][0], done) if nxt < len(tails) else done
                kept = done - k0
                if kept:
                    self.pool[:kept] = self.pool[pos + k0 - base:pos + done - base].clone()
                pos, base = 0, k0
            self.pool[pos + f0 - base:pos + f0 + keep - base] = y
            done = f0 + keep
            self.pool_end = pos + done - base
            while nxt < len(tails) and tails[nxt][0] + self.T5 <= done:
                f, wid = tails[nxt]
                self.add_tail(wid, (pos + f - base) * 512)
                nxt += 1
        if nxt != len(tails):
            raise RuntimeError("a window's layer-5 frames were never produced")


def score_timeline(model, recordings, window=64000, hop=4000, sample_rate=16000, warmup=True, cover_end=False,
                   batch_windows=None, state_dict=None, block_rows=BLOCK_ROWS, chunk_frames=CHUNK_FRAMES):
    """Score every hop of long recordings (see the module docstring) -> one ``Timeline`` per recording.

    model: an afx ``Engine`` with the ``state_dict`` it was loaded from (reference key names, as for ``IncrementalScorer``;
    without it the conv stack is not reused), or a drop-in ``models.*`` module (its engine and own weights).  recordings: a
    list of 1-D waveforms of any lengths (>= 400 samples) at ``sample_rate``, on the host or on the GPU.  The windows of all
    recordings -- tiled warm-up, steady, fallback -- share batches of at most ``batch_windows`` (default: 64 for the
    Conformer student, 16 for XLS-R + AASIST).  block_rows / chunk_frames: the fast path's conv blocks (rows per launch,
    layer-5 frames per row); they change no score."""
    eng, sd = _resolve(model, state_dict)
    if window <= 0 or hop <= 0:
        raise ValueError("window and hop must be positive")
    if block_rows <= 0 or chunk_frames <= 0:
        raise ValueError("block_rows and chunk_frames must be positive")
    batch = int(batch_windows or default_batch(eng))
    if batch <= 0:
        raise ValueError("batch_windows must be positive")
    recs = [torch.as_tensor(x).reshape(-1) for x in recordings]
    for i, x in enumerate(recs):
        if x.numel() < MIN_SAMPLES:
            raise ValueError(f"recording {i} has {x.numel()} samples: every recording needs at least {MIN_SAMPLES} (one SSL frame)")
    rate, delay, hop_in = 16000, 0.0, hop
    if sample_rate != 16000:
        from .resample import Resampler
        hop_in = input_hop(hop, sample_rate)
        rs = Resampler(sample_rate, eng.device)
        rate, delay = rs.rate, rs.delay
        with torch.cuda.device(eng.device):
            recs = rs.clips(recs)  # (each whole, once: bit-identical to the hop-by-hop stream)
    plans = [plan_windows(x.numel(), window, hop, warmup, cover_end) for x in recs]
    fast = fast_path_ok(eng, window, hop, sd)
    T5 = _frames5(window)
    hf = hop // FRAME
    cap = T5 + block_rows * chunk_frames + batch * min(max(hf, 1), T5)
    with torch.cuda.device(eng.device):
        run = _Run(eng, window, batch, sum(len(p) for p in plans), _ConvStack(eng, sd) if fast else None, T5, cap)
        wid = 0
        for x, plan in zip(recs, plans):
            run.recording(x, plan, wid, chunk_frames, block_rows)
            wid += len(plan)
        run.flush_tail()
        run.flush_full()
        scores = run.scores.cpu()
    out, wid = [], 0
    scale = rate / 16000.0
    for plan in plans:
        st = torch.tensor([s for s, _, _ in plan], dtype=torch.float64)
        en = torch.tensor([e for _, e, _ in plan], dtype=torch.float64)
        if delay:  # 16 kHz sample k of the resampled stream is input time (k - delay) / 16000 s
            st, en = (st - delay).clamp(min=0), (en - delay).clamp(min=0)
        out.append(Timeline(scores[wid:wid + len(plan)], st * scale, en * scale, rate))
        wid += len(plan)
    return out

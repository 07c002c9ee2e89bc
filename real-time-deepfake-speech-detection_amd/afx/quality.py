"""Input quality on the GPU: every hop the scorers are pushed is measured on the device, the hops that are not fit to judge
are flagged, and the score of a stream whose recent hops were flagged is replaced by NaN -- "I cannot judge this".

Every layer behind a scorer trusts the score: a clipped microphone, a stuck sample from a dead codec leg, a 200-ms gap of
zeros or a caller's NaN all produce a number, the verdict layer smooths it and the evidence layer records a clip of it.
``QualityScorer(scorer, policy)`` stands between the scorer and those layers.  It measures the hops the model actually saw
(one ``afx_k_quality`` launch per push, nothing read back) and hands on the inner score bit for bit, or the quiet NaN.
``Quality(S, policy, hop, window, device)`` is the state on its own, ``QualityPolicy.measure`` the offline counterpart.

An abstained score is a NaN, like the speech gate's "no hop completed": the verdict layer's NaN row "changes nothing and logs
nothing", so nothing behind this layer needs to know it.  ``valid`` and ``last_meas`` are what tell the two apart: the gate's
NaN belongs to a push in which this layer was not reached (``last_meas`` has no row for it), an abstention is a row of
``last_meas`` whose slot is not ``valid``.

The function (also stated in include/afx.h).  ``QualityPolicy(clip=0.98, clip_count=8, flat_run=320, quiet=1e-7, dc=0.05,
mask=31, max_bad=0, abstain=True)``: each float is rounded to fp32 once; ``E_quiet = fp32(quiet * hop)`` and ``D = fp32(dc *
hop)`` are computed in float64 and rounded once.  ``W = ceil(window / hop)``, 1 <= W <= 1024.  Per slot the state is
``q_ring`` ((S, W) uint8: the flags of hop k at position (k-1) mod W), ``q_state`` ((S, 3) int32 = (last, run, bad): the bits
of the newest sample, the length of the run of identical samples it ends, the flagged hops of the window; (0, 0, 0) for a
new stream) and ``q_totals`` ((S, 6) int32 saturating at 2^31 - 1: the hops seen and the hops with each of the five flags).
``reset`` clears ``q_state`` and ``q_totals`` only: the bound k >= 1 below keeps a new session from reading the ring entries
of the one before it.

An update names rows i = 0..A-1, A <= 8192: slot b_i (distinct), hop index k_i >= 1 (the host's ``samples_seen // hop`` after
this hop), the hop x[0..h-1] in fp32 and optionally the inner score s_i.  Every arithmetic operation is a single correctly
rounded fp32 operation, no fma::

    nonfinite = the samples with (bits & 0x7f800000) == 0x7f800000
    clipped   = the samples with |x| >= clip                        (an fp32 compare: a NaN is not counted)
    peak      = the largest |x| over the samples that are not NaN, +0.0 if there are none
    e, s      = the sum of x * x (one multiply each) and the sum of x, both in one fixed order that suits 16-byte loads:
                the hop padded with +0.0 to a multiple of 1024 and viewed as (tiles, 256, 4);
                q[t, c] = tile 0's element, then + tile 1's, ... in ascending tile order;
                r[t] = (q[t, 0] + q[t, 1]) + (q[t, 2] + q[t, 3]);
                for w = 128, 64, ..., 1: r[t] = r[t] + r[t + w] for t < w;  the result is r[0].
                Non-finite values follow IEEE; a NaN result is recorded as 0x7fc00000 (IEEE fixes no payload or sign)
    longest   = the longest run of identical samples, over the STREAM: r_i = 1 if sample i is the session's first or
                bits(x[i]) != bits(x[i-1]), else r_{i-1} + 1 (saturating); (last, run) carry across hops; longest is the
                maximum of r_i over this hop.  The compare is bitwise: +0 and -0 differ, two NaNs of equal bits are equal
    flags     = 1 NONFINITE: nonfinite > 0  |  2 CLIPPED: clipped >= clip_count  |  4 FLAT: longest >= flat_run
              | 8 QUIET: e < E_quiet  |  16 DC: |s| > D            (a NaN e or s sets neither 8 nor 16)
    q_ring[b, (k-1) mod W] = flags
    bad       = the hops j in [max(1, k-W+1), k] whose ring entry has a bit of ``mask``;  valid = bad <= max_bad
    meas[i]   = (flags, nonfinite, clipped, longest, bits(e), bits(s), bits(peak), bad), 8 int32
    out[i]    = s_i, bit for bit, when valid or abstain is off, else the quiet NaN 0x7fc00000

(A new stream's ``run`` is 0, so joining it to the first sample gives r = 1 whatever ``last`` holds.)  Without scores (a
KV-cached push that returned ``None``) the measurement still runs.  A row with a slot outside [0, S) or k < 1 is skipped
whole: the state is untouched, its ``meas`` row is all -1 and ``out[i] = s_i``.

``QualityPolicy.step_reference`` restates one update in numpy on host mirrors of the whole state and ``run_reference`` drives
it for one fresh stream; the kernel is bit-exact to it (tests/test_gpu_quality.py).

All defaults are engineering defaults, not tuned ones: there is no labelled corpus behind them.  ``clip`` / ``clip_count``:
eight samples at 98 % of full scale in a hop; ``flat_run``: 20 ms of one repeated value at 16 kHz; ``quiet``: a mean square
of 1e-7 (-70 dBFS); ``dc``: a mean of 5 % of full scale; ``max_bad=0``: one flagged hop in the window withholds the score.
"""
import numpy as np
import torch

from ._layer import N_MAX, Field, HopTable, WindowState, WithholdingLayer, _on, fp32, hop_indices, integer, need_gpu, slot_count, slots_of
from ._lib import call_on, check, lib, ptr

QUALITY_FORMAT = 1   # layout of the quality part of a StreamState: import_slots refuses any other
MAX_W = 1024         # hops of window
MAX_HOP = 1 << 24    # samples of a hop
QNAN_BITS = 0x7fc00000
NONFINITE, CLIPPED, FLAT, QUIET, DC = 1, 2, 4, 8, 16
FLAG_NAMES = ("nonfinite", "clipped", "flat", "quiet", "dc")


def window_hops(window, hop):
    """W = ceil(window / hop), the hops the window count looks back over; 1 <= W <= 1024 and 1 <= hop <= 2^24."""
    hop = integer("hop", hop, 1, MAX_HOP)
    window = integer("window", window, 1)
    W = -(-window // hop)
    if W > MAX_W:
        raise ValueError(f"a window of {window} samples is {W} hops of {hop}: at most {MAX_W}")
    return W


class QualityState(WindowState):
    """Host mirrors of the whole quality state of S slots: ``ring`` (S, W) uint8, ``st`` (S, 3) int32 = (last, run, bad),
    ``totals`` (S, 6) int32; a new stream everywhere."""

    ring_dtype, new, n_totals = np.uint8, (0, 0, 0), 6


def hop_sums(x):
    """(A, h) float32 -> (e, s), each (A,) float32: the sum of squares and the sum of every row in the stated order."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    A, h = x.shape
    tiles = -(-h // 1024)
    y = np.zeros((A, tiles * 1024), dtype=np.float32)
    y[:, :h] = x
    y = y.reshape(A, tiles, 256, 4)
    out = []
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for v in (y * y, y):             # (one fp32 multiply per sample)
            q = v[:, 0].copy()
            for t in range(1, tiles):
                q = q + v[:, t]          # fp32 array operations: one rounding each
            r = (q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3])
            w = 128
            while w >= 1:
                r = r[:, :w] + r[:, w:2 * w]
                w //= 2
            out.append(r[:, 0].astype(np.float32))
    return out[0], out[1]


def _canonical_bits(v):
    """The bits of fp32 values as int32, every NaN as 0x7fc00000."""
    return np.where(np.isnan(v), np.int32(QNAN_BITS), v.view(np.int32)).astype(np.int32)


class QualityPolicy:
    """When a hop is not fit to judge and when a stream's score is withheld; see the module docstring for the function.

    clip / clip_count: CLIPPED when ``clip_count`` samples of a hop have ``|x| >= clip``.  flat_run (>= 2): FLAT when a run of
    identical samples reaches it (runs cross hop borders).  quiet: QUIET when the hop's mean square is below it.  dc: DC when
    the magnitude of the hop's mean exceeds it.  mask: the flags that count against a hop (bits 1, 2, 4, 8, 16 = NONFINITE,
    CLIPPED, FLAT, QUIET, DC).  max_bad: the score is withheld while more than this many of the window's hops count.
    abstain=False: measure and flag only, every score passes.  All defaults are engineering defaults, not tuned ones."""

    def __init__(self, clip=0.98, clip_count=8, flat_run=320, quiet=1e-7, dc=0.05, mask=31, max_bad=0, abstain=True):
        self.clip32 = fp32("clip", clip, True)
        self.quiet32, self.dc32 = fp32("quiet", quiet, False), fp32("dc", dc, False)
        self.clip_count = integer("clip_count", clip_count, 1)
        self.flat_run = integer("flat_run", flat_run, 2)
        self.mask = integer("mask", mask, 0, 31)
        self.max_bad = integer("max_bad", max_bad, 0)
        if not isinstance(abstain, (bool, np.bool_)):
            raise ValueError(f"abstain: True or False, got {abstain!r}")
        self.abstain = bool(abstain)
        self.clip, self.quiet, self.dc = float(self.clip32), float(self.quiet32), float(self.dc32)

    def params(self):
        """What identifies this policy (plain ints, floats and bools)."""
        return dict(clip=self.clip, clip_count=self.clip_count, flat_run=self.flat_run, quiet=self.quiet, dc=self.dc,
                    mask=self.mask, max_bad=self.max_bad, abstain=self.abstain)

    def bounds(self, hop):
        """(E_quiet, D) for hops of ``hop`` samples: fp32(quiet * hop) and fp32(dc * hop), the products in float64."""
        with np.errstate(over="ignore"):
            return np.float32(np.float64(self.quiet32) * hop), np.float32(np.float64(self.dc32) * hop)

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def step_reference(self, slots, hops, hop_index, scores, state):
        """One update in numpy.  slots (A,) distinct ints, hops (A, h) fp32, hop_index an int or (A,) ints, scores (A,) fp32
        or None; ``state`` (a ``QualityState`` of the whole scorer) is UPDATED IN PLACE (rows of slots not named are not
        written) -> ``(out, meas)``: (A,) float32 or None, and (A, 8) int32.  A row with ``hop_index < 1`` is skipped whole
        as the kernel skips it (its meas row is -1, its score passes)."""
        if not isinstance(state, QualityState):
            raise ValueError("state: a QualityState")
        S, W = state.ring.shape
        b = slots_of(slots, S)
        A = b.size
        x = np.ascontiguousarray(hops, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != A or not 1 <= x.shape[1] <= MAX_HOP:
            raise ValueError("hops: (A, h) float32, one hop per named slot")
        h = x.shape[1]
        k = hop_indices(hop_index, A).copy()
        s_in = None if scores is None else np.asarray(scores, dtype=np.float32).reshape(-1).copy()
        if s_in is not None and s_in.size != A:
            raise ValueError("slots, hops, hop_index and scores name the same rows")
        meas = np.full((A, 8), -1, dtype=np.int32)
        out = None if s_in is None else s_in.copy()
        live = np.flatnonzero(k >= 1)
        if not live.size:
            return out, meas
        b, k, x = b[live], k[live], x[live]
        e_quiet, d = self.bounds(h)
        bits = x.view(np.uint32)
        nonfinite = ((bits & 0x7f800000) == 0x7f800000).sum(axis=1)
        with np.errstate(invalid="ignore"):
            ax = np.abs(x)
            clipped = (ax >= self.clip32).sum(axis=1)
            peak = np.where(np.isnan(x), np.float32(0), ax).max(axis=1).astype(np.float32)
        e, s = hop_sums(x)
        # the runs: r_j over the stream, the carried (last, run) in front of the hop
        last, run = state.st[b, 0].view(np.uint32), state.st[b, 1].astype(np.int64)
        prev = np.concatenate([last[:, None], bits[:, :-1]], axis=1)
        change = bits != prev                                   # (A', h): sample j starts a run
        j = np.arange(h, dtype=np.int64)[None, :]
        start = np.maximum.accumulate(np.where(change, j, -1), axis=1)  # where the run of sample j started, -1: before the hop
        r = np.where(start >= 0, j - start + 1, np.minimum(run[:, None] + j + 1, N_MAX))
        longest, run1 = r.max(axis=1), r[:, -1]
        with np.errstate(invalid="ignore"):
            flags = ((nonfinite > 0) * NONFINITE | (clipped >= self.clip_count) * CLIPPED | (longest >= self.flat_run) * FLAT
                     | (e < e_quiet) * QUIET | (np.abs(s) > d) * DC).astype(np.int64)
        state.ring[b, (k - 1) % W] = flags.astype(np.uint8)
        i = np.arange(W, dtype=np.int64)[None, :]
        inside = i < np.minimum(k, W)[:, None]                  # hops k, k-1, ..: never before the session's first
        entries = state.ring[b[:, None], (k[:, None] - 1 - i) % W]
        bad = (inside & ((entries & self.mask) != 0)).sum(axis=1)
        state.st[b] = np.stack([bits[:, -1].view(np.int32).astype(np.int64), run1, bad], axis=1).astype(np.int32)
        tot = state.totals[b].astype(np.int64)
        tot[:, 0] += 1
        for n in range(5):
            tot[:, 1 + n] += (flags >> n) & 1
        state.totals[b] = np.minimum(tot, N_MAX).astype(np.int32)
        meas[live] = np.stack([flags, nonfinite, clipped, longest, _canonical_bits(e), _canonical_bits(s), peak.view(np.int32), bad],
                              axis=1).astype(np.int32)
        if out is not None and self.abstain:
            o = out.view(np.int32)
            o[live[bad > self.max_bad]] = QNAN_BITS
        return out, meas

    def run_reference(self, stream, hop, window):
        """One fresh stream, hop by hop (a trailing part of a hop is left out) -> ``(meas (n, 8) int32, valid (n,) bool)``:
        the measurement of every hop and whether the stream's score passes after it."""
        x = np.asarray(stream, dtype=np.float32).reshape(-1)
        W = window_hops(window, hop)
        n = x.size // hop
        st = QualityState(1, W)
        meas = np.zeros((n, 8), dtype=np.int32)
        for j in range(n):
            meas[j] = self.step_reference([0], x[None, j * hop:(j + 1) * hop], j + 1, None, st)[1][0]
        return meas, meas[:, 7] <= self.max_bad

    # ---- offline -----------------------------------------------------------------------------------------------------------
    def measure(self, clips, hop, window, device="cuda"):
        """clips: 1-D fp32 tensors (or one (n, L) tensor), each a recording from its start -> per clip a (hops, 8) int32
        numpy array, ``meas`` of every whole hop with fresh state.  One launch per hop index over all clips (the hop is a
        strided view of one padded matrix on the device; a clip that has ended rides along as a skipped row)."""
        clips = list(clips.unbind(0)) if isinstance(clips, torch.Tensor) and clips.ndim == 2 else list(clips)
        for c in clips:
            if not isinstance(c, torch.Tensor) or c.ndim != 1 or c.dtype != torch.float32:
                raise ValueError("clips: 1-D fp32 tensors")
        n = len(clips)
        if not n:
            return []
        q = Quality(n, self, hop, window, device)
        hops = np.array([c.numel() // q.hop for c in clips], dtype=np.int64)
        most = int(hops.max())
        if not most:
            return [np.zeros((0, 8), dtype=np.int32) for _ in clips]
        with _on(q.device):
            mat = torch.zeros(n, most * q.hop, dtype=torch.float32, device=q.device)
            for i, c in enumerate(clips):
                mat[i, :hops[i] * q.hop] = c[:hops[i] * q.hop].to(q.device)
            per_hop = [q._update(mat[:, j * q.hop:(j + 1) * q.hop], np.where(hops > j, np.arange(n), -1), np.full(n, j + 1), None)[1]
                       for j in range(most)]
            all_meas = torch.stack(per_hop, dim=1).cpu().numpy()  # (n, most, 8)
        return [all_meas[i, :hops[i]].copy() for i in range(n)]


class Quality(HopTable):
    """The per-slot quality state of ``S`` streams under ``policy`` for hops of ``hop`` samples and a window of ``window``
    samples, on ``device``; see the module docstring.  ``update`` is one pinned upload of the header and one
    ``afx_k_quality`` launch, with no synchronisation; ``valid`` and ``bad`` are views of the state on the device;
    ``stats()`` is the only read-back."""

    meas_cols = 8

    def __init__(self, S, policy, hop, window, device="cuda"):
        S = slot_count(S, policy, QualityPolicy)
        self.W = window_hops(window, hop)
        self.policy, self.hop, self.window = policy, int(hop), int(window)
        self.e_quiet, self.d = (float(v) for v in policy.bounds(self.hop))
        # (``reset`` leaves the ring alone: a new session's window count never reaches back before its first hop)
        self._allocate(S, device, Field("quality_ring", "ring", (self.W,), torch.uint8),
                       Field("quality_state", "st", (3,), torch.int32, host=True, new=(0, 0, 0)),
                       Field("quality_totals", "totals", (6,), torch.int32, host=True, new=0))

    # ---- views ---------------------------------------------------------------------------------------------------------------
    @property
    def bad(self):
        """(S,) int32 on the device: the flagged hops in each slot's window."""
        return self.st[:, 2]

    @property
    def valid(self):
        """(S,) bool on the device: which slots' scores pass (``bad <= max_bad``; a new stream is valid)."""
        return self.st[:, 2] <= self.policy.max_bad

    def flags_at(self, hop_index):
        """hop_index: (S,) ints on the host, each slot's newest hop (0: none yet) -> (S,) uint8 on the device: the flags of
        that hop (0 where there is none).  One small upload, no synchronisation."""
        k = np.asarray(hop_index, dtype=np.int64).reshape(-1)
        if k.size != self.S or (k < 0).any():
            raise ValueError(f"hop_index: {self.S} hop indices of 0 or more")
        with _on(self.device):
            tab = torch.empty(self.S, 2, dtype=torch.int64, pin_memory=self.device.type == "cuda")
            tab.numpy()[:] = np.stack([np.where(k > 0, (k - 1) % self.W, 0), k > 0], axis=1)
            d = tab.to(self.device, non_blocking=True)
            return self.ring.gather(1, d[:, :1]).squeeze(1) * d[:, 1].to(torch.uint8)

    def stats(self):
        """Per slot, since its last ``reset``: (S,) int64 host tensors ``hops`` and ``nonfinite``, ``clipped``, ``flat``,
        ``quiet``, ``dc`` (the hops that had the flag).  Reads ``q_totals`` back: the only read-back of this layer."""
        t = self.totals.to("cpu", torch.int64)
        return dict(hops=t[:, 0].clone(), **{name: t[:, 1 + n].clone() for n, name in enumerate(FLAG_NAMES)})

    # ---- the update ------------------------------------------------------------------------------------------------------
    def update(self, hops, slots=None, *, hop_index, scores=None):
        """hops: (A, hop) fp32 on the device (any row stride of at least a hop: a chunk that is a view is read in place),
        row i the hop of slot slots[i] (None: every slot, in order; the slots are distinct); hop_index: an int or (A,) ints
        on the host, 1 or more; scores: (A,) fp32 on the device (any stride: a column is read in place) or None -> ``(out,
        meas)`` on the device: (A,) fp32 or None, (A, 8) int32.  One pinned upload, one launch, no synchronisation."""
        b = slots_of(slots, self.S)
        A = b.size
        if (not isinstance(hops, torch.Tensor) or hops.dtype != torch.float32 or hops.shape != (A, self.hop)
                or hops.device != self.device):
            raise ValueError(f"hops: an fp32 tensor of shape {(A, self.hop)} on {self.device}")
        k, scores = self._hop_rows(A, hop_index, scores)
        return self._update(hops, b, k, scores) if A else self._no_rows(scores)

    def _update(self, hops, slots, hop_index, scores):
        need_gpu(self.device, "hops are measured")
        p, A = self.policy, len(slots)
        if hops.stride(1) != 1 or (A > 1 and hops.stride(0) < self.hop):  # (a transposed or expanded view)
            hops = hops.contiguous()
        with torch.cuda.device(self.device):
            d, meas, out = self._buffers(slots, hop_index, scores)
            check(call_on(self.ring, lib().afx_k_quality, ptr(hops), max(hops.stride(0), self.hop), A, self.hop, ptr(d), ptr(scores),
                          1 if scores is None else max(scores.stride(0), 1), p.clip, p.clip_count, p.flat_run, self.e_quiet, self.d,
                          p.mask, p.max_bad, int(p.abstain), ptr(self.ring), self.W, ptr(self.st), ptr(self.totals), self.S,
                          ptr(meas), ptr(out)))
        return out, meas

    # ---- sessions ------------------------------------------------------------------------------------------------------------
    def check_rows(self, rows, n, seen):
        """Refuses (ValueError) what cannot be the state of n sessions of this window; -> (ring, st, totals)."""
        self.check_shapes(rows, n)
        ring, st, totals = rows[0], rows[1].cpu(), rows[2].cpu()
        last, run, bad = st.unbind(1)
        if bool(((last < -(1 << 31)) | (last > N_MAX)).any()):
            raise ValueError("import_slots: a session's newest sample is not 32 bits")
        if bool(((run < 0) | (run > N_MAX)).any()):
            raise ValueError("import_slots: a session's run is negative (or beyond 2^31 - 1)")
        if bool(((bad < 0) | (bad > self.W)).any()):
            raise ValueError(f"import_slots: a session's flagged hops are outside 0..{self.W}")
        if bool(((totals < 0) | (totals > N_MAX) | (totals > totals[:, :1])).any()):
            raise ValueError("import_slots: a session's totals are negative, or a flag was counted more often than hops were")
        if bool((ring.cpu() > 31).any()):
            raise ValueError("import_slots: a ring entry has a bit that is no flag")
        return ring, st, totals


class QualityScorer(WithholdingLayer):
    """``scorer`` (whatever stands below the quality layer in the stack order of ``afx._layer``) with the quality layer
    behind it under ``policy``; see the module docstring.  It presents the surface the verdict layer, the gate and the
    fronts drive an inner scorer through and goes where the cascade goes, inside the verdict layer:
    ``JitterScorer(GatedScorer(EvidenceScorer(VerdictScorer(QualityScorer(CascadeScorer(...), qpolicy), vpolicy), epolicy)),
    8000, "mulaw", depth)``.

    ``push`` runs the inner ``push``, then one update on the same chunk with ``hop_index = samples_seen // hop`` (one small
    upload, one launch, no synchronisation) and returns ``out``: the inner scores, bit for bit, with the quiet NaN where the
    slot is not valid (a KV-cached ``None`` stays ``None``; the hop is measured all the same).

    Results, all on the device: ``last_meas`` ((A, 8) int32, the rows of the newest push), ``valid`` ((S,) bool),
    ``flags`` ((S,) uint8, each slot's newest flags).  ``stats()`` is the only read-back.  Around a cascade ``verified``,
    ``verified_at`` and ``take_events`` are the cascade's, and with ``abstain`` on ``last_verified()`` has NaN for the
    verifier scores of the slots that are not valid (on the device, no synchronisation): an invalid slot's verifier score
    raises nothing in the verdict layer.

    Sessions: the part of a ``StreamState`` is ``quality_ring`` ((n, W) uint8), ``quality_state`` ((n, 3) int64: last, run,
    bad) and ``quality_totals`` ((n, 6) int64), meta ``quality`` (format) and ``quality_window`` (W and hop); rows that
    cannot belong to a session (a negative ``run``, ``bad > W``) are refused.  The ring holds raw flags, so ``clip``,
    ``flat_run``, ``mask`` and ``max_bad`` may differ where the sessions go (``bad`` is recounted under the new ``mask`` at
    the slot's next hop)."""

    layer = "quality"
    _part = "quality part (it was not exported by a QualityScorer)"
    _does = "hops are scored and measured"

    def __init__(self, scorer, policy=None):
        super().__init__(scorer, QualityPolicy() if policy is None else policy, Quality)
        self.quality = self._table

    @property
    def flags(self):
        """(S,) uint8 on the device: the flags of each slot's newest hop, 0 before its first."""
        return self.quality.flags_at((self.samples_seen // self.hop).numpy())

    def _operand(self, chunk, idx):
        return chunk  # (the hops the model saw are the hops measured)

    # ---- sessions (afx._layer.Layer) -----------------------------------------------------------------------------------------
    def _meta(self):
        return dict(quality=QUALITY_FORMAT, quality_window=dict(W=self.quality.W, hop=self.hop))

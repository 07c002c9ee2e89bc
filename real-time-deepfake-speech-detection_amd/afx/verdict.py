"""Per-stream verdicts on the GPU: the scores of the streaming scorers smoothed, held against two thresholds with confirm
and release run lengths, and the raise / clear events kept in a device log.

The scorers hand back one fp32 bonafide score per slot per hop.  ``VerdictScorer(scorer, policy)`` turns them into the
answer a caller acts on -- is this stream in alarm, since when, what happened -- without reading a score back: the state is
per slot on the device, one ``afx_k_verdict`` launch per push advances it, and the only read-back is ``take_events()``.
``Verdicts(S, policy, device)`` is the state and the log on their own, for a caller with scores of another origin;
``Timeline.alarms(policy)`` is the offline counterpart.

The function (also stated in include/afx.h).  ``VerdictPolicy(enter, exit, alpha, confirm, release, min_scores, latch,
verifier_enter)``: the thresholds and ``alpha`` are rounded to fp32 once.  Per slot the state is ``m`` (fp32, the smoothed
score, NaN for a new stream) and ``(n, run, on, since)`` (int32; (0, 0, 0, -1) for a new stream): the scores taken
(saturating at 2^31 - 1), the current run length, 0 for clear / 1 for alarm, and the hop index at which the current alarm was
raised (-1 while clear).  An update names rows i = 0..A-1: row i has slot b_i (distinct), the bonafide score s_i (fp32, low
means spoof), the hop index k_i (int32: the host's ``samples_seen // hop`` after this hop) and optionally v_i (fp32), the
verifier's score of this slot in this push, NaN if none.  All compares are fp32 and every arithmetic operation is a single
correctly rounded fp32 operation (no fma)::

    if isnan(s_i): the row changes nothing and logs nothing (a gate's "no hop completed")
    n1 = n if n == 2^31-1 else n + 1
    m1 = s_i if n == 0 else m + alpha * (s_i - m)          # sub, mul, add: three roundings
    kind = 0
    if on == 0:
        if not isnan(v_i) and v_i < verifier_enter:  on, run, since, kind = 1, 0, k_i, 2     # raised by the verifier
        elif not isnan(v_i):                         run = 0                                 # the verifier cleared this window: the run starts over
        elif n1 >= min_scores and m1 < enter:        run += 1; if run >= confirm: on, run, since, kind = 1, 0, k_i, 1
        else:                                        run = 0
    elif not latch:
        if m1 >= exit:                               run += 1; if run >= release: on, run, since, kind = 0, 0, -1, 3
        else:                                        run = 0
    m = m1; n = n1

Infinite scores follow IEEE; a NaN ``m1`` is neither ``< enter`` nor ``>= exit``.  With ``verifier_enter=None`` there is no
verifier column: every v_i is NaN.  While an alarm is on the verifier plays NO part: a verifier score above its threshold does
not clear an alarm.  Its veto acts before the alarm, by restarting the confirm run of a slot the screen is about to raise.

The event log.  A row with ``kind != 0`` appends one event ``(slot, kind, k_i, bits of m1)``, four int32, to a device log:
the events of one update in ascending row position, updates in order.  ``log[0]`` is the number of events since the log was
last cleared, event e sits at ``log[1 + 4e ..]``; events at or past the capacity are not stored but still counted, and the
state always advances.  Kinds: 1 raised by the smoothed score, 2 raised by the verifier, 3 cleared.

``VerdictPolicy.step_reference`` restates one update in numpy; the kernel is bit-exact to it (tests/test_gpu_verdict.py).

The defaults (``alpha=1``, ``confirm = release = min_scores = 1``, ``exit = enter``: a plain threshold on the raw score) are
engineering defaults, not tuned ones: there is no labelled speech behind them, and the score is not calibrated.
"""
import numpy as np
import torch

from ._layer import N_MAX, Field, Layer, SlotTable, fp32, hop_indices, integer, need_gpu, returned_scores, slot_count, slots_of, upload_pairs
from ._lib import call_on, check, lib, ptr

VERDICT_FORMAT = 1  # layout of the verdict part of a StreamState: import_slots refuses any other
RAISED, RAISED_BY_VERIFIER, CLEARED = 1, 2, 3


class VerdictPolicy:
    """When a stream is in alarm; see the module docstring for the function.

    enter: the alarm is raised when the smoothed score has been below it for ``confirm`` consecutive scores.  exit
    (default: ``enter``; not below it): the alarm is cleared when the smoothed score has been at or above it for ``release``
    consecutive scores.  alpha in (0, 1]: the weight of the newest score in the smoothed one (1: no smoothing).
    min_scores: no alarm is raised by the smoothed score before a stream has this many scores.  latch: an alarm is never
    cleared (until ``reset``).  verifier_enter (default None: verifier scores are ignored): a verifier score below it
    raises the alarm at once, whatever ``min_scores`` and ``confirm``; any other verifier score restarts the confirm run."""

    def __init__(self, enter, exit=None, alpha=1.0, confirm=1, release=1, min_scores=1, latch=False, verifier_enter=None):
        self.enter32 = fp32("enter", enter)
        self.exit32 = self.enter32 if exit is None else fp32("exit", exit)
        if self.exit32 < self.enter32:
            raise ValueError(f"exit {exit!r} is below enter {enter!r}")
        self.verifier_enter32 = None if verifier_enter is None else fp32("verifier_enter", verifier_enter)
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)):
            raise ValueError(f"alpha: a number, got {alpha!r}")
        self.alpha32 = np.float32(alpha)
        if not (0.0 < float(alpha) <= 1.0 and self.alpha32 > 0):
            raise ValueError(f"alpha {alpha!r}: in (0, 1] (as an fp32 number)")
        self.confirm, self.release = integer("confirm", confirm, 1), integer("release", release, 1)
        self.min_scores = integer("min_scores", min_scores, 1)
        if not isinstance(latch, (bool, np.bool_)):
            raise ValueError(f"latch: True or False, got {latch!r}")
        self.latch = bool(latch)
        self.enter, self.exit, self.alpha = float(self.enter32), float(self.exit32), float(self.alpha32)
        self.verifier_enter = None if self.verifier_enter32 is None else float(self.verifier_enter32)

    def params(self):
        """What identifies this policy (plain ints, floats and bools; verifier_enter None = verifier scores ignored)."""
        return dict(enter=self.enter, exit=self.exit, alpha=self.alpha, confirm=self.confirm, release=self.release,
                    min_scores=self.min_scores, latch=self.latch, verifier_enter=self.verifier_enter)

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def step_reference(self, slots, scores, hop_index, m, st, verified=None):
        """One update in numpy.  slots (A,) distinct ints, scores (A,) fp32, hop_index an int or (A,) ints, verified (A,)
        fp32 or None; ``m`` (S,) float32 and ``st`` (S, 4) integer numpy arrays are the state and are UPDATED IN PLACE (the
        rows of slots not named are not written).  -> the events, a list of ``(slot, kind, hop_index, bits of m1 as an
        int32)`` in ascending row position."""
        if not (isinstance(m, np.ndarray) and m.dtype == np.float32 and m.ndim == 1 and isinstance(st, np.ndarray)
                and np.issubdtype(st.dtype, np.integer) and st.shape == (m.size, 4)):
            raise ValueError("m: a (S,) float32 array, st: a (S, 4) integer array")
        b = slots_of(slots, m.size)
        s = np.asarray(scores, dtype=np.float32).reshape(-1)
        k = np.broadcast_to(np.asarray(hop_index, dtype=np.int64).reshape(-1), b.shape) if np.ndim(hop_index) == 0 \
            else np.asarray(hop_index, dtype=np.int64).reshape(-1)
        v = np.full(b.size, np.nan, dtype=np.float32)
        if verified is not None and self.verifier_enter32 is not None:
            v = np.asarray(verified, dtype=np.float32).reshape(-1)
        if not (b.size == s.size == k.size == v.size):
            raise ValueError("slots, scores, hop_index and verified name the same rows")
        live = ~np.isnan(s)
        mo, n, run, on, since = m[b], st[b, 0].astype(np.int64), st[b, 1].astype(np.int64), st[b, 2].astype(np.int64), st[b, 3].astype(np.int64)
        n1 = np.where(n == N_MAX, n, n + 1)
        with np.errstate(invalid="ignore", over="ignore"):
            d = s - mo                       # three fp32 array operations: one rounding each
            p = self.alpha32 * d
            m1 = np.where(n == 0, s, mo + p).astype(np.float32)
            hv = ~np.isnan(v)
            clear = on == 0
            by_v = clear & hv & (v < (self.verifier_enter32 if self.verifier_enter32 is not None else np.float32(0)))
            below = clear & ~hv & (n1 >= self.min_scores) & (m1 < self.enter32)
            above = (on != 0) & (not self.latch) & (m1 >= self.exit32)
        run1 = np.where(below | above, run + 1, 0)
        if self.latch:
            run1 = np.where(on != 0, run, run1)  # a latched alarm: the run is not touched
        raised = below & (run1 >= self.confirm)
        cleared = above & (run1 >= self.release)
        run1 = np.where(by_v | raised | cleared, 0, run1)
        kind = np.where(by_v, RAISED_BY_VERIFIER, np.where(raised, RAISED, np.where(cleared, CLEARED, 0)))
        up = by_v | raised
        on1 = np.where(up, 1, np.where(cleared, 0, on))
        since1 = np.where(up, k, np.where(cleared, -1, since))
        rows = b[live]
        m[rows] = m1[live]
        st[rows] = np.stack([n1, run1, on1, since1], axis=1)[live].astype(st.dtype)
        bits = m1.view(np.int32)
        return [(int(b[i]), int(kind[i]), int(k[i]), int(bits[i])) for i in np.flatnonzero(live & (kind != 0))]

    def run_reference(self, scores, hop_index=None):
        """One fresh stream over a score sequence (NaN: no score at that position) -> (events as ``step_reference`` gives
        them with slot 0, the ``on`` flag after every score as a list of bools).  hop_index: the hop index of each score
        (default 1, 2, ...: a stream scored at every hop from its start)."""
        s = np.asarray(scores, dtype=np.float32).reshape(-1)
        k = np.arange(1, s.size + 1) if hop_index is None else np.asarray(hop_index, dtype=np.int64).reshape(-1)
        if k.size != s.size:
            raise ValueError("one hop index per score")
        m, st = new_state(1)
        events, on = [], []
        for j in range(s.size):
            events += self.step_reference([0], s[j:j + 1], int(k[j]), m, st)
            on.append(bool(st[0, 2]))
        return events, on


def new_state(S):
    """The state of S new streams as numpy arrays: m (S,) float32 of NaN, st (S, 4) int32 of (0, 0, 0, -1)."""
    st = np.zeros((S, 4), dtype=np.int32)
    st[:, 3] = -1
    return np.full(S, np.nan, dtype=np.float32), st


class Verdicts(SlotTable):
    """The per-slot verdict state of ``S`` streams under ``policy`` on ``device``, and the event log; see the module
    docstring.  ``update`` is one pinned upload of the header and one ``afx_k_verdict`` launch, with no synchronisation;
    ``alarm`` / ``smoothed`` / ``alarm_since`` are views of the state on the device; ``take_events()`` is the only
    read-back.

    The log holds ``cap = max(4 S, 1024)`` events.  The host keeps an upper bound on the events not yet taken (the sum of A
    over the updates since the last take); when the next update could overflow the log, the host takes the events itself
    before launching and keeps them for the caller: no event is lost, and a caller who never collects pays one read-back
    every few pushes."""

    def __init__(self, S, policy, device="cuda"):
        self.policy = policy
        self._allocate(slot_count(S, policy, VerdictPolicy), device, Field("verdict_m", "m", (), torch.float32, new=float("nan")),
                       Field("verdict_state", "st", (4,), torch.int32, host=True, new=(0, 0, 0, -1)))
        self.cap = max(4 * self.S, 1024)
        self.log = torch.zeros(1 + 4 * self.cap, dtype=torch.int32, device=self.device)
        self._pending = 0  # upper bound on log[0]: the rows of the updates since the log was last cleared
        self._kept = []    # events the host took itself before an overflow, (n, 4) int32 arrays in log order

    # ---- views ---------------------------------------------------------------------------------------------------------------
    @property
    def alarm(self):
        """(S,) bool on the device: which slots are in alarm."""
        return self.st[:, 2] != 0

    @property
    def smoothed(self):
        """(S,) fp32 on the device: the smoothed score of each slot, NaN before its first score."""
        return self.m

    @property
    def alarm_since(self):
        """(S,) int32 on the device: the hop index at which each slot's current alarm was raised, -1 while clear."""
        return self.st[:, 3]

    # ---- the update ------------------------------------------------------------------------------------------------------
    def update(self, scores, slots=None, *, hop_index, verified=None):
        """scores: (A,) fp32 on the device (any stride: a column of a logits matrix is read in place), row i the score of
        slot slots[i] (None: every slot, in order; the slots are distinct); hop_index: an int or (A,) ints on the host;
        verified: (A,) fp32 on the device, NaN where the verifier gave no score (ignored when the policy has no
        ``verifier_enter``).  One pinned upload, one launch, no synchronisation."""
        b = slots_of(slots, self.S)
        A = b.size
        if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.shape != (A,) or scores.device != self.device:
            raise ValueError(f"scores: an fp32 tensor of shape {(A,)} on {self.device}")
        k = hop_indices(hop_index, A, 0)
        if self.policy.verifier_enter32 is None:
            verified = None
        if verified is not None and (not isinstance(verified, torch.Tensor) or verified.dtype != torch.float32
                                     or verified.shape != (A,) or verified.device != self.device):
            raise ValueError(f"verified: an fp32 tensor of shape {(A,)} on {self.device}")
        if not A:
            return
        if self._pending + A > self.cap:  # this update could overflow the log: take what is there first
            ev = self._drain()
            if ev.shape[0]:
                self._kept.append(ev)
        self._launch(scores, None if verified is None else verified.contiguous(), b, k)
        self._pending += A

    def _launch(self, scores, verified, slots, hop_index):
        need_gpu(self.device, "verdicts are updated")
        p, A = self.policy, slots.size
        if A > 1 and scores.stride(0) < 1:  # (an expanded or reversed view: the kernel reads scores[i * stride], stride >= 1)
            scores = scores.contiguous()
        with torch.cuda.device(self.device):
            d = upload_pairs(slots, hop_index, self.device)
            check(call_on(self.m, lib().afx_k_verdict, ptr(scores), max(scores.stride(0), 1), ptr(verified), ptr(d), A, ptr(self.m),
                          ptr(self.st), self.S, p.alpha, p.enter, p.exit, 0.0 if p.verifier_enter is None else p.verifier_enter,
                          p.confirm, p.release, p.min_scores, int(p.latch), ptr(self.log), self.cap))

    # ---- the log -------------------------------------------------------------------------------------------------------------
    def _drain(self):
        """Reads the log back ((n, 4) int32, in log order) and clears it on the same stream."""
        if not self._pending:  # nothing was launched since the log was cleared
            return np.zeros((0, 4), dtype=np.int32)
        bound = min(self._pending, self.cap)
        src = self.log[:1 + 4 * bound]
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                host = torch.empty(src.shape, dtype=torch.int32, pin_memory=True)
                host.copy_(src, non_blocking=True)
                self.log[:1].zero_()
                torch.cuda.current_stream(self.device).synchronize()
        else:
            host = src.clone()
            self.log[:1].zero_()
        self._pending = 0  # (the device count is cleared either way: the bound follows it)
        h = host.numpy()
        total = int(h[0])
        if total > bound or total < 0:
            raise RuntimeError(f"the verdict log counts {total} events for at most {bound}: events were lost")
        return h[1:1 + 4 * total].reshape(-1, 4).copy()

    def take_events(self):
        """The events since the last call, in log order: host arrays ``(slot, kind, hop_index, smoothed)`` ((n,) int32,
        int32, int32, float32; kind 1 raised, 2 raised by the verifier, 3 cleared; ``smoothed`` the smoothed score at the
        event).  The one read-back of this layer; the log is cleared on the same stream."""
        ev = np.concatenate(self._kept + [self._drain()], axis=0)
        self._kept = []
        return ev[:, 0].copy(), ev[:, 1].copy(), ev[:, 2].copy(), ev[:, 3].copy().view(np.float32)

    # ---- sessions ------------------------------------------------------------------------------------------------------------
    # (``reset``: ``m = NaN``, ``(n, run, on, since) = (0, 0, 0, -1)``; the log is untouched)
    def check_rows(self, rows, n, seen):
        """Refuses (ValueError) what cannot be the state of n sessions under this policy; -> (m, st) on the host."""
        self.check_shapes(rows, n)
        m, st = rows[0].cpu(), rows[1].cpu()
        cnt, run, on, since = st.unbind(1)
        p = self.policy
        if bool(((on != 0) & (on != 1)).any()):
            raise ValueError("import_slots: a session's alarm flag is neither 0 nor 1")
        if bool(((cnt < 0) | (cnt > N_MAX)).any()):
            raise ValueError("import_slots: a session's score count is negative (or beyond 2^31 - 1)")
        limit = torch.where(on == 1, torch.tensor(p.release), torch.tensor(p.confirm))
        if bool(((run < 0) | (run >= limit)).any()):
            raise ValueError(f"import_slots: a session's run is outside [0, {p.confirm}) while clear or [0, {p.release}) in alarm")
        if bool(((since >= 0) != (on == 1)).any()) or bool(((since < -1) | (since > N_MAX)).any()):
            raise ValueError("import_slots: a session's alarm_since is set without an alarm, or an alarm has none")
        if bool((torch.isnan(m) != (cnt == 0)).any()):
            raise ValueError("import_slots: a session's smoothed score is NaN after a score, or a number before the first")
        return m, st


class VerdictScorer(Layer):
    """``scorer`` (whatever stands below the verdict layer in the stack order of ``afx._layer``; a quality layer's withheld
    scores are NaN rows, which change nothing) with the verdict layer behind it under ``policy``; see the module docstring.
    It presents the surface the fronts and the gate drive an inner scorer through and goes where the cascade goes:
    ``JitterScorer(GatedScorer(VerdictScorer(CascadeScorer(...), policy)), 8000, "mulaw", depth)``.

    ``push`` returns exactly what the inner ``push`` returns (a KV-cached ``None`` updates nothing), then updates the
    verdicts with ``hop_index = samples_seen // hop``: one small upload and one launch, no synchronisation.  With a
    ``CascadeScorer`` below and a policy with ``verifier_enter``, the verifier scores of this push go with it (read from
    the inner ``last_verified()`` on the device; the cascade's own event log is left for its caller).

    Results: ``alarm`` ((S,) bool), ``smoothed`` ((S,) fp32), ``alarm_since`` ((S,) int32), all on the device, and
    ``take_events()``, the only read-back.  The event log belongs to the scorer, not to a session: ``reset`` and session
    moves leave it.

    Sessions: the part of a ``StreamState`` is ``verdict_m`` ((n,) fp32) and ``verdict_state`` ((n, 4) int64: n, run, on,
    since), meta ``verdict`` (format) and ``verdict_policy``; rows that cannot be a session's under this policy are
    refused."""

    layer = "verdict"
    _part = "verdict part (it was not exported by a VerdictScorer)"

    def __init__(self, scorer, policy):
        super().__init__(scorer)
        self.policy = policy
        self.verdicts = self._own(Verdicts(scorer.S, policy, scorer.device))
        # (a quality layer in between hands the verifier scores on)
        self._verified = self._below("cascade") is not None and policy.verifier_enter is not None

    @property
    def alarm(self):
        return self.verdicts.alarm

    @property
    def smoothed(self):
        return self.verdicts.smoothed

    @property
    def alarm_since(self):
        return self.verdicts.alarm_since

    def take_events(self):
        """``Verdicts.take_events``: host arrays ``(slot, kind, hop_index, smoothed)`` in log order; the only read-back."""
        return self.verdicts.take_events()

    def push(self, chunk, slots=None):
        """chunk and slots: the inner scorer's own rule -> exactly what the inner ``push`` returns; then one
        ``Verdicts.update`` over the named slots (none when the inner scorer emitted no score)."""
        need_gpu(self.device, "hops are scored and judged")
        inner = self.scorer
        scores = inner.push(chunk, slots)
        if scores is None:
            return None
        idx = self._named(slots)
        A = len(idx)
        if not A:
            return scores
        returned_scores(scores, A, self.device)
        verified = None
        last = inner.last_verified() if self._verified else None
        if last is not None:  # this push verified something: its scores, by row
            chosen, v = last
            row_of = {s: i for i, s in enumerate(idx)}
            with torch.cuda.device(self.device):
                rows = torch.empty(chosen.numel(), dtype=torch.int64, pin_memory=True)
                rows.numpy()[:] = [row_of[int(s)] for s in chosen.tolist()]
                verified = torch.full((A,), float("nan"), dtype=torch.float32, device=self.device)
                verified.index_copy_(0, rows.to(self.device, non_blocking=True), v)
        self.verdicts.update(scores, idx, hop_index=(inner.samples_seen[idx] // self.hop).numpy(), verified=verified)
        return scores

    # ---- sessions (afx._layer.Layer) -----------------------------------------------------------------------------------------
    def _meta(self):
        return dict(verdict=VERDICT_FORMAT, verdict_policy=self.policy.params())

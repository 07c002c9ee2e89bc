"""Cascade of the two models in streaming: the cheap screen scores every slot at every hop, the verifier re-scores the
current window of the slots whose screen score looks suspicious.

The distilled student keeps up with thousands of streams, the XLS-R + AASIST teacher carries the reference's accuracy at a
quarter of them.  ``CascadeScorer(screen, verifier, policy)`` runs the screen (one of the three streaming scorers) on every
push and hands the verifier a batch of at most ``budget`` windows per push, chosen on the GPU: ``afx_k_cascade_store`` keeps
the audio (only where the screen keeps no sample ring of its own), ``afx_k_cascade_select`` ranks the candidates and advances
the per-slot cooldown, ``afx_k_cascade_windows`` gathers the chosen slots' windows.  The cascade never changes a screen score.

The function (also stated in include/afx.h).  ``CascadePolicy(threshold, budget, cooldown, min_samples)``: ``threshold`` is
rounded to fp32 once.  Per slot the state is ``wait``, an int32 that is 0 for a new stream.  A push names rows i = 0..A-1:
row i has slot b_i (distinct), the screen's bonafide score s_i (fp32) and ``elig_i = samples_seen[b_i] after this hop >=
min_samples``.  Then, with fp32 compares::

    cand_i   = elig_i and wait[b_i] == 0 and (s_i < threshold)     # NaN: false; threshold = +inf: every finite or -inf score
    before(j, i) = s_j < s_i or (not (s_i < s_j) and b_j < b_i)     # ties, -0.0 / +0.0 included, go to the lower slot
    rank_i   = number of candidates j with before(j, i)
    chosen_i = cand_i and rank_i < budget
    wait[b_i] = cooldown if chosen_i else max(wait[b_i] - 1, 0)     # named slots only; every other slot's wait is untouched

The selection list is the chosen rows in ascending rank; it depends on the set of (slot, score, elig, wait), not on the order
in which the rows were named.  This policy has NO ageing: a candidate the budget passed over keeps ``wait == 0`` and competes
again at its next hop, with no credit for having waited, so a slot whose score stays just under the threshold can be passed
over for as long as ``budget`` lower scores turn up.  ``CascadePolicy.select_reference`` restates the selection in numpy.

The window of a chosen slot.  The slot has seen ``n_seen`` samples since its reset, counting this hop.  With ``n =
min(n_seen, window)`` and ``h[0..n)`` its last n samples, oldest first, ``W[j] = h[j mod n]`` for j < window: the reference's
pad-by-tiling policy, ``afx_k_tile_crop``'s function with start 0, what ``SlidingWindowScorer`` gives the screen.

The verified score is ``verifier.forward(W[None])[0, 1]``, bit for bit: every kernel behind a score is row-wise and
accumulates a row in one order whatever the batch (afx/streaming.py), so verifying several windows in one batch does not
change the bits.

The one read-back.  How many windows the verifier is given depends on the scores, so a push copies ``sel`` ((1 + budget)
int32: the count, then the chosen rows) to pinned host memory and waits for it, once.  A push whose screen emitted no score
(a KV-cached hop that completed no frame) stores the audio and selects nothing: no ``wait`` moves.
"""
import numpy as np
import torch

from ._layer import Layer, _on, fp32, integer, need_gpu, rows_on, sample_cols, slot_count
from ._lib import call_on, check, lib, ptr
from .streaming import weights_fingerprint

CASCADE_FORMAT = 1  # layout of the cascade part of a StreamState: import_slots refuses any other
MAX_BUDGET = 1024
MIN_CLIP = 400      # the shortest clip the engines take (one SSL frame)
_STATE_KEYS = ("cascade_wait", "cascade_verified", "cascade_verified_at")
_RING_KEY = "cascade_samples"


class CascadePolicy:
    """Which slots the verifier looks at; see the module docstring for the function.

    threshold: an fp32 number or +inf (rounded to fp32 once; NaN and -inf are refused): a slot is a candidate when its
    screen score is below it.  budget (1..1024): at most this many windows are verified per push.  cooldown (>= 0): the
    hops of a slot after a verification during which it is not verified again.  min_samples (default: the scorer's
    window; 400..window): a slot is eligible once it has seen this many samples."""

    def __init__(self, threshold, budget, cooldown=0, min_samples=None):
        self.threshold32 = fp32("threshold", threshold)
        if self.threshold32 == -np.inf:
            raise ValueError(f"threshold {threshold!r}: an fp32 number or +inf")
        self.threshold = float(self.threshold32)
        self.budget, self.cooldown = integer("budget", budget, 1, MAX_BUDGET), integer("cooldown", cooldown, 0)
        self.min_samples = None if min_samples is None else integer("min_samples", min_samples, MIN_CLIP)  # (the shortest clip the engines take)

    def params(self):
        """What identifies this policy (plain ints and floats; min_samples None = the scorer's window)."""
        return dict(threshold=self.threshold, budget=self.budget, cooldown=self.cooldown, min_samples=self.min_samples)

    # ---- the numpy restatement -------------------------------------------------------------------------------------------
    def select_reference(self, slots, scores, elig, wait):
        """The selection in numpy.  slots (A,) distinct ints, scores (A,) fp32, elig (A,) bool, wait (S,) ints (not
        modified) -> (the chosen row positions in ascending rank, as a list; wait after the push, (S,) int64)."""
        b = np.asarray(slots, dtype=np.int64).reshape(-1)
        s = np.asarray(scores, dtype=np.float32).reshape(-1)
        e = np.asarray(elig, dtype=bool).reshape(-1)
        w = np.array(wait, dtype=np.int64).reshape(-1)
        if not (b.size == s.size == e.size):
            raise ValueError("slots, scores and elig name the same rows")
        if b.size and (b.min() < 0 or b.max() >= w.size or np.unique(b).size != b.size):
            raise ValueError("slots: distinct indices into wait")
        with np.errstate(invalid="ignore"):
            cand = e & (w[b] == 0) & (s < self.threshold32)
            ci = np.flatnonzero(cand)
            sc, bc = s[ci], b[ci]
            lt = sc[:, None] < sc[None, :]  # lt[j, i] = s_j < s_i
            before = lt | (~lt.T & (bc[:, None] < bc[None, :]))
        rank = before.sum(axis=0)
        chosen = np.zeros(b.size, dtype=bool)
        chosen[ci[rank < self.budget]] = True
        order = ci[np.argsort(rank, kind="stable")]
        sel = [int(i) for i in order if chosen[i]]
        w[b] = np.where(chosen, self.cooldown, np.maximum(w[b] - 1, 0))
        return sel, w


def _verifier_device(v):
    d = getattr(v, "device", None)
    if d is None and hasattr(v, "parameters"):
        p = next(iter(v.parameters()), None)
        d = None if p is None else p.device
    return None if d is None else torch.device(d)


class CascadeScorer(Layer):
    """``screen`` (a SlidingWindowScorer, IncrementalScorer or KVCachedScorer: the cascade is the first layer of the stack
    order of ``afx._layer``) with ``verifier`` (an Engine, or a drop-in model, with ``forward((B, window)) -> (B, 2)`` on
    the screen's device) behind it under ``policy``; see the module docstring for the contract.  ``state_dict``: the
    verifier's weights, for the fingerprint session moves compare (default: ``verifier.state_dict()`` when it has one).

    It presents the surface the fronts and the gate drive an inner scorer through and goes innermost:
    ``JitterScorer(GatedScorer(CascadeScorer(screen, teacher, policy)), 8000, "mulaw", depth)``; both models then see the
    same gated stream.

    Results: ``verified`` ((S,) fp32 on the device: the latest verifier score of each slot since its reset, NaN if none),
    ``verified_at`` ((S,) int64 on the host: the slot's ``samples_seen`` at that verification, -1 if none),
    ``take_events()`` and ``stats()``.

    Sessions: the part of a ``StreamState`` is ``cascade_wait`` ((n,) int64, 0..cooldown), ``cascade_verified`` ((n,) fp32),
    ``cascade_verified_at`` ((n,) int64, at most the session's samples) and, when the cascade owns the ring,
    ``cascade_samples`` ((n, window) fp32: the last min(seen, window) samples, oldest first, zeros after, the layout of the
    sliding scorer's ``samples``); meta ``cascade`` (format), ``cascade_policy`` and ``cascade_verifier``."""

    layer = "cascade"
    _part = "cascade part (it was not exported by a CascadeScorer of this kind)"

    def __init__(self, screen, verifier, policy, state_dict=None):
        super().__init__(screen)
        slot_count(screen.S, policy, CascadePolicy)
        if not (hasattr(verifier, "forward") or callable(verifier)):
            raise ValueError("verifier: an Engine or a model with forward((B, window)) -> (B, 2)")
        if policy.budget > screen.S:
            raise ValueError(f"a budget of {policy.budget} windows per push for {screen.S} slots")
        self.min_samples = screen.window if policy.min_samples is None else policy.min_samples
        if not MIN_CLIP <= self.min_samples <= screen.window:
            raise ValueError(f"min_samples {self.min_samples}: {MIN_CLIP} to the window, {screen.window}")
        vd = _verifier_device(verifier)
        if vd is not None and (vd.type != screen.device.type or (vd.index is not None and screen.device.index is not None
                                                                  and vd.index != screen.device.index)):
            raise ValueError(f"the verifier is on {vd}, the screen on {screen.device}")
        self.verifier, self.policy = verifier, policy
        self._weights, self._fingerprint = state_dict, None
        dev, S, B = screen.device, screen.S, policy.budget
        # the retained audio: the screen's own sample ring where it keeps one (same layout, read in place), else a second ring
        self.hist = None if screen.ring is not None else torch.zeros(S, screen.window, dtype=torch.float32, device=dev)
        self._keys = _STATE_KEYS + ((_RING_KEY,) if self.hist is not None else ())
        self.wait = torch.zeros(S, dtype=torch.int32, device=dev)
        self.verified = torch.full((S,), float("nan"), dtype=torch.float32, device=dev)
        self.verified_at = torch.full((S,), -1, dtype=torch.int64)
        self._counts = torch.zeros(S, 2, dtype=torch.int32, device=dev)  # per slot: candidates, candidates passed over
        self._screened = np.zeros(S, dtype=np.int64)
        self._verifications = np.zeros(S, dtype=np.int64)
        self._sel = torch.zeros(1 + B, dtype=torch.int32, device=dev)
        self._batch = torch.empty(B, screen.window, dtype=torch.float32, device=dev)
        self._sel_host = None  # (pinned, on the first push: a scorer on the host can be built and moved, not pushed)
        self._events = []
        self._last = None  # (slots, verifier scores) of the newest push, None when it verified nothing

    @property
    def screen(self):
        """The inner scorer, by the name this layer has for it."""
        return self.scorer

    def _ring(self):
        return self.hist if self.hist is not None else self.screen.ring

    def push(self, chunk, slots=None):
        """chunk: (S, hop) fp32 on the GPU, or (len(slots), hop) with ``slots`` (the screen's own rule for both) ->
        exactly what ``screen.push`` returns.  Then: ``afx_k_cascade_store`` (only when the cascade owns the ring),
        ``afx_k_cascade_select``, ``afx_k_cascade_windows``, ONE read-back of ``sel`` and, when it names n > 0 rows,
        ``verifier.forward`` on the n windows; the results go to ``verified``, ``verified_at`` and the event log."""
        scr = self.screen
        idx = self._named(slots)
        dev, hop, window, A = self.device, self.hop, self.window, len(idx)
        need_gpu(dev, "hops are screened, selected and verified")
        if (not isinstance(chunk, torch.Tensor) or not chunk.is_cuda or chunk.device != dev or chunk.dtype != torch.float32
                or chunk.shape != (A, hop)):
            raise ValueError(f"expected a CUDA fp32 tensor of shape {(A, hop)} on {dev} (one hop per named slot)")
        self._last = None
        scores = scr.push(chunk, None if slots is None else idx)
        if not A:
            return scores
        slot = np.asarray(idx, dtype=np.int64)
        seen = scr._seen[idx].numpy()  # (counts this hop)
        own = self.hist is not None
        with torch.cuda.device(dev):
            # one pinned upload: the store table (slot, wpos) when the ring is ours, then select's (slot, elig), then
            # windows' (slot, n, start)
            o_sel = 2 * A if own else 0
            hdr = torch.empty(o_sel + 5 * A, dtype=torch.int32, pin_memory=True)
            h = hdr.numpy()
            if own:
                h[:o_sel] = np.stack([slot, (seen - hop) % window], axis=1).reshape(-1)
            h[o_sel:o_sel + 2 * A] = np.stack([slot, seen >= self.min_samples], axis=1).reshape(-1)
            n = np.minimum(seen, window)
            h[o_sel + 2 * A:] = np.stack([slot, n, np.where(seen >= window, seen % window, 0)], axis=1).reshape(-1)
            d = hdr.to(dev, non_blocking=True)
            if own:
                check(call_on(self.hist, lib().afx_k_cascade_store, ptr(chunk.contiguous()), A, hop, ptr(d), ptr(self.hist),
                              self.S, window))
            if scores is None:
                return None
            if scores.shape != (A,) or scores.device != dev:
                raise RuntimeError(f"the screen returned {tuple(scores.shape)} scores on {scores.device} for {A} rows")
            s32 = scores if scores.dtype == torch.float32 else scores.to(torch.float32)
            p = self.policy
            check(call_on(self.wait, lib().afx_k_cascade_select, ptr(s32), s32.stride(0) or 1, ptr(d[o_sel:]), A, ptr(self.wait),
                          ptr(self._counts), self.S, p.threshold, p.budget, p.cooldown, ptr(self._sel)))
            check(call_on(self.wait, lib().afx_k_cascade_windows, ptr(self._ring()), self.S, window, ptr(d[o_sel + 2 * A:]), A,
                          ptr(self._sel), p.budget, ptr(self._batch)))
            if self._sel_host is None:
                self._sel_host = torch.empty(1 + p.budget, dtype=torch.int32, pin_memory=True)
            self._sel_host.copy_(self._sel, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()  # the one read-back: the verifier's batch size is in the scores
            self._screened[slot] += 1
            k = int(self._sel_host[0])
            if k:
                rows = self._sel_host[1:1 + k].numpy().astype(np.int64)
                out = self.verifier.forward(self._batch[:k]) if hasattr(self.verifier, "forward") else self.verifier(self._batch[:k])
                v = out[:, 1].to(torch.float32).clone()
                chosen, at = torch.from_numpy(slot[rows]), torch.from_numpy(seen[rows].astype(np.int64))
                self.verified.index_copy_(0, chosen.to(dev), v)
                self.verified_at[chosen] = at
                self._verifications[slot[rows]] += 1
                self._events.append((chosen, at, s32.index_select(0, self._sel[1:1 + k].long()), v))
                self._last = (chosen, v)
        return scores

    def last_verified(self):
        """What the newest ``push`` verified: ``(slots (n,) int64 host, verifier_scores (n,) fp32 device)`` in rank order,
        or None when it verified nothing.  The event log is not touched: a layer above reads this and leaves
        ``take_events()`` to the caller."""
        return self._last

    def take_events(self):
        """One entry per push since the last call that verified something: ``(slots (n,) int64 host, at (n,) int64 host,
        screen_scores (n,) fp32 device, verifier_scores (n,) fp32 device)`` in rank order; ``at`` is the slot's
        ``samples_seen`` at the verification.  A front may run several pushes per ``feed``: the log shows all of them."""
        ev, self._events = self._events, []
        return ev

    def stats(self):
        """Per slot, since the scorer was built (a ``reset`` and a session move leave them): (S,) int64 host tensors
        ``screened`` (hops that got a screen score), ``candidates``, ``verified`` and ``passed_over`` (candidates the
        budget passed over).  Reads two counters back from the device."""
        c = self._counts.cpu().to(torch.int64)
        return dict(screened=torch.from_numpy(self._screened.copy()), candidates=c[:, 0].clone(),
                    verified=torch.from_numpy(self._verifications.copy()), passed_over=c[:, 1].clone())

    def _reset(self, idx):
        """``wait = 0``, ``verified = NaN``, ``verified_at = -1``; the retained audio starts over with the session's sample count."""
        if idx:
            with _on(self.device):
                rows = rows_on(idx, self.device)
                self.wait[rows] = 0
                self.verified[rows] = float("nan")
            self.verified_at[idx] = -1

    # ---- sessions ------------------------------------------------------------------------------------------------------------
    def _verifier_fingerprint(self):
        if self._fingerprint is None:
            sd = self._weights
            if sd is None:
                if not hasattr(self.verifier, "state_dict"):
                    raise ValueError("the verifier has no state_dict(): build the CascadeScorer with state_dict= (the weights "
                                     "the verifier was loaded with) to move its sessions")
                sd = self.verifier.state_dict()
            self._fingerprint = weights_fingerprint(sd)
        return self._fingerprint

    def _meta(self):
        v = self.verifier
        dt = getattr(v, "dtype", None)
        return dict(cascade=CASCADE_FORMAT, cascade_policy=dict(self.policy.params(), min_samples=self.min_samples),
                    cascade_verifier=dict(arch=getattr(v, "arch", type(v).__name__), dtype=dt if dt is None or isinstance(dt, str) else str(dt),
                                          fingerprint=self._verifier_fingerprint()))

    def _export(self, idx, st):
        with _on(self.device):
            rows = rows_on(idx, self.device)
            tensors = dict(cascade_wait=self.wait[rows].to("cpu", torch.int64), cascade_verified=self.verified[rows].clone(),
                           cascade_verified_at=self.verified_at[idx].clone())
            if self.hist is not None:
                cols, m = sample_cols(st.seen, self.window, self.device)
                smp = self.hist[rows[:, None], cols]
                smp.masked_fill_(torch.arange(self.window, device=self.device)[None, :] >= m, 0.0)
                tensors[_RING_KEY] = smp
        return tensors

    def _check(self, state, n):
        t = state.tensors
        for k in ("cascade_wait", "cascade_verified_at"):
            if t[k].dtype != torch.int64 or tuple(t[k].shape) != (n,):
                raise ValueError(f"import_slots: {k} is (n,) int64")
        wait, at = t["cascade_wait"].cpu(), t["cascade_verified_at"].cpu()
        ver = t["cascade_verified"]
        if ver.dtype != torch.float32 or tuple(ver.shape) != (n,):
            raise ValueError("import_slots: cascade_verified is (n,) float32")
        if bool(((wait < 0) | (wait > self.policy.cooldown)).any()):
            raise ValueError(f"import_slots: a session's wait is outside 0..{self.policy.cooldown} hops")
        if bool(((at < -1) | (at > state.seen)).any()):
            raise ValueError("import_slots: a session was verified at a sample count it has not seen")
        if self.hist is not None and (t[_RING_KEY].dtype != torch.float32 or tuple(t[_RING_KEY].shape) != (n, self.window)):
            raise ValueError(f"import_slots: {_RING_KEY} {tuple(t[_RING_KEY].shape)} {t[_RING_KEY].dtype} is not {(n, self.window)} float32")
        return wait, ver, at, state.seen, t.get(_RING_KEY)

    def _import(self, idx, rows):
        wait, ver, at, seen, smp = rows
        if idx:
            with _on(self.device):
                dev_rows = rows_on(idx, self.device)
                self.wait[dev_rows] = wait.to(self.device, torch.int32)
                self.verified[dev_rows] = ver.to(self.device)
                if self.hist is not None:  # sample i of a session to column i % window: the whole row, as the sliding scorer
                    cols, _ = sample_cols(seen, self.window, self.device)
                    self.hist[dev_rows[:, None], cols] = smp.to(self.device)
            self.verified_at[idx] = at

"""What the streaming stack shares: the order in which its objects nest, how each one's part rides in a ``StreamState``,
and the argument checks of the per-slot state classes.

The stack, innermost first (``ORDER``): a streaming scorer (``SlidingWindowScorer`` and its subclasses), the cascade, the
quality layer, the provenance layer, the verdict layer, the evidence layer, the speech gate, the fronts.  Every class
carries its kind as ``layer``.  The one rule: a layer goes around any kind that stands before it in ``ORDER`` -- except a kind named in
``EXACTLY``, which goes around that one kind only (the evidence layer reads the verdict layer's state).  The fronts take
whatever presents the surface below.

``Layer`` is the base of the six layers between a scorer and the fronts: the surface a layer above drives an inner scorer
through (``S``, ``device``, ``hop``, ``window``, ``samples_seen``, ``_slot_list``, ``state_meta``), ``reset`` and the session
moves.  A layer states its ``_meta()``, its state tensors ``_keys`` and the words ``_part`` for a state that lacks them, and
four hooks: ``_export(idx, st)``, ``_check(state, n)``, ``_import(idx, rows)``, ``_reset(idx)``; and its ``push``.
"""
import contextlib
import math

import numpy as np
import torch

from ._lib import AfxError

ORDER = ("scorer", "cascade", "quality", "provenance", "verdict", "evidence", "gate", "front")
EXACTLY = {"evidence": "verdict"}

STATE_FORMAT = 1  # StreamState layout version: import_slots refuses any other
MAX_ROWS = 8192   # rows of one launch of a per-slot state kernel (cascade select, quality, provenance, verdict, evidence)
N_MAX = (1 << 31) - 1
_HOST_KEYS = ("kv_meta", "c6w")  # StreamState tensors that stay on the host whatever ``to`` is given


def _on(device):
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


def need_gpu(device, what):
    if device.type != "cuda":
        raise AfxError(f"{what} on the GPU; there is no CPU fallback")


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def integer(name, v, lo, hi=N_MAX):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name}: an integer, got {v!r}")
    v = int(v)
    if not lo <= v <= hi:
        raise ValueError(f"{name} {v!r}: {lo} to {hi}")
    return v


def fp32(name, v, positive=None):
    """``v`` rounded to fp32 once; NaN and a finite number that is not an fp32 number are refused.  ``positive`` False: a
    negative number is refused too; True: and zero.  +inf is a number."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name}: a number, got {v!r}")
    if math.isnan(v):
        raise ValueError(f"{name} is NaN")
    with np.errstate(over="ignore"):
        t = np.float32(v)
    if np.isinf(t) and not math.isinf(v):
        raise ValueError(f"{name} {v!r} is not an fp32 number")
    if positive is not None and (t < 0 or (positive and t == 0)):
        raise ValueError(f"{name} {v!r}: {'above 0' if positive else '0 or more'} (as an fp32 number)")
    return t


def slot_count(S, policy, policy_type):
    """``S``: a number of slots one launch takes; ``policy``: a ``policy_type`` -> int(S)."""
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or S < 1:
        raise ValueError(f"S {S!r}: a positive number of slots")
    if S > MAX_ROWS:
        raise ValueError(f"{S} slots: one update takes at most {MAX_ROWS} rows")
    if not isinstance(policy, policy_type):
        raise ValueError(f"policy: a {policy_type.__name__}")
    return int(S)


def slots_of(slots, S):
    """Distinct slot indices in [0, S), in the order given (None: every slot) -> (A,) int64 array."""
    if slots is None:
        return np.arange(S, dtype=np.int64)
    b = np.asarray(slots)
    if b.dtype == bool or (b.size and not np.issubdtype(b.dtype, np.integer)) or b.ndim > 1:
        raise ValueError("slots: a list of slot indices")
    b = b.astype(np.int64).reshape(-1)
    if b.size and (b.min() < 0 or b.max() >= S):
        raise ValueError(f"a slot index outside 0..{S - 1}")
    if np.unique(b).size != b.size:
        raise ValueError("a slot is named twice")
    return b


def hop_indices(hop_index, A, least=None):
    """``hop_index``: an int or A ints -> (A,) int64 array (a read-only broadcast of an int); ``least``: its lower bound
    (with the upper bound 2^31 - 1), None: any."""
    k = np.asarray(hop_index)
    if k.dtype == bool or not np.issubdtype(k.dtype, np.integer) or k.ndim > 1 or (k.ndim == 1 and k.size != A):
        raise ValueError(f"hop_index: an int or {A} ints")
    k = np.broadcast_to(k.astype(np.int64).reshape(-1), (A,))
    if least is not None and A and (k.min() < least or k.max() > N_MAX):
        raise ValueError(f"hop_index: {least} or more, below 2^31")
    return k


def upload_pairs(first, second, device):
    """The (A, 2) int32 header of an update -- (slot, hop_index) or (slot, ring position) rows -- through pinned memory to
    ``device``, without synchronisation (the caller has made ``device`` current)."""
    hdr = torch.empty(len(first), 2, dtype=torch.int32, pin_memory=True)
    hdr.numpy()[:] = np.stack([first, second], axis=1)
    return hdr.to(device, non_blocking=True)


def rows_on(idx, device):
    return torch.tensor(idx, dtype=torch.long, device=device)


# ---- rings ---------------------------------------------------------------------------------------------------------------------
def sample_cols(seen, window, device):
    """(ring columns (n, window) of each session's last min(seen, window) samples, oldest first; their count (n, 1)), on
    ``device``: sample i since a session's start sits at ring column i % window."""
    m = seen.clamp(max=window).to(device)[:, None]
    j = torch.arange(window, device=device)
    return (seen.to(device)[:, None] - m + j) % window, m


def export_pending(ring, idx, head, fill, width):
    """-> (n, width), the ring's dtype: the pending samples of the slots ``idx`` of a pending ring ((S, ring_len) fp32, or the
    uint8 ring of their provenance marks; ring heads ``head``, ``fill`` samples each: int64 arrays over idx), left-aligned,
    zeros after."""
    dev = ring.device
    with _on(dev):
        j = torch.arange(width)
        cols = (torch.from_numpy(head)[:, None] + j) % ring.shape[1]
        pend = ring[rows_on(idx, dev)[:, None], cols.to(dev)]
        return pend.masked_fill_((j[None, :] >= torch.from_numpy(fill)[:, None]).to(dev), 0.0)


def check_pending(key, pend, fill, n, most):
    """The checks of an exported pending ring ``pend`` (state tensor ``key``) with ``fill`` (n,) samples per session, at
    most ``most``."""
    if pend.ndim != 2 or pend.shape[0] != n or pend.dtype != torch.float32:
        raise ValueError(f"import_slots: {key} {tuple(pend.shape)} {pend.dtype} is not (n, pending) float32")
    if (fill < 0).any() or (fill > pend.shape[1]).any() or (fill > most).any():
        raise ValueError(f"import_slots: a session holds more than {most} pending samples (or than its own buffer)")


def import_pending(ring, idx, pend):
    """The slots ``idx`` of a pending ring take the pending samples ``pend`` (checked), at ring head 0."""
    with _on(ring.device):
        w = min(pend.shape[1], ring.shape[1])
        ring[rows_on(idx, ring.device), :w] = pend[:, :w].to(ring.device)


# ---- a layer's part of a StreamState -------------------------------------------------------------------------------------
class StreamState:
    """A copy of some slots' streaming sessions (``export_slots``), in the order they were named: ``seen`` (n,) samples per
    session, ``tensors`` the per-session state (row i = session i), ``meta`` what the sessions need of a scorer to continue
    in it (format, scorer kind, engine arch and head, dtype, layers, extractor mode, window, hop, weights fingerprint) and
    the library build id (for information)."""

    def __init__(self, meta, seen, tensors):
        self.meta = dict(meta)
        self.seen = torch.as_tensor(seen, dtype=torch.int64).cpu().reshape(-1)
        self.tensors = dict(tensors)
        for k, t in self.tensors.items():
            if t.shape[0] != len(self):
                raise ValueError(f"state tensor {k!r} has {t.shape[0]} rows for {len(self)} sessions")

    def __len__(self):
        return int(self.seen.numel())

    def to(self, device, pin_memory=False):
        """A copy on ``device`` ("cpu", "cuda:1", ...); pin_memory: host tensors in page-locked memory (device-to-host
        copies without staging, host-to-device copies that can overlap)."""
        dev = torch.device(device)
        out = {}
        for k, t in self.tensors.items():
            if k in _HOST_KEYS:
                out[k] = t
            elif dev.type == "cpu" and pin_memory:
                out[k] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                out[k].copy_(t, non_blocking=True)
            else:
                out[k] = t.to(dev)
        if dev.type == "cpu" and pin_memory:
            for d in {t.device for t in self.tensors.values() if t.is_cuda}:
                torch.cuda.current_stream(d).synchronize()
        return StreamState(self.meta, self.seen, out)

    def state_dict(self):
        """Plain tensors, strings and ints (``torch.save`` / ``torch.load(weights_only=True)``)."""
        return {"meta": dict(self.meta), "seen": self.seen.clone(), "tensors": dict(self.tensors)}

    @classmethod
    def from_state_dict(cls, d):
        if not isinstance(d, dict) or set(d) != {"meta", "seen", "tensors"}:
            raise ValueError("a StreamState state_dict has the keys 'meta', 'seen' and 'tensors'")
        if d["meta"].get("format") != STATE_FORMAT:
            raise ValueError(f"StreamState format {d['meta'].get('format')!r}, this build reads format {STATE_FORMAT}")
        return cls(d["meta"], d["seen"], d["tensors"])


def wrap(st, meta, **tensors):
    """The inner state ``st`` with a layer's or a front's own ``meta`` and ``tensors`` added."""
    return StreamState(dict(st.meta, **meta), st.seen, dict(st.tensors, **tensors))


def peel(state, state_keys, mine, what, names=None, seen=None):
    """``state`` must be a StreamState that has the tensors ``state_keys`` and the meta of ``mine`` (the caller's own, equal
    value by value; ``names``: how a message calls a key), else a ValueError -> the inner scorer's StreamState, without
    them.  ``seen``: the state tensor that holds the inner sessions' sample counts (None: they are the state's own)."""
    if not isinstance(state, StreamState):
        raise ValueError("import_slots takes a StreamState (export_slots / StreamState.from_state_dict)")
    if any(k not in state.tensors for k in state_keys) or any(k not in state.meta for k in mine):
        raise ValueError(f"import_slots: the state has no {what}")
    for k, v in mine.items():
        if state.meta[k] != v:
            raise ValueError(f"import_slots: the state's {(names or {}).get(k, k)} {state.meta[k]!r} is not this scorer's {v!r}")
    return StreamState({k: v for k, v in state.meta.items() if k not in mine}, state.seen if seen is None else state.tensors[seen],
                       {k: t for k, t in state.tensors.items() if k not in state_keys})


class Layer:
    """The base of the layers between a streaming scorer and the fronts; see the module docstring.  ``scorer`` is what
    stands directly below."""

    layer = None        # this class's kind, one of ORDER
    _keys = ()          # the state tensors of this layer's part
    _part = ""          # how a refusal calls a state without them: "the state has no ..."
    _inner_seen = None  # the state tensor that holds the inner sessions' sample counts, where they are not the state's own

    def _state_keys(self, state):
        """The state tensors of this layer's part that ``state`` must have: ``_keys``, and for a layer with an optional part
        also that part's keys where the state carries it (a part the layer cannot take is a ValueError here)."""
        return self._keys

    def __init__(self, scorer):
        below, only = getattr(scorer, "layer", None), EXACTLY.get(self.layer)
        if not isinstance(below, str) or below not in ORDER or (
                below != only if only else ORDER.index(below) >= ORDER.index(self.layer)):
            fits = only or " / ".join(ORDER[:ORDER.index(self.layer)])
            raise ValueError(f"{type(self).__name__} goes around a {fits} and inside what follows it (stack order: "
                             f"{', '.join(ORDER)}); got {type(scorer).__name__}")
        self.scorer = scorer

    # ---- the surface the layers above, the gate and the fronts use -------------------------------------------------------
    @property
    def S(self):
        return self.scorer.S

    @property
    def device(self):
        return self.scorer.device

    @property
    def hop(self):
        return self.scorer.hop

    @property
    def window(self):
        return self.scorer.window

    @property
    def samples_seen(self):
        """(S,) int64: the samples each slot's session has seen since its last ``reset`` (the inner scorer's count)."""
        return self.scorer.samples_seen

    def _slot_list(self, slots, ordered=False):
        return self.scorer._slot_list(slots, ordered=ordered)

    def _named(self, slots):
        """The slots a ``push`` names, in its row order (None: every slot)."""
        return list(range(self.S)) if slots is None else self._slot_list(slots, ordered=True)

    def _below(self, kind):
        """The layer of ``kind`` below this one, or None."""
        s = self.scorer
        while isinstance(s, Layer) and s.layer != kind:
            s = s.scorer
        return s if isinstance(s, Layer) else None

    def state_meta(self):
        return dict(self.scorer.state_meta(), **self._meta())

    def reset(self, slots):
        """The named slots begin a new stream: the inner session, then this layer's own part."""
        idx = self._slot_list(slots)
        self.scorer.reset(idx)
        self._reset(idx)

    # ---- sessions ------------------------------------------------------------------------------------------------------------
    def export_slots(self, slots):
        """The inner scorer's ``StreamState`` of the named slots plus this layer's tensors (``_export``) and meta
        (``_meta``).  No byte of the scorer changes."""
        idx = self._slot_list(slots, ordered=True)
        meta = self._meta()
        st = self.scorer.export_slots(idx)
        return wrap(st, meta, **self._export(idx, st))

    def import_slots(self, slots, state):
        """The named slots take over the sessions of ``state``, a state of this kind of layer with equal meta around the
        same kind of scorer.  Anything else, a state without this layer's part, another number of sessions or rows that
        ``_check`` refuses is a ValueError before anything changes, here or below."""
        idx = self._slot_list(slots, ordered=True)
        inner = peel(state, self._state_keys(state), self._meta(), self._part, seen=self._inner_seen)
        if len(state) != len(idx):
            raise ValueError(f"the state holds {len(state)} sessions for {len(idx)} named slots")
        rows = self._check(state, len(state))
        self.scorer.import_slots(idx, inner)  # (refuses a foreign state before changing anything)
        self._import(idx, rows)

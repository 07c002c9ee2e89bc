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

A layer whose part is per-slot tensors writes none of the four hooks.  Its state class is a ``SlotTable``: it declares
its tensors once, as ``Field`` rows in export order, and inherits their allocation, ``reset``, ``export_rows``,
``import_rows`` and the dtype and shape refusals of ``check_rows``; the layer names the table with ``_own`` and ``Layer``
derives ``_keys`` and the hooks from it (the quality, provenance, verdict and evidence layers; the cascade's part, with a
tensor on the host and a ring exported in session order, and the gate's stay written out).  What such a layer still writes
is its function: its policy and numpy reference, its ``update`` with the launch spelled out, and ``check_rows`` with the
rules only it knows (``bad > W``, "the total is the ring's sum").  ``HopTable`` adds what an update with one row per named
slot shares (the checks of ``hop_index`` and ``scores``, the header upload, the ``meas`` / ``out`` buffers), ``WindowState``
is its numpy mirror, and ``WithholdingLayer`` is the base of the two layers that hand a score on or withhold it (quality,
provenance): the whole ``push``, the verifier hand-on and the pass-throughs; a subclass states its policy, its state
class, its words for ``need_gpu`` and ``_operand``, what its update takes of a push.
"""
import collections
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


def returned_scores(scores, A, device, cast=False):
    """What an inner ``push`` returned for A rows: None, or (A,) scores on ``device`` -- fp32, or with ``cast`` of any dtype and
    made fp32 here; anything else is a RuntimeError."""
    if scores is None:
        return None
    if scores.shape != (A,) or scores.device != device or not (cast or scores.dtype == torch.float32):
        raise RuntimeError(f"the inner scorer returned {tuple(scores.shape)} {scores.dtype} scores on {scores.device} for {A} rows")
    return scores if scores.dtype == torch.float32 else scores.to(torch.float32)


# ---- per-slot state tables -------------------------------------------------------------------------------------------------
class Field(collections.namedtuple("Field", "key name shape dtype host new", defaults=(False, None))):
    """One per-slot tensor of a ``SlotTable``, (S, *shape) of ``dtype`` on the device: its ``StreamState`` key, its attribute
    name, ``host=True``: exported to the host as int64 (the default: as a clone on the device, as it is), ``new``: the row of
    a new stream, a number or a tuple (the default, None: zeros at first, and ``reset`` leaves it alone)."""


class SlotTable:
    """The per-slot tensors of a state class, declared once as ``Field`` rows in export order (``_allocate``): their
    allocation, ``reset``, the session moves and the dtype and shape refusals.  A subclass adds its ``update`` and, in
    ``check_rows``, the rules only it knows."""

    def _allocate(self, S, device, *fields):
        self.S, self._fields, self.keys, self._new = S, fields, tuple(f.key for f in fields), {}
        for f in fields:
            t = torch.zeros(S, *f.shape, dtype=f.dtype, device=device)
            device = t.device
            if f.new is not None:
                self._new[f.name] = torch.tensor(f.new, dtype=f.dtype, device=device)
                t[:] = self._new[f.name]
            setattr(self, f.name, t)
        self.device = device  # (the first tensor's, with its index: every launch of an update goes to THIS GPU)

    def reset(self, slots):
        """The named slots begin a new stream: every field with a new-stream row takes it, the others are left alone."""
        b = slots_of(slots, self.S)
        if b.size and self._new:
            with _on(self.device):
                rows = torch.from_numpy(b).to(self.device)
                for name, new in self._new.items():
                    getattr(self, name)[rows] = new

    def export_rows(self, slots):
        """-> the rows of the named slots, one tensor per field in the declared order: a clone on the device, or int64 on the
        host."""
        with _on(self.device):
            rows = torch.from_numpy(slots_of(slots, self.S)).to(self.device)
            return tuple(getattr(self, f.name)[rows].to("cpu", torch.int64) if f.host else getattr(self, f.name)[rows].clone()
                         for f in self._fields)

    def check_shapes(self, rows, n):
        """Refuses (ValueError) a row set that is not one tensor per field as ``export_rows`` gives them for n sessions."""
        for f, t in zip(self._fields, rows):
            dtype = torch.int64 if f.host else f.dtype
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n, *f.shape):
                raise ValueError(f"import_slots: {f.key} is {(n, *f.shape)} {str(dtype).split('.')[-1]}")

    def check_rows(self, rows, n, seen):
        """Refuses (ValueError) what cannot be the state of n sessions that have seen ``seen`` (n,) samples -> the rows
        ``import_rows`` takes.  Here: the dtypes and shapes; a subclass checks them first (``check_shapes``), then its own
        rules."""
        self.check_shapes(rows, n)
        return tuple(rows)

    def import_rows(self, slots, *rows):
        """The named slots take the (checked) state rows."""
        b = slots_of(slots, self.S)
        if b.size:
            with _on(self.device):
                at = torch.from_numpy(b).to(self.device)
                for f, t in zip(self._fields, rows):
                    getattr(self, f.name)[at] = t.to(self.device, f.dtype)


class HopTable(SlotTable):
    """A table that one launch per push advances, a row per named slot: what such updates share around the launch.
    ``meas_cols``: the int32 columns of a row of ``meas``."""

    meas_cols = 0

    def _hop_rows(self, A, hop_index, scores):
        """The checks of an update's ``hop_index`` (an int or A ints, 1 or more) and ``scores`` ((A,) fp32 on the device, or
        None) -> (the hop indices, the scores with a stride the kernel can read: a column is read in place)."""
        k = hop_indices(hop_index, A, 1)
        if scores is not None and (not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.shape != (A,)
                                   or scores.device != self.device):
            raise ValueError(f"scores: an fp32 tensor of shape {(A,)} on {self.device}")
        if scores is not None and A > 1 and scores.stride(0) < 1:
            scores = scores.contiguous()
        return k, scores

    def _no_rows(self, scores):
        """``(out, meas)`` of an update that names no slot."""
        out = None if scores is None else torch.empty(0, dtype=torch.float32, device=self.device)
        return out, torch.empty(0, self.meas_cols, dtype=torch.int32, device=self.device)

    def _buffers(self, slots, hop_index, scores):
        """-> (the (slot, hop_index) header on the device, ``meas``, ``out``) of a launch (the caller has made the device
        current)."""
        A = len(slots)
        return (upload_pairs(slots, hop_index, self.device), torch.empty(A, self.meas_cols, dtype=torch.int32, device=self.device),
                None if scores is None else torch.empty(A, dtype=torch.float32, device=self.device))


class WindowState:
    """Host mirrors of a ``HopTable`` of ``ring`` (S, W), ``st`` (S, k) int32 and ``totals`` (S, m) int32, a new stream
    everywhere.  A subclass states ``ring_dtype``, ``new`` (the k values of a new stream's ``st``) and ``n_totals``."""

    def __init__(self, S, W):
        self.ring = np.zeros((S, W), dtype=self.ring_dtype)
        self.st = np.tile(np.array(self.new, dtype=np.int32), (S, 1))
        self.totals = np.zeros((S, self.n_totals), dtype=np.int32)

    def reset(self, slots):
        """What the table's ``reset`` does: ``st`` a new stream's and ``totals`` cleared, the ring left alone."""
        self.st[slots] = self.new
        self.totals[slots] = 0

    def copy(self):
        c = type(self)(*self.ring.shape)
        c.ring, c.st, c.totals = self.ring.copy(), self.st.copy(), self.totals.copy()
        return c


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
    _table = None       # the ``SlotTable`` that is this layer's whole part (``_own``): ``_keys`` and the four hooks are its

    def _own(self, table):
        """``table`` is this layer's part of a ``StreamState`` -> table."""
        self._table, self._keys = table, table.keys
        return table

    def _reset(self, idx):
        self._table.reset(idx)

    def _export(self, idx, st):
        return dict(zip(self._keys, self._table.export_rows(idx)))

    def _check(self, state, n):
        return self._table.check_rows([state.tensors[k] for k in self._keys], n, state.seen)

    def _import(self, idx, rows):
        self._table.import_rows(idx, *rows)

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


class WithholdingLayer(Layer):
    """The base of the layers that hand the inner score on bit for bit or withhold it (the quiet NaN): ``push`` runs the
    inner ``push``, then one update of the layer's ``HopTable`` with ``hop_index = samples_seen // hop`` (one small upload,
    one launch, no synchronisation) and returns its ``out`` (a KV-cached ``None`` stays ``None``; the hop is measured all the
    same).  ``last_meas`` holds the ``meas`` rows of the newest push.  Around a cascade ``verified``, ``verified_at`` and
    ``take_events`` are the cascade's, and with ``abstain`` on ``last_verified()`` has NaN for the verifier scores of the
    slots that are not valid (on the device, no synchronisation).

    A subclass states ``_does`` (the words for ``need_gpu``), builds its policy and names its state class (both to
    ``__init__``) and writes ``_operand``."""

    _does = ""

    def __init__(self, scorer, policy, table_type):
        super().__init__(scorer)
        self.policy = policy
        table = self._own(table_type(scorer.S, policy, scorer.hop, scorer.window, scorer.device))
        self.last_meas = torch.empty(0, table.meas_cols, dtype=torch.int32, device=table.device)
        # what stands directly below hands the verifier scores on: the cascade, or a layer of this kind that has made its own
        # invalid slots' NaN; this layer's NaN go on top, and the verdict layer reads ``last_verified`` of what is directly below IT
        self._cascade = self._below("cascade") is not None
        self._last = None  # (slots, verifier scores with the invalid slots' made NaN) of the newest push

    @property
    def valid(self):
        return self._table.valid

    def stats(self):
        """The state's ``stats``."""
        return self._table.stats()

    # (around a cascade: its results, for the caller and for the verdict layer)
    @property
    def verified(self):
        return self.scorer.verified

    @property
    def verified_at(self):
        return self.scorer.verified_at

    def take_events(self):
        """``CascadeScorer.take_events`` (the verifier scores as the verifier gave them)."""
        return self.scorer.take_events()

    def last_verified(self):
        """``CascadeScorer.last_verified`` of the newest push; with ``abstain`` on, the verifier scores of the slots that
        are not valid are NaN."""
        return self._last

    def _operand(self, chunk, idx):
        """The first operand of the state's ``update`` for the push of ``chunk`` to the slots ``idx``; called before the
        chunk is checked and the inner scorer pushed, so what it refuses changes nothing."""
        raise NotImplementedError

    def push(self, chunk, slots=None):
        """chunk and slots: the inner scorer's own rule (an fp32 chunk on the scorer's GPU) -> the inner scores with NaN
        where the slot's score is withheld, ``None`` where the inner ``push`` returned ``None``."""
        need_gpu(self.device, self._does)
        inner, table = self.scorer, self._table
        dev = table.device
        idx = self._named(slots)
        A = len(idx)
        operand = self._operand(chunk, idx)
        if not isinstance(chunk, torch.Tensor) or chunk.device != dev or chunk.dtype != torch.float32 or chunk.shape != (A, self.hop):
            raise ValueError(f"expected a CUDA fp32 tensor of shape {(A, self.hop)} on {dev} (one hop per named slot)")
        self._last = None
        scores = inner.push(chunk, slots)
        if not A:
            return scores
        scores = returned_scores(scores, A, dev, cast=True)
        out, self.last_meas = table.update(operand, idx, hop_index=(inner.samples_seen[idx] // self.hop).numpy(), scores=scores)
        last = inner.last_verified() if self._cascade else None
        if last is not None and self.policy.abstain:
            chosen, v = last
            with torch.cuda.device(dev):
                rows = torch.empty(chosen.numel(), dtype=torch.int64, pin_memory=True)
                rows.copy_(chosen)
                ok = table.valid.index_select(0, rows.to(dev, non_blocking=True))
                last = (chosen, torch.where(ok, v, torch.full_like(v, float("nan"))))
        self._last = last
        return out

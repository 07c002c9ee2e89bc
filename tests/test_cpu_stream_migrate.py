"""Moving sessions (afx/streaming.py ``export_slots`` / ``import_slots`` / ``StreamState``) without a GPU: a host-side
SlidingWindowScorer exports and imports its sessions, the state round-trips through torch.save / torch.load, foreign
states and bad slot lists are refused before anything changes, and the library exports the new C entry points."""
import ctypes
import io
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, W, H = 4, 16000, 4000


@pytest.fixture(scope="module", autouse=True)
def built():
    """A state records the library build id: the library is built (hipcc cross-compiles gfx950 without a GPU)."""
    import __graft_entry__ as ge
    ge.build()


def _scorer(n=S, window=W, hop=H):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, n, window=window, hop=hop, device="cpu")


def _filled():
    """Slot 2: 5 hops (its ring wrapped), slot 0: 1 hop (warm-up), slots 1 and 3: none."""
    sc = _scorer()
    sc._store_slots(torch.arange(2 * H, dtype=torch.float32).reshape(2, H), [2, 0])
    for t in range(4):
        sc._store_slots(torch.full((1, H), float(t + 1)), [2])
    return sc


def _window(sc, s):
    """A slot's last min(seen, window) samples, oldest first."""
    seen = int(sc.samples_seen[s])
    m = min(seen, sc.window)
    return torch.stack([sc.ring[s, i % sc.window] for i in range(seen - m, seen)]) if m else torch.empty(0)


def test_empty_sessions_export_and_import():
    a, b = _scorer(), _scorer(3)
    st = a.export_slots([3, 1])
    assert len(st) == 2 and st.seen.tolist() == [0, 0]
    assert st.meta["kind"] == "SlidingWindowScorer" and st.meta["window"] == W and st.meta["hop"] == H
    b.import_slots([2, 0], st)
    assert b.samples_seen.tolist() == [0, 0, 0]
    assert len(a.export_slots([])) == 0


def test_sessions_keep_their_samples_in_absolute_order():
    from afx.streaming import StreamState
    a = _filled()
    ring = a.ring.clone()
    st = a.export_slots(torch.tensor([True, False, True, False]))  # a mask: ascending order
    assert st.seen.tolist() == [H, 5 * H]
    assert torch.equal(a.ring, ring) and a.samples_seen.tolist() == [H, 0, 5 * H, 0]  # export is read-only
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    back = StreamState.from_state_dict(torch.load(buf, weights_only=True))
    assert back.meta == st.meta and torch.equal(back.seen, st.seen)
    assert all(torch.equal(back.tensors[k], st.tensors[k]) for k in st.tensors)
    b = _scorer(3)
    b._store_slots(torch.full((3, H), -7.0), [0, 1, 2])  # every slot of b holds another session
    b.import_slots([1, 0], back)
    assert b.samples_seen.tolist() == [5 * H, H, H]
    assert torch.equal(_window(b, 1), _window(a, 0)) and torch.equal(_window(b, 0), _window(a, 2))
    assert torch.equal(_window(b, 2), torch.full((H,), -7.0))  # the slot that was not named
    # the next hop lands behind the imported history, as in the source
    nxt = torch.full((1, H), 9.0)
    a._store_slots(nxt, [2])
    b._store_slots(nxt, [0])
    assert torch.equal(_window(b, 0), _window(a, 2))


def test_a_scorer_compacts_its_own_slots():
    a = _filled()
    want = _window(a, 2)
    a.import_slots([1], a.export_slots([2]))
    a.reset([2])
    assert a.samples_seen.tolist() == [H, 5 * H, 0, 0]
    assert torch.equal(_window(a, 1), want)


def test_foreign_states_and_bad_slot_lists_are_refused_before_anything_changes():
    from afx.streaming import StreamState
    a = _filled()
    st = a.export_slots([0, 2])
    b = _filled()
    ring, seen = b.ring.clone(), b.samples_seen
    for other in (_scorer(window=W + H), _scorer(hop=2000)):
        with pytest.raises(ValueError):
            b.import_slots([0, 1], other.export_slots([0, 1]))
    bad = StreamState(dict(st.meta, fingerprint="0" * 32), st.seen, st.tensors)
    with pytest.raises(ValueError):
        b.import_slots([0, 1], bad)
    for key in ("format", "kind"):
        with pytest.raises(ValueError):
            b.import_slots([0, 1], StreamState(dict(st.meta, **{key: "x"}), st.seen, st.tensors))
    for slots in ([0], [0, 1, 3], [1, 1], [0, S], [-1, 0], [0.5, 1]):
        with pytest.raises(ValueError):
            b.import_slots(slots, st)
    with pytest.raises(ValueError):
        b.import_slots([0, 1], st.state_dict())  # a state_dict is not a StreamState
    with pytest.raises(ValueError):
        b.import_slots([0, 1], StreamState(st.meta, st.seen, {"samples": st.tensors["samples"][:, :W - 1]}))
    for slots in ([S], [2, 2]):
        with pytest.raises(ValueError):
            b.export_slots(slots)
    assert torch.equal(b.ring, ring) and torch.equal(b.samples_seen, seen)


def test_state_dict_checks():
    from afx.streaming import StreamState
    st = _filled().export_slots([2])
    d = st.state_dict()
    with pytest.raises(ValueError):
        StreamState.from_state_dict(dict(d, meta=dict(d["meta"], format=99)))
    with pytest.raises(ValueError):
        StreamState.from_state_dict({"meta": d["meta"]})
    with pytest.raises(ValueError):  # rows per tensor must match the session count
        StreamState(d["meta"], torch.tensor([0, 0]), d["tensors"])


def test_weights_fingerprint_follows_the_weights_only():
    from afx.streaming import weights_fingerprint
    sd = {"a.weight": torch.ones(3, 2), "b.bias": torch.zeros(2)}
    f = weights_fingerprint(sd)
    assert f == weights_fingerprint({"module." + k: v.clone() for k, v in reversed(list(sd.items()))})
    assert f != weights_fingerprint(dict(sd, **{"b.bias": torch.tensor([0.0, 1e-6])}))
    assert f != weights_fingerprint({"a.weight": torch.ones(2, 3), "b.bias": torch.zeros(2)})


def test_the_library_exports_the_migration_entry_points():
    from afx import _lib
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    assert re.search(r"#define AFX_KV_META\s+8\b", src) and _lib.KV_META == 8
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("afx_kv_slot_bytes", "afx_kv_export", "afx_kv_import"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    l = _lib.lib()
    assert l.afx_kv_slot_bytes(None) == 0
    assert l.afx_kv_export(None, None, 0, None, None, None) != 0 and b"null" in l.afx_last_error()
    assert l.afx_kv_import(None, None, 0, None, None, None) != 0

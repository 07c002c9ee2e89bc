"""The cascade on the host (afx/cascade.py): the selection function restated in numpy on hand-made cases, argument
validation of ``CascadePolicy`` and ``CascadeScorer``, and the three entry points in the header, the ctypes table and the
built library.  No GPU: the kernels are held against ``select_reference`` in tests/test_gpu_cascade.py.

One case follows the stated function rather than a looser reading of it: ``cand`` is the fp32 compare ``s < threshold``, so
a score of +inf is never below a finite threshold, and is not below ``threshold = +inf`` either (inf < inf is false): under
``+inf`` every finite or -inf score is a candidate, as the function states."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4000
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as entry
    entry.build()
    from afx import _lib
    return _lib


def _sel(policy, slots, scores, elig=None, wait=None, S=None):
    S = (max(slots) + 1 if slots else 1) if S is None else S
    elig = [True] * len(slots) if elig is None else elig
    wait = [0] * S if wait is None else wait
    sel, w = policy.select_reference(slots, np.array(scores, dtype=np.float32), elig, wait)
    return sel, w.tolist()


def _by_definition(policy, slots, scores, elig, wait):
    """The function of the module docstring, written out row by row with scalar fp32 compares."""
    thr = np.float32(policy.threshold)
    s = [np.float32(v) for v in scores]
    cand = [bool(elig[i]) and wait[slots[i]] == 0 and bool(s[i] < thr) for i in range(len(slots))]
    before = lambda j, i: bool(s[j] < s[i]) or (not bool(s[i] < s[j]) and slots[j] < slots[i])  # noqa: E731
    rank = [sum(1 for j in range(len(slots)) if cand[j] and before(j, i)) for i in range(len(slots))]
    chosen = [cand[i] and rank[i] < policy.budget for i in range(len(slots))]
    w = list(wait)
    for i, b in enumerate(slots):
        w[b] = policy.cooldown if chosen[i] else max(w[b] - 1, 0)
    return [i for _, i in sorted((rank[i], i) for i in range(len(slots)) if chosen[i])], w


def test_ties_go_to_the_lower_slot_and_zeros_of_either_sign_tie():
    from afx.cascade import CascadePolicy
    p = CascadePolicy(1.0, 2)
    # rows name slots 5, 2, 7, 0: three equal scores, the budget of 2 goes to slots 2 and 5 (rows 1, 0); slot 0's is higher
    assert _sel(p, [5, 2, 7, 0], [0.25, 0.25, 0.25, 0.5])[0] == [1, 0]
    # -0.0 and +0.0 tie: the lower slot first whatever the sign
    assert _sel(p, [3, 1], [-0.0, 0.0])[0] == [1, 0]
    assert _sel(p, [3, 1], [0.0, -0.0])[0] == [1, 0]
    assert _sel(p, [1, 3], [0.0, -0.0])[0] == [0, 1]
    # and both come before the smallest positive number, after the smallest negative one
    tiny = float(np.float32(1e-45))
    assert _sel(CascadePolicy(1.0, 4), [0, 1, 2, 3], [tiny, 0.0, -tiny, -0.0])[0] == [2, 1, 3, 0]


def test_nan_is_never_chosen_and_the_infinities():
    from afx.cascade import CascadePolicy
    for thr in (0.5, INF):
        sel, w = _sel(CascadePolicy(thr, 4, cooldown=3), [0, 1, 2], [NAN, 0.0, NAN])
        assert sel == [1] and w == [0, 3, 0]
    # -inf is ranked first, under a finite threshold and under +inf
    for thr in (-1.0, INF):
        assert _sel(CascadePolicy(thr, 2), [0, 1, 2], [-5.0, -3.0e38, -INF])[0] == [2, 1]
    # +inf: not below a finite threshold; the compare inf < inf is false too, so threshold = +inf takes every finite or -inf
    # score and nothing else
    assert _sel(CascadePolicy(3.0e38, 4), [0, 1], [INF, 1.0])[0] == [1]
    assert _sel(CascadePolicy(INF, 4), [0, 1, 2, 3], [INF, 3.4e38, NAN, -INF])[0] == [3, 1]
    # a score equal to the threshold is not below it
    assert _sel(CascadePolicy(0.5, 4), [0, 1], [0.5, float(np.nextafter(np.float32(0.5), np.float32(0)))])[0] == [1]
    # the threshold is rounded to fp32 once: 0.1 (double) rounds UP to fp32(0.1), so the score fp32(0.1) is not below it
    assert _sel(CascadePolicy(0.1, 4), [0], [0.1])[0] == []


def test_budget_one_budget_beyond_the_rows_and_ineligible_rows():
    from afx.cascade import CascadePolicy
    slots, scores = [4, 0, 3, 1], [0.3, 0.1, -0.2, 0.1]
    assert _sel(CascadePolicy(1.0, 1), slots, scores)[0] == [2]
    assert _sel(CascadePolicy(1.0, 4), slots, scores)[0] == [2, 1, 3, 0]
    assert _sel(CascadePolicy(1.0, 1024), slots, scores)[0] == [2, 1, 3, 0]
    assert _sel(CascadePolicy(0.2, 1024), slots, scores)[0] == [2, 1, 3]
    assert _sel(CascadePolicy(1.0, 2), slots, scores, elig=[True, False, False, True])[0] == [3, 0]
    assert _sel(CascadePolicy(-1.0, 2), slots, scores) == ([], [0] * 5)
    assert _sel(CascadePolicy(1.0, 2), [], []) == ([], [0])


def test_the_cooldown_counts_down_on_named_slots_only_and_a_passed_over_candidate_competes_again():
    from afx.cascade import CascadePolicy
    p = CascadePolicy(1.0, 1, cooldown=2)
    wait = [0, 0, 0, 7]
    sel, wait = _sel(p, [0, 1, 2], [0.1, 0.2, 0.3], wait=wait)
    assert sel == [0] and wait == [2, 0, 0, 7]  # slots 1 and 2 were passed over: wait stays 0; slot 3 was not named
    sel, wait = _sel(p, [1, 0], [0.2, -9.0], wait=wait)  # slot 0 cools down whatever its score; slot 2 is not named
    assert sel == [0] and wait == [1, 2, 0, 7]
    sel, wait = _sel(p, [2], [0.3], wait=wait)  # only slot 2 is named: the others' counters do not move
    assert sel == [0] and wait == [1, 2, 2, 7]
    sel, wait = _sel(p, [0, 1, 2, 3], [0.0, 0.0, 0.0, 5.0], wait=wait)
    assert sel == [] and wait == [0, 1, 1, 6]
    sel, wait = _sel(p, [0, 1, 2, 3], [0.0, 0.0, 0.0, 5.0], wait=wait)
    assert sel == [0] and wait == [2, 0, 0, 5]
    # cooldown 0: verified at every hop
    p0 = CascadePolicy(1.0, 1)
    for _ in range(3):
        assert _sel(p0, [0], [0.0], wait=[0]) == ([0], [0])
    # the wait handed in is not modified
    w0 = np.array([0, 3], dtype=np.int32)
    p.select_reference([0, 1], np.zeros(2, np.float32), [True, True], w0)
    assert w0.tolist() == [0, 3]


def test_the_result_does_not_depend_on_the_order_of_the_rows_and_equals_the_definition():
    from afx.cascade import CascadePolicy
    g = np.random.default_rng(5)
    values = np.array([-INF, -1.5, -0.0, 0.0, 0.25, 0.25, 0.5, 1.0, INF, NAN], dtype=np.float32)
    for case in range(40):
        S = int(g.integers(1, 24))
        A = int(g.integers(1, S + 1))
        slots = g.permutation(S)[:A].tolist()
        scores = values[g.integers(0, values.size, A)]
        elig = (g.random(A) < 0.8).tolist()
        wait = (g.integers(0, 3, S) * (g.random(S) < 0.4)).tolist()
        p = CascadePolicy([0.5, INF, 0.0, -2.0][case % 4], int(g.integers(1, A + 2)), cooldown=int(g.integers(0, 4)))
        sel, w = p.select_reference(slots, scores, elig, wait)
        want_sel, want_w = _by_definition(p, slots, scores.tolist(), elig, wait)
        assert sel == want_sel and w.tolist() == want_w, case
        perm = g.permutation(A)
        sel2, w2 = p.select_reference([slots[i] for i in perm], scores[perm], [elig[i] for i in perm], wait)
        assert [slots[i] for i in sel] == [slots[perm[i]] for i in sel2] and w2.tolist() == w.tolist(), case


def test_policy_arguments_are_validated_and_identify_the_policy():
    from afx.cascade import CascadePolicy
    p = CascadePolicy(0.1, 3, cooldown=2, min_samples=8000)
    assert p.params() == dict(threshold=float(np.float32(0.1)), budget=3, cooldown=2, min_samples=8000)
    assert all(type(v) in (int, float) for v in p.params().values())
    assert CascadePolicy(INF, 1).params() == dict(threshold=INF, budget=1, cooldown=0, min_samples=None)
    assert CascadePolicy(np.float32(-2.5), np.int64(1024), np.int32(0), 400).params()["budget"] == 1024
    for bad in (dict(threshold=NAN), dict(threshold=-INF), dict(threshold="0.5"), dict(threshold=None), dict(threshold=True),
                dict(threshold=1e39), dict(threshold=-1e39), dict(budget=0), dict(budget=1025), dict(budget=1.5), dict(budget=True),
                dict(cooldown=-1), dict(cooldown=0.5), dict(cooldown=1 << 31), dict(min_samples=399), dict(min_samples=8000.0)):
        with pytest.raises(ValueError):
            CascadePolicy(**dict(dict(threshold=0.0, budget=1), **bad))
    with pytest.raises(ValueError):
        p.select_reference([0, 0], np.zeros(2, np.float32), [True, True], [0])  # a slot named twice
    with pytest.raises(ValueError):
        p.select_reference([1], np.zeros(1, np.float32), [True], [0])  # a slot outside wait


def _bare(S=2, hop=H, window=16000):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=window, hop=hop, device="cpu")


class _Model:
    def forward(self, batch):
        return torch.zeros(batch.shape[0], 2)

    def state_dict(self):
        return {"w": torch.ones(3)}


def test_cascade_scorer_refuses_what_it_cannot_wrap_and_presents_the_inner_surface(built):
    from afx._lib import AfxError
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.ingest import PacketScorer
    from afx.streaming import ResamplingScorer
    from afx.vad import GatedScorer
    pol = CascadePolicy(0.0, 2, cooldown=1)
    inner = CascadeScorer(_bare(), _Model(), pol)
    for front in (ResamplingScorer(_bare(), 8000), PacketScorer(_bare(), 8000, "mulaw"), GatedScorer(_bare()), inner):
        with pytest.raises(ValueError):
            CascadeScorer(front, _Model(), pol)
    for args in ((object(), _Model(), pol), (_bare(), _Model(), "default"), (_bare(), object(), pol),
                 (_bare(S=1), _Model(), pol),  # a budget above S
                 (_bare(), _Model(), CascadePolicy(0.0, 1, min_samples=16001)),  # min_samples above the window
                 (_bare(S=8193, hop=400, window=400), _Model(), pol)):
        with pytest.raises(ValueError):
            CascadeScorer(*args)
    cs = CascadeScorer(_bare(S=3), _Model(), CascadePolicy(0.0, 3, min_samples=8000))
    assert (cs.S, cs.hop, cs.window, cs.device.type, cs.min_samples) == (3, H, 16000, "cpu", 8000)
    assert inner.min_samples == 16000  # the default: the window
    assert cs._slot_list([2, 0], ordered=True) == [2, 0] and cs.samples_seen.tolist() == [0, 0, 0]
    assert cs.hist is None  # the sliding screen's own ring is read in place
    assert torch.isnan(cs.verified).all() and cs.verified_at.tolist() == [-1] * 3 and cs.take_events() == []
    assert all(v.tolist() == [0, 0, 0] for v in cs.stats().values()) and set(cs.stats()) == {"screened", "candidates", "verified", "passed_over"}
    with pytest.raises(AfxError):
        cs.push(torch.zeros(3, H))  # no CPU fallback
    with pytest.raises(ValueError):
        cs.push(torch.zeros(1, H), [3])
    # the gate and the fronts accept it in place of a scorer, and what the gate refused it still refuses
    ps = PacketScorer(GatedScorer(cs), 8000, "mulaw")
    meta = ps.state_meta()
    assert meta["cascade"] == 1 and meta["gate"] == 1 and meta["cascade_policy"] == dict(threshold=0.0, budget=3, cooldown=0, min_samples=8000)
    assert meta["cascade_verifier"]["arch"] == "_Model" and len(meta["cascade_verifier"]["fingerprint"]) == 32
    with pytest.raises(ValueError):
        GatedScorer(GatedScorer(cs))
    with pytest.raises(ValueError):
        GatedScorer(object())


def test_export_and_import_on_the_host_and_every_refusal_leaves_the_scorer_unchanged(built):
    from afx.cascade import CascadePolicy, CascadeScorer
    from afx.streaming import StreamState
    from afx.vad import GatedScorer
    pol = CascadePolicy(0.0, 2, cooldown=2)
    a = CascadeScorer(_bare(S=3), _Model(), pol)
    a.screen.ring[:] = torch.arange(3 * 16000, dtype=torch.float32).reshape(3, 16000)
    a.screen._seen[:] = torch.tensor([8000, 20000, 0])
    a.wait[:] = torch.tensor([2, 0, 1], dtype=torch.int32)
    a.verified[0], a.verified_at[0] = 0.75, 8000
    st = a.export_slots([1, 0])
    assert st.tensors["cascade_wait"].tolist() == [0, 2] and st.tensors["cascade_verified_at"].tolist() == [-1, 8000]
    assert st.tensors["cascade_wait"].dtype == torch.int64 and "cascade_samples" not in st.tensors and st.seen.tolist() == [20000, 8000]
    assert torch.isnan(st.tensors["cascade_verified"][0]) and float(st.tensors["cascade_verified"][1]) == 0.75
    b = CascadeScorer(_bare(S=4), _Model(), pol)

    def snap(c):
        return [c.wait.clone(), c.verified.clone().nan_to_num(-7.0), c.verified_at.clone(), c.screen.ring.clone(), c.screen.samples_seen]

    before = snap(b)
    t = st.tensors
    foreign = [
        a.screen.export_slots([1, 0]),                                                        # no cascade part
        GatedScorer(_bare(S=3)).export_slots([1, 0]),                                         # a GatedScorer state
        st.tensors, None,
        StreamState(dict(st.meta, cascade=2), st.seen, t),                                    # another format
        StreamState(dict(st.meta, cascade_policy=dict(st.meta["cascade_policy"], budget=1)), st.seen, t),
        StreamState(dict(st.meta, cascade_verifier=dict(st.meta["cascade_verifier"], fingerprint="0" * 32)), st.seen, t),
        StreamState(st.meta, st.seen, dict(t, cascade_wait=torch.tensor([0, 3]))),            # wait above the cooldown
        StreamState(st.meta, st.seen, dict(t, cascade_wait=torch.tensor([-1, 0]))),
        StreamState(st.meta, st.seen, dict(t, cascade_wait=torch.tensor([0, 2], dtype=torch.int32))),
        StreamState(st.meta, st.seen, dict(t, cascade_verified_at=torch.tensor([-1, 8001]))),  # verified beyond what it has seen
        StreamState(st.meta, st.seen, dict(t, cascade_verified=torch.zeros(2, dtype=torch.float64))),
        StreamState(dict(st.meta, window=32000), st.seen, t),                                  # the screen's own refusal
        CascadeScorer(_bare(S=3), _Model(), CascadePolicy(0.0, 2, cooldown=3)).export_slots([1, 0]),
    ]
    for f in foreign:
        with pytest.raises(ValueError):
            b.import_slots([3, 1], f)
        assert all(torch.equal(u, v) for u, v in zip(before, snap(b)))
    with pytest.raises(ValueError):
        b.import_slots([3], st)  # two sessions for one slot
    with pytest.raises(ValueError):
        b.screen.import_slots([3, 1], st)  # a bare scorer refuses a cascade state
    b.import_slots([3, 1], StreamState.from_state_dict(st.state_dict()))
    assert b.wait.tolist() == [0, 2, 0, 0] and b.verified_at.tolist() == [-1, 8000, -1, -1] and b.samples_seen.tolist() == [0, 8000, 0, 20000]
    assert float(b.verified[1]) == 0.75 and torch.isnan(b.verified[[0, 2, 3]]).all()
    back = b.export_slots([3, 1])
    assert all(torch.equal(back.tensors[k].nan_to_num(-7.0), st.tensors[k].nan_to_num(-7.0)) for k in st.tensors)
    # reset: the screen's session, wait, verified, verified_at
    b.reset([1])
    assert b.wait.tolist() == [0] * 4 and b.verified_at.tolist() == [-1] * 4 and torch.isnan(b.verified).all() and b.samples_seen.tolist() == [0, 0, 0, 20000]
    # a verifier without state_dict() needs state_dict= to move sessions
    class Bare:  # noqa: E306
        def forward(self, x):
            return x
    with pytest.raises(ValueError):
        CascadeScorer(_bare(), Bare(), pol).export_slots([0])
    assert CascadeScorer(_bare(), Bare(), pol, state_dict={"w": torch.ones(3)}).state_meta()["cascade_verifier"]["fingerprint"] == \
        st.meta["cascade_verifier"]["fingerprint"]


def test_cascade_entry_points_are_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in ("afx_k_cascade_store", "afx_k_cascade_select", "afx_k_cascade_windows"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in built.SIGNATURES
    l = built.lib()
    # refused on the host: nothing launched
    assert l.afx_k_cascade_store(None, 1, 1, None, None, 1, 1, None) != 0 and b"cascade_store" in l.afx_last_error()
    assert l.afx_k_cascade_select(None, 1, None, 1, None, None, 1, 0.0, 1, 0, None, None) != 0 and b"cascade_select" in l.afx_last_error()
    assert l.afx_k_cascade_windows(None, 1, 1, None, 1, None, 1, None, None) != 0 and b"cascade_windows" in l.afx_last_error()
    # sizes that are not positive, with pointers that would pass the NULL check (never dereferenced: nothing is launched)
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((p, 0, 8, p, p, 2, 16), (p, 1, 0, p, p, 2, 16), (p, 1, 8, p, p, 0, 16), (p, 1, 8, p, p, 2, 0), (p, 1, 17, p, p, 2, 16)):
        assert l.afx_k_cascade_store(*args, None) != 0 and b"cascade_store" in l.afx_last_error(), args
    for args in ((p, 1, p, 0, p, None, 2, 0.0, 1, 0, p), (p, 1, p, 8193, p, None, 2, 0.0, 1, 0, p), (p, 1, p, 1, p, None, 0, 0.0, 1, 0, p),
                 (p, 1, p, 1, p, None, 2, 0.0, 0, 0, p), (p, 1, p, 1, p, None, 2, 0.0, 1, -1, p), (p, 0, p, 1, p, None, 2, 0.0, 1, 0, p),
                 (p, 1, p, 1, p, None, 2, float("nan"), 1, 0, p)):
        assert l.afx_k_cascade_select(*args, None) != 0 and b"cascade_select" in l.afx_last_error(), args
    for args in ((p, 0, 16, p, 1, p, 1, p), (p, 2, 0, p, 1, p, 1, p), (p, 2, 16, p, 0, p, 1, p), (p, 2, 16, p, 1, p, 0, p)):
        assert l.afx_k_cascade_windows(*args, None) != 0 and b"cascade_windows" in l.afx_last_error(), args

"""Non-paced streams (afx/streaming.py ``push(chunk, slots)``): slot-list and row-count validation and the per-slot
``samples_seen`` bookkeeping, no GPU needed."""
import pytest
import torch

S, W, H = 4, 16000, 4000


def _scorer():
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=W, hop=H, device="cpu")


def test_push_with_slots_refuses_bad_lists_rows_and_host_tensors():
    sc = _scorer()
    rows = lambda n: torch.zeros(n, H)
    for bad in ([S], [-1], [2, 2], [0.5], [[1]], torch.tensor([True, False])):
        with pytest.raises(ValueError):
            sc.push(rows(1), slots=bad)
    for slots, n in (([0, 2], 1), ([0, 2], 3), (torch.tensor([True, False, True, True]), 2), ([], 1)):
        with pytest.raises(ValueError):
            sc.push(rows(n), slots=slots)
    with pytest.raises(ValueError):  # a host tensor of the right shape: the chunk must be on the GPU
        sc.push(rows(2), slots=[1, 3])
    with pytest.raises(ValueError):
        sc.push(torch.zeros(2, H - 1), slots=[1, 3])
    assert sc.samples_seen.tolist() == [0] * S  # nothing was refused half-way


def test_slot_order_is_the_callers_and_a_mask_is_ascending():
    sc = _scorer()
    assert sc._slot_list([3, 0, 2], ordered=True) == [3, 0, 2]
    assert sc._slot_list([3, 0, 2]) == [0, 2, 3]  # (reset's order)
    assert sc._slot_list(torch.tensor([True, False, True, True]), ordered=True) == [0, 2, 3]
    assert sc._slot_list([], ordered=True) == []


def test_named_slots_advance_alone_at_their_own_phase():
    sc = _scorer()
    a = torch.arange(2 * H, dtype=torch.float32).reshape(2, H)
    sc._store_slots(a, [2, 0])
    assert sc.samples_seen.tolist() == [H, 0, H, 0]
    assert torch.equal(sc.ring[2, :H], a[0]) and torch.equal(sc.ring[0, :H], a[1])
    b = -torch.ones(1, H)
    sc._store_slots(b, [2])
    assert sc.samples_seen.tolist() == [H, 0, 2 * H, 0]
    assert torch.equal(sc.ring[2, H:2 * H], b[0]) and torch.equal(sc.ring[0, H:2 * H], torch.zeros(H))
    assert not sc.ring[1].any() and not sc.ring[3].any()
    for _ in range(3):  # slot 2 wraps its ring (16 000 samples) while slot 0 stays put
        sc._store_slots(b * 2, [2])
    assert sc.samples_seen.tolist() == [H, 0, 5 * H, 0]
    assert torch.equal(sc.ring[2, :H], 2 * b[0]) and torch.equal(sc.ring[0, :H], a[1])
    sc.reset([2])
    assert sc.samples_seen.tolist() == [H, 0, 0, 0]

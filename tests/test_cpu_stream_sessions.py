"""Per-slot streaming sessions (afx/streaming.py ``reset`` / ``samples_seen``): the host-side bookkeeping, no GPU needed."""
import pytest
import torch


def _scorer(S=4):
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=16000, hop=4000, device="cpu")


def test_reset_takes_indices_or_a_mask_and_refuses_bad_slots():
    sc = _scorer()
    assert sc.samples_seen.dtype == torch.int64 and torch.equal(sc.samples_seen, torch.zeros(4, dtype=torch.int64))
    sc._seen += 12000  # three hops in
    sc.reset([1, 3])
    assert sc.samples_seen.tolist() == [12000, 0, 12000, 0]
    sc.reset(torch.tensor([True, False, True, False]))
    assert sc.samples_seen.tolist() == [0, 0, 0, 0]
    sc.reset([])  # nothing named: nothing changes
    for bad in ([4], [-1], [2, 2], [0.5], [[1]], torch.tensor([True, False])):
        with pytest.raises(ValueError):
            sc.reset(bad)


def test_samples_seen_is_a_copy():
    sc = _scorer()
    sc.samples_seen[0] = 5
    assert int(sc.samples_seen[0]) == 0

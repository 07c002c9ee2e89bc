"""What the packet tests (ingest, codecs, jitter) share and that needs torch or a scorer.  A plain module: no fixtures.  The
numpy reference of the jitter buffer, the decode tables and the traffic are oracle/jitter.py."""
import numpy as np
import torch

H = 4000


def built():
    """What a file's own autouse ``built`` fixture returns: a state records the library's build id, and the entry points are
    looked up in the built library."""
    import __graft_entry__ as ge
    ge.build()
    from afx import _lib
    return _lib


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def inner(S, hop=H):
    """A host-only inner scorer: it is never pushed."""
    from afx.streaming import SlidingWindowScorer
    return SlidingWindowScorer(None, S, window=16000, hop=hop, device="cpu")


def tap(S, window=4 * H, hop=H, clear_on_reset=False):
    """A scorer on the GPU that only records the hops it is pushed, per slot, in ``got``."""
    from afx.streaming import SlidingWindowScorer

    class Tap(SlidingWindowScorer):
        def __init__(self):
            super().__init__(None, S, window=window, hop=hop, device="cuda")
            self.got = [[] for _ in range(S)]

        def _reset_slots(self, idx):
            super()._reset_slots(idx)
            if clear_on_reset:
                for s in idx:
                    self.got[s] = []

        def push(self, chunk, slots=None):
            idx = self._slot_list(slots, ordered=True)
            assert chunk.is_cuda and chunk.dtype == torch.float32 and chunk.shape == (len(idx), hop)
            for i, s in enumerate(idx):
                self.got[s].append(chunk[i].clone())
            self._seen[idx] += hop
            return torch.zeros(len(idx), device=chunk.device)

    return Tap()


def offline(E, rate):
    """The offline ``Resampler`` on the GPU over a whole stream of fp32 samples."""
    from afx.resample import Resampler
    return Resampler(rate)(torch.from_numpy(np.ascontiguousarray(np.asarray(E, dtype=np.float32))).cuda()[None])[0]


def ref64(x, rate):
    """float64 upfirdn of the designed filter over a whole stream."""
    from scipy import signal
    from afx.resample import design_filter
    L, M, h = design_filter(rate)
    if L == M:
        return np.asarray(x, dtype=np.float64)
    return signal.upfirdn(h, np.asarray(x, dtype=np.float64), L, M)[: -(-len(x) * L // M)]


def go(js, dev, plan, pay=()):
    """Run a plan on the numpy device and commit its book -> the plan."""
    dev.run(plan, list(pay))
    js._commit(plan.book)
    return plan


def snap(js):
    """Everything a refused call must leave alone: the public counters, the stats and every tensor of an export of all slots."""
    e = js.export_slots(list(range(js.S)))
    extra = [js.rates] if getattr(js, "_rated", False) else []
    return [js.pending, js.samples_in, js.buffered, js.samples_seen] + extra + list(js.stats().values()) + [e.tensors[k] for k in sorted(e.tensors)]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))

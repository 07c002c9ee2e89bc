"""Resampling to 16 kHz on the GPU (afx/resample.py, afx_k_resample / afx_k_resample_stream) and the streaming wrapper
(afx/streaming.py ``ResamplingScorer``).  The kernels are within 2e-6 * max|x| of float64 upfirdn at every rate; the
streaming form over hops is bit-identical to the offline form over the whole signal, also with named subsets in shuffled
order; a wrapped scorer emits, bit for bit, what its inner scorer emits on the offline-resampled stream, through resets,
non-paced pushes and a session moved through host memory and torch.save into another scorer; foreign states are refused
before anything changes; batch_adjust_duration at 48 kHz scores like the CPU oracle on float64-resampled input."""
import io
import random

import numpy as np
import pytest
import torch
from scipy import signal

pytestmark = pytest.mark.gpu

RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000, 192000]  # 192 kHz: the largest staged input span
H = 4000


def _ref(x, rate):
    """float64 upfirdn, causal, ceil(N*L/M) outputs."""
    from afx.resample import design_filter
    L, M, h = design_filter(rate)
    x = np.asarray(x, dtype=np.float64)
    return signal.upfirdn(h, x, L, M)[: -(-len(x) * L // M)]


@pytest.mark.parametrize("rate", RATES)
def test_kernel_matches_upfirdn(rate):
    from afx.resample import Resampler
    rs = Resampler(rate)
    g = torch.Generator().manual_seed(rate)
    x = torch.randn(3, rate // 4 + 13, generator=g)
    y = rs(x.cuda()).cpu()
    assert y.shape == (3, rs.n_out(x.shape[1]))
    for b in range(3):
        ref = _ref(x[b].numpy(), rate)
        assert np.abs(y[b].double().numpy() - ref).max() <= 2e-6 * float(x[b].abs().max())
    lens = [1, 2, rs.T - 1, rs.T + 1, 997, 4001, rate // 10 + 3]  # one sample, shorter than the filter, primes
    clips = [torch.randn(n, generator=g) * (1 + i) for i, n in enumerate(lens)]
    out = rs.clips(clips)
    assert [o.numel() for o in out] == [rs.n_out(n) for n in lens]
    for c, o in zip(clips, out):
        ref = _ref(c.numpy(), rate)
        assert o.is_cuda and np.abs(o.cpu().double().numpy() - ref).max() <= 2e-6 * float(c.abs().max())


def test_identity_rate_launches_nothing():
    from afx.resample import Resampler
    x = torch.randn(2, 1000).cuda()
    assert Resampler(16000)(x) is x


@pytest.mark.parametrize("rate,n_in", [(8000, 2000), (44100, 11025), (48000, 12000), (96000, 24000), (48000, 30),
                                       (11025, 2205), (22050, 4410)])
def test_streaming_equals_offline(rate, n_in):
    """Named subsets of slots in shuffled order, one chunk each per tick; n_in = 30 at 48 kHz: chunks shorter than the
    T - 1 = 60 carried samples; 11 025 Hz: the tap table stays in global memory (640 phases); 22 050 Hz: 8 sub-tiles per
    workgroup, so a chunk's 3 200 outputs span two workgroups."""
    from afx.resample import Resampler
    rs = Resampler(rate)
    S, ticks = 5, 7
    rng = random.Random(rate + n_in)
    audio = torch.randn(S, ticks * n_in, generator=torch.Generator().manual_seed(n_in))
    hist = torch.zeros(S, rs.history, device="cuda")
    pos, outs = [0] * S, [[] for _ in range(S)]
    for t in range(ticks + 3):
        named = [s for s in range(S) if pos[s] < ticks and rng.random() < 0.7]
        rng.shuffle(named)
        if not named:
            continue
        chunk = torch.stack([audio[s, pos[s] * n_in:(pos[s] + 1) * n_in] for s in named]).cuda()
        y = rs.stream(chunk, hist, named)
        assert y.shape == (len(named), n_in * rs.L // rs.M)
        for i, s in enumerate(named):
            outs[s].append(y[i].cpu())
            pos[s] += 1
    for s in range(S):
        got = torch.cat(outs[s]) if outs[s] else torch.empty(0)
        whole = rs(audio[s:s + 1, :pos[s] * n_in].cuda()).cpu()[0] if pos[s] else torch.empty(0)
        assert torch.equal(got, whole), s


# ---- the streaming wrapper ---------------------------------------------------------------------------------------------
_ENGINES = {}


def _engine(dtype):
    if dtype not in _ENGINES:
        from afx import engine, synth
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
        eng.load_state_dict(sd)
        _ENGINES[dtype] = (eng, sd)
    return _ENGINES[dtype]


def _inner(kind, S):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    eng, sd = _engine("fp16x3" if kind == "kv-fp16x3" else "fp16")
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=16000, hop=H, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=16000, hop=H)
    return KVCachedScorer(eng, sd, S, window=64000, hop=H)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a.cpu(), b.cpu()))


class _Sessions:
    """Audio of every session (input rate) and its offline 16 kHz version; ``hop(sess, k)``: the k-th hop of each."""

    def __init__(self, rate, hops, seed):
        from afx.resample import Resampler
        self.rs, self.hops, self.seed, self.rate = Resampler(rate), hops, seed, rate
        self.hop_in = H * rate // 16000
        self.cache = {}

    def _get(self, sess):
        if sess not in self.cache:
            x = torch.randn(1, self.hops * self.hop_in, generator=torch.Generator().manual_seed(self.seed * 1000 + sess)) * 0.1
            self.cache[sess] = (x[0], self.rs(x.cuda())[0].cpu())
        return self.cache[sess]

    def hop(self, sess, k):
        x, y = self._get(sess)
        return x[k * self.hop_in:(k + 1) * self.hop_in], y[k * H:(k + 1) * H]


def _drive(pairs, ses, state, named):
    """One tick of wrapped scorer W and reference R (inner scorer fed the offline-resampled hops) over the slots ``named``
    (caller's order; None: lock-stepped).  state: slot -> [session id, hops pushed]."""
    order = list(range(len(state))) if named is None else named
    hx, hy = zip(*[ses.hop(*state[s]) for s in order])
    outs = []
    for sc, h in zip(pairs, (hx, hy)):
        outs.append(sc.push(torch.stack(h).cuda(), slots=named))
    for s in order:
        state[s][1] += 1
    return outs


@pytest.mark.parametrize("rate", [8000, 44100, 48000])
@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv", "kv-fp16x3"])
def test_wrapper_scores_equal_inner_on_resampled_stream(kind, rate):
    from afx.streaming import ResamplingScorer, StreamState
    SX, SY, ticks = 3, 2, 7
    ses = _Sessions(rate, ticks + 4, seed=rate // 100 + len(kind))
    rng = random.Random(rate)
    W, R = ResamplingScorer(_inner(kind, SX), rate), _inner(kind, SX)
    assert W.hop_in == ses.hop_in and W.delay == (20 if rate == 8000 else 10)
    state = {s: [s, 0] for s in range(SX)}
    next_sess = SX
    for t in range(ticks):
        if t > 0 and rng.random() < 0.4:  # resets at random ticks
            slot = rng.randrange(SX)
            W.reset([slot])
            R.reset([slot])
            state[slot] = [next_sess, 0]
            next_sess += 1
        if t < 2:
            named = None
        else:  # non-paced: a random non-empty subset in random order
            named = rng.sample(range(SX), rng.randint(1, SX))
        a, b = _drive((W, R), ses, state, named)
        assert _same(a, b), (t, named)
        assert torch.equal(W.samples_seen, R.samples_seen)
    # move slot 1's session into slot 0 of a 2-slot scorer through host memory and torch.save
    Y, RY = ResamplingScorer(_inner(kind, SY), rate), _inner(kind, SY)
    ystate = {0: [next_sess, 0], 1: [next_sess + 1, 0]}
    for t in range(2):
        a, b = _drive((Y, RY), ses, ystate, None if t == 0 else [1, 0])
        assert _same(a, b)
    st = W.export_slots([1])
    assert set(st.tensors) >= {"resample_hist"} and st.meta["input_rate"] == rate and st.meta["resampler"] == "kaiser5-hl10"
    buf = io.BytesIO()
    torch.save(st.to("cpu").state_dict(), buf)
    buf.seek(0)
    st2 = StreamState.from_state_dict(torch.load(buf, weights_only=True))
    Y.import_slots([0], st2)
    RY.import_slots([0], R.export_slots([1]))
    ystate[0] = list(state[1])
    for t in range(3):
        a, b = _drive((Y, RY), ses, ystate, [[1, 0], None, [1]][t])
        assert _same(a, b), t
    # the source keeps going, untouched by the export
    a, b = _drive((W, R), ses, state, None)
    assert _same(a, b)


def test_refusals_change_nothing():
    from afx.streaming import ResamplingScorer
    W = ResamplingScorer(_inner("sliding", 3), 48000)
    other_rate = ResamplingScorer(_inner("sliding", 3), 24000)
    bare = _inner("sliding", 3)
    g = torch.Generator().manual_seed(5)
    for sc, n in ((W, 12000), (other_rate, 6000)):
        sc.push((0.1 * torch.randn(3, n, generator=g)).cuda())
    bare.push((0.1 * torch.randn(3, H, generator=g)).cuda())

    def snap():
        st = W.export_slots([0, 1, 2])
        return st.seen.clone(), {k: t.clone() for k, t in st.tensors.items()}

    before = snap()
    for foreign in (other_rate.export_slots([1]), bare.export_slots([1])):
        with pytest.raises(ValueError):
            W.import_slots([2], foreign)
        after = snap()
        assert torch.equal(before[0], after[0]) and all(torch.equal(before[1][k], after[1][k]) for k in before[1])
    bare_before = bare.export_slots([0, 1, 2])
    with pytest.raises(ValueError):
        bare.import_slots([2], W.export_slots([1]))  # the extra tensor key: a bare scorer refuses a wrapped state
    bare_after = bare.export_slots([0, 1, 2])
    assert torch.equal(bare_before.seen, bare_after.seen)
    assert all(torch.equal(bare_before.tensors[k], bare_after.tensors[k]) for k in bare_before.tensors)
    with pytest.raises(ValueError):
        ResamplingScorer(_inner("sliding", 2), 22050)  # a 4000-sample hop is 5512.5 samples at 22.05 kHz
    with pytest.raises(ValueError):
        W.push(torch.zeros(3, H).cuda())  # a 16 kHz hop given to a 48 kHz scorer


def test_batch_adjust_duration_at_48k_matches_oracle():
    from afx import engine, harness, synth
    from oracle import models as om
    sd = synth.model_state_dict("ConformerModel", n_layers=2, n_encoders=2)
    eng = engine.Engine("conformer", n_layers=2, dtype="fp16", conf_blocks=2)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(48)
    clips = [0.1 * torch.randn(n, generator=g) for n in (48000 + 17, 30011, 96000 + 5)]
    dur = 16000
    batch = harness.batch_adjust_duration(clips, dur, sample_rate=48000)
    ref_in = torch.stack([harness.adjust_duration(torch.from_numpy(_ref(c.numpy(), 48000)).float(), dur) for c in clips])
    assert (batch.cpu() - ref_in).abs().max() <= 2e-6 * max(float(c.abs().max()) for c in clips)
    got = eng.forward(batch).cpu()
    ref = om.conformer_forward(sd, ref_in)
    assert (got - ref).abs().max() <= 1e-3
    clips16 = [0.1 * torch.randn(n, generator=g) for n in (16000 + 3, 9001, 40000)]
    starts = [2, 0, 1000]
    assert torch.equal(harness.batch_adjust_duration(clips16, dur, starts=starts, sample_rate=16000),
                       harness.batch_adjust_duration(clips16, dur, starts=starts))

"""Offline timelines (afx/timeline.py): every score equals, bit for bit, the score a one-slot streaming scorer emits at that
hop -- on the fast path (conv layers 0-5 once over the recording, afx_tail_forward_windows on windows of a shared buffer)
and on the fallback path (Engine.forward on window rows)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H = 16000, 4000
# shorter than a hop (cover_end only), shorter than a window, several windows and not a multiple of the hop
LENGTHS = [3000, 11000, 16000 * 3 + 1700]


def _engine(arch, dtype="fp16", extractor_mode="layer_norm"):
    from afx import engine, synth
    if arch == "conformer" and extractor_mode == "group_norm":
        sd = synth.ssl_state_dict(1, extractor_mode="group_norm")
        sd.update(synth.conformer_head_state_dict(n_encoders=1))
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1, extractor_mode=extractor_mode)
    elif arch == "conformer":
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1, extractor_mode=extractor_mode)
    else:
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype=dtype, extractor_mode=extractor_mode)
    eng.load_state_dict(sd)
    return eng, sd


def _recordings(lengths=LENGTHS, seed=7100):
    from afx import synth
    return [synth.waveforms(1, n, batch_idx=seed + i)[0] for i, n in enumerate(lengths)]


def _stream_scores(scorer, x, hop):
    """A one-slot scorer pushed hop by hop over x -> its (n // hop,) scores."""
    out = [scorer.push(x[None, j * hop:(j + 1) * hop].cuda()).clone().cpu() for j in range(x.numel() // hop)]
    return torch.cat(out) if out else torch.empty(0)


def _cover_end(eng, x, w=W):
    from afx import harness
    win = harness.batch_adjust_duration([x.cuda()], w) if x.numel() < w else x[None, -w:].cuda()
    return eng.forward(win)[:, 1].cpu()


def _reference(eng, sd, x, incremental=True):
    from afx.streaming import IncrementalScorer, SlidingWindowScorer
    ref = _stream_scores(SlidingWindowScorer(eng, 1, window=W, hop=H), x, H)
    if incremental:
        inc = _stream_scores(IncrementalScorer(eng, sd, 1, window=W, hop=H), x, H)
        assert torch.equal(inc, ref)
    return torch.cat([ref, _cover_end(eng, x)])


@pytest.mark.parametrize("arch", ["conformer", "xlsr_aasist"])
def test_mixed_lengths_equal_streaming_scorers(arch):
    from afx.timeline import fast_path_ok, score_timeline
    eng, sd = _engine(arch)
    assert fast_path_ok(eng, W, H, sd)
    recs = _recordings()
    tls = score_timeline(eng, recs, window=W, hop=H, cover_end=True, state_dict=sd)
    assert len(tls) == len(recs)
    for x, tl in zip(recs, tls):
        ref = _reference(eng, sd, x)
        assert tl.scores.shape == ref.shape
        assert torch.equal(tl.scores, ref), (x.numel(), (tl.scores - ref).abs().max())
        assert tl.ends.tolist()[:-1] == [float((j + 1) * H) for j in range(x.numel() // H)]
        assert tl.ends.tolist()[-1] == float(x.numel())
    # warmup=False drops exactly the tiled windows
    tls2 = score_timeline(eng, recs, window=W, hop=H, warmup=False, state_dict=sd)
    for x, tl, tl2 in zip(recs, tls, tls2):
        n_warm = sum(1 for j in range(x.numel() // H) if (j + 1) * H < W)
        assert torch.equal(tl2.scores, tl.scores[n_warm:-1])


@pytest.mark.parametrize("dtype,mode", [("fp16x3", "layer_norm"), ("fp32", "layer_norm"), ("fp16", "group_norm")])
def test_fallback_equals_sliding_scorer(dtype, mode):
    from afx.timeline import fast_path_ok, score_timeline
    eng, sd = _engine("conformer", dtype, mode)
    assert not fast_path_ok(eng, W, H, sd)
    recs = _recordings()
    tls = score_timeline(eng, recs, window=W, hop=H, cover_end=True, state_dict=sd)
    for x, tl in zip(recs, tls):
        assert torch.equal(tl.scores, _reference(eng, sd, x, incremental=False))


def test_hop_off_the_frame_grid_falls_back_exactly():
    from afx.streaming import SlidingWindowScorer
    from afx.timeline import fast_path_ok, score_timeline
    eng, sd = _engine("conformer")
    w, h = 16000, 2500  # 2500 % 160 != 0
    assert not fast_path_ok(eng, w, h, sd)
    x = _recordings([40000], seed=7300)[0]
    tl = score_timeline(eng, [x], window=w, hop=h, state_dict=sd)[0]
    assert torch.equal(tl.scores, _stream_scores(SlidingWindowScorer(eng, 1, window=w, hop=h), x, h))


def test_batch_and_block_independence():
    from afx.timeline import score_timeline
    eng, sd = _engine("conformer")
    recs = _recordings([16000 * 5 + 300, 9000, 16000 * 4])
    base = score_timeline(eng, recs, window=W, hop=H, cover_end=True, state_dict=sd)
    for kw in (dict(batch_windows=1), dict(batch_windows=256), dict(block_rows=1, chunk_frames=7),
               dict(block_rows=3, chunk_frames=50, batch_windows=5)):
        got = score_timeline(eng, recs, window=W, hop=H, cover_end=True, state_dict=sd, **kw)
        for a, b in zip(base, got):
            assert torch.equal(a.scores, b.scores), kw


@pytest.mark.parametrize("rate", [44100, 48000])
def test_other_rates_equal_resampling_scorer(rate):
    from afx.streaming import ResamplingScorer, SlidingWindowScorer
    from afx.resample import Resampler
    from afx.timeline import score_timeline
    eng, sd = _engine("conformer")
    hop_in = H * rate // 16000
    n = hop_in * 7 + 333
    x = (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(rate))).float()
    tl = score_timeline(eng, [x], window=W, hop=H, sample_rate=rate, state_dict=sd)[0]
    rsc = ResamplingScorer(SlidingWindowScorer(eng, 1, window=W, hop=H), rate)
    ref = _stream_scores(rsc, x, hop_in)
    assert torch.equal(tl.scores, ref)
    d = Resampler(rate).delay
    assert tl.sample_rate == rate
    assert torch.allclose(tl.ends, torch.tensor([((j + 1) * H - d) * rate / 16000 for j in range(7)], dtype=torch.float64))


def test_tail_forward_windows_direct():
    from afx import _lib
    from afx.engine import torch_dtype
    eng, sd = _engine("conformer")
    T5 = 99  # a 16000-sample window
    g = torch.Generator().manual_seed(5)
    buf = (torch.randn(700, 512, generator=g) * 0.5).to(torch_dtype(eng.dtype)).cuda()
    # overlapping windows of one "recording" (frames 0..) and windows of a second one stored after it (frames 400..)
    frames = [0, 25, 50, 400, 411, 700 - T5, 3]
    got = eng.tail_windows(buf, [f * 512 for f in frames], T5)
    ref = eng.tail(torch.stack([buf[f:f + T5] for f in frames]))
    assert torch.equal(got, ref)
    one = eng.tail_windows(buf, [411 * 512], T5)
    assert torch.equal(one[0], ref[4])
    torch.cuda.synchronize()
    for bad in ([4], [-8], [(700 - T5) * 512 + 8], [700 * 512]):
        with pytest.raises(_lib.AfxError):
            eng.tail_windows(buf, [0] + bad, T5)


def test_drop_in_module_as_model():
    from afx.streaming import SlidingWindowScorer
    from afx.timeline import score_timeline
    from models.conformer_baseline import MyModel
    m = MyModel(device="cuda", ssl_cpkt_path=None, num_layers=1, order="first", n_encoders=1).to("cuda").eval()
    x = _recordings([16000 * 2 + 4000], seed=7400)[0]
    tl = score_timeline(m, [x], window=W, hop=H)[0]
    assert torch.equal(tl.scores, _stream_scores(SlidingWindowScorer(m, 1, window=W, hop=H), x, H))


def test_memory_bounded_by_blocks_not_length():
    from afx import synth
    from afx.timeline import score_timeline
    eng, sd = _engine("conformer")
    kw = dict(window=64000, hop=4000, state_dict=sd, block_rows=8)
    score_timeline(eng, [synth.waveforms(1, 16000 * 20, batch_idx=7500)[0]], **kw)  # (workspaces at their size)
    peaks = []
    for sec in (60, 120):
        x = synth.waveforms(1, 16000 * sec, batch_idx=7500 + sec)[0]  # (host: the recording is not device memory)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tl = score_timeline(eng, [x], **kw)[0]
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert len(tl) == sec * 4
    out_bytes = 2048  # the longer recording's 480 fp32 scores, in the allocator's 512-byte blocks
    assert peaks[1] <= peaks[0] + out_bytes, peaks


def test_timeline_file_from_dataset(tmp_path):
    from afx import harness
    from afx.timeline import score_timeline
    eng, sd = _engine("conformer")
    recs = _recordings([20000, 9000])

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return len(recs)

        def __getitem__(self, i):
            return f"utt{i}", recs[i], 0

    path = tmp_path / "timeline.txt"
    names, tls = harness.produce_timeline_file(DS(), eng, "cuda", str(path), window=W, hop=H, batch_size=2, num_workers=0,
                                               state_dict=sd)
    ref = score_timeline(eng, recs, window=W, hop=H, state_dict=sd)
    lines = path.read_text().splitlines()
    assert len(lines) == sum(len(t) for t in ref) == 5 + 2
    assert lines[0] == f"utt0 0.000 0.250 {ref[0].scores[0].item()}"
    assert lines[-1].startswith("utt1 0.000 0.500 ")

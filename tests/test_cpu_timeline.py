"""Offline timelines, host side (afx/timeline.py): the window plan, the chunk-row plan, the fast-path decision, the input-rate
hop, Timeline.segments / summary, the timeline file format and the new C entry points' declarations.  No GPU."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from afx import timeline as T  # noqa: E402
from afx.streaming import _frames5  # noqa: E402


def test_window_plan_ticks_bounds_and_warmup():
    plan = T.plan_windows(50000, 16000, 4000)
    assert len(plan) == 50000 // 4000 == 12
    assert [e for _, e, _ in plan] == [4000 * (j + 1) for j in range(12)]
    assert [w for _, _, w in plan] == [True] * 3 + [False] * 9  # 4000, 8000, 12000 < 16000; 16000 is a whole window
    assert [s for s, _, _ in plan] == [0, 0, 0] + [4000 * (j + 1) - 16000 for j in range(3, 12)]
    assert T.plan_windows(50000, 16000, 4000, warmup=False) == plan[3:]


def test_window_plan_cover_end_and_short_recordings():
    # a hop that does not divide N: the last partial hop gets no tick, cover_end adds the window ending at N
    plan = T.plan_windows(50001, 16000, 4000, cover_end=True)
    assert len(plan) == 13 and plan[-1] == (50001 - 16000, 50001, False)
    assert T.plan_windows(3000, 16000, 4000) == []
    assert T.plan_windows(3000, 16000, 4000, cover_end=True) == [(0, 3000, True)]  # tiled whole recording
    assert T.plan_windows(3000, 16000, 4000, warmup=False, cover_end=True) == [(0, 3000, True)]
    assert T.plan_windows(16000, 16000, 4000, cover_end=True)[-1] == (0, 16000, False)


@pytest.mark.parametrize("m", [1, 7, 50, 100])
def test_chunk_row_yields_exactly_m_frames(m):
    L = 160 * m + 80
    n = L
    lens = []
    for k, s in T.CONV_KS[:6]:
        n = (n - k) // s + 1
        lens.append(n)
    assert lens == [32 * m + 15, 16 * m + 7, 8 * m + 3, 4 * m + 1, 2 * m, m]
    assert _frames5(L) == m and _frames5(L - 1) == m - 1


@pytest.mark.parametrize("n,m,rows", [(400, 100, 64), (16000, 100, 64), (160 * 1000 + 79, 100, 3), (123457, 7, 5),
                                      (64000 * 9 + 17, 100, 2)])
def test_row_blocks_produce_every_frame_once(n, m, rows):
    F, R = T.chunk_rows(n, m)
    assert F == _frames5(n) == (n - 240) // 160 + 1
    seen = []
    for r0, nb, f0, keep in T.row_blocks(n, m, rows):
        assert 1 <= nb <= rows and f0 == r0 * m and 0 < keep <= nb * m
        seen.extend(range(f0, f0 + keep))
    assert seen == list(range(F))  # each frame once, in order
    assert R * m >= F > (R - 1) * m
    # kept frames read inside the recording; the first dropped one would read past its end
    assert 160 * (F - 1) + 240 <= n < 160 * F + 240


def _eng(**kw):
    d = dict(dtype="fp16", extractor_mode="layer_norm", pre_emphasis=False, arch="conformer")
    d.update(kw)
    return SimpleNamespace(**d)


def test_fast_path_decision():
    sd = {}
    assert T.fast_path_ok(_eng(), 64000, 4000, sd)
    assert T.fast_path_ok(_eng(dtype="bf16", arch="xlsr_aasist"), 16000, 4000, sd)
    assert T.fast_path_ok(_eng(), 64000, 160, sd)
    assert not T.fast_path_ok(_eng(), 64000, 4000, None)  # no conv weights at hand
    for kw in (dict(dtype="fp32"), dict(dtype="fp16x3"), dict(extractor_mode="group_norm"), dict(pre_emphasis=True),
               dict(arch="ssl")):
        assert not T.fast_path_ok(_eng(**kw), 64000, 4000, sd), kw
    assert not T.fast_path_ok(_eng(), 64000, 2500, sd)   # hop off the frame grid
    assert not T.fast_path_ok(_eng(), 64080 + 40, 4000, sd)  # window off the frame grid


def test_input_rate_hop_and_refusal():
    assert T.input_hop(4000, 8000) == 2000
    assert T.input_hop(4000, 44100) == 11025
    assert T.input_hop(4000, 48000) == 12000
    assert T.input_hop(4000, 16000) == 4000
    with pytest.raises(ValueError, match="not a whole number"):
        T.input_hop(4001, 44100)
    with pytest.raises(ValueError, match="not a whole number"):
        T.input_hop(4000, 22050)  # 5512.5 input samples
    with pytest.raises(ValueError):
        T.input_hop(4000, 1000)


def test_segments_and_summary_on_hand_made_scores():
    sc = [0.9, 0.1, 0.2, 0.8, 0.3, 0.95, 0.05, 0.04, 0.01]
    ends = [4000 * (j + 1) for j in range(len(sc))]
    starts = [max(e - 16000, 0) for e in ends]
    tl = T.Timeline(sc, starts, ends)
    assert len(tl) == 9
    assert tl.times()[0].tolist() == [0.0, 0.25] and tl.times()[-1].tolist() == [1.25, 2.25]
    assert tl.segments(0.5) == [(0.0, 0.75), (0.25, 1.25), (0.75, 2.25)]
    assert tl.segments(0.5, min_windows=2) == [(0.0, 0.75), (0.75, 2.25)]
    assert tl.segments(0.5, min_windows=3) == [(0.75, 2.25)]
    assert tl.segments(0.0) == []
    s = tl.summary(0.5)
    assert s["windows"] == 9 and s["min"] == pytest.approx(0.01) and s["flagged"] == pytest.approx(6 / 9)
    assert s["mean"] == pytest.approx(sum(sc) / 9)
    assert T.Timeline([], [], []).summary(0.5)["windows"] == 0
    with pytest.raises(ValueError):
        T.Timeline([0.1], [0, 1], [1])


def test_timeline_file_format(tmp_path):
    from afx import harness
    tls = [T.Timeline([0.5, -1.25], [0, 0], [4000, 8000]), T.Timeline([], [], []),
           T.Timeline([2.0], [22050.0], [44100.0], sample_rate=44100)]
    path = tmp_path / "sub" / "timeline.txt"
    harness.write_timeline_file(str(path), ["a", "b", "c"], tls)
    assert path.read_text().splitlines() == ["a 0.000 0.250 0.5", "a 0.000 0.500 -1.25", "c 0.500 1.000 2.0"]
    line = re.compile(r"^\S+ \d+\.\d{3} \d+\.\d{3} \S+$")
    assert all(line.match(l) for l in path.read_text().splitlines())


def test_short_recordings_are_refused():
    eng = SimpleNamespace(arch="conformer", dtype="fp16")
    with pytest.raises(ValueError, match="400"):
        T.score_timeline(T.Engine.__new__(T.Engine), [torch.zeros(399)], state_dict=None)
    with pytest.raises(ValueError):
        T.score_timeline(eng, [torch.zeros(16000)])  # neither an Engine nor a drop-in module


def test_new_entry_points_declared_and_bound():
    from afx import _lib
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    for name in ("afx_tail_windows_workspace_bytes", "afx_tail_forward_windows"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES, name
    assert T.default_batch(SimpleNamespace(arch="conformer")) == 64
    assert T.default_batch(SimpleNamespace(arch="xlsr_aasist")) == 16

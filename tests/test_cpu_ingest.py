"""The packet front (afx/ingest.py) without a GPU: the G.711 tables the formulas give, the host arithmetic that says how
many 16 kHz samples a packet completes and at which filter phase (a float64 restatement of afx_k_ingest's index plan with
carried counters equals the whole-signal plan of tests/test_cpu_resample.py for ragged cuts at every rate), the staging
buffer's layout, every refusal of ``PacketScorer`` on a host-only scorer leaving it unchanged, the state an export adds,
and the new entry points in the header, the library and the ctypes table."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import packet_helpers
from oracle.jitter import TABLES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 11025, 22050, 44100, 48000, 192000]
H = 4000


def test_g711_tables_known_answers_and_symmetry():
    mu, al = ((TABLES[law] * np.float32(32768)).astype(np.int64) for law in ("mulaw", "alaw"))  # (whole numbers, exact in fp32)
    assert (mu[0x00], mu[0x80], mu[0x7F], mu[0xFF]) == (-32124, 32124, 0, 0)
    assert (al[0xD5], al[0x55], al[0xAA], al[0x2A]) == (8, -8, 32256, -32256)
    c = np.arange(128)
    assert np.array_equal(mu[c], -mu[c | 0x80]) and np.array_equal(al[c], -al[c | 0x80])
    assert np.abs(mu).max() == 32124 and np.abs(al).max() == 32256
    assert len(set(np.abs(mu[:128]).tolist())) == 128 and len(set(al.tolist())) == 256
    try:
        import audioop
    except ImportError:
        audioop = None
    if audioop is not None:  # (gone in Python 3.13: only this comparison is left out there)
        codes = bytes(range(256))
        assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2"), mu)
        assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2"), al)


# ---- the index plan ------------------------------------------------------------------------------------------------------
def _chain(taps, v, i, p):
    """sum_j taps[p][j] * v[T-1 + i - j] in ascending j, float64 (v carries T-1 samples before position 0)."""
    T = taps.shape[1]
    acc = np.zeros(len(i))
    for j in range(T):
        acc = acc + taps[p, j] * v[T - 1 + i - j]
    return acc


def _whole(x, L, M, taps):
    """tests/test_cpu_resample.py::_plan over the whole signal: zero history, ceil(N*L/M) outputs."""
    n = np.arange(-(-len(x) * L // M))
    return _chain(taps, np.concatenate([np.zeros(taps.shape[1] - 1), x]), n * M // L, n * M % L)


def _ragged(x, cuts, L, M, taps):
    """afx_k_ingest's plan: per packet the reduced (n_out, p0, d0) of the absolute counters, the packet's own positions,
    the carried T-1 samples before it."""
    from afx.ingest import plan
    T = taps.shape[1]
    hist, N, parts, counts = np.zeros(T - 1), 0, [], []
    for n in cuts:
        pk = x[N:N + n]
        n_out, p0, d0 = plan(N, n, L, M)
        assert 0 <= p0 < L and 0 <= d0 <= -(-M // L)
        q = np.arange(n_out) * M + p0
        i = d0 + q // L
        assert n_out == 0 or (i.max() < n and i.min() >= 0)  # the newest input of every new output lies in the packet
        v = np.concatenate([hist, pk])
        parts.append(_chain(taps, v, i, q % L))
        hist = v[len(v) - (T - 1):]
        counts.append(n_out)
        N += n
    return np.concatenate(parts), counts


def _cuts(rate, total, rng):
    hop_in = -(-H * rate // 16000)
    cuts = [int(2.3 * hop_in), 0, 1, 7]  # every kind at least once, the rest at random
    left = total - sum(cuts)
    while left:
        n = min(left, rng.choice([0, 1, 1, 7, rate // 50, 3 * rate // 100 + 1]))
        cuts.append(n)
        left -= n
    rng.shuffle(cuts)
    return cuts


@pytest.mark.parametrize("rate", RATES)
def test_plan_counts_and_ragged_index_plan_equal_the_whole_signal(rate):
    from afx.resample import design_filter, phase_taps
    L, M, h = design_filter(rate)
    taps = phase_taps(L, h)
    rng = random.Random(rate)
    total = int(5.2 * H * rate / 16000) + 3
    x = np.random.default_rng(rate).standard_normal(total)
    whole = _whole(x, L, M, taps)
    for trial in range(3):
        cuts = _cuts(rate, total, rng) if trial else [1] * 40 + [0, total - 40]
        got, counts = _ragged(x, cuts, L, M, taps)
        assert sum(counts) == -(-total * L // M) == len(whole)
        assert max(cuts) > 2 * H * rate // 16000 and 0 in cuts and 1 in cuts
        assert np.array_equal(got, whole)


def test_plan_reduces_long_sessions_to_small_numbers():
    from afx.ingest import plan
    from afx.resample import ratio
    for rate in (192000, 44100, 11025, 8000):
        L, M = ratio(rate)
        N = rate * 3600 * 30 + 17  # thirty hours in
        n_out, p0, d0 = plan(N, rate // 50, L, M)
        assert abs(n_out - 320) <= 1 and 0 <= p0 < L and 0 <= d0 <= -(-M // L)


# ---- the packer, the refusals and the state, on a host-only scorer -------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    return packet_helpers.built()


def _host(S=2, rate=8000, encoding="pcm_s16le", max_pending=4):
    from afx.ingest import PacketScorer
    from afx.streaming import SlidingWindowScorer
    return PacketScorer(SlidingWindowScorer(None, S, window=16000, hop=H, device="cpu"), rate, encoding, max_pending)


def test_payloads_of_mixed_types_and_the_staging_layout():
    from afx.ingest import ALIGN, HDR, layout, pack, payload
    pcm = np.arange(-5, 6, dtype=np.int16)
    raw = pcm.astype("<i2").tobytes()
    for form in (raw, bytearray(raw), memoryview(raw), np.frombuffer(raw, dtype=np.uint8), pcm, torch.from_numpy(pcm.copy()),
                 torch.frombuffer(bytearray(raw), dtype=torch.uint8)):
        a = payload(form, "pcm_s16le")
        assert a.dtype == np.uint8 and a.ndim == 1 and a.tobytes() == raw
    f = np.linspace(-1, 1, 7, dtype=np.float32)
    assert payload(f, "pcm_f32le").tobytes() == f.astype("<f4").tobytes() == payload(f.tobytes(), "pcm_f32le").tobytes()
    assert payload(b"\x00\xff\x7f", "mulaw").tolist() == [0, 255, 127] and payload(b"", "alaw").size == 0
    for bad, enc in ((b"abc", "pcm_s16le"), (b"abcde", "pcm_f32le"), (pcm, "mulaw"), (pcm.astype(np.float64), "pcm_s16le"),
                     (f, "pcm_s16le"), (pcm.reshape(1, -1), "pcm_s16le"), ("text", "mulaw"), ([1, 2], "mulaw"), (raw, "opus")):
        with pytest.raises(ValueError):
            payload(bad, enc)
    pays = [payload(raw, "pcm_s16le"), payload(b"", "pcm_s16le"), payload(pcm[:3], "pcm_s16le")]
    offs, total = layout([p.size for p in pays])
    assert offs == [0, 32, 32] and total == 48
    tables = [np.arange(2 * HDR, dtype=np.int32).reshape(2, HDR), np.array([[1, 7]], dtype=np.int32)]
    buf, po, to = pack(pays, tables)
    assert po == offs and all(o % ALIGN == 0 for o in po + to) and buf.dtype == torch.uint8 and buf.numel() % ALIGN == 0
    b = buf.numpy()
    assert b[:22].tobytes() == raw and b[32:38].tobytes() == raw[:6]
    assert np.array_equal(b[to[0]:to[0] + 64].view(np.int32).reshape(2, HDR), tables[0])
    assert b[to[1]:to[1] + 8].view(np.int32).tolist() == [1, 7]


def test_header_fields_of_a_planned_feed():
    from afx.ingest import plan
    ps = _host(S=3, rate=11025, encoding="mulaw", max_pending=2)
    L, M = ps.L, ps.M
    assert (L, M) == (640, 441) and ps.ring_len == 3 * H
    ops, counts, (head, fill, nin) = ps._plan([2, 0], [221, 9000], [0, 224], score=True)
    kinds = [op[0] for op in ops]
    assert kinds[0] == "ingest" and "pop" in kinds
    first = ops[0][1]
    assert first.dtype == np.int32 and first.shape == (2, 8)
    assert first[0].tolist() == [2, 0, 221, plan(0, 221, L, M)[0], 0, 0, 0, 0]
    assert first[1].tolist()[:3] == [0, 224, min(9000, 3 * H * M // L)]  # what the ring has room for
    total = -(-9000 * L // M)
    assert counts == [0, total // H] and fill == [total % H, 0, plan(0, 221, L, M)[0]] and nin == [9000, 0, 221]
    assert head[0] == (total // H) * H % ps.ring_len
    # the rows of the later rounds continue the packet where the first stopped, at the phase the counters give
    rest = [op[1][0] for op in ops[1:] if op[0] == "ingest"]
    done = int(first[1][2])
    for r in rest:
        n_out, p0, d0 = plan(done, int(r[2]), L, M)
        assert r.tolist()[:6] == [0, 224 + done, int(r[2]), n_out, p0, d0]
        done += int(r[2])
    assert done == 9000
    assert torch.equal(ps.pending, torch.zeros(3, dtype=torch.int64))  # planning changes nothing


def test_refusals_leave_a_host_scorer_unchanged(built):
    from afx._lib import AfxError
    from afx.ingest import ENCODINGS, PacketScorer
    from afx.streaming import SlidingWindowScorer
    assert ENCODINGS == ("pcm_f32le", "pcm_s16le", "mulaw", "alaw")
    sc = SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu")
    for rate in (7999, 192001, 44100.5, "8000", True):
        with pytest.raises(ValueError):
            PacketScorer(sc, rate)
    for kw in (dict(encoding="g722"), dict(max_pending=0), dict(max_pending=1.5)):
        with pytest.raises(ValueError):
            PacketScorer(sc, 8000, **kw)
    for rate in (11025, 22050, 16000, 8000, 192000):
        assert PacketScorer(sc, np.int64(rate)).input_rate == rate
    ps = _host()
    assert ps.S == 2 and ps.device.type == "cpu" and ps.delay == 20 and ps.hop == H
    # a session with pending samples: 50 input samples at 8 kHz made 100 outputs, none scored yet
    st = ps.export_slots([0])
    st.tensors["ingest_fill"] = torch.tensor([100])
    st.tensors["ingest_in"] = torch.tensor([50])
    st.tensors["ingest_pending"][0, :100] = torch.arange(100.0)
    ps.import_slots([1], st)

    def snap():
        e = ps.export_slots([0, 1])
        return [ps.pending, ps.samples_in, ps.samples_seen, ps.scorer.samples_seen] + [e.tensors[k] for k in sorted(e.tensors)]

    before = snap()
    assert before[0].tolist() == [0, 100] and before[1].tolist() == [0, 50]
    pk = np.zeros(160, dtype=np.int16)
    bad = [(([pk], [0, 1]), {}), (([pk, pk], [0]), {}), (([pk, pk], [0, 2]), {}), (([pk, pk], [1, 1]), {}),
           (([pk, b"abc"], [0, 1]), {}), (([pk, pk.astype(np.float32)], [0, 1]), {}), ((pk.tobytes(), [0]), {}),
           (([pk, pk], [True, False, True]), {}), (([pk, pk], [0.0, 1.0]), {}),
           (([np.zeros((4 * H - 100) // 2 + 1, dtype=np.int16)], [1]), dict(score=False)),  # 100 + 2n > 4 hops
           (([np.zeros(4 * H // 2 + 1, dtype=np.int16), pk], [0, 1]), dict(score=False))]
    for args, kw in bad:
        with pytest.raises(ValueError):
            ps.feed(*args, **kw)
        assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    with pytest.raises(ValueError):
        ps.drain([2])
    with pytest.raises(AfxError):  # valid, but there is no GPU behind this scorer: nothing changes either
        ps.feed([pk, pk], [0, 1])
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    res = ps.feed([b"", bytearray()], [1, 0])  # empty packets are legal and complete nothing
    assert res.counts.tolist() == [0, 0] and res.scores.numel() == 0 and res.split()[0].numel() == 0
    assert ps.drain().counts.tolist() == [0, 0]
    ps.reset([1])
    assert ps.pending.tolist() == [0, 0] and ps.samples_in.tolist() == [0, 0]


def test_state_keys_meta_and_cross_refusals(built):
    from afx.ingest import INGEST_FORMAT
    from afx.streaming import ResamplingScorer, SlidingWindowScorer, StreamState
    ps = _host(S=2, rate=48000, max_pending=3)
    st = ps.export_slots([1, 0])
    assert set(st.tensors) == {"samples", "ingest_pending", "ingest_fill", "ingest_in", "resample_hist"}
    assert tuple(st.tensors["ingest_pending"].shape) == (2, 3 * H) and tuple(st.tensors["resample_hist"].shape) == (2, 60)
    assert st.tensors["ingest_fill"].dtype == st.tensors["ingest_in"].dtype == torch.int64
    assert not st.tensors["ingest_pending"].any() and st.tensors["ingest_fill"].tolist() == [0, 0]
    assert st.meta["input_rate"] == 48000 and st.meta["resampler"] == "kaiser5-hl10" and st.meta["ingest"] == INGEST_FORMAT
    assert ps.state_meta() == st.meta and "encoding" not in st.meta
    st2 = StreamState.from_state_dict(st.to("cpu").state_dict())
    _host(S=3, rate=48000, encoding="alaw", max_pending=1).import_slots([2, 0], st2)  # any encoding, any S, any max_pending that fits
    bare = SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu")
    wrapped = ResamplingScorer(SlidingWindowScorer(None, 2, window=16000, hop=H, device="cpu"), 48000)
    for dst in (bare, wrapped):
        with pytest.raises(ValueError):
            dst.import_slots([0, 1], st)
    for foreign in (bare.export_slots([0, 1]), wrapped.export_slots([0, 1]), _host(rate=24000).export_slots([0, 1]),
                    st.tensors, None):
        with pytest.raises(ValueError):
            ps.import_slots([0, 1], foreign)
    for key, val in (("resampler", "other"), ("ingest", INGEST_FORMAT + 1), ("hop", 2000)):
        with pytest.raises(ValueError):
            ps.import_slots([0, 1], StreamState(dict(st.meta, **{key: val}), st.seen, st.tensors))
    with pytest.raises(ValueError):
        ps.import_slots([0], st)  # two sessions for one slot
    # more pending samples than the destination holds; counters that contradict each other
    full = _host(S=1, rate=48000, max_pending=3).export_slots([0])
    full.tensors["ingest_fill"] = torch.tensor([2 * H + 1])
    full.tensors["ingest_in"] = torch.tensor([3 * (2 * H + 1)])
    small = _host(S=1, rate=48000, max_pending=2)
    with pytest.raises(ValueError):
        small.import_slots([0], full)
    ps.import_slots([0], full)
    assert ps.pending.tolist() == [2 * H + 1, 0] and ps.samples_in.tolist() == [3 * (2 * H + 1), 0]
    full.tensors["ingest_in"] = torch.tensor([17])
    with pytest.raises(ValueError):
        ps.import_slots([1], full)
    assert ps.pending.tolist() == [2 * H + 1, 0]


def test_ingest_entry_points_are_in_header_library_and_ctypes_table(built):
    src = open(os.path.join(ROOT, "include", "afx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(built.LIB_PATH)
    for name in ("afx_k_ingest", "afx_k_ingest_pop"):
        assert re.search(r"\b%s\s*\(" % name, src) and hasattr(lib, name) and name in built.SIGNATURES
    l = built.lib()
    assert l.afx_k_ingest(None, 0, None, 1, 0, 0, None, 1, 1, 1, None, None, 1, 1, None) != 0  # refused on the host: nothing launched
    assert b"ingest" in l.afx_last_error()
    assert l.afx_k_ingest_pop(None, 1, 1, None, 1, 1, None, None) != 0 and b"ingest_pop" in l.afx_last_error()

"""Moving sessions (afx/streaming.py ``export_slots`` / ``import_slots`` / ``StreamState``).  The contract: a session that has
received n hops in slot a of scorer X and is imported into slot b of scorer Y emits as its j-th score after the import,
bit for bit, X's uninterrupted score at hop n + j -- whatever Y's number of slots, whatever Y's other slots hold, through
host memory and torch.save / torch.load, exported before the first hop, during warm-up, in the steady state or after the
KV ring wrapped.  Y's other slots emit what they would without the import, and X is not changed by the export."""
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 4000
W_EXACT, W_KV = 16000, 64000  # the KV-cached mode keeps its 4-s window: 17+ hops wrap its 16-group ring
SX, SY = 4, 3
A, B = 1, 2  # the session moves from slot A of X to slot B of Y


def _engine(arch, dtype="fp16", perturb=False):
    from afx import engine, synth
    if arch == "conformer":
        sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
        eng = engine.Engine("conformer", n_layers=1, dtype=dtype, conf_blocks=1)
    else:
        sd = synth.model_state_dict("XLSR_AASIST", n_layers=1)
        eng = engine.Engine("xlsr_aasist", n_layers=1, dtype=dtype)
    if perturb:  # the same architecture, other weights
        g = torch.Generator().manual_seed(77)
        sd = {k: (v + 1e-3 * torch.randn(v.shape, generator=g) if torch.is_tensor(v) and v.dtype.is_floating_point else v)
              for k, v in sd.items()}
    eng.load_state_dict(sd)
    return eng, sd


def _make(kind, eng, sd, S, window=None, hop=H):
    from afx.streaming import IncrementalScorer, KVCachedScorer, SlidingWindowScorer
    if kind == "sliding":
        return SlidingWindowScorer(eng, S, window=window or W_EXACT, hop=hop, state_dict=sd)
    if kind == "incremental":
        return IncrementalScorer(eng, sd, S, window=window or W_EXACT, hop=hop)
    return KVCachedScorer(eng, sd, S, window=window or W_KV, hop=hop)


def _audio(n_streams, hops, seed):
    from afx import synth
    return synth.waveforms(n_streams, hops * H, batch_idx=seed).reshape(n_streams, hops, H)


def _tick(sc, chunk, mode, t, S):
    """One tick: 'lock' pushes every slot; 'list' names every slot in a rotating order (slot A's score is at its position)."""
    if mode == "lock":
        return sc.push(chunk.cuda()).clone().cpu()
    order = [(i + t) % S for i in range(S)]
    out = sc.push(chunk[order].cuda(), slots=order).clone().cpu()
    res = torch.empty(S)
    res[order] = out
    return res


def _run_x(kind, eng, sd, audio, mode, exports=()):
    """X over every hop of ``audio`` (SX, N, H); exports slot A after the hops in ``exports`` -> (scores (N, SX), {n: state})."""
    sc = _make(kind, eng, sd, SX)
    scores, states = [], {}
    for t in range(audio.shape[1]):
        if t in exports:
            states[t] = sc.export_slots([A])
        scores.append(_tick(sc, audio[:, t], mode, t, SX))
    return torch.stack(scores), states


def _run_y(kind, eng, sd, other, session, mode, state=None, pre=3):
    """Y: SY slots busy at other phases (slot 0 reset after one hop), ``pre`` hops of ``other``; then (with ``state``) slot B
    takes over the session and every slot goes on: slot B with ``session`` (its hops after the export), the others with
    ``other`` -> scores (hops after the import, SY)."""
    sc = _make(kind, eng, sd, SY)
    for t in range(pre):
        if t == 1:
            sc.reset([0])
        _tick(sc, other[:, t], mode, t, SY)
    before = sc.samples_seen
    if state is not None:
        sc.import_slots([B], state)
        want = before.clone()
        want[B] = int(state.seen[0])
        assert torch.equal(sc.samples_seen, want)
    out = []
    for j in range(session.shape[0]):
        chunk = other[:, pre + j].clone()
        chunk[B] = session[j]
        out.append(_tick(sc, chunk, mode, pre + j, SY))
    return torch.stack(out)


def _through_host(state):
    from afx.streaming import StreamState
    buf = io.BytesIO()
    torch.save(state.to("cpu").state_dict(), buf)
    buf.seek(0)
    return StreamState.from_state_dict(torch.load(buf, weights_only=True))


CASES = [("sliding", "conformer", "fp16"), ("sliding", "xlsr_aasist", "fp16"), ("incremental", "conformer", "fp16"),
         ("incremental", "xlsr_aasist", "fp16"), ("kv", "conformer", "fp16"), ("kv", "xlsr_aasist", "fp16"),
         ("kv", "xlsr_aasist", "fp16x3")]


@pytest.mark.parametrize("kind,arch,dtype", CASES)
def test_a_moved_session_continues_bit_for_bit(kind, arch, dtype):
    eng, sd = _engine(arch, dtype)
    kv = kind == "kv"
    # export points: before the first hop, during warm-up, steady state, after the ring wrapped (KV: 17 chunks; exact: the
    # 16-s sample ring), each with its own X -> Y path: lock-stepped / non-paced on either side
    N = 20 if kv else 9
    points = [(0, "lock", "list"), (5 if kv else 2, "list", "lock"), (12 if kv else 5, "lock", "lock"), (17 if kv else 7, "list", "list")]
    audio = _audio(SX, N, 6100)
    other = _audio(SY, 3 + N, 6200)
    x = {}
    for mode in ("lock", "list"):
        x[mode] = _run_x(kind, eng, sd, audio, mode, exports=[n for n, m, _ in points if m == mode])
    twin, _ = _run_x(kind, eng, sd, audio, "lock")
    # the export changed nothing: every slot of X scores as in a twin that exported nothing (and both paths agree on slot A)
    assert torch.equal(x["lock"][0], twin), f"{kind} {arch} {dtype}: X changed by its exports"
    assert torch.equal(x["list"][0][:, A], twin[:, A])
    for n, xmode, ymode in points:
        state = _through_host(x[xmode][1][n])
        assert len(state) == 1 and int(state.seen[0]) == n * H
        got = _run_y(kind, eng, sd, other, audio[A, n:], ymode, state)
        ref = twin[n:, A]
        for j in range(ref.shape[0]):
            assert torch.equal(got[j, B], ref[j]), \
                f"{kind} {arch} {dtype}: exported after {n} hops ({xmode} -> {ymode}), hop {j} after the import: {(got[j, B] - ref[j]).abs().item():.2e}"
        # Y's other slots: what a twin Y without the import emits (and slot B itself: not what it emits without the import)
        ytwin = _run_y(kind, eng, sd, other, audio[A, n:], ymode, None)
        keep = [k for k in range(SY) if k != B]
        assert torch.equal(got[:, keep], ytwin[:, keep]), f"{kind} {arch} {dtype}: the import changed another slot of Y"
        assert not torch.equal(got[:, B], ytwin[:, B])


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_park_on_the_host_and_return_to_another_slot(kind):
    """Export to the host, torch.save / torch.load, reset the slot, run another session in it, import the parked session into
    another slot of the same scorer: it continues as the uninterrupted twin's slot does."""
    eng, sd = _engine("conformer")
    n, N, gap = (9, 14, 3) if kind == "kv" else (5, 10, 3)
    audio = _audio(SX, N, 6300)
    filler = _audio(1, gap + N, 6400)[0]
    twin = _make(kind, eng, sd, SX)
    ref = torch.stack([_tick(twin, audio[:, t], "lock", t, SX) for t in range(N)])
    sc = _make(kind, eng, sd, SX)
    for t in range(n):
        _tick(sc, audio[:, t], "lock", t, SX)
    parked = _through_host(sc.export_slots([1]))
    sc.reset([1])
    for t in range(gap):  # slot 1 runs another session; slot 3 idles (fed silence) -- its session is dropped by the import
        chunk = audio[:, n].clone() * 0
        chunk[0], chunk[2] = audio[0, min(n + t, N - 1)], audio[2, min(n + t, N - 1)]
        chunk[1] = filler[t]
        _tick(sc, chunk, "list" if t % 2 else "lock", t, SX)
    sc.import_slots([3], parked)
    assert int(sc.samples_seen[3]) == n * H and int(sc.samples_seen[1]) == gap * H
    for j in range(N - n):
        chunk = torch.zeros(SX, H)
        chunk[3], chunk[1] = audio[1, n + j], filler[gap + j]
        out = _tick(sc, chunk, "lock", j, SX)
        assert torch.equal(out[3], ref[n + j, 1]), f"{kind}: the parked session, hop {j} after its return"


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_compacting_a_scorer_moves_slot_3_to_slot_0(kind):
    eng, sd = _engine("xlsr_aasist")
    n, N = (6, 10) if kind == "kv" else (3, 8)
    audio = _audio(SX, N, 6500)
    twin = _make(kind, eng, sd, SX)
    ref = torch.stack([_tick(twin, audio[:, t], "lock", t, SX) for t in range(N)])
    sc = _make(kind, eng, sd, SX)
    for t in range(n):
        _tick(sc, audio[:, t], "lock", t, SX)
    sc.import_slots([0], sc.export_slots([3]))
    sc.reset([3])
    for j in range(N - n):
        chunk = audio[:, n + j].clone()
        chunk[0] = audio[3, n + j]
        out = _tick(sc, chunk, "list", j, SX)
        assert torch.equal(out[0], ref[n + j, 3]), (kind, j)
        assert torch.equal(out[[1, 2]], ref[n + j, [1, 2]]), (kind, j)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: the cuda:0 -> cuda:1 migration was NOT run on this machine")
@pytest.mark.parametrize("kind", ["incremental", "kv"])
def test_migrate_between_gpus(kind):
    from afx import engine, synth
    sd = synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1)
    engs = []
    for d in (0, 1):
        e = engine.Engine("conformer", n_layers=1, dtype="fp16", conf_blocks=1, device=f"cuda:{d}")
        e.load_state_dict(sd)
        engs.append(e)
    n, N = (8, 12) if kind == "kv" else (5, 8)
    audio = _audio(SX, N, 6600)
    x = _make(kind, engs[0], sd, SX)
    ref = torch.stack([x.push(audio[:, t].to("cuda:0")).cpu() for t in range(N)])
    x = _make(kind, engs[0], sd, SX)
    for t in range(n):
        x.push(audio[:, t].to("cuda:0"))
    st = x.export_slots([A]).to("cuda:1")
    y = _make(kind, engs[1], sd, SY)
    y.import_slots([B], st)
    for j in range(N - n):
        chunk = torch.zeros(SY, H)
        chunk[B] = audio[A, n + j]
        out = y.push(chunk.to("cuda:1")).cpu()
        assert torch.equal(out[B], ref[n + j, A]), (kind, j)


def _unchanged_after(sc, twin, fn, exc):
    """fn(sc) raises exc; sc's samples_seen and next scores are those of its twin."""
    seen = sc.samples_seen
    with pytest.raises(exc):
        fn(sc)
    assert torch.equal(sc.samples_seen, seen)
    chunk = _audio(sc.S, 1, 6800)[:, 0].cuda()
    assert torch.equal(sc.push(chunk).cpu(), twin.push(chunk).cpu())


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_refusals_leave_the_destination_unchanged(kind):
    from afx._lib import AfxError
    eng, sd = _engine("conformer")
    audio = _audio(SY, 2, 6700)

    def dest():
        sc = _make(kind, eng, sd, SY)
        for t in range(2):
            sc.push(audio[:, t].cuda())
        return sc
    src = _make(kind, eng, sd, SX)
    src.push(_audio(SX, 1, 6750)[:, 0].cuda())
    st = src.export_slots([0, 2])
    others = {"kind": _make("incremental" if kind != "incremental" else "sliding", eng, sd, SX),
              "window": _make(kind, eng, sd, SX, window=(W_KV if kind == "kv" else W_EXACT) + 2 * H),
              "hop": _make(kind, eng, sd, SX, window=W_KV if kind == "kv" else 24000, hop=2 * H if kind != "sliding" else 3000)}
    e16b, sdb = _engine("conformer", "bf16")
    others["dtype"] = _make(kind, e16b, sdb, SX)
    e2, sd2 = _engine("conformer", perturb=True)
    others["weights"] = _make(kind, e2, sd2, SX)
    for what, o in others.items():
        foreign = o.export_slots([0, 1])
        _unchanged_after(dest(), dest(), lambda sc: sc.import_slots([0, 1], foreign), ValueError)
    _unchanged_after(dest(), dest(), lambda sc: sc.import_slots([0], st), ValueError)  # two sessions, one slot
    _unchanged_after(dest(), dest(), lambda sc: sc.import_slots([1, 1], st), ValueError)
    if kind == "kv":  # a corrupted layout word passes the scorer's checks and is refused by the library
        bad = st.to("cpu")
        bad.tensors["kv_meta"] = bad.tensors["kv_meta"].clone()
        bad.tensors["kv_meta"][1, 0] ^= 1
        _unchanged_after(dest(), dest(), lambda sc: sc.import_slots([0, 2], bad), AfxError)
        kvs = eng.kv_state(2)
        p, m = kvs.export([1])
        m[0, 0] ^= 1 << 8  # another dtype
        with pytest.raises(AfxError):
            kvs.import_([0], p, m)


@pytest.mark.parametrize("kind", ["sliding", "incremental", "kv"])
def test_a_session_before_its_first_hop_into_a_used_scorer_whose_slots_all_restart(kind):
    """After the import every slot of the destination is at samples_seen 0, so it takes the lock-stepped path again: the
    carries of the sessions it dropped must not reach the first hop.  It scores as a fresh scorer of its size does."""
    eng, sd = _engine("conformer")
    state = _through_host(_make(kind, eng, sd, SX).export_slots([A]))  # before the first hop
    for S in (1, 2):
        y = _make(kind, eng, sd, S)
        used = _audio(S, 3, 6900)
        for t in range(3):
            y.push(used[:, t].cuda())
        if S == 2:
            y.reset([0])
        y.import_slots([S - 1], state)
        assert y.samples_seen.tolist() == [0] * S
        fresh = _make(kind, eng, sd, S)
        audio = _audio(S, 6, 6950)
        for t in range(6):
            a, b = y.push(audio[:, t].cuda()).cpu(), fresh.push(audio[:, t].cuda()).cpu()
            assert torch.equal(a, b), (kind, S, t)


@pytest.mark.parametrize("kind,arch,dtype", [("incremental", "conformer", "fp16"), ("kv", "conformer", "fp16"),
                                             ("kv", "xlsr_aasist", "fp16x3")])
def test_a_session_reset_mid_ring_moves_twice(kind, arch, dtype):
    """A session reset at tick 3 (KV: its first chunk in ring group 3) moves X (lock-stepped, per-stream sessions) -> Y
    (non-paced) -> Z (lock-stepped, one slot reset at another tick), each export from a non-zero base group, and wraps its
    ring in Z.  Every hop scores as the same audio in a fresh scorer."""
    eng, sd = _engine(arch, dtype)
    L = 22
    sess = _audio(1, L, 7000)[0]
    fresh = _make(kind, eng, sd, 1)
    ref = [fresh.push(sess[j:j + 1].cuda()).cpu()[0] for j in range(L)]
    got = []
    x, bg = _make(kind, eng, sd, SX), _audio(SX, 8, 7100)
    for t in range(8):  # session hops 0..4 in X
        if t == 3:
            x.reset([A])
        chunk = bg[:, t].clone()
        if t >= 3:
            chunk[A] = sess[t - 3]
        out = x.push(chunk.cuda()).cpu()
        if t >= 3:
            got.append(out[A])
    state = _through_host(x.export_slots([A]))
    y, ybg = _make(kind, eng, sd, SY), _audio(SY, 8, 7200)
    for t in range(2):
        _tick(y, ybg[:, t], "list", t, SY)
    y.import_slots([B], state)
    for j in range(6):  # session hops 5..10 in Y
        chunk = ybg[:, 2 + j].clone()
        chunk[B] = sess[5 + j]
        got.append(_tick(y, chunk, "list", j, SY)[B])
    state = _through_host(y.export_slots([B]))
    z, zbg = _make(kind, eng, sd, 2), _audio(2, 5 + L - 11, 7300)
    for t in range(5):
        if t == 2:
            z.reset([0])
        z.push(zbg[:, t].cuda())
    z.import_slots([1], state)
    for j in range(L - 11):  # session hops 11..21 in Z
        chunk = zbg[:, 5 + j].clone()
        chunk[1] = sess[11 + j]
        got.append(z.push(chunk.cuda()).cpu()[1])
    for j in range(L):
        assert torch.equal(got[j], ref[j]), f"{kind} {arch} {dtype}: session hop {j}: {(got[j] - ref[j]).abs().item():.2e}"

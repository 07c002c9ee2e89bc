"""The KV step's state model and references (oracle/insitu_kv.py) must catch what they claim, without a GPU.

A simulated CORRECT step (``SimKv``: torch fp32 ops on the rounded operands, its own ring / history / window state, the
tap names of the library) is walked launch by launch with ``kv_walk``:

  * in fp32, lock-stepped over 19 hops of a short random stream (the ring wraps), every per-launch check passes and the
    windows the model accumulates equal those of the offline restatement ``oracle/streaming.block_causal_scores`` to
    fp32 noise -- the new bookkeeping is tied to the function the project already states;
  * in fp16, as ragged sessions, every check passes, and each injected defect of the last step fails its own check: a
    value check by at least 10x its bound, an exact statement (pad rows, left context, window, head input) by its own
    measure.

The q projection is scaled by ``Q_GAIN`` so that the softmax over ~200 keys is peaked enough for ONE wrong slot to clear
10x the attention bound (as the dropped-key test of tests/test_cpu_insitu.py draws unit-variance q and k)."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import insitu as I
from oracle import insitu_kv as K

S, D, C, HOP, HOPS = 2, 1024, 512, 4000, 19
Q_GAIN = 2.0


class SimKv:
    """A correct step in fp32 arithmetic on operands rounded to `dt`, with the state the library keeps: rings (layers, S,
    256, 3 D), 64 history rows and a 208-row window per stream, a group per hop.  `defect` (set for one step) injects one
    bookkeeping error.  step() -> the step's taps, by the library's names."""

    def __init__(self, sd, dt, S, n_layers=1):
        self.sd, self.dt, self.S, self.L = sd, dt, S, n_layers
        self.hop, self.defect = 0, None
        self.rings = torch.zeros(n_layers, S, K.SLOTS, 3 * D)
        self.hist = torch.zeros(S, K.HIST, D)
        self.win = torch.zeros(S, K.FEAT, D)
        self.cnt = [[0] * K.GROUPS for _ in range(S)]
        self.nfeat = [0] * S
        self.w_pos = self.rnd(I.pos_weight({k: v.float() for k, v in sd.items() if k.startswith("encoder.pos_conv")}).float())

    def rnd(self, x):
        return I.op(x.double(), self.dt).float()

    def ln(self, x, p):
        return F.layer_norm(x, (x.shape[-1],), self.sd[p + "weight"], self.sd[p + "bias"], I.LN_EPS)

    def lin(self, a, w, b):
        return a @ self.rnd(w).t() + b

    def attend(self, ring, s, g, n, cnt, old):
        H, dh = 16, D // 16
        cnt = list(cnt)
        if self.defect == "stale_slot_live":  # the group keeps its previous occupant's count
            cnt[g] = max(cnt[g], old)
        live = [K.GROUP_SLOTS * j + r for j in range(K.GROUPS) for r in range(cnt[j])]
        if self.defect == "oldest_last_slot_masked":
            oldest = next(j % K.GROUPS for j in range(g + 1, g + 1 + K.GROUPS) if cnt[j % K.GROUPS])
            live.remove(K.GROUP_SLOTS * oldest + cnt[oldest] - 1)
        qg = (g - 1) % K.GROUPS if self.defect == "queries_from_previous_group" else g
        ks = (s + 1) % self.S if self.defect == "keys_from_neighbour_stream" else s
        q = ring[s, K.GROUP_SLOTS * qg:K.GROUP_SLOTS * qg + n, :D].reshape(n, H, dh)
        k = ring[ks, live, D:2 * D].reshape(len(live), H, dh)
        v = ring[s, live, 2 * D:].reshape(len(live), H, dh)
        sc = torch.einsum("rhd,thd->rht", q, k) * dh ** -0.5
        p = torch.exp(sc - sc.amax(-1, keepdim=True))
        o = torch.einsum("rht,thd->rhd", self.rnd(p), v) / p.sum(-1)[..., None]  # (P rounded to the operand type before P.V)
        return o.reshape(n, D)

    def step(self, feats6, n_frames=None):
        sd, S, n = self.sd, self.S, feats6.shape[1]
        ns = [n] * S if n_frames is None else list(n_frames)
        g = self.hop % K.GROUPS
        t = {}
        feats = self.rnd(self.ln(feats6.float().reshape(S * n, C), "layer_norm."))
        proj = self.lin(feats, sd["post_extract_proj.weight"], sd["post_extract_proj.bias"])
        xpad = torch.zeros(S, 3 * K.HIST + n, D)
        for s in range(S):
            xpad[s, K.HIST:2 * K.HIST] = self.hist[(s + 1) % S if self.defect == "left_context_of_wrong_stream" else s]
            xpad[s, 2 * K.HIST:2 * K.HIST + ns[s]] = self.rnd(proj).reshape(S, n, D)[s, :ns[s]]
        if self.defect == "nonzero_row_past_the_chunk":
            xpad[S - 1, 2 * K.HIST + ns[S - 1], 7] = 2.0 ** -14
        view = xpad[:, K.HIST:]
        if self.defect == "posconv_window_shifted":
            view = torch.cat([view[:, 1:], torch.zeros(S, 1, D)], 1)
        y = F.conv1d(view.transpose(1, 2), self.w_pos, sd["encoder.pos_conv.0.bias"], groups=16)[:, :, :n]
        x = proj + F.gelu(y.transpose(1, 2).reshape(S * n, D))
        t.update({"kv.feats": feats, "kv.proj": proj, "kv.xpad": xpad, "kv.pos": x})
        for s in range(S):
            self.hist[s] = xpad[s, K.HIST + ns[s]:2 * K.HIST + ns[s]].clone()
        old = [self.cnt[s][g] for s in range(S)]
        for s in range(S):
            self.cnt[s][g] = ns[s]
        for l in range(self.L):
            p, m = f"encoder.layers.{l}.", f"kv.l{l}."
            ln1 = self.rnd(self.ln(x, p + "self_attn_layer_norm."))
            w = torch.cat([sd[p + f"self_attn.{c}_proj.weight"] for c in "qkv"], 0)
            b = torch.cat([sd[p + f"self_attn.{c}_proj.bias"] for c in "qkv"], 0)
            qkv = self.rnd(self.lin(ln1, w, b)).reshape(S, n, 3 * D)
            wg = (g + 1) % K.GROUPS if self.defect == "chunk_written_one_group_off" else g
            self.rings[l][:, K.GROUP_SLOTS * wg:K.GROUP_SLOTS * wg + n] = qkv
            att = torch.zeros(S, K.GROUP_SLOTS, D)
            for s in range(S):
                att[s, :n] = self.attend(self.rings[l], s, g, n, self.cnt[s], old[s])
            att = self.rnd(att)
            mid = x + self.lin(att[:, :n].reshape(S * n, D), sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
            ln2 = self.rnd(self.ln(mid, p + "final_layer_norm."))
            ff = self.rnd(F.gelu(self.lin(ln2, sd[p + "fc1.weight"], sd[p + "fc1.bias"])))
            x = mid + self.lin(ff, sd[p + "fc2.weight"], sd[p + "fc2.bias"])
            t.update({m + "ln1": ln1, m + "ring": self.rings[l].clone(), m + "att": att, m + "mid": mid, m + "ln2": ln2, m + "ff": ff,
                      f"kv.layer{l}": x})
        fl = self.ln(x, "encoder.layer_norm.").reshape(S, n, D)
        th = [min(self.nfeat[s] + ns[s], K.WINDOW) for s in range(S)]
        for s in range(S):
            up = n if self.defect == "window_shifted_by_n_max" else ns[s]
            self.win[s] = torch.cat([self.win[s][up:], fl[s, :up]])
            self.nfeat[s] = min(self.nfeat[s] + ns[s], K.FEAT)
        t["kv.win"] = self.win.clone()
        if n_frames is None:
            t["ssl"] = self.win[:, K.FEAT - th[0]:].clone()
        else:
            t["kv.fl"] = fl
            head = torch.zeros(S, max(th), D)
            for s in range(S):
                if self.defect == "head_window_right_aligned":
                    head[s, max(th) - th[s]:] = self.win[s, K.FEAT - th[s]:]
                else:
                    head[s, :th[s]] = self.win[s, K.FEAT - th[s]:]
            t["ssl"] = head
        self.hop += 1
        return t


def walk(sim, model, sd, frames, n_frames, prev):
    """One simulated step, walked: -> (results, fails, rings)."""
    plan = model.begin(frames.shape[1], n_frames)
    t = sim.step(frames, n_frames)
    return K.kv_walk(sd, sim.dt, lambda name: t[name].double().reshape(-1), model, plan, frames, prev)


def worst(res):
    return max(res, key=lambda r: r[2]["ratio"])


@pytest.fixture(scope="module")
def stream():
    """A short random stream, its conv features, a one-layer Conformer student with the q projection scaled."""
    from afx import synth
    from oracle import models as om
    from oracle import ssl_trunk
    sd = dict(synth.model_state_dict("ConformerModel", n_layers=1, n_encoders=1))
    for k in list(sd):
        if "self_attn.q_proj" in k:
            sd[k] = sd[k] * Q_GAIN
    ssl, _head = om.split(sd)
    wave = torch.cat([synth.waveforms(S, HOP, batch_idx=7100 + i) for i in range(HOPS)], dim=1)
    with torch.no_grad():
        feats = ssl_trunk.feature_extractor(ssl, wave)  # (S, T, 512)
    return sd, ssl, wave, feats


def test_model_and_references_reproduce_the_restatement_in_fp32(stream):
    from oracle import streaming as ostream
    sd, ssl, wave, feats = stream
    wins = []
    _, sizes = ostream.block_causal_scores(sd, wave, HOP, windows=wins)
    assert len(sizes) == HOPS and sizes[:4] == [12, 12, 13, 12] and sum(sizes) > K.FEAT
    sim, model = SimKv(ssl, "fp32", S), K.KvModel(S)
    prev, t0, top, rel = [torch.zeros(S, K.SLOTS, 3 * D, dtype=torch.float64)], 0, {}, 0.0
    with torch.no_grad():
        for i, n in enumerate(sizes):
            res, fails, prev = walk(sim, model, ssl, feats[:, t0:t0 + n], None, prev)
            t0 += n
            assert not fails, (i, fails)
            for cls, name, r, _op in res:
                assert r["ratio"] <= 1.0, (i, name, r)
                top[cls] = max(top.get(cls, 0.0), r["ratio"])
            assert model.hop == i + 1 and model.group(0) == (i + 1) % K.GROUPS
            for s in range(S):
                w = model.head_window(s)
                assert w.shape == wins[i][s].shape
                rel = max(rel, float((w - wins[i][s].double()).norm() / wins[i][s].double().norm()))
    print(f"fp32 simulated step, {HOPS} hops: worst ratio per class {top}; windows vs the restatement rel L2 <= {rel:.1e}")
    assert set(top) == {"kv_layernorm", "kv_product", "kv_posconv", "kv_ring"}
    assert rel <= 1e-5  # (fp32 noise: one transformer layer, unit-scale LayerNorm outputs)


# ragged sessions in fp16: stream 0 brings the restatement's chunk sizes, stream 1 fewer frames; 18 steps, the last one
# rewrites group 1 (13 -> 12 frames for stream 0) with the oldest group next to it
RAGGED = [(12, 5), (13, 7), (12, 12), (12, 1), (16, 9), (12, 3)] * 3


@pytest.fixture(scope="module")
def sessions(stream):
    """The simulated fp16 sessions up to the last step (every launch of every step checked), and the last step's input."""
    sd, ssl, wave, feats = stream
    sim, model = SimKv(ssl, "fp16", S), K.KvModel(S)
    prev, t0 = [torch.zeros(S, K.SLOTS, 3 * D, dtype=torch.float64)], [0, 0]

    def frames(ns):
        f = torch.zeros(S, max(ns), C)
        for s in range(S):
            f[s] = feats[s, t0[s]:t0[s] + max(ns)]  # (the rows past n_s: the frames that follow -- read, never scored)
            t0[s] += ns[s]
        return f

    with torch.no_grad():
        for i, ns in enumerate(RAGGED[:-1]):
            res, fails, prev = walk(sim, model, ssl, frames(ns), ns, prev)
            assert not fails, (i, fails)
            assert worst(res)[2]["ratio"] <= 1.0, (i, worst(res))
    assert sim.cnt[0][1] == 13 and RAGGED[-1][0] < 16 and model.feat[0].shape[0] >= K.WINDOW > model.feat[1].shape[0]
    return ssl, sim, model, prev, frames(RAGGED[-1]), RAGGED[-1]


def last_step(sessions, defect):
    ssl, sim, model, prev, f, ns = sessions
    sim, model = copy.deepcopy(sim), copy.deepcopy(model)
    sim.defect = defect
    with torch.no_grad():
        res, fails, _ = walk(sim, model, ssl, f, list(ns), prev)
    return {name: r["ratio"] for _cls, name, r, _op in res}, fails


def test_correct_last_step_passes(sessions):
    ratios, fails = last_step(sessions, None)
    assert not fails and max(ratios.values()) <= 1.0, (ratios, fails)


@pytest.mark.parametrize("defect,tap", [
    ("oldest_last_slot_masked", "kv.l0.att"),
    ("stale_slot_live", "kv.l0.att"),
    ("queries_from_previous_group", "kv.l0.att"),
    ("keys_from_neighbour_stream", "kv.l0.att"),
    ("chunk_written_one_group_off", "kv.l0.ring"),
    ("posconv_window_shifted", "kv.pos"),
])
def test_injected_defect_fails_its_value_check_by_10x(sessions, defect, tap):
    ratios, fails = last_step(sessions, defect)
    print(f"{defect}: {tap} at {ratios[tap]:.1f} x its bound")
    assert ratios[tap] >= 10, (defect, ratios[tap])
    others = {k: v for k, v in ratios.items() if k != tap and not (defect == "chunk_written_one_group_off" and k == "kv.l0.att")}
    assert max(others.values()) <= 1.0, others  # (every other launch is judged on its own tapped inputs: it still passes)
    if defect == "chunk_written_one_group_off":
        assert any("does not write moved" in f for f in fails), fails


@pytest.mark.parametrize("defect,tap,what", [
    ("left_context_of_wrong_stream", "kv.xpad", "left context"),
    ("nonzero_row_past_the_chunk", "kv.xpad", "nonzero rows past 64 + n_s"),
    ("window_shifted_by_n_max", "kv.win", "window buffer"),
    ("head_window_right_aligned", "ssl", "head's input"),
])
def test_injected_defect_fails_its_exact_statement(sessions, defect, tap, what):
    ratios, fails = last_step(sessions, defect)
    assert any(f.startswith(tap + ":") and what in f for f in fails), (defect, fails)
    assert max(ratios.values()) <= 1.0, ratios  # (the value checks use the launch's own tapped inputs: they still pass)

"""Per-launch fp64 references and a host-side state model for the KV-cached streaming step (TEST INFRASTRUCTURE).

The step (``afx_kv_step`` / ``afx_kv_step_ragged`` / ``afx_kv_step_active``, one body ``kv_trunk``) runs the trunk's kernel
families on the chunk's rows only, so its launches are checked with the references of ``oracle/insitu.py`` as they are
(``layernorm``, ``product``, ``posconv``, ``_softmax_av``, ``check`` and their constants).  What is new here is the
bookkeeping around them:

  * ``ring_mhsa``   the ring attention of one layer against the tapped ring: each row block's query slots attend to the
                    block's live slots; ``mhsa``'s bound formula over the live keys (at most 256).
  * ``KvModel``     what include/afx.h documents of the state, and nothing read from the library's tables: per stream its
                    base group, its next group, 16 valid counts, the last 64 projected operand rows and the feature rows
                    accumulated so far.  Lock-step and ragged steps write group ``hop % 16``; active steps write the
                    stream's own next group and advance it; ``reset`` starts a stream at the current group (in an active
                    state: the stream's own next group) with no valid slot, a zero left context and an empty window.
  * ``kv_walk``     every launch of ONE step against its reference, each built from the launch's own tapped inputs
                    (``Engine.tap``, the ``kv.`` names), and the exact statements: the pad rows of the padded buffer are 0,
                    its left context is the model's 64 rows bit for bit, every ring row the step does not write keeps
                    every bit, the window buffer and the head's input are the model's bit for bit.

Rows of a ragged block past its own ``n_s`` are unread by contract (include/afx.h): they get no value check; the walk
asserts that they are zero in the padded buffer, and the model never counts them live.

Launch classes (tests/test_gpu_insitu_kv.py prints the worst ratio |got - ref| / bound per class and dtype; no new
constant): ``kv_layernorm`` (feature / ln1 / ln2 / final LayerNorm), ``kv_product`` (projection, QKV into the ring, out
projection, fc1, fc2), ``kv_posconv`` (the chunk-only positional conv), ``kv_ring`` (the ring attention).  Measured on an
MI355X: see the summary recorded in ``oracle/insitu.py``.
"""
import torch

from . import insitu as I

GROUPS, GROUP_SLOTS, SLOTS, HIST, FEAT, WINDOW = 16, 16, 256, 64, 208, 200


def ring_mhsa(ring, live, q_slots, dt, streams=None, heads=16):
    """Ring attention launch.  ring (S, 256, 3 D): one layer's tapped ring, operand values, [q | k | v] per slot (q
    unscaled); live[b] / q_slots[b]: the live slots and the query slots of row block b (LongTensors), whose ring is
    streams[b] (default b).  -> (ref, bound) for the query rows of every block, block-major: softmax over the live keys of
    the fp32 logits scaled by dh^-0.5, P rounded to the operand type before P.V -- ``mhsa``'s formula."""
    D = ring.shape[2] // 3
    dh = D // heads
    refs, bnds = [], []
    for b, (lv, qs) in enumerate(zip(live, q_slots)):
        x = ring[b if streams is None else streams[b]].reshape(SLOTS, 3, heads, dh)
        q = x[qs, 0]  # (R, H, dh)
        k = x[lv, 1][None].expand(len(qs), -1, -1, -1)  # (R, keys, H, dh)
        v = x[lv, 2][None].expand(len(qs), -1, -1, -1)
        s = torch.einsum("rhd,rthd->rht", q, k) * dh ** -0.5
        sa = torch.einsum("rhd,rthd->rht", q.abs(), k.abs()) * dh ** -0.5
        r, e = I._softmax_av(s, sa, v, dt)
        refs.append(r)
        bnds.append(e)
    return torch.cat(refs), torch.cat(bnds)


class KvModel:
    """The documented state of an ``afx_kv`` of S streams, kept on the host from the steps' own arguments and taps."""

    def __init__(self, S, D=1024):
        self.S, self.D = S, D
        self.hop, self.active = 0, False
        self.base = [0] * S
        self.next = [0] * S
        self.cnt = [[0] * GROUPS for _ in range(S)]
        self.hist = [torch.zeros(HIST, D, dtype=torch.float64) for _ in range(S)]
        self.feat = [torch.zeros(0, D, dtype=torch.float64) for _ in range(S)]

    def group(self, s):
        """The group stream s's next chunk is written to."""
        return self.next[s] if self.active else self.hop % GROUPS

    def reset(self, slots):
        for s in slots:
            self.base[s] = self.group(s)
            self.cnt[s] = [0] * GROUPS
            self.hist[s] = torch.zeros(HIST, self.D, dtype=torch.float64)
            self.feat[s] = torch.zeros(0, self.D, dtype=torch.float64)

    def live(self, s):
        """Stream s's live slots (no rotation: attention has no positional term, the set is what matters)."""
        return torch.tensor([GROUP_SLOTS * g + r for g in range(GROUPS) for r in range(self.cnt[s][g])], dtype=torch.long)

    def begin(self, n_max, n_frames=None, slots=None):
        """The plan of one step before it runs: n_frames None = lock-step (form 1), per-stream counts = sessions (form 2),
        slots = an active list (form 3; n_frames then per list entry, default n_max each).  Per row block: its stream, its
        frames, the group and first ring row of its chunk, its query slots, its live slots (the chunk's own included) and
        the 64 rows its positional conv must find as left context."""
        if slots is not None and not self.active:  # (the first active step: every stream's next group = the lock-stepped one)
            self.next = [self.hop % GROUPS] * self.S
            self.active = True
        assert slots is not None or not self.active, "an active state takes lists only"
        streams = list(range(self.S)) if slots is None else [int(s) for s in slots]
        ns = [n_max] * len(streams) if n_frames is None else [int(v) for v in n_frames]
        blocks = []
        for s, n_s in zip(streams, ns):
            g = self.group(s)
            self.cnt[s][g] = n_s
            blocks.append(dict(stream=s, n=n_s, group=g, row=SLOTS * s + GROUP_SLOTS * g, live=self.live(s),
                               q=GROUP_SLOTS * g + torch.arange(n_s), hist=self.hist[s]))
        return dict(form=3 if slots is not None else 2 if n_frames is not None else 1, n=n_max, blocks=blocks)

    def end(self, plan, chunk_rows, feat_rows):
        """The step has run: block b's projected operand rows (n_b, D) and final feature rows (n_b, D) join its stream."""
        for b, c, f in zip(plan["blocks"], chunk_rows, feat_rows):
            s = b["stream"]
            self.hist[s] = torch.cat([self.hist[s], c[:b["n"]]])[-HIST:]
            self.feat[s] = torch.cat([self.feat[s], f[:b["n"]]])[-FEAT:]
            if self.active:
                self.next[s] = (b["group"] + 1) % GROUPS
        if not self.active:
            self.hop += 1

    def window(self, s):
        """(208, D): stream s's window buffer, right-aligned, zeros above the frames it has."""
        return torch.cat([torch.zeros(FEAT - self.feat[s].shape[0], self.D, dtype=torch.float64), self.feat[s]])

    def head_window(self, s):
        """The rows the head scores: the last min(frames, 200)."""
        return self.feat[s][-WINDOW:]


def kv_walk(sd, dt, tap, model, plan, feats6, prev_rings, heads=16, buckets=False, check_kw=None):
    """Every launch of ONE step against its reference.  sd: the trunk's state dict (oracle key names); tap(name) -> the
    tapped buffer (flat, float64); model / plan: the ``KvModel`` and its ``begin`` plan of this step; feats6 the step's
    input (blocks, n, 512); prev_rings: per layer the previous step's tapped ring (S, 256, 3 D) (zeros before the first).
    buckets: the back-end is the AASIST bucket loop, which in the per-stream forms gathers the entries by window length
    (ascending, stable) into one uniform batch per length, tapped as kv.bucket{i}, instead of one left-aligned batch.
    check_kw: further keywords of ``insitu.check`` (unique_rows / rounding_only, for streams that repeat rows).
    -> (results, fails, rings): results = [(class, tap name, check() dict, operand-typed output?)], fails = the exact
    statements that do not hold, rings = this step's tapped rings.  Advances the model (``end``)."""
    res, fails = [], []
    n, blocks = plan["n"], plan["blocks"]
    R, S, C, D = len(blocks), model.S, feats6.shape[-1], model.D
    M = R * n
    rows = torch.tensor([i * n + r for i, b in enumerate(blocks) for r in range(b["n"])], dtype=torch.long)
    streams = [b["stream"] for b in blocks]

    def put(cls, name, got, rb, op_dt):
        res.append((cls, name, I.check(got, rb[0], rb[1], dt if op_dt else None, rows, **(check_kw or {})), op_dt))

    def same(name, a, b, what):
        if a.shape != b.shape or not torch.equal(a, b):
            k = int((a != b).sum()) if a.shape == b.shape else -1
            fails.append(f"{name}: {what} ({k} elements differ)")

    # ---- front: feature LayerNorm, projection, the padded operand buffer, the chunk-only positional conv
    x6 = I.d(feats6).reshape(M, C)
    feats = tap("kv.feats").reshape(M, C)
    put("kv_layernorm", "kv.feats", feats[rows], I.layernorm(x6[rows], sd["layer_norm.weight"], sd["layer_norm.bias"], dt), True)
    proj = tap("kv.proj").reshape(M, D)
    pw, pb = sd["post_extract_proj.weight"], sd["post_extract_proj.bias"]
    put("kv_product", "kv.proj", proj[rows], I.product(feats[rows], pw, pb, dt), False)
    xpad = tap("kv.xpad").reshape(R, HIST + HIST + n + HIST, D)  # [64 zero | 64 cached | chunk | 64 zero]
    chunk = xpad[:, 2 * HIST:2 * HIST + n]
    put("kv_product", "kv.xpad", chunk.reshape(M, D)[rows], I.product(feats[rows], pw, pb, dt, out="op"), True)
    for i, b in enumerate(blocks):
        if bool((xpad[i, :HIST] != 0).any()):
            fails.append(f"kv.xpad: block {i}: nonzero rows in the left zero padding")
        if bool((xpad[i, 2 * HIST + b["n"]:] != 0).any()):
            fails.append(f"kv.xpad: block {i}: nonzero rows past 64 + n_s = {HIST + b['n']} (counted from the first cached row)")
        same("kv.xpad", xpad[i, HIST:2 * HIST], b["hist"], f"block {i}: the left context is not stream {b['stream']}'s last 64 projected rows")
    x = tap("kv.pos").reshape(M, D)
    put("kv_posconv", "kv.pos", x[rows], I.posconv(sd, xpad[:, HIST:], proj, rows, n, dt), False)
    # ---- transformer layers
    wqkv = lambda p, k: torch.cat([sd[p + f"self_attn.{m}_proj.{k}"] for m in "qkv"], 0)
    ring_rows = torch.cat([b["row"] + torch.arange(b["n"]) for b in blocks])  # (flat over (S, 256)) the rows `rows` must land on
    written = torch.zeros(S * SLOTS, dtype=torch.bool)
    for b in blocks:
        written[b["row"]:b["row"] + n] = True  # (a block's rows past its own n_s are written and never live)
    rings, l = [], 0
    while f"encoder.layers.{l}.fc2.weight" in sd:
        p, t = f"encoder.layers.{l}.", f"kv.l{l}."
        ln1 = tap(t + "ln1").reshape(M, D)
        put("kv_layernorm", t + "ln1", ln1[rows], I.layernorm(x[rows], sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"], dt), True)
        ring = tap(t + "ring").reshape(S, SLOTS, 3 * D)
        rings.append(ring)
        flat = ring.reshape(S * SLOTS, 3 * D)
        put("kv_product", t + "ring", flat[ring_rows], I.product(ln1[rows], wqkv(p, "weight"), wqkv(p, "bias"), dt, out="op"), True)
        same(t + "ring", flat[~written], prev_rings[l].reshape(S * SLOTS, 3 * D)[~written], "a ring row the step does not write moved")
        att = tap(t + "att").reshape(R, GROUP_SLOTS, D)
        got = torch.cat([att[i, :b["n"]] for i, b in enumerate(blocks)])
        put("kv_ring", t + "att", got, ring_mhsa(ring, [b["live"] for b in blocks], [b["q"] for b in blocks], dt, streams, heads), True)
        mid = tap(t + "mid").reshape(M, D)
        put("kv_product", t + "mid", mid[rows], I.product(got, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"], dt, resid=x[rows]), False)
        ln2 = tap(t + "ln2").reshape(M, D)
        put("kv_layernorm", t + "ln2", ln2[rows], I.layernorm(mid[rows], sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"], dt), True)
        ff = tap(t + "ff").reshape(M, -1)
        put("kv_product", t + "ff", ff[rows], I.product(ln2[rows], sd[p + "fc1.weight"], sd[p + "fc1.bias"], dt, act="gelu", out="op"), True)
        x = tap(f"kv.layer{l}").reshape(M, D)
        put("kv_product", f"kv.layer{l}", x[rows], I.product(ff[rows], sd[p + "fc2.weight"], sd[p + "fc2.bias"], dt, resid=mid[rows]), False)
        l += 1
    # ---- final LayerNorm, the window, the head's input
    win = tap("kv.win").reshape(S, FEAT, D)
    fl = win[:, FEAT - n:].reshape(M, D) if plan["form"] == 1 else tap("kv.fl").reshape(M, D)
    put("kv_layernorm", "kv.fl", fl[rows], I.layernorm(x[rows], sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], dt, out="f32"), False)
    model.end(plan, [chunk[i] for i in range(R)], [fl[i * n:(i + 1) * n] for i in range(R)])
    for s in range(S):
        same("kv.win", win[s], model.window(s), f"stream {s}'s window buffer is not its frames, right-aligned" +
             ("" if s in streams else " (a stream the step does not name)"))
    wins = [model.head_window(s) for s in streams]
    if buckets and plan["form"] != 1:
        order = sorted(range(R), key=lambda i: wins[i].shape[0])
        for bi, t in enumerate(sorted({w.shape[0] for w in wins})):
            members = [i for i in order if wins[i].shape[0] == t]
            got = tap(f"kv.bucket{bi}").reshape(len(members), t, D)
            for j, i in enumerate(members):
                same(f"kv.bucket{bi}", got[j], wins[i], f"entry {j} is not the last {t} rows of stream {streams[i]}'s window")
        return res, fails, rings
    th = max(w.shape[0] for w in wins)
    head = tap("ssl").reshape(R, th, D)
    for i, w in enumerate(wins):
        same("ssl", head[i, :w.shape[0]], w, f"block {i}: the head's input is not the last {w.shape[0]} rows of stream {streams[i]}'s window, left-aligned")
        if bool((head[i, w.shape[0]:] != 0).any()):
            fails.append(f"ssl: block {i}: nonzero rows after the window's {w.shape[0]} frames")
    return res, fails, rings

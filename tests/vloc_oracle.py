"""VoxCPM2's local networks in numpy, written from the reference's semantics (Sources/VoxCPM2TTS/MiniCPM4.swift): the float64 oracle
and its twin, the device's precision plan restated on the CPU (float32 everywhere, the operands of every Linear rounded to bfloat16,
float32 accumulation).  The twin's distance to the oracle is what the device's distance is bounded by (tests/vloc_cases.py).

Patches are [P][feat_dim] rows.  `geom` is a geometry of qasr.synth (VLOC_REAL), `sd` a state dict of bfloat16-valued float32 arrays.
"""
import math

import numpy as np

LM_ORIGINAL_MAX_POS = 32768            # LMConfig.originalMaxPositionEmbeddings: no coding key, so never anything else


def bf16(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def rel(a, b):
    """max |a - b| / max |b|"""
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def schedule(n_steps):
    """makeUnifiedCFMTimeSpan (:152-166): in double, rounded to Float."""
    n = max(int(n_steps), 1)
    u = 1.0 - np.arange(n + 1, dtype=np.float64) / n
    return (u + (np.cos(np.pi / 2.0 * u) - 1.0 + u)).astype(np.float32)


def zero_steps(n_steps):
    """:687 with tSpan.count = n + 1"""
    return max(1, int(float(n_steps + 1) * 0.04))


def rope_tables(head_dim, n_pos, theta=10000.0, max_pos=32768, scaling=None, lm_original=LM_ORIGINAL_MAX_POS):
    """MiniCPMLongRoPE (:43-89) in float64: (cos, sin) [n_pos, head_dim].  scaling: rope_scaling of config.json.  lm_original is the field
    the amplitude reads; config.json cannot set it (32768); the reference's own test sets it by hand, pass that value to restate it."""
    half = head_dim // 2
    scaling = scaling or {}
    orig = max(1, int(scaling.get("original_max_position_embeddings", 32768)))
    fac = scaling.get("long_factor" if max(1, max_pos) > orig else "short_factor") or []
    if len(fac) not in (0, 1, half):
        raise ValueError("factor list of length %d" % len(fac))
    fac = np.ones(half) if len(fac) == 0 else np.broadcast_to(np.asarray(fac, dtype=np.float64), (half,))
    inv = np.exp(np.arange(half, dtype=np.float64) / half * -math.log(theta))
    ang = np.arange(n_pos, dtype=np.float64)[:, None] * (1.0 / fac)[None, :] * inv[None, :]
    s = math.sqrt(1.0 + math.log(max(max(max_pos, 1) / max(lm_original, 1), 1.0)) / math.log(max(lm_original, 2)))
    emb = np.concatenate([ang, ang], axis=1)
    return np.cos(emb) * s, np.sin(emb) * s


def sinusoid(t, dim):
    """SinusoidalPosEmb (:552-559), scale 1000"""
    half = dim // 2
    freq = np.exp(np.arange(half, dtype=np.float64) * -(math.log(10000.0) / (half - 1)))
    e = 1000.0 * np.asarray(t, dtype=np.float64).reshape(-1, 1) * freq[None, :]
    return np.concatenate([np.sin(e), np.cos(e)], axis=1)


def dequantise(wq, scales, biases, group=64):
    """MLX affine: scale q + bias per group of 64 along the input, in float64 (exact); wq holds the uint32 words"""
    wq = np.asarray(wq).astype(np.int64) & 0xFFFFFFFF
    s, z = np.asarray(scales, dtype=np.float64), np.asarray(biases, dtype=np.float64)
    N, G = s.shape
    bits = wq.shape[1] * 32 // (G * group)
    per = 32 // bits
    q = ((wq[:, :, None] >> (np.arange(per) * bits)[None, None, :]) & ((1 << bits) - 1)).reshape(N, G, group)
    return (s[:, :, None] * q + z[:, :, None]).reshape(N, G * group)


def plain(sd):
    """A state dict with quantised triplets (torch tensors, qasr.synth.quantize_voxcpm2_local_state_dict) -> float64 arrays, the
    triplets as the weight the reference multiplies by, scale q + bias unrounded"""
    out = {}
    for k, v in sd.items():
        if k.endswith((".scales", ".biases")):
            continue
        stem = k[:-len(".weight")] if k.endswith(".weight") else None
        if stem and stem + ".scales" in sd:
            out[k] = dequantise(sd[k].numpy(), sd[stem + ".scales"].float().numpy(), sd[stem + ".biases"].float().numpy())
        else:
            out[k] = np.asarray(v.numpy() if hasattr(v, "numpy") else v, dtype=np.float64)
    return out


class Model:
    """twin False: float64 throughout.  twin True: the device's plan; weights are rounded to bfloat16 (a no-op for bfloat16 checkpoints;
    the dequantised image of a 4-bit / 8-bit one, as the device holds it)."""

    def __init__(self, sd, geom, twin=False):
        self.g, self.twin = geom, twin
        self.kv_edit = None                            # (k, v) [n, S, kv heads, 128] -> what attention reads (tests/test_syn_attn_cases_cpu.py)
        self.dt = np.float32 if twin else np.float64
        self.w = {k: (bf16(v) if twin and np.ndim(v) == 2 else np.asarray(v, dtype=self.dt)) for k, v in sd.items()}
        lm = geom["lm"]
        self.eps, self.kv = lm.get("rms_norm_eps", 1e-5), lm.get("num_key_value_heads", 2)
        cos, sin = rope_tables(128, 32, lm.get("rope_theta", 10000.0), lm.get("max_position_embeddings", 32768), lm.get("rope_scaling"))
        self.cos, self.sin = cos.astype(self.dt), sin.astype(self.dt)

    def scale(self, which):
        lm, st = self.g["lm"], self.g[which]
        if not lm.get("use_mup", False):
            return self.dt(1.0)
        return self.dt(np.float32(lm.get("scale_depth", 1.4)) / np.sqrt(np.float32(st["num_layers"])))

    def lin(self, x, key, bias=True):
        a = bf16(x) if self.twin else x
        y = a @ self.w[key + ".weight"].T
        return y + self.w[key + ".bias"] if bias else y

    def rms(self, x, key):
        var = (x * x).mean(axis=-1, keepdims=True)
        return (x / np.sqrt(var + self.dt(self.eps))) * self.w[key]

    def rope(self, x):                                 # x [n, S, heads, 128]
        S = x.shape[1]
        c, s = self.cos[:S, None, :], self.sin[:S, None, :]
        rot = np.concatenate([-x[..., 64:], x[..., :64]], axis=-1)
        return x * c + rot * s

    def layer(self, x, p, which):
        st = self.g[which]
        n, S, _ = x.shape
        heads = st["num_heads"]
        h = self.rms(x, p + ".input_layernorm.weight")
        q = self.rope(self.lin(h, p + ".self_attn.q_proj", False).reshape(n, S, heads, 128))
        k = self.rope(self.lin(h, p + ".self_attn.k_proj", False).reshape(n, S, self.kv, 128))
        v = self.lin(h, p + ".self_attn.v_proj", False).reshape(n, S, self.kv, 128)
        if self.kv_edit is not None:
            k, v = self.kv_edit(k, v)
        rep = heads // self.kv
        k, v = np.repeat(k, rep, axis=2), np.repeat(v, rep, axis=2)
        sc = np.einsum("nihd,njhd->nhij", q, k) * self.dt(1.0 / math.sqrt(128.0))
        sc = np.exp(sc - sc.max(axis=-1, keepdims=True))
        pr = sc / sc.sum(axis=-1, keepdims=True)
        att = np.einsum("nhij,njhd->nihd", pr, v).reshape(n, S, heads * 128)
        s = self.scale(which)
        x = x + s * self.lin(att, p + ".self_attn.o_proj", False)
        h = self.rms(x, p + ".post_attention_layernorm.weight")
        g, u = self.lin(h, p + ".mlp.gate_proj", False), self.lin(h, p + ".mlp.up_proj", False)
        act = g / (1.0 + np.exp(-g)) * u
        return x + s * self.lin(act, p + ".mlp.down_proj", False)

    def prefix(self, which):
        return "feat_encoder.encoder" if which == "enc" else "feat_decoder.estimator.decoder"

    def stack(self, which, x, n_layers=None):
        depth = self.g[which]["num_layers"]
        n_layers = depth if n_layers is None else n_layers
        x = np.asarray(x, dtype=self.dt)
        for l in range(n_layers):
            x = self.layer(x, "%s.layers.%d" % (self.prefix(which), l), which)
        return self.rms(x, self.prefix(which) + ".norm.weight") if n_layers == depth else x

    def encode(self, feats):
        """-> (cls [n, H], embed [n, lm_hidden])"""
        f = np.asarray(feats, dtype=self.dt)
        n = f.shape[0]
        tok = self.lin(f, "feat_encoder.in_proj")
        sp = np.broadcast_to(self.w["feat_encoder.special_token"].reshape(1, 1, -1), (n, 1, tok.shape[2]))
        cls = self.stack("enc", np.concatenate([sp, tok], axis=1))[:, 0]
        return cls, self.lin(cls, "enc_to_lm_proj")

    def mu(self, lm_hidden, res_hidden):
        return np.concatenate([self.lin(np.asarray(lm_hidden, dtype=self.dt), "lm_to_dit_proj"),
                               self.lin(np.asarray(res_hidden, dtype=self.dt), "res_to_dit_proj")], axis=1)

    def time_mlp(self, emb, p):
        h = self.lin(emb.astype(self.dt), p + ".linear_1")
        return self.lin(h / (1.0 + np.exp(-h)), p + ".linear_2")

    def time_token(self, t):
        H = self.g["dit"]["hidden_dim"]
        e = "feat_decoder.estimator."
        t = np.float32(t)
        if self.twin:                                  # the sinusoid in float32, as the host forms it
            half = H // 2
            es = np.float32(math.log(10000.0)) / np.float32(half - 1)
            arg = np.float32(1000.0) * t * np.exp(np.arange(half, dtype=np.float32) * -es)
            emb = np.concatenate([np.sin(arg), np.cos(arg)])[None, :]
        else:
            emb = sinusoid([t], H)
        return self.time_mlp(emb, e + "time_mlp") + self.time_mlp(sinusoid([0.0], H), e + "delta_time_mlp")

    def velocity(self, x, mu, cond, t):
        """VoxCPMLocDiTV2 with dt = 0: x, cond [B, P, F], mu [B, mu_dim] -> [B, P, F]"""
        e = "feat_decoder.estimator."
        x, mu, cond = (np.asarray(a, dtype=self.dt) for a in (x, mu, cond))
        B, P, _ = x.shape
        H = self.g["dit"]["hidden_dim"]
        tt = np.broadcast_to(self.time_token(t).reshape(1, 1, H), (B, 1, H))
        hid = np.concatenate([mu.reshape(B, -1, H), tt, self.lin(cond, e + "cond_proj"), self.lin(x, e + "in_proj")], axis=1)
        out = self.stack("dit", hid)
        return self.lin(out[:, -P:], e + "out_proj")

    def solve(self, mu, cond, z, n_steps, cfg):
        """UnifiedCFM.solveEuler with CFG-zero-star -> (x, the last derivative, the smallest |neg|^2 met, x after each step)"""
        t = schedule(n_steps)
        x = np.asarray(z, dtype=self.dt)
        mu = np.asarray(mu, dtype=self.dt)
        B = x.shape[0]
        d, least, trace = np.zeros_like(x), np.inf, []
        for step in range(1, n_steps + 1):
            dt = self.dt(np.float32(t[step - 1] - t[step]))
            if step <= zero_steps(n_steps):
                d = np.zeros_like(x)
            else:
                pos, neg = self.velocity(x, mu, cond, t[step - 1]), self.velocity(x, np.zeros_like(mu), cond, t[step - 1])
                pf, nf = pos.reshape(B, -1), neg.reshape(B, -1)
                sq = (nf * nf).sum(axis=1)
                least = min(least, float(sq.min()))
                st = ((pf * nf).sum(axis=1) / (sq + self.dt(1e-8))).reshape(B, 1, 1)
                d = neg * st + self.dt(cfg) * (pos - neg * st)
            x = x - dt * d
            trace.append(x.copy())
        return x, d, least, trace

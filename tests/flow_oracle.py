"""float64 restatement of the CosyVoice3 flow-matching mel decoder (Sources/CosyVoiceTTS/FlowMatching.swift, DiT.swift), from the
dequantised weights of a synthetic flow.safetensors state dict (qasr.synth.synth_cosyvoice_flow_state_dict).

FlowOracle(sd) is the reference arithmetic in float64.  FlowOracle(sd, twin=True) is the device's precision plan,
not its kernels: weights of the dense GEMMs and their A operands rounded to bf16, products accumulated exactly, the residual stream,
modulation and solver kept in f32.  Rounding points of the twin: [x | cond | mu | spks]; proj's output as the first conv's operand;
the first conv's Mish output; every LN-modulate output; q (after RoPE), k (after RoPE), v; the softmax numerators and the attention
output; the GELU output.  Rows are frames: x, mu, cond, v are [T, 80].
"""
import math

import numpy as np

DIM, HEADS, HD, FF, MEL, SPK, FREQ, CONV_K, GROUPS, CFG = 1024, 16, 64, 2048, 80, 192, 256, 31, 16, 0.7


def bf16(x):
    """round to nearest even bf16 (through f32), returned as float64"""
    u = np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def silu(x):
    return x / (1.0 + np.exp(-x))


def mish(x):
    return x * np.tanh(np.log1p(np.exp(x)))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def sinusoid(t):
    """DiT.swift:22-32: [sin | cos] of 1000 t exp(-i ln(10000) / 127), i < 128"""
    f = np.exp(np.arange(FREQ // 2, dtype=np.float64) * -(math.log(10000.0) / (FREQ // 2 - 1)))
    a = 1000.0 * float(t) * f
    return np.concatenate([np.sin(a), np.cos(a)])


def schedule(n):
    """FlowMatching.swift:141-144"""
    return np.array([1.0 - math.cos(i / n * 0.5 * math.pi) for i in range(n + 1)])


def rope(x, all_heads=False):
    """MLXNN.RoPE(dimensions: 64, traditional: true, base: 10000) on [T, 1024] before the head split: features 0 .. 63 only
    (DiT.swift:161-171).  all_heads=True is the mistake the tests must tell apart: the rotation on every head."""
    T = x.shape[0]
    ang = np.arange(T, dtype=np.float64)[:, None] * (10000.0 ** (-np.arange(HD // 2, dtype=np.float64) / (HD // 2)))[None, :]
    c, s = np.cos(ang), np.sin(ang)
    y = x.copy()
    for h in range(HEADS if all_heads else 1):
        a, b = x[:, h * HD:(h + 1) * HD:2], x[:, h * HD + 1:(h + 1) * HD:2]
        y[:, h * HD:(h + 1) * HD:2] = a * c - b * s
        y[:, h * HD + 1:(h + 1) * HD:2] = a * s + b * c
    return y


def causal_group_conv(h, w, b, groups=GROUPS):
    """Conv1d(groups) on [T, C] with left padding k - 1 (DiT.swift:311-320); w [C, k, C / groups] as stored"""
    T, C = h.shape
    k, cg = w.shape[1], w.shape[2]
    og = w.shape[0] // groups
    pad = np.concatenate([np.zeros((k - 1, C)), h], axis=0)
    out = np.empty((T, w.shape[0]))
    for g in range(groups):
        cols = np.stack([pad[j:j + T, g * cg:(g + 1) * cg] for j in range(k)], axis=1).reshape(T, k * cg)
        out[:, g * og:(g + 1) * og] = cols @ w[g * og:(g + 1) * og].reshape(og, k * cg).T
    return out + b


def lookahead_conv(x, w, b):
    """CausalDilatedConv1d(.right) (HiFiGAN.swift:35-84): row t reads t .. t + k - 1, zeros past the end; w [out, k, in]"""
    T, k = x.shape[0], w.shape[1]
    pad = np.concatenate([x, np.zeros((k - 1, x.shape[1]))], axis=0)
    return sum(pad[j:j + T] @ w[:, j, :].T for j in range(k)) + b


def left_conv(x, w, b):
    """CausalDilatedConv1d(.left): row t reads t - k + 1 .. t"""
    T, k = x.shape[0], w.shape[1]
    pad = np.concatenate([np.zeros((k - 1, x.shape[1])), x], axis=0)
    return sum(pad[j:j + T] @ w[:, j, :].T for j in range(k)) + b


def repeat2(x):
    """RepeatInterleaveUpsampler (FlowMatching.swift:23-33): a b -> a a b b"""
    return np.repeat(x, 2, axis=0)


def adaln_chunks(p):
    """AdaLayerNormZero (DiT.swift:88-101): shift, scale, gate (attention), shift, scale, gate (MLP)"""
    names = ("shift_msa", "scale_msa", "gate_msa", "shift_mlp", "scale_mlp", "gate_mlp")
    return dict(zip(names, np.split(p, 6)))


def final_chunks(p):
    """AdaLayerNormZeroFinal (DiT.swift:121-125): scale, then shift"""
    scale, shift = np.split(p, 2)
    return {"scale": scale, "shift": shift}


def layer_norm(x, eps=1e-6):
    m = x.mean(axis=-1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=-1, keepdims=True)
    return (x - m) / np.sqrt(v + eps)


def dequantise(sd, stem, group=64):
    """MLX affine: w = scale q + bias per group of 64 along the input, in float64"""
    wq = sd[stem + ".weight"].numpy().astype(np.int64) & 0xFFFFFFFF
    s, z = sd[stem + ".scales"].float().numpy().astype(np.float64), sd[stem + ".biases"].float().numpy().astype(np.float64)
    N, G = s.shape
    bits = wq.shape[1] * 32 // (G * group)
    per = 32 // bits
    q = ((wq[:, :, None] >> (np.arange(per) * bits)[None, None, :]) & ((1 << bits) - 1)).reshape(N, G, group)
    return (s[:, :, None] * q + z[:, :, None]).reshape(N, G * group)


class FlowOracle:
    def __init__(self, sd, twin=False):
        self.twin = twin
        self.r = bf16 if twin else (lambda a: a)           # rounding of GEMM operands
        self.s = f32 if twin else (lambda a: a)            # rounding of the f32 stream
        self.depth = 0
        while f"decoder.transformer_blocks.{self.depth}.attn.to_q.weight" in sd:
            self.depth += 1
        fl = lambda k: sd[k].float().numpy().astype(np.float64)
        D = "decoder."

        def lin(stem, operand=True):                       # (weight, bias); operand: a dense GEMM's bf16 image on the device
            w = f32(dequantise(sd, stem))
            return (self.r(w) if operand else w), fl(stem + ".bias")

        self.emb = fl("input_embedding.weight")
        self.spk_w, self.spk_b = fl("spk_embed_affine_layer.weight"), fl("spk_embed_affine_layer.bias")
        self.look1 = (fl("pre_lookahead_layer.conv1.weight"), fl("pre_lookahead_layer.conv1.bias"))
        self.look2 = (fl("pre_lookahead_layer.conv2.weight"), fl("pre_lookahead_layer.conv2.bias"))
        self.time1, self.time2 = lin(D + "time_embed.time_mlp.0", False), lin(D + "time_embed.time_mlp.2", False)
        self.proj = lin(D + "input_embed.proj")
        self.conv = [(self.r(fl(D + f"input_embed.conv_pos_embed.conv{i}.0.weight")), fl(D + f"input_embed.conv_pos_embed.conv{i}.0.bias")) for i in (1, 2)]
        self.blocks = []
        for i in range(self.depth):
            p = D + f"transformer_blocks.{i}."
            self.blocks.append({"ada": lin(p + "attn_norm.linear", False), "q": lin(p + "attn.to_q"), "k": lin(p + "attn.to_k"), "v": lin(p + "attn.to_v"),
                                "o": lin(p + "attn.to_out.0"), "ff1": lin(p + "ff.ff.0.0"), "ff2": lin(p + "ff.ff.2")})
        self.norm_out = lin(D + "norm_out.linear", False)
        self.out = (self.r(fl(D + "proj_out.weight")), fl(D + "proj_out.bias"))

    # ---- stages ----
    def mu(self, tokens):
        e = self.emb[np.asarray(tokens, dtype=np.int64)]
        h = np.maximum(lookahead_conv(e, *self.look1), 0.0)
        return repeat2(left_conv(h, *self.look2))

    def spks(self, emb):
        if emb is None:
            return np.zeros(MEL)
        e = np.asarray(emb, dtype=np.float64)
        return self.spk_w @ (e / (math.sqrt(float((e * e).sum())) + 1e-8)) + self.spk_b

    def time_embed(self, t):
        h = silu(self.time1[0] @ sinusoid(t) + self.time1[1])
        return self.time2[0] @ h + self.time2[1]

    def velocity(self, x, mu, spks, cond, t, rope_all_heads=False, trace=None):
        r, s = self.r, self.s
        x, mu = np.asarray(x, dtype=np.float64), np.asarray(mu, dtype=np.float64)
        T = x.shape[0]
        cond = np.zeros((T, MEL)) if cond is None else np.asarray(cond, dtype=np.float64)
        spks = np.zeros(MEL) if spks is None else np.asarray(spks, dtype=np.float64)
        act = s(silu(self.time_embed(t)))
        rows = r(np.concatenate([x, cond, mu, np.tile(spks[None, :], (T, 1))], axis=1))
        h0 = s(rows @ self.proj[0].T + self.proj[1])
        c1 = r(mish(causal_group_conv(r(h0), *self.conv[0])))
        h = s(h0 + mish(causal_group_conv(c1, *self.conv[1])))
        if trace is not None:
            trace.append(float(np.sqrt((h ** 2).mean())))
        for b in self.blocks:
            m = adaln_chunks(s(b["ada"][0] @ act + b["ada"][1]))
            a = r(layer_norm(h) * (1.0 + m["scale_msa"]) + m["shift_msa"])
            q = r(rope(a @ b["q"][0].T + b["q"][1], rope_all_heads))
            k = r(rope(a @ b["k"][0].T + b["k"][1], rope_all_heads))
            v = r(a @ b["v"][0].T + b["v"][1])
            o = np.empty((T, DIM))
            for hd in range(HEADS):
                sl = slice(hd * HD, (hd + 1) * HD)
                sc = (q[:, sl] @ k[:, sl].T) * (1.0 / math.sqrt(HD))
                p = np.exp(sc - sc.max(axis=1, keepdims=True))
                o[:, sl] = (r(p) @ v[:, sl]) / p.sum(axis=1, keepdims=True)
            h = s(h + m["gate_msa"] * (r(o) @ b["o"][0].T + b["o"][1]))
            a = r(layer_norm(h) * (1.0 + m["scale_mlp"]) + m["shift_mlp"])
            u = r(gelu_tanh(a @ b["ff1"][0].T + b["ff1"][1]))
            h = s(h + m["gate_mlp"] * (u @ b["ff2"][0].T + b["ff2"][1]))
            if trace is not None:
                trace.append(float(np.sqrt((h ** 2).mean())))
                trace.append((float(np.abs(m["gate_msa"]).mean()), float(np.abs(m["gate_mlp"]).mean())))
        f = final_chunks(s(self.norm_out[0] @ act + self.norm_out[1]))
        a = r(layer_norm(h) * (1.0 + f["scale"]) + f["shift"])
        return s(a @ self.out[0].T + self.out[1])

    def solve(self, mu, spks, cond, z, n_steps, wrong_cfg=False, rope_all_heads=False):
        """FlowMatching.swift:146-195.  wrong_cfg=True feeds mu to the unconditioned branch: the mistake the tests must tell apart."""
        s = self.s
        t = f32(schedule(n_steps)) if self.twin else schedule(n_steps)
        x = np.asarray(z, dtype=np.float64).copy()
        mu = np.asarray(mu, dtype=np.float64)
        for i in range(n_steps):
            vc = self.velocity(x, mu, spks, cond, t[i], rope_all_heads)
            vu = self.velocity(x, mu if wrong_cfg else np.zeros_like(mu), None, None, t[i], rope_all_heads)
            v = s(s((1.0 + CFG) * vc) - s(CFG * vu))
            x = s(x + s(s(t[i + 1] - t[i]) * v))
        return x, vc, vu

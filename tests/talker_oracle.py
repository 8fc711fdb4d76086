"""Oracle of the Qwen3-TTS Talker + code predictor (csrc/tts_talker.hip): one restatement of both networks, the prefill builder and the
frame loop, run under two policies, plus a numpy restatement of the sampler.

TEST INFRASTRUCTURE ONLY.  Reference: Sources/Qwen3TTS/Talker.swift, CodePredictor.swift, Sampling.swift, Qwen3TTS.swift:1268-1584.

  * F64: float64 throughout on the dequantised weights scale * q + bias (oracle.quant.dequantize_f32 is exact in f32: q < 256, one
    product and one sum of bf16 values, then widened).  This is the oracle.
  * TWIN: the device's arithmetic in torch: values of bf16 at every op boundary the device rounds at, f32 inside (x @ w_hat^T with f32
    accumulation -- the identity oracle.quant.qmv_factored states -- f32 norms and softmax, f32 logits).
The prompt and the frames are one causal sequence per row, so a forced pass is one pass over [prompt | next inputs]; the code predictor's
16 positions of a frame are one causal pass per (row, frame).
"""
import math

import numpy as np
import torch

from oracle import quant

GROUPS = 16
F64 = dict(dtype=torch.float64, bf16=False)
TWIN = dict(dtype=torch.float32, bf16=True)


def r(x, pol):
    return x.to(torch.bfloat16).to(x.dtype) if pol["bf16"] else x


class Weights:
    """The checkpoint (qasr.synth.synth_tts_talker_state_dict) as float tensors: quantised Linears dequantised exactly."""

    def __init__(self, sd, geometry):
        self.g = dict(geometry)
        self.t = {}
        for k, v in sd.items():
            if k.endswith(".scales") or k.endswith(".biases"):
                continue
            if v.dtype == torch.int32:
                stem = k[:-len(".weight")]
                wq = v.numpy().view(np.uint32)
                self.t[k] = quant.dequantize_f32(wq, sd[stem + ".scales"].to(torch.float32).numpy(),
                                                 sd[stem + ".biases"].to(torch.float32).numpy(), self.g["bits"])
            else:
                self.t[k] = v.to(torch.float32)
        self._cast = {}

    def get(self, key, pol):
        ck = (key, pol["dtype"])
        if ck not in self._cast:
            self._cast[ck] = self.t[key].to(pol["dtype"])
        return self._cast[ck]


def rms(x, w, eps, pol):
    inv = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return r(w * r(x * inv, pol), pol)


def rope_tables(theta, half, positions, pol):
    if pol["bf16"]:                                    # the device's f32 tables (decoder.hip)
        k = np.float32(-math.log(float(theta)) / half)
        inv = np.exp(np.arange(half, dtype=np.float32) * k).astype(np.float32)
        ang = (np.asarray(positions, dtype=np.float32)[:, None] * inv[None]).astype(np.float32)
        return torch.from_numpy(np.cos(ang).astype(np.float32)), torch.from_numpy(np.sin(ang).astype(np.float32))
    inv = np.exp(-np.arange(half, dtype=np.float64) * math.log(float(theta)) / half)
    ang = np.asarray(positions, dtype=np.float64)[:, None] * inv[None]
    return torch.from_numpy(np.cos(ang)), torch.from_numpy(np.sin(ang))


def layers_forward(x, W, prefix, n_layers, heads, kv, hd, eps, theta, pol, p_bf16, mask_edit=None):
    """x [N, S, H] (N independent causal sequences at positions 0 .. S-1) -> the residual stream after the last layer.  mask_edit: a
    function of the causal mask [S, S] (True = hidden) that returns the mask to use (tests/test_syn_attn_cases_cpu.py)."""
    N, S, H = x.shape
    half = hd // 2
    cos, sin = rope_tables(theta, half, np.arange(S), pol)
    cos, sin = cos.to(pol["dtype"]), sin.to(pol["dtype"])
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    if mask_edit is not None:
        mask = mask_edit(mask)
    scale = 1.0 / math.sqrt(hd)

    def lin(h, key):
        return h @ W.get(prefix + key + ".weight", pol).T

    def qk(t, nh, wkey):
        t = t.reshape(N, S, nh, hd)
        y = rms(t, W.get(prefix + wkey, pol), eps, pol)
        y1, y2 = y[..., :half], y[..., half:]
        c, s = cos[None, :, None, :], sin[None, :, None, :]
        return torch.cat([r(y1 * c - y2 * s, pol), r(y1 * s + y2 * c, pol)], dim=-1).permute(0, 2, 1, 3)    # [N, nh, S, hd]

    for l in range(n_layers):
        p = f"model.layers.{l}."
        h = rms(x, W.get(prefix + p + "input_layernorm.weight", pol), eps, pol)
        q = qk(r(lin(h, p + "self_attn.q_proj"), pol), heads, p + "self_attn.q_norm.weight")
        k = qk(r(lin(h, p + "self_attn.k_proj"), pol), kv, p + "self_attn.k_norm.weight")
        v = r(lin(h, p + "self_attn.v_proj"), pol).reshape(N, S, kv, hd).permute(0, 2, 1, 3)
        rep = heads // kv
        k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
        sc = (q @ k.transpose(-1, -2)) * scale
        sc = sc.masked_fill(mask, float("-inf"))
        e = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        num = (r(e, pol) if p_bf16 else e) @ v
        att = r(num / e.sum(dim=-1, keepdim=True), pol).permute(0, 2, 1, 3).reshape(N, S, heads * hd)
        x = r(x + r(lin(att, p + "self_attn.o_proj"), pol), pol)
        h = rms(x, W.get(prefix + p + "post_attention_layernorm.weight", pol), eps, pol)
        g, u = r(lin(h, p + "mlp.gate_proj"), pol), r(lin(h, p + "mlp.up_proj"), pol)
        act = r(r(g * torch.sigmoid(g), pol) * u, pol)
        x = r(x + r(lin(act, p + "mlp.down_proj"), pol), pol)
    return x


T_, C_ = "talker.", "talker.code_predictor."


def embed_text(ids, W, pol):
    e = W.get(T_ + "model.text_embedding.weight", pol)[torch.as_tensor(ids, dtype=torch.long)]
    h = e @ W.get(T_ + "text_projection.linear_fc1.weight", pol).T + W.get(T_ + "text_projection.linear_fc1.bias", pol)
    h = r(h * torch.sigmoid(h), pol)
    return r(h @ W.get(T_ + "text_projection.linear_fc2.weight", pol).T + W.get(T_ + "text_projection.linear_fc2.bias", pol), pol)


def codec_prefix(tokens, language, speaker=None):
    """buildCodecPrefix: 6 ids, 7 with a speaker token."""
    p = [tokens["codec_think"], tokens["codec_think_bos"], int(language), tokens["codec_think_eos"]]
    if speaker is not None:
        p.append(int(speaker))
    return p + [tokens["codec_pad"], tokens["codec_bos"]]


def prefill_plan(text, tokens, language, speaker=None, xvector=False, instruct=None):
    """buildPrefillEmbeddings as a plan: per prompt position (text-side id or None, codec-side id | "xvec" | None), and the trailing
    text-side ids.  Written from the doc comment of the Swift function; the embedding arithmetic is prefill_embeddings."""
    codec = codec_prefix(tokens, language, speaker)
    if xvector:
        codec = codec[:4] + ["xvec"] + codec[4:]
    L = len(codec)
    plan = [(t, None) for t in (instruct or [])]
    plan += [(t, None) for t in text[:3]]
    overlay = [tokens["tts_pad"]] * (L - 2) + [tokens["tts_bos"]]
    plan += list(zip(overlay, codec[:L - 1]))
    plan.append((text[3], codec[L - 1]))
    trail_end = len(text) - 5
    trailing = (list(text[4:trail_end]) if trail_end > 4 else []) + [tokens["tts_eos"]]
    return plan, trailing


def prefill_embeddings(plan, W, pol, xvector=None):
    H = W.g["hidden"]
    ce = W.get(T_ + "model.codec_embedding.weight", pol)
    rows = []
    for t, c in plan:
        v = torch.zeros(H, dtype=pol["dtype"])
        if t is not None:
            v = v + embed_text([t], W, pol)[0]
        if c == "xvec":
            v = v + torch.as_tensor(xvector, dtype=pol["dtype"])
        elif c is not None:
            v = v + ce[c]
        rows.append(r(v, pol))
    return torch.stack(rows)


def next_input(text_vec, codes16, W, pol):
    """text side + codec_embedding(code 0) + sum of the 15 code-predictor embeddings, in that order, one rounding."""
    s = text_vec + W.get(T_ + "model.codec_embedding.weight", pol)[int(codes16[0])]
    for g in range(GROUPS - 1):
        s = s + W.get(C_ + f"model.codec_embedding.{g}.weight", pol)[int(codes16[g + 1])]
    return r(s, pol)


def talker_pass(x_seq, W, pol):
    """x_seq [S, H] -> (post-norm hidden [S, H], logits [S, codec_vocab])."""
    g = W.g
    x = layers_forward(x_seq[None], W, T_, g["layers"], g["heads"], g["kv_heads"], g["head_dim"], 1e-6, 1e6, pol, p_bf16=pol["bf16"])[0]
    hn = rms(x, W.get(T_ + "model.norm.weight", pol), 1e-6, pol)
    return hn, hn @ W.get(T_ + "codec_head.weight", pol).T


def cp_pass(hn, codes, W, pol, n_groups=GROUPS - 1, mask_edit=None):
    """hn [N, H], codes [N, >= n_groups] (codes 0 .. n_groups-1 are read) -> logits [N, n_groups, cp_vocab]: logits g give code g + 1."""
    g = W.g
    N = hn.shape[0]
    codes = torch.as_tensor(np.asarray(codes), dtype=torch.long)
    seq = [hn, W.get(T_ + "model.codec_embedding.weight", pol)[codes[:, 0]]]
    for j in range(1, n_groups):
        seq.append(W.get(C_ + f"model.codec_embedding.{j - 1}.weight", pol)[codes[:, j]])
    x = torch.stack(seq, dim=1)                                           # [N, n_groups + 1, E]
    if g["cp_embedding_dim"] != g["cp_hidden"]:
        x = r(x @ W.get(C_ + "small_to_mtp_projection.weight", pol).T + W.get(C_ + "small_to_mtp_projection.bias", pol), pol)
    x = layers_forward(x, W, C_, g["cp_layers"], g["cp_heads"], g["cp_kv_heads"], g["cp_head_dim"], 1e-6, 1e6, pol, p_bf16=False, mask_edit=mask_edit)
    hn2 = rms(x, W.get(C_ + "model.norm.weight", pol), 1e-6, pol)
    out = [hn2[:, j + 1] @ W.get(C_ + f"lm_head.{j}.weight", pol).T for j in range(n_groups)]
    return torch.stack(out, dim=1)


def row_inputs(row, W, pol, tokens):
    plan, trailing = prefill_plan(row["text"], tokens, row["language"], row.get("speaker"), row.get("xvector") is not None,
                                  row.get("instruct"))
    pf = prefill_embeddings(plan, W, pol, row.get("xvector"))
    trail = embed_text(trailing, W, pol)
    pad = embed_text([tokens["tts_pad"]], W, pol)[0]
    return pf, trail, pad


def forced_pass(row, codes, W, pol, tokens):
    """codes [16, T] -> dict(talker [T, codec_vocab], cp [T, 15, cp_vocab], hidden [T, H]) with every fed input taken from `codes`."""
    codes = np.asarray(codes)
    T = codes.shape[1]
    with torch.no_grad():
        pf, trail, pad = row_inputs(row, W, pol, tokens)
        xs = [pf]
        for f in range(T - 1):
            xs.append(next_input(trail[f] if f < len(trail) else pad, codes[:, f], W, pol)[None])
        hn, logits = talker_pass(torch.cat(xs), W, pol)
        P = pf.shape[0]
        hn, logits = hn[P - 1:], logits[P - 1:]
        cp = cp_pass(hn, codes.T, W, pol)
    return {"talker": logits.numpy(), "cp": cp.numpy(), "hidden": hn.numpy()}


def greedy_run(row, T, W, pol, tokens, suppress=(2048, 3072), eos=2150):
    """The frame loop with SamplingConfig.greedy (no penalty effect on an argmax but the penalised logits are what is compared: the
    default 1.05 is applied) -> codes [16, n_frames]."""
    with torch.no_grad():
        pf, trail, pad = row_inputs(row, W, pol, tokens)
        xs, out, hist = [pf], [], set()
        for f in range(T):
            hn, logits = talker_pass(torch.cat(xs), W, pol)
            lg = logits[-1].clone().to(torch.float32)
            lg[suppress[0]:eos] = -1e9
            lg[eos + 1:suppress[1]] = -1e9
            for t in hist:
                lg[t] = lg[t] * 1.05 if lg[t] < 0 else lg[t] / 1.05
            c0 = int(torch.argmax(lg))
            if c0 == eos:
                break
            hist.add(c0)
            frame = [c0]
            for j in range(GROUPS - 1):
                cl = cp_pass(hn[-1:], np.asarray([frame + [0] * (GROUPS - len(frame))]), W, pol, n_groups=j + 1)
                frame.append(int(torch.argmax(cl[0, j].to(torch.float32))))
            out.append(frame)
            xs.append(next_input(trail[f] if f < len(trail) else pad, frame, W, pol)[None])
    return np.asarray(out, dtype=np.int32).reshape(-1, GROUPS).T


# ---- the sampler (Sampling.swift:36-160 with the counter-based splitmix64 stream of csrc/tts_talker.h) ---------------------------------
M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def stream_key(seed, row, frame, group):
    a = splitmix64((seed ^ 0x5174735454533031) & M64)
    b = splitmix64((a + (row & M64)) & M64)
    return splitmix64((b + ((frame & 0xffffffff) << 8) + group) & M64)


def uniforms(key, V):
    u = np.empty(V, dtype=np.float32)
    for i in range(V):
        rr = float(splitmix64((key + i) & M64) >> 11) * (1.0 / 9007199254740992.0)
        u[i] = np.float32(1e-6 + rr * (1.0 - 1e-6))
    return u


def sample(logits, temperature=0.9, top_k=50, repetition_penalty=1.05, eos_logit_bias=0.0, history=(), talker=True, seed=0, row=0,
           frame=0, group=0, suppress=(2048, 3072), eos=2150, return_perturbed=False):
    v = np.array(logits, dtype=np.float32)
    V = v.size
    f32 = np.float32
    if talker:
        for i in range(max(suppress[0], 0), min(suppress[1], V)):
            if i != eos:
                v[i] = f32(-1e9)
        if repetition_penalty != 1.0:
            for t in set(int(h) for h in history):
                if 0 <= t < V:
                    v[t] = v[t] * f32(repetition_penalty) if v[t] < 0 else v[t] / f32(repetition_penalty)
    if temperature <= 0:
        return int(np.argmax(v))
    v = (v / f32(temperature)).astype(np.float32)
    eos_ok = talker and eos < V
    saved = v[eos] if eos_ok else f32(0)
    if 0 < top_k < V:
        thr = np.sort(v)[V - top_k]
        v = np.where(v < thr, f32(-1e9), v).astype(np.float32)
    if eos_ok:
        v[eos] = saved + f32(eos_logit_bias) if eos_logit_bias != 0 else saved
    u = uniforms(stream_key(seed, row, frame, group), V)
    with np.errstate(divide="ignore"):
        pert = (v - np.log(-np.log(u)).astype(np.float32)).astype(np.float32)
    return pert if return_perturbed else int(np.argmax(pert))

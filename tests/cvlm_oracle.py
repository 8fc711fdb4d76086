"""Oracle of the CosyVoice3 speech-token LLM (csrc/llm_cosyvoice.hip): one restatement of the network, the prefix builder and the token
loop, run under two policies, plus a numpy restatement of the sampler.

TEST INFRASTRUCTURE ONLY.  Reference: Sources/CosyVoiceTTS/LLM.swift (sampleToken :12-123, CosyVoiceAttention :131-216, CosyVoiceBlock
:219-262, buildInputSequence :387-417, forwardStep :425-468, generate :479-560), Configuration.swift:5-41,124-133.

  * F64: float64 throughout on the dequantised weights scale * q + bias (exact in f32, then widened).  This is the oracle.
  * TWIN: the device's arithmetic in torch: values of bf16 at every op boundary the device rounds at, f32 inside (x @ w_hat^T with f32
    accumulation, f32 norms and softmax with f32 probabilities, f32 logits).  q, k and v take the reference's two roundings
    bf16(bf16(acc) + bias) (MLX adds the bias to the rounded quantised product, LLM.swift:181-183 on bf16 tensors).
The prefix and the tokens are one causal sequence per row, so a forced pass is one pass over [prefix | fed tokens].
"""
import math

import numpy as np
import torch

from talker_oracle import F64, TWIN, Weights, r, rms, rope_tables, stream_key, uniforms     # shared test infrastructure

EPS, THETA = 1e-6, 1e6                       # Configuration.swift:11-12
STOPS = 3                                    # speech_tokens + 0 .. 2 (Configuration.swift:33-35)


def layers_forward(x, W, pol, mask_edit=None):
    """x [S, H] at positions 0 .. S-1 -> the residual stream after the last layer (CosyVoiceBlock, LLM.swift:238-260).  mask_edit: a function
    of the causal mask [S, S] (True = hidden) that returns the mask to use: tests/test_syn_attn_cases_cpu.py measures with it what a wrong
    key set does to the network's outputs."""
    g = W.g
    heads, kv, hd = g["heads"], g["kv_heads"], g["head_dim"]
    S = x.shape[0]
    half = hd // 2
    cos, sin = rope_tables(THETA, half, np.arange(S), pol)
    cos, sin = cos.to(pol["dtype"]), sin.to(pol["dtype"])
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    if mask_edit is not None:
        mask = mask_edit(mask)
    scale = 1.0 / math.sqrt(hd)

    def lin(h, key):
        return h @ W.get(key + ".weight", pol).T

    def biased(h, key):                                                      # LLM.swift:181-183
        return r(r(lin(h, key), pol) + W.get(key + ".bias", pol), pol)

    def rope(t, nh):                                                         # MLXNN.RoPE(traditional: false), LLM.swift:165,195-196
        t = t.reshape(S, nh, hd)
        y1, y2 = t[..., :half], t[..., half:]
        c, s = cos[:, None, :], sin[:, None, :]
        return torch.cat([r(y1 * c - y2 * s, pol), r(y1 * s + y2 * c, pol)], dim=-1).permute(1, 0, 2)        # [nh, S, hd]

    for l in range(g["layers"]):
        p = f"layers.{l}."
        h = rms(x, W.get(p + "input_layernorm.weight", pol), EPS, pol)
        q = rope(biased(h, p + "self_attn.q_proj"), heads)
        k = rope(biased(h, p + "self_attn.k_proj"), kv)
        v = biased(h, p + "self_attn.v_proj").reshape(S, kv, hd).permute(1, 0, 2)
        rep = heads // kv
        k, v = k.repeat_interleave(rep, dim=0), v.repeat_interleave(rep, dim=0)
        sc = (q @ k.transpose(-1, -2)) * scale
        sc = sc.masked_fill(mask, float("-inf"))
        e = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        att = r((e @ v) / e.sum(dim=-1, keepdim=True), pol).permute(1, 0, 2).reshape(S, heads * hd)
        x = r(x + r(lin(att, p + "self_attn.o_proj"), pol), pol)
        h = rms(x, W.get(p + "post_attention_layernorm.weight", pol), EPS, pol)
        gt, up = r(lin(h, p + "mlp.gate_proj"), pol), r(lin(h, p + "mlp.up_proj"), pol)
        act = r(r(gt * torch.sigmoid(gt), pol) * up, pol)
        x = r(x + r(lin(act, p + "mlp.down_proj"), pol), pol)
    return x


def prefix_plan(text, prompt, speech_tokens):
    """buildInputSequence (LLM.swift:387-417) as a plan: ("speech" | "text", id) per position."""
    plan = [("speech", speech_tokens)] + [("text", int(t)) for t in text] + [("speech", speech_tokens + 2)]
    return plan + [("speech", int(t)) for t in (prompt if prompt is not None else [])]


def embed(plan, W, pol):
    te, se = W.get("text_embedding.weight", pol), W.get("speech_embedding.weight", pol)
    return torch.stack([se[i] if kind == "speech" else te[i] for kind, i in plan])


def forced_pass(row, tokens, W, pol, mask_edit=None):
    """tokens [T] -> dict(logits [T, V], hidden [T, H]): logits[f] at position prefix - 1 + f after feeding tokens 0 .. f - 1."""
    tokens = [int(t) for t in tokens]
    with torch.no_grad():
        plan = prefix_plan(row["text"], row.get("prompt"), W.g["speech_tokens"])
        P = len(plan)
        x = embed(plan + [("speech", t) for t in tokens[:-1]], W, pol)
        hn = rms(layers_forward(x, W, pol, mask_edit), W.get("norm.weight", pol), EPS, pol)[P - 1:]
        logits = hn @ W.get("speech_head.weight", pol).T
    return {"logits": logits.numpy(), "hidden": hn.numpy()}


def mask_logits(logits, speech_tokens, mask_stops):
    """Steps 1 and 2 of sampleToken (LLM.swift:76-98) in float32."""
    v = np.array(logits, dtype=np.float32)
    V = v.size
    stops = range(speech_tokens, speech_tokens + STOPS)
    for i in range(speech_tokens, V):
        if i not in stops:
            v[i] = np.float32(-1e9)
    if mask_stops:
        for i in stops:
            v[i] = np.float32(-1e9)
    return v


def greedy_run(row, T, W, pol):
    """generate with top_k = 1 and win_size = 0 (the first maximum of the masked logits), a large min_len: T tokens."""
    toks = []
    with torch.no_grad():
        for f in range(T):
            lg = forced_pass(row, toks + [0], W, pol)["logits"][-1]
            toks.append(int(np.argmax(mask_logits(lg, W.g["speech_tokens"], True))))
    return np.asarray(toks, dtype=np.int32)


# ---- the sampler (LLM.swift:12-123 with the counter-based splitmix64 stream of csrc/tts_talker.h) ---------------------------------------
def top_p_boundaries(v, top_p):
    """cum - p of every survivor in (value descending, index ascending) order, in float64."""
    idx = [i for i in range(v.size) if v[i] > np.float32(-1e9)]
    idx.sort(key=lambda i: (-float(v[i]), i))
    e = np.exp(np.asarray([float(v[i]) for i in idx], dtype=np.float64) - float(v[idx[0]]))
    p = e / e.sum()
    return idx, np.cumsum(p) - p


def sample(logits, speech_tokens, top_k=25, top_p=0.8, win_size=10, tau_r=0.1, history=(), step=0, below_min=False, seed=0, row=0,
           return_info=False):
    """sampleToken in numpy: masks and the Gumbel perturbation in float32 as the reference computes them, the nucleus sums in float64.
    return_info: also (perturbed values of the deciding draw, the smallest |cum - p - top_p| over the survivors)."""
    f32 = np.float32
    mask_stops = bool(below_min) or step == 0
    base = mask_logits(logits, speech_tokens, mask_stops)
    v = base.copy()
    V = v.size
    if 0 < top_k < V:
        thr = np.sort(v)[V - top_k]
        v = np.where(v < thr, f32(-1e9), v).astype(np.float32)
    gap = np.inf
    if top_p < 1.0:
        idx, excl = top_p_boundaries(v, top_p)
        gap = float(np.abs(excl - float(f32(top_p))).min())
        for i, c in zip(idx, excl):
            if c > float(f32(top_p)):
                v[i] = f32(-1e9)
    with np.errstate(divide="ignore"):
        pert = (v - np.log(-np.log(uniforms(stream_key(seed, row, step, 0), V))).astype(np.float32)).astype(np.float32)
    tok = int(np.argmax(pert))
    history = [int(h) for h in history]
    if win_size > 0 and history:
        window = history[-win_size:]
        if window.count(tok) >= max(int(f32(win_size) * f32(tau_r)), 1):
            v = base.copy()
            v[tok] = f32(-1e9)
            with np.errstate(divide="ignore"):
                pert = (v - np.log(-np.log(uniforms(stream_key(seed, row, step, 1), V))).astype(np.float32)).astype(np.float32)
            tok = int(np.argmax(pert))
    return (tok, pert, gap) if return_info else tok

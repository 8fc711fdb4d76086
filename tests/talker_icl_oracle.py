"""Oracle of the Qwen3-TTS ICL voice-cloning prompt (csrc/tts_talker.hip: the ICL plan of TtsTalker::prefill, the packed prompt pass) on
top of tests/talker_oracle.py: embed_text, next_input, talker_pass and cp_pass are that file's, under its F64 and TWIN policies.

TEST INFRASTRUCTURE ONLY.  Reference: Sources/Qwen3TTS/Qwen3TTS+ICL.swift:149-242 (buildICLPrefillEmbeddings); the plan below is written
from that function's doc comment:

    [role_embed]                                    <- <|im_start|>assistant\\n
    [tts_pad...tts_bos + codec_prefix]              <- codec prefix overlay (its own trailing codec_bos dropped)
    [ref_text + target_text + tts_eos + codec_pad]  <- text overlay
    [codec_bos + ref_codec_embeds]                  <- codec ICL context, tts_pad on the text side

A forced pass is one causal pass over [ICL prompt | next inputs]; the trailing text is empty, so every next input adds tts_pad.

The twin's flag `packed` restates where the device's packed prompt pass (tuning knob tts_packed_prompt = 1) rounds differently from the
step path: the positions 0 .. P-2 multiply by the dequantised weights ROUNDED TO bf16 (one scratch of bf16 weights per layer), the last
prompt position and every frame by scale * q + bias in f32.  The prompt attention's P is bf16 in both (the Talker's twin already rounds it);
its 64-key tiling is a summation order, not a rounding point the twin restates."""
import math

import numpy as np
import torch

import talker_oracle as O

GROUPS = O.GROUPS
F64, TWIN = O.F64, O.TWIN
FIXED = 11                        # role 3 + prefix 6 + tts_eos + codec_bos


def icl_plan(text, ref_text, n_frames, tokens, language):
    """Per prompt position (text-side id, codec-side id | "xvec" | ("frame", f)).  text is templated: role = text[:3], target = text[3:-5]."""
    prefix = O.codec_prefix(tokens, language)
    prefix = prefix[:4] + ["xvec"] + prefix[4:]                          # think, think_bos, language, think_eos, x-vector, pad, bos
    L = len(prefix)
    plan = [(t, None) for t in text[:3]]
    plan += list(zip([tokens["tts_pad"]] * (L - 2) + [tokens["tts_bos"]], prefix[:L - 1]))
    plan += [(int(t), tokens["codec_pad"]) for t in list(ref_text) + list(text[3:len(text) - 5])]
    plan.append((tokens["tts_eos"], tokens["codec_pad"]))
    plan.append((tokens["tts_pad"], tokens["codec_bos"]))
    plan += [(tokens["tts_pad"], ("frame", f)) for f in range(n_frames)]
    return plan


def prompt_length(n_ref_text, n_text, n_frames):
    return FIXED + n_ref_text + (n_text - 8) + n_frames


def icl_embeddings(row, W, pol, tokens):
    """-> (prompt rows [P, H], tts_pad embedding [H])."""
    ref_codes = np.asarray(row["ref_codes"])
    plan = icl_plan(row["text"], row["ref_text"], ref_codes.shape[1], tokens, row["language"])
    pad = O.embed_text([tokens["tts_pad"]], W, pol)[0]
    head = [e for e in plan if not isinstance(e[1], tuple)]
    rows = [O.prefill_embeddings(head, W, pol, row["xvector"])]
    frames = [O.next_input(pad, ref_codes[:, e[1][1]], W, pol) for e in plan if isinstance(e[1], tuple)]
    return torch.cat(rows + [torch.stack(frames)]), pad


def talker_pass_packed_twin(x_seq, W, pol, n_packed):
    """talker_pass of the twin with the first n_packed positions multiplied by bf16-rounded weights (see the module docstring)."""
    g = W.g
    heads, kv, hd, eps, theta = g["heads"], g["kv_heads"], g["head_dim"], 1e-6, 1e6
    x = x_seq[None]
    N, S, H = x.shape
    half = hd // 2
    cos, sin = O.rope_tables(theta, half, np.arange(S), pol)
    cos, sin = cos.to(pol["dtype"]), sin.to(pol["dtype"])
    mask = torch.triu(torch.ones(S, S, dtype=torch.bool), diagonal=1)
    scale = 1.0 / math.sqrt(hd)
    r, rms, T_ = O.r, O.rms, O.T_

    def lin(h, key):
        w = W.get(T_ + key + ".weight", pol)
        y = h @ w.T
        y[:, :n_packed] = h[:, :n_packed] @ r(w, pol).T
        return y

    def qk(t, nh, wkey):
        t = t.reshape(N, S, nh, hd)
        y = rms(t, W.get(T_ + wkey, pol), eps, pol)
        y1, y2 = y[..., :half], y[..., half:]
        c, s = cos[None, :, None, :], sin[None, :, None, :]
        return torch.cat([r(y1 * c - y2 * s, pol), r(y1 * s + y2 * c, pol)], dim=-1).permute(0, 2, 1, 3)

    for l in range(g["layers"]):
        p = f"model.layers.{l}."
        h = rms(x, W.get(T_ + p + "input_layernorm.weight", pol), eps, pol)
        q = qk(r(lin(h, p + "self_attn.q_proj"), pol), heads, p + "self_attn.q_norm.weight")
        k = qk(r(lin(h, p + "self_attn.k_proj"), pol), kv, p + "self_attn.k_norm.weight")
        v = r(lin(h, p + "self_attn.v_proj"), pol).reshape(N, S, kv, hd).permute(0, 2, 1, 3)
        rep = heads // kv
        k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
        sc = ((q @ k.transpose(-1, -2)) * scale).masked_fill(mask, float("-inf"))
        e = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        att = r((r(e, pol) @ v) / e.sum(dim=-1, keepdim=True), pol).permute(0, 2, 1, 3).reshape(N, S, heads * hd)
        x = r(x + r(lin(att, p + "self_attn.o_proj"), pol), pol)
        h = rms(x, W.get(T_ + p + "post_attention_layernorm.weight", pol), eps, pol)
        gt, u = r(lin(h, p + "mlp.gate_proj"), pol), r(lin(h, p + "mlp.up_proj"), pol)
        act = r(r(gt * torch.sigmoid(gt), pol) * u, pol)
        x = r(x + r(lin(act, p + "mlp.down_proj"), pol), pol)
    hn = rms(x[0], W.get(T_ + "model.norm.weight", pol), eps, pol)
    return hn, hn @ W.get(T_ + "codec_head.weight", pol).T


def _talker(xs, P, W, pol, packed):
    if packed and pol["bf16"]:
        return talker_pass_packed_twin(torch.cat(xs), W, pol, P - 1)
    return O.talker_pass(torch.cat(xs), W, pol)


def forced_pass(row, codes, W, pol, tokens, packed=False):
    """codes [16, T] -> dict(talker [T, codec_vocab], cp [T, 15, cp_vocab], hidden [T, H], prompt [P, H])."""
    codes = np.asarray(codes)
    T = codes.shape[1]
    with torch.no_grad():
        pf, pad = icl_embeddings(row, W, pol, tokens)
        P = pf.shape[0]
        xs = [pf] + [O.next_input(pad, codes[:, f], W, pol)[None] for f in range(T - 1)]
        hn, logits = _talker(xs, P, W, pol, packed)
        hn, logits = hn[P - 1:], logits[P - 1:]
        cp = O.cp_pass(hn, codes.T, W, pol)
    return {"talker": logits.numpy(), "cp": cp.numpy(), "hidden": hn.numpy(), "prompt": pf.numpy()}


def greedy_run(row, T, W, pol, tokens, packed=False, suppress=(2048, 3072), eos=2150):
    """talker_oracle.greedy_run over the ICL prompt -> codes [16, n_frames]."""
    with torch.no_grad():
        pf, pad = icl_embeddings(row, W, pol, tokens)
        P = pf.shape[0]
        xs, out, hist = [pf], [], set()
        for f in range(T):
            hn, logits = _talker(xs, P, W, pol, packed)
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
                cl = O.cp_pass(hn[-1:], np.asarray([frame + [0] * (GROUPS - len(frame))]), W, pol, n_groups=j + 1)
                frame.append(int(torch.argmax(cl[0, j].to(torch.float32))))
            out.append(frame)
            xs.append(O.next_input(pad, frame, W, pol)[None])
    return np.asarray(out, dtype=np.int32).reshape(-1, GROUPS).T

"""NumPy restatement of the Qwen3-TTS 12.5 Hz speech tokenizer encoder, written from the reference's source
(Sources/Qwen3TTS/SpeechTokenizerEncoder.swift, TTSWeightLoading+Encoder.swift; SpeechTokenizerDecoder.swift:11-47 CausalConv1d, :414-424
and :467-485 the quantizer's encode).

It takes its primitives from tests/codec_oracle.py and adds only what the encoder has and the decoder has not: the strided causal conv,
the unmasked attention, the encoder chain and the RVQ encode.  Tensors are channel-last [T, C]; `dtype` of the Weights is the precision of
every array and intermediate (float64 is the oracle).  Nothing here reads the library under test.
"""
import math

import numpy as np

from codec_oracle import (REAL, REDUCED, SAMPLES_PER_FRAME, Weights, causal_conv, codebook, convnext, rms_norm, rope, silu,  # noqa: F401
                          snake_beta)


def strides(g):
    """The six strides in the order applied (:181, :197-203): upsample_rates reversed, then upsamplingRatios[1], [0]."""
    return tuple(reversed(g["upsample_rates"])) + tuple(reversed(g["upsampling_ratios"]))


def lengths(n, g):
    """Rows of a clip of n samples at every rate: a CausalConv1d of stride s pads k - 1 = 2 s - 1 on the left, so T -> ceil(T / s)."""
    out = [int(n)]
    for s in strides(g):
        out.append(-(-out[-1] // s))
    return out


def strided_causal_conv(x, w, b, stride):
    """CausalConv1d with stride (:11-47 of the decoder file): left pad k - 1 zeros, output t reads padded rows t s .. t s + k - 1."""
    T, k = x.shape[0], w.shape[2]
    xp = np.concatenate([np.zeros((k - 1, x.shape[1]), x.dtype), x])
    To = (T - 1) // stride + 1
    wt = np.ascontiguousarray(w.transpose(2, 1, 0))                               # [k, Cin, Cout]
    y = np.zeros((To, w.shape[0]), x.dtype)
    for j in range(k):
        y = y + xp[j:j + (To - 1) * stride + 1:stride] @ wt[j]
    return y + b


def residual_unit(x, W, p, dilation):
    """EncoderResidualUnit (:31-38)."""
    h = snake_beta(x, W[p + ".act1.alpha"], W[p + ".act1.beta"])
    h = causal_conv(h, W[p + ".conv1.conv.weight"], W[p + ".conv1.conv.bias"], dilation)
    h = snake_beta(h, W[p + ".act2.alpha"], W[p + ".act2.beta"])
    return causal_conv(h, W[p + ".conv2.conv.weight"], W[p + ".conv2.conv.bias"]) + x


def encoder_block(x, W, p, stride):
    """EncoderBlock (:63-70): three residual units, SnakeBeta, strided conv."""
    h = x
    for j, d in enumerate((1, 3, 9)):
        h = residual_unit(h, W, p + ".block.%d" % j, d)
    h = snake_beta(h, W[p + ".block.3.alpha"], W[p + ".block.3.beta"])
    return strided_causal_conv(h, W[p + ".block.4.conv.weight"], W[p + ".block.4.conv.bias"], stride)


def conv(pcm, W, g, trace=None):
    """callAsFunction up to postConv (:224-237): pcm [n] -> [frames, latent].  trace: a list that receives every level's row count."""
    st = strides(g)
    h = causal_conv(np.asarray(pcm).astype(W.dtype)[:, None], W["encoder.encoder.0.conv.weight"], W["encoder.encoder.0.conv.bias"])
    rows = [h.shape[0]]
    for i in range(4):
        h = encoder_block(h, W, "encoder.encoder.%d" % (i + 1), st[i])
        rows.append(h.shape[0])
    h = causal_conv(h, W["encoder.encoder.5.conv.weight"], W["encoder.encoder.5.conv.bias"])
    for i in range(2):
        p = "encoder.downsample.%d" % i
        h = convnext(h, W, p + ".0")
        h = strided_causal_conv(h, W[p + ".1.conv.weight"], W[p + ".1.conv.bias"], st[4 + i])
        rows.append(h.shape[0])
    if trace is not None:
        trace.extend(rows)
    return causal_conv(h, W["encoder.post_conv.conv.weight"], W["encoder.post_conv.conv.bias"])


def attention(h, W, p, g):
    """DecoderTransformerAttention with attentionMask nil (EncoderTransformer :96-98): every frame attends to every frame."""
    T, nh, hd = h.shape[0], g["num_heads"], g["head_dim"]
    q = rope((h @ W[p + ".q_proj.weight"].T).reshape(T, nh, hd))
    k = rope((h @ W[p + ".k_proj.weight"].T).reshape(T, nh, hd))
    v = (h @ W[p + ".v_proj.weight"].T).reshape(T, nh, hd)
    scale = h.dtype.type(1.0 / math.sqrt(hd))
    out = np.empty((T, nh, hd), h.dtype)
    for n in range(nh):
        s = (q[:, n] @ k[:, n].T) * scale
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        out[:, n] = (e / e.sum(axis=-1, keepdims=True)) @ v[:, n]
    return out.reshape(T, nh * hd) @ W[p + ".o_proj.weight"].T


def transformer(x, W, g):
    """EncoderTransformer (:94-102): x [T, latent] -> [T, hidden]; output_proj is not applied."""
    P = "encoder.pre_transformer."
    h = x @ W[P + "input_proj.weight"].T + W[P + "input_proj.bias"]
    for l in range(g["num_layers"]):
        L = P + "layers.%d." % l
        a = attention(rms_norm(h, W[L + "input_layernorm.weight"], g["rms_norm_eps"]), W, L + "self_attn", g)
        h = h + a * W[L + "self_attn_layer_scale.scale"]
        n = rms_norm(h, W[L + "post_attention_layernorm.weight"], g["rms_norm_eps"])
        m = (silu(n @ W[L + "mlp.gate_proj.weight"].T) * (n @ W[L + "mlp.up_proj.weight"].T)) @ W[L + "mlp.down_proj.weight"].T
        h = h + m * W[L + "mlp_layer_scale.scale"]
    return rms_norm(h, W[P + "norm.weight"], g["rms_norm_eps"])


def latent(pcm, W, g):
    return transformer(conv(pcm, W, g), W, g)


def distances(r, cb):
    """VectorQuantizerCodebook.encode's expanded form (:417-422): |r|^2 - 2 r.c + |c|^2, [T, size]."""
    return ((r * r).sum(axis=-1, keepdims=True) - r.dtype.type(2.0) * (r @ cb.T)) + (cb * cb).sum(axis=-1)[None, :]


def chains(g):
    """(name, first code row, codebooks) of the two quantizers."""
    return (("rvq_first", 0, 1), ("rvq_rest", 1, g["num_quantizers"] - 1))


def rvq_chain(r, W, name, count):
    """ResidualVectorQuantizer.encode's loop (:477-483) on a projected residual r [T, D]: codes [count, T]; argmin = lowest index."""
    codes = []
    for i in range(count):
        cb = codebook(W, "encoder.quantizer.%s.vq.layers.%d._codebook" % (name, i))
        c = distances(r, cb).argmin(axis=-1)
        r = r - cb[c]
        codes.append(c)
    return np.stack(codes)


def project(h, W, name):
    return h @ W["encoder.quantizer.%s.input_proj.weight" % name][:, :, 0]


def rvq_encode(h, W, g):
    """EncoderRVQ.encode (:130-134): h [T, hidden] -> codes [Q, T]; both quantizers encode the same h."""
    h = np.asarray(h).astype(W.dtype)
    return np.concatenate([rvq_chain(project(h, W, name), W, name, count) for name, _, count in chains(g)]).astype(np.int32)


def rvq_encode_split(h, W, g):
    """What the encoder must NOT compute: SplitResidualVectorQuantizer.encode (:526-532), the acoustic quantizer on h minus the decoded
    first code.  The decode side's projection is stood in by the pseudo-inverse of input_proj: any form that removes the first code's
    contribution from h serves the test that tells the two apart."""
    h = np.asarray(h).astype(W.dtype)
    first = rvq_chain(project(h, W, "rvq_first"), W, "rvq_first", 1)
    cb = codebook(W, "encoder.quantizer.rvq_first.vq.layers.0._codebook")
    back = cb[first[0]] @ np.linalg.pinv(W["encoder.quantizer.rvq_first.input_proj.weight"][:, :, 0].astype(np.float64)).astype(W.dtype)
    rest = rvq_chain(project(h - back, W, "rvq_rest"), W, "rvq_rest", g["num_quantizers"] - 1)
    return np.concatenate([first, rest]).astype(np.int32)


def encode(pcm, W, g):
    """SpeechTokenizerEncoder.callAsFunction (:223-241): pcm [n] -> codes [Q, ceil(n / 1920)]."""
    return rvq_encode(latent(pcm, W, g), W, g)


def make_pcm(seed, n):
    """Seeded mono PCM [n] (float32) for the tests: three tones under a slow envelope plus noise, peak below 1."""
    rng = np.random.default_rng(5200 + seed)
    t = np.arange(n, dtype=np.float64) / 24000.0
    f = rng.uniform(80.0, 3000.0, size=3)
    x = sum(a * np.sin(2 * np.pi * fk * t + ph) for a, fk, ph in zip((0.3, 0.2, 0.1), f, rng.uniform(0, 6.28, size=3)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 1.7 * t)) + 0.05 * rng.standard_normal(n)
    return x.astype(np.float32)

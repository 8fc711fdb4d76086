"""NumPy restatement of the Qwen3-TTS 12.5 Hz speech tokenizer decoder, written from the reference's source
(Sources/Qwen3TTS/SpeechTokenizerDecoder.swift, Configuration.swift:128-148, TTSWeightLoading.swift:190-301, :347-381, :458-480).

Every stage is its own function over a state dict in the checkpoint's names and PyTorch layouts (conv [out, in, k], transposed conv
[in, out, k], Linear [out, in]).  Tensors are channel-last [T, C]; every convolution is causal.  `dtype` is the precision of every array
and intermediate: float64 is the oracle, float32 its twin (tests/test_codec_cpu.py::test_f32_distance measures their distance, the source
of the GPU bounds).  Nothing here reads the library under test.
"""
import math

import numpy as np

REAL = dict(latent_dim=1024, decoder_dim=1536, hidden_size=512, num_heads=16, head_dim=64, num_layers=8, upsample_rates=(8, 5, 4, 3),
            upsampling_ratios=(2, 2), num_quantizers=16, semantic_codebook_size=2048, acoustic_codebook_size=2048, codebook_dim=256,
            rms_norm_eps=1e-8)
REDUCED = dict(REAL, latent_dim=96, decoder_dim=48, hidden_size=64, num_heads=2, num_layers=2, semantic_codebook_size=64,
               acoustic_codebook_size=64, codebook_dim=24)
SAMPLES_PER_FRAME, SAMPLE_RATE, CHUNK, LEFT_CONTEXT = 1920, 24000, 25, 10
_erf = np.vectorize(math.erf, otypes=[np.float64])


class Weights:
    """The state dict at one precision."""

    def __init__(self, sd, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.sd = {k: np.asarray(v).astype(self.dtype) for k, v in sd.items()}

    def __getitem__(self, k):
        return self.sd[k]

    def __contains__(self, k):
        return k in self.sd


# ---- primitives -------------------------------------------------------------------------------------------------------------------
def causal_conv(x, w, b=None, dilation=1):
    """CausalConv1d (:11-47): x [T, Cin], w [Cout, Cin, k]; left pad (k - 1) dilation zeros."""
    T, k = x.shape[0], w.shape[2]
    xp = np.concatenate([np.zeros(((k - 1) * dilation, x.shape[1]), x.dtype), x])
    wt = np.ascontiguousarray(w.transpose(2, 1, 0))                               # [k, Cin, Cout]
    y = np.zeros((T, w.shape[0]), x.dtype)
    for j in range(k):
        y = y + xp[j * dilation:j * dilation + T] @ wt[j]
    return y if b is None else y + b


def depthwise_causal_conv(x, w, b):
    """groups = channels: w [C, 1, k]."""
    T, k = x.shape[0], w.shape[2]
    xp = np.concatenate([np.zeros((k - 1, x.shape[1]), x.dtype), x])
    y = np.zeros_like(x)
    for j in range(k):
        y = y + xp[j:j + T] * w[:, 0, j]
    return y + b


def causal_transpose_conv(x, w, b, stride):
    """CausalTransposeConv1d (:52-86): w [Cin, Cout, k]; the full transposed conv with its last k - stride outputs trimmed."""
    T, k = x.shape[0], w.shape[2]
    wt = np.ascontiguousarray(w.transpose(2, 0, 1))                               # [k, Cin, Cout]
    full = np.zeros(((T - 1) * stride + k, w.shape[1]), x.dtype)
    for j in range(k):
        full[j:j + (T - 1) * stride + 1:stride] += x @ wt[j]
    return full[:full.shape[0] - (k - stride)] + b


def snake_beta(x, alpha, beta):
    """SnakeBeta (:92-111): x + (1 / exp(beta)) sin^2(exp(alpha) x)."""
    one = x.dtype.type(1.0)
    s = np.sin(np.exp(alpha) * x)
    return x + (one / np.exp(beta)) * (s * s)


def rms_norm(x, w, eps):
    return x * (one_over_sqrt((x * x).mean(axis=-1, keepdims=True) + x.dtype.type(eps))) * w


def one_over_sqrt(v):
    return v.dtype.type(1.0) / np.sqrt(v)


def layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) * one_over_sqrt(var + x.dtype.type(eps)) * w + b


def gelu(x):
    """Exact erf GELU (MLXNN.gelu)."""
    half, one = x.dtype.type(0.5), x.dtype.type(1.0)
    return half * x * (one + _erf(x * x.dtype.type(math.sqrt(0.5))).astype(x.dtype))


def silu(x):
    return x / (x.dtype.type(1.0) + np.exp(-x))


def rope(x, base=10000.0):
    """MLXNN.RoPE(dimensions: head_dim, traditional: false): x [T, heads, D], positions 0..T-1; element i pairs with i + D / 2."""
    T, D = x.shape[0], x.shape[-1]
    half = D // 2
    inv = (base ** (-np.arange(half, dtype=np.float64) / half)).astype(x.dtype)
    ang = np.arange(T, dtype=np.float64).astype(x.dtype)[:, None] * inv[None, :]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    return np.concatenate([x1 * c - x2 * s, x1 * s + x2 * c], axis=-1)


def rope_interleaved(x, base=10000.0):
    """The other convention (traditional: true), pairs (2i, 2i + 1): what the decoder must NOT compute."""
    T, D = x.shape[0], x.shape[-1]
    half = D // 2
    inv = (base ** (-np.arange(half, dtype=np.float64) / half)).astype(x.dtype)
    ang = np.arange(T, dtype=np.float64).astype(x.dtype)[:, None] * inv[None, :]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    out = np.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return out


# ---- stages -----------------------------------------------------------------------------------------------------------------------
def codebook(W, prefix):
    """TTSWeightLoading.swift:280-301: `embed`, else embedding_sum / max(cluster_usage, 1e-7)."""
    if prefix + ".embed" in W:
        return W[prefix + ".embed"]
    usage = np.maximum(W[prefix + ".cluster_usage"], W.dtype.type(1e-7))
    return W[prefix + ".embedding_sum"] / usage[:, None]


def quantizer_decode(codes, W, g):
    """SplitResidualVectorQuantizer.decode (:513-521): codes [Q, T] -> [T, hidden]."""
    codes = np.asarray(codes)
    first = codebook(W, "decoder.quantizer.rvq_first.vq.layers.0._codebook")[codes[0]]
    rest = None
    for i in range(g["num_quantizers"] - 1):
        e = codebook(W, "decoder.quantizer.rvq_rest.vq.layers.%d._codebook" % i)[codes[1 + i]]
        rest = e if rest is None else rest + e
    a = first @ W["decoder.quantizer.rvq_first.output_proj.weight"][:, :, 0].T
    return a + rest @ W["decoder.quantizer.rvq_rest.output_proj.weight"][:, :, 0].T


def pre_conv(x, W):
    return causal_conv(x, W["decoder.pre_conv.conv.weight"], W["decoder.pre_conv.conv.bias"])


def attention(h, W, p, g, rope_fn=rope):
    """DecoderTransformerAttention (:262-289) with the additive causal mask of DecoderTransformer (:371-382)."""
    T, nh, hd = h.shape[0], g["num_heads"], g["head_dim"]
    q = rope_fn((h @ W[p + ".q_proj.weight"].T).reshape(T, nh, hd))
    k = rope_fn((h @ W[p + ".k_proj.weight"].T).reshape(T, nh, hd))
    v = (h @ W[p + ".v_proj.weight"].T).reshape(T, nh, hd)
    scale = h.dtype.type(1.0 / math.sqrt(hd))
    out = np.empty((T, nh, hd), h.dtype)
    for n in range(nh):
        s = (q[:, n] @ k[:, n].T) * scale
        if T > 1:
            s = s + np.where(np.arange(T)[None, :] > np.arange(T)[:, None], h.dtype.type(-1e9), h.dtype.type(0))
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        out[:, n] = (e / e.sum(axis=-1, keepdims=True)) @ v[:, n]
    return out.reshape(T, nh * hd) @ W[p + ".o_proj.weight"].T


def pre_transformer(x, W, g, rope_fn=rope):
    """DecoderTransformer (:368-391): x [T, latent] -> [T, latent]."""
    P = "decoder.pre_transformer."
    h = x @ W[P + "input_proj.weight"].T + W[P + "input_proj.bias"]
    for l in range(g["num_layers"]):
        L = P + "layers.%d." % l
        a = attention(rms_norm(h, W[L + "input_layernorm.weight"], g["rms_norm_eps"]), W, L + "self_attn", g, rope_fn)
        h = h + a * W[L + "self_attn_layer_scale.scale"]
        n = rms_norm(h, W[L + "post_attention_layernorm.weight"], g["rms_norm_eps"])
        m = (silu(n @ W[L + "mlp.gate_proj.weight"].T) * (n @ W[L + "mlp.up_proj.weight"].T)) @ W[L + "mlp.down_proj.weight"].T
        h = h + m * W[L + "mlp_layer_scale.scale"]
    h = rms_norm(h, W[P + "norm.weight"], g["rms_norm_eps"])
    return h @ W[P + "output_proj.weight"].T + W[P + "output_proj.bias"]


def convnext(x, W, p):
    """ConvNeXtBlock (:156-165)."""
    h = depthwise_causal_conv(x, W[p + ".dwconv.conv.weight"], W[p + ".dwconv.conv.bias"])
    h = layer_norm(h, W[p + ".norm.weight"], W[p + ".norm.bias"])
    h = gelu(h @ W[p + ".pwconv1.weight"].T + W[p + ".pwconv1.bias"])
    h = h @ W[p + ".pwconv2.weight"].T + W[p + ".pwconv2.bias"]
    return h * W[p + ".gamma"] + x


def upsample(x, W, g):
    for s, ratio in enumerate(g["upsampling_ratios"]):
        p = "decoder.upsample.%d" % s
        x = causal_transpose_conv(x, W[p + ".0.conv.weight"], W[p + ".0.conv.bias"], ratio)
        x = convnext(x, W, p + ".1")
    return x


def residual_unit(x, W, p, dilation):
    """DecoderResidualUnit (:190-197)."""
    h = snake_beta(x, W[p + ".act1.alpha"], W[p + ".act1.beta"])
    h = causal_conv(h, W[p + ".conv1.conv.weight"], W[p + ".conv1.conv.bias"], dilation)
    h = snake_beta(h, W[p + ".act2.alpha"], W[p + ".act2.beta"])
    return causal_conv(h, W[p + ".conv2.conv.weight"], W[p + ".conv2.conv.bias"]) + x


def decoder_block(x, W, p, stride):
    """DecoderBlock (:221-228)."""
    h = snake_beta(x, W[p + ".block.0.alpha"], W[p + ".block.0.beta"])
    h = causal_transpose_conv(h, W[p + ".block.1.conv.weight"], W[p + ".block.1.conv.bias"], stride)
    for j, d in enumerate((1, 3, 9)):
        h = residual_unit(h, W, p + ".block.%d" % (j + 2), d)
    return h


def vocoder(x, W, g, clip=True):
    """decoder.decoder.0 .. 6 (:674-685): [4 T, latent] -> [1920 T]."""
    h = causal_conv(x, W["decoder.decoder.0.conv.weight"], W["decoder.decoder.0.conv.bias"])
    for i, s in enumerate(g["upsample_rates"]):
        h = decoder_block(h, W, "decoder.decoder.%d" % (i + 1), s)
    h = snake_beta(h, W["decoder.decoder.5.alpha"], W["decoder.decoder.5.beta"])
    h = causal_conv(h, W["decoder.decoder.6.conv.weight"], W["decoder.decoder.6.conv.bias"])[:, 0]
    return np.clip(h, -1.0, 1.0).astype(h.dtype) if clip else h


def forward(codes, W, g, clip=True):
    """SpeechTokenizerDecoder.callAsFunction (:658-688): codes [Q, T] -> [1920 T]."""
    h = quantizer_decode(codes, W, g)
    h = pre_conv(h, W)
    h = pre_transformer(h, W, g)
    h = upsample(h, W, g)
    return vocoder(h, W, g, clip)


def window_positions(T, chunk=CHUNK, left=LEFT_CONTEXT):
    """chunkedDecode's windows (:696-733) as (start, context, end): frames start..end are decoded, the first `context` dropped."""
    if T <= chunk + left:
        return [(0, 0, T)]
    out, offset = [], 0
    while offset < T:
        end = min(offset + chunk, T)
        start = max(offset - left, 0)
        out.append((start, offset - start, end))
        offset = end
    return out


def decode(codes, W, g, clip=True):
    """decode(codes:) (:739-744): chunked; always 1920 T samples."""
    codes = np.asarray(codes)
    parts = []
    for start, ctx, end in window_positions(codes.shape[1]):
        parts.append(forward(codes[:, start:end], W, g, clip)[ctx * SAMPLES_PER_FRAME:])
    return np.concatenate(parts)


def make_codes(seed, T, g):
    """Seeded codes [Q, T] (int32) for the tests."""
    rng = np.random.default_rng(4100 + seed)
    c = rng.integers(0, g["acoustic_codebook_size"], size=(g["num_quantizers"], T))
    c[0] = rng.integers(0, g["semantic_codebook_size"], size=T)
    return c.astype(np.int32)

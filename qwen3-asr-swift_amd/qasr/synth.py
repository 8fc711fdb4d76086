"""Synthetic weights and waveforms (there is no checkpoint or dataset offline).

Recipes are the ones SURVEY.md section 8(d) fixes, so bench numbers and parity tests are
reproducible:
  * weights: `torch.manual_seed(seed)`; N(0, 0.02) for Linear/Conv/Embedding, norm weight 1,
    bias 0 (HF `initializer_range`), cast to bf16.  `init="stress"` instead draws
    N(0, 1/fan_in) weights, non-zero biases and non-unit norm gains so that attention is
    peaked and every bias/gain path is exercised by the parity tests.
  * waveform k: 0.4 sin(2 pi f1 t) + 0.2 sin(2 pi f2 t) + 0.05 N(0,1), f1 = 220 + 37k,
    f2 = 1200 + 91k, rng(20260418 + k), quantised to PCM16 and back.
Tensor names/layouts are the reference checkpoint's (Sources/Qwen3ASR/WeightLoading.swift:
235-323): conv weights [out, kH, kW, in]; Linear [out, in]; float decoder (FloatTextDecoder).
"""
import math
import numpy as np
import torch


def synth_waveform(k: int, seconds: float, sample_rate: int = 16000) -> np.ndarray:
    n = int(round(seconds * sample_rate))
    rng = np.random.default_rng(20260418 + k)
    t = np.arange(n, dtype=np.float64) / sample_rate
    f1, f2 = 220.0 + 37.0 * k, 1200.0 + 91.0 * k
    x = 0.4 * np.sin(2 * np.pi * f1 * t) + 0.2 * np.sin(2 * np.pi * f2 * t) + 0.05 * rng.standard_normal(n)
    pcm16 = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return (pcm16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def synth_state_dict(audio_cfg, text_cfg, seed: int = 0, init: str = "hf", dtype=torch.bfloat16, classify_num: int = 0):
    """audio_cfg / text_cfg: any objects with the fields of qasr.config presets.  classify_num > 0 adds the forced
    aligner's `lm_head.{weight,bias}` Linear(hidden, classify_num) (WeightLoading.swift:228-230)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def w(name, *shape, fan_in=None):
        std = 0.02 if init == "hf" else 1.0 / math.sqrt(fan_in if fan_in else shape[-1])
        sd[name] = (torch.randn(*shape, generator=g) * std).to(dtype)

    def b(name, n):
        sd[name] = (torch.zeros(n) if init == "hf" else torch.randn(n, generator=g) * 0.05).to(dtype)

    def gain(name, n):
        sd[name] = (torch.ones(n) if init == "hf" else 1.0 + 0.1 * torch.randn(n, generator=g)).to(dtype)

    a = audio_cfg
    C = a.conv_channels
    w("audio_tower.conv2d1.weight", C, 3, 3, 1, fan_in=9)
    b("audio_tower.conv2d1.bias", C)
    for n in ("conv2d2", "conv2d3"):
        w(f"audio_tower.{n}.weight", C, 3, 3, C, fan_in=9 * C)
        b(f"audio_tower.{n}.bias", C)
    w("audio_tower.conv_out.weight", a.d_model, a.conv_out_in)
    for i in range(a.layers):
        p = f"audio_tower.layers.{i}"
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            w(f"{p}.self_attn.{n}.weight", a.d_model, a.d_model)
            b(f"{p}.self_attn.{n}.bias", a.d_model)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            gain(f"{p}.{n}.weight", a.d_model)
            b(f"{p}.{n}.bias", a.d_model)
        w(f"{p}.fc1.weight", a.ffn_dim, a.d_model)
        b(f"{p}.fc1.bias", a.ffn_dim)
        w(f"{p}.fc2.weight", a.d_model, a.ffn_dim)
        b(f"{p}.fc2.bias", a.d_model)
    gain("audio_tower.ln_post.weight", a.d_model)
    b("audio_tower.ln_post.bias", a.d_model)
    w("audio_tower.proj1.weight", a.d_model, a.d_model)
    b("audio_tower.proj1.bias", a.d_model)
    w("audio_tower.proj2.weight", a.output_dim, a.d_model)
    b("audio_tower.proj2.bias", a.output_dim)

    t = text_cfg
    sd["model.embed_tokens.weight"] = (torch.randn(t.vocab, t.hidden, generator=g) *
                                       (0.02 if init == "hf" else 0.05)).to(dtype)
    for i in range(t.layers):
        p = f"model.layers.{i}"
        w(f"{p}.self_attn.q_proj.weight", t.heads * t.head_dim, t.hidden)
        w(f"{p}.self_attn.k_proj.weight", t.kv_heads * t.head_dim, t.hidden)
        w(f"{p}.self_attn.v_proj.weight", t.kv_heads * t.head_dim, t.hidden)
        w(f"{p}.self_attn.o_proj.weight", t.hidden, t.heads * t.head_dim)
        gain(f"{p}.self_attn.q_norm.weight", t.head_dim)
        gain(f"{p}.self_attn.k_norm.weight", t.head_dim)
        gain(f"{p}.input_layernorm.weight", t.hidden)
        gain(f"{p}.post_attention_layernorm.weight", t.hidden)
        w(f"{p}.mlp.gate_proj.weight", t.inter, t.hidden)
        w(f"{p}.mlp.up_proj.weight", t.inter, t.hidden)
        w(f"{p}.mlp.down_proj.weight", t.hidden, t.inter)
    gain("model.norm.weight", t.hidden)
    if classify_num:
        std = 0.02 if init == "hf" else 1.0 / math.sqrt(t.hidden)
        sd["lm_head.weight"] = (torch.randn(classify_num, t.hidden, generator=g) * std).to(dtype)
        sd["lm_head.bias"] = (torch.randn(classify_num, generator=g) * 0.05).to(dtype)
    return sd


QUANT_GROUP = 64


def quantize_linear(w, bits, group=QUANT_GROUP):
    """MLX affine quantisation of one [out, in] weight (mlx `quantize`: per 64-element group of a row, scale and bias from
    the group's min / max, q in [0, 2^bits)) -> (packed int32 [out, in * bits / 32] holding the uint32 words, LSB-first
    element order, scales, biases in w's dtype).  This is how a synthetic MLX-4bit / 8bit checkpoint is made for the tests
    and the W4 / W8 bench legs; the on-disk format is the reference's (Sources/MLXCommon/WeightLoading.swift:48-96)."""
    dt = w.dtype
    x = w.to(torch.float32)
    out, n = x.shape
    assert n % group == 0 and bits in (4, 8)
    g = x.reshape(out, n // group, group)
    n_bins = float((1 << bits) - 1)
    w_max, w_min = g.max(dim=-1).values, g.min(dim=-1).values
    mask = w_min.abs() > w_max.abs()
    scales = torch.clamp((w_max - w_min) / n_bins, min=1e-7)
    scales = torch.where(mask, scales, -scales)
    edge = torch.where(mask, w_min, w_max)
    q0 = torch.round(edge / scales)
    scales = torch.where(q0 != 0, edge / q0, scales)
    biases = torch.where(q0 == 0, torch.zeros_like(edge), edge)
    scales, biases = scales.to(dt), biases.to(dt)
    q = torch.clamp(torch.round((g - biases.to(torch.float32)[..., None]) / scales.to(torch.float32)[..., None]), 0, n_bins)
    q = q.reshape(out, n).to(torch.int64)
    per = 32 // bits
    q = q.reshape(out, n // per, per)
    shifts = torch.arange(per, dtype=torch.int64) * bits
    words = (q << shifts).sum(dim=-1)                       # < 2^32
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return words.contiguous(), scales.contiguous(), biases.contiguous()


def quantize_state_dict(sd, bits, group=QUANT_GROUP):
    """Float decoder state dict -> the quantised checkpoint layout: every `model.layers.*` Linear and the tied
    `model.embed_tokens` become {weight: packed uint32 (as int32 bits), scales, biases}; norms and the audio tower stay
    float (QuantizedTextDecoder.swift:178-199, AudioEncoder is not quantised)."""
    out = {}
    for k, v in sd.items():
        is_lin = k.startswith("model.layers.") and k.endswith("_proj.weight")
        if is_lin or k == "model.embed_tokens.weight":
            stem = k[:-len(".weight")]
            out[k], out[stem + ".scales"], out[stem + ".biases"] = quantize_linear(v, bits, group)
        else:
            out[k] = v
    return out


class _TensorSink(dict):
    """dict stand-in that hands every assigned tensor to a callback and keeps nothing (a 7B variant is 26 GB of f32 on the host otherwise)."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def __setitem__(self, name, tensor):
        self.fn(name, tensor)


def synth_omnilingual_state_dict(cfg, seed=0, bits=0, dtype=torch.float32, sink=None):
    """Seeded random weights of an Omnilingual (wav2vec2-CTC) model under the reference's fairseq2 tensor names
    (MLX/OmnilingualMLXWeightLoader.swift:40-135): PyTorch Conv1d layout [out, in, k], weight_g / weight_v for the
    positional conv, every encoder / head Linear with a bias.  cfg: object with model_dim, layers, heads, ffn_dim,
    feature_dim, pos_kernel, pos_groups, vocab.  bits 4 / 8: the encoder and head linears as MLX triplets (f32 scales, as
    the reference's loader widens them), else float weights.  sink(name, tensor): stream the tensors to a consumer instead of returning
    them (same seeded values in the same order)."""
    g = torch.Generator().manual_seed(seed)
    sd = {} if sink is None else _TensorSink(sink)
    kernels = (10, 3, 3, 3, 3, 2, 2)

    def rnd(*shape, std):
        return (torch.randn(*shape, generator=g) * std).to(dtype)

    C, D, F = cfg.feature_dim, cfg.model_dim, cfg.ffn_dim
    for i, k in enumerate(kernels):
        p = f"encoder_frontend.feature_extractor.layers.{i}"
        cin = 1 if i == 0 else C
        sd[p + ".conv.weight"] = rnd(C, cin, k, std=1.0 / math.sqrt(cin * k))
        sd[p + ".conv.bias"] = rnd(C, std=0.05)
        sd[p + ".layer_norm.weight"] = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dtype)
        sd[p + ".layer_norm.bias"] = rnd(C, std=0.05)
    sd["encoder_frontend.post_extract_layer_norm.weight"] = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dtype)
    sd["encoder_frontend.post_extract_layer_norm.bias"] = rnd(C, std=0.05)
    sd["encoder_frontend.model_dim_proj.weight"] = rnd(D, C, std=1.0 / math.sqrt(C))
    sd["encoder_frontend.model_dim_proj.bias"] = rnd(D, std=0.05)
    cpg = D // cfg.pos_groups
    sd["encoder_frontend.pos_encoder.conv.weight_v"] = rnd(D, cpg, cfg.pos_kernel, std=1.0)
    sd["encoder_frontend.pos_encoder.conv.weight_g"] = (0.5 + 0.1 * torch.randn(1, 1, cfg.pos_kernel, generator=g)).abs().to(dtype)
    sd["encoder_frontend.pos_encoder.conv.bias"] = rnd(D, std=0.05)

    def lin(stem, n, k):
        w = rnd(n, k, std=1.0 / math.sqrt(k))
        if bits in (4, 8):
            wq, s, b = quantize_linear(w.to(torch.bfloat16), bits)
            sd[stem + ".weight"], sd[stem + ".scales"], sd[stem + ".biases"] = wq, s.to(torch.float32), b.to(torch.float32)
        else:
            sd[stem + ".weight"] = w
        sd[stem + ".bias"] = rnd(n, std=0.05)

    for l in range(cfg.layers):
        p = f"encoder.layers.{l}"
        for nme in ("q_proj", "k_proj", "v_proj", "output_proj"):
            lin(f"{p}.self_attn.{nme}", D, D)
        lin(f"{p}.ffn.inner_proj", F, D)
        lin(f"{p}.ffn.output_proj", D, F)
        for nme in ("self_attn_layer_norm", "ffn_layer_norm"):
            sd[f"{p}.{nme}.weight"] = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dtype)
            sd[f"{p}.{nme}.bias"] = rnd(D, std=0.05)
    sd["encoder.layer_norm.weight"] = (1.0 + 0.1 * torch.randn(D, generator=g)).to(dtype)
    sd["encoder.layer_norm.bias"] = rnd(D, std=0.05)
    lin("final_proj", cfg.vocab, D)
    return sd


# ---- Silero VAD v5 (Sources/SpeechVAD/SileroModel.swift; keys and MLX layouts of SileroWeightLoading.swift) -------------------------
SILERO_SHAPES = {
    "stft.weight": (258, 256, 1),
    "encoder.0.weight": (128, 3, 129), "encoder.0.bias": (128,),
    "encoder.1.weight": (64, 3, 128), "encoder.1.bias": (64,),
    "encoder.2.weight": (64, 3, 64), "encoder.2.bias": (64,),
    "encoder.3.weight": (128, 3, 64), "encoder.3.bias": (128,),
    "lstm.Wx": (512, 128), "lstm.Wh": (512, 128), "lstm.bias": (512,),
    "decoder.weight": (1, 1, 128), "decoder.bias": (1,),
}


def synth_silero_state_dict(seed: int = 0) -> dict:
    """Seeded Silero-shaped weights (float32 numpy, reference key names and layouts: conv weights [out, k, in]).

    stft.weight is a real Hann-windowed DFT basis (rows 0..128 cos, 129..257 -sin; scaled by 1/16), so the magnitudes behave like the
    real model's.  The rest is fan-in scaled with a positive lean in the encoder, the g / o gates and the decoder, and negative biases,
    so that silence gives a low probability and loud frames a high one (the hysteresis then has something to find)."""
    rng = np.random.default_rng(77 + seed)
    n = np.arange(256)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / 256)
    k = np.arange(129)[:, None]
    ang = 2 * np.pi * k * n[None, :] / 256
    stft = np.concatenate([hann * np.cos(ang), -hann * np.sin(ang)], 0) / 16.0
    sd = {"stft.weight": stft[:, :, None]}
    for i, (co, ci) in enumerate([(128, 129), (64, 128), (64, 64), (128, 64)]):
        fan = 3 * ci
        sd[f"encoder.{i}.weight"] = (rng.standard_normal((co, 3, ci)) + 0.35) / np.sqrt(fan)
        sd[f"encoder.{i}.bias"] = -0.002 * np.abs(rng.standard_normal(co))
    wx = rng.standard_normal((512, 128)) / np.sqrt(128)
    wx[256:] += 0.6 / np.sqrt(128)                                     # g and o gates lean positive with the encoder output
    sd["lstm.Wx"] = wx
    sd["lstm.Wh"] = 0.5 * rng.standard_normal((512, 128)) / np.sqrt(128)
    b = 0.1 * rng.standard_normal(512)
    b[128:256] += 1.0                                                  # forget gate
    b[256:384] -= 1.0                                                  # g: negative cell input in silence
    sd["lstm.bias"] = b
    sd["decoder.weight"] = (np.abs(rng.standard_normal((1, 1, 128))) * 0.6 / np.sqrt(128))
    sd["decoder.bias"] = np.array([-2.0])
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


def write_silero_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), reshape=None) -> str:
    """Writes `sd` as model_dir/model.safetensors (dtype F32 | F16 | BF16).  `drop`: keys left out, `reshape`: {key: shape} written with a
    wrong shape (both for the loader's error tests).  Returns the file path."""
    return _write_safetensors(sd, model_dir, dtype, drop, reshape)


def _write_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), reshape=None, filename: str = "model.safetensors") -> str:
    import json
    import os
    os.makedirs(model_dir, exist_ok=True)
    header, blobs, off = {}, [], 0
    for key in sorted(sd):
        if key in drop:
            continue
        a = np.asarray(sd[key], dtype=np.float32)
        if reshape and key in reshape:
            a = np.resize(a, reshape[key])
        if dtype == "F32":
            raw = a.astype("<f4").tobytes()
        elif dtype == "F16":
            raw = a.astype("<f2").tobytes()
        elif dtype == "BF16":
            u = a.astype("<f4").view("<u4")
            raw = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype("<u2").tobytes()
        elif dtype == "F64":                                           # a dtype no loader accepts (error tests)
            raw = a.astype("<f8").tobytes()
        else:
            raise ValueError(dtype)
        header[key] = {"dtype": dtype, "shape": list(a.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    h = json.dumps(header).encode()
    h += b" " * ((8 - len(h) % 8) % 8)
    path = os.path.join(model_dir, filename)
    with open(path, "wb") as f:
        f.write(len(h).to_bytes(8, "little"))
        f.write(h)
        for raw in blobs:
            f.write(raw)
    return path


WESPEAKER_BLOCKS = (3, 4, 6, 3)


def wespeaker_tensor_shapes() -> dict:
    """key -> shape of every WeSpeaker ResNet34 tensor (WeSpeakerModel.swift; MLX conv layout [out, kH, kW, in])."""
    s = {"conv1.weight": (32, 3, 3, 1), "conv1.bias": (32,)}
    for st, nb in enumerate(WESPEAKER_BLOCKS):
        C, Cp = 32 << st, (16 << st if st else 32)
        for i in range(nb):
            cin = Cp if i == 0 else C
            p = f"layer{st + 1}.{i}."
            s[p + "conv1.weight"], s[p + "conv1.bias"] = (C, 3, 3, cin), (C,)
            s[p + "conv2.weight"], s[p + "conv2.bias"] = (C, 3, 3, C), (C,)
            if st > 0 and i == 0:
                s[p + "shortcut.weight"], s[p + "shortcut.bias"] = (C, 1, 1, Cp), (C,)
    s["embedding.weight"], s["embedding.bias"] = (256, 5120), (256,)
    return s


def synth_wespeaker_state_dict(seed: int = 0) -> dict:
    """Seeded WeSpeaker-shaped weights (float32 numpy, reference keys and layouts), shaped like a BN-fused ResNet34:
    He-scaled 3x3 convs with a small negative bias after each (a fused BN's shift), the second conv of every block and the shortcut scaled
    down so the 16 residual sums keep activations O(1); the embedding reads the pooled statistics with zero-mean rows over each
    (mean | std) half so the shared positive level of post-ReLU statistics does not dominate and different inputs give clearly
    different embeddings."""
    rng = np.random.default_rng(4242 + seed)
    sd = {}
    for k, shp in wespeaker_tensor_shapes().items():
        if k.endswith(".bias"):
            continue
        fan = int(np.prod(shp[1:]))
        w = rng.standard_normal(shp) * np.sqrt(2.0 / fan)
        if ".conv2." in k:
            w *= 0.35
        elif ".shortcut." in k:
            w *= 0.7
        sd[k] = w
    for k, shp in wespeaker_tensor_shapes().items():
        if k.endswith(".bias") and k != "embedding.bias":
            sd[k] = -0.05 + 0.05 * rng.standard_normal(shp)
    e = rng.standard_normal((256, 5120)) / np.sqrt(5120)
    for h in (slice(0, 2560), slice(2560, 5120)):
        e[:, h] -= e[:, h].mean(axis=1, keepdims=True)
    sd["embedding.weight"] = e
    sd["embedding.bias"] = 0.01 * rng.standard_normal(256)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


def write_wespeaker_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), extra=(), reshape=None) -> str:
    """Writes `sd` as model_dir/model.safetensors (dtype F32 | F16 | BF16; F64 for the dtype error).  `drop`: keys left out, `extra`:
    (key, array) pairs added (unknown keys), `reshape`: {key: shape} written with a wrong shape.  Returns the file path."""
    d = dict(sd)
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        d[k] = np.asarray(v, dtype=np.float32)
    return _write_safetensors(d, model_dir, dtype, drop, reshape)


def pyannote_tensor_shapes() -> dict:
    """key -> shape of every PyanNet segmentation tensor (Segmentation.swift, SincNet.swift, BiLSTM.swift; MLX conv layout [out, k, in])."""
    s = {"sincnet.wav_norm.weight": (1,), "sincnet.wav_norm.bias": (1,)}
    for i, (co, k, ci) in enumerate([(80, 251, 1), (60, 5, 80), (60, 5, 60)]):
        s[f"sincnet.conv.{i}.weight"], s[f"sincnet.conv.{i}.bias"] = (co, k, ci), (co,)
        s[f"sincnet.norm.{i}.weight"], s[f"sincnet.norm.{i}.bias"] = (co,), (co,)
    for d in ("lstm_fwd", "lstm_bwd"):
        for l in range(4):
            p = f"{d}.layers.{l}."
            s[p + "Wx"], s[p + "Wh"], s[p + "bias"] = (512, 60 if l == 0 else 256), (512, 128), (512,)
    s["linear.0.weight"], s["linear.0.bias"] = (128, 256), (128,)
    s["linear.1.weight"], s["linear.1.bias"] = (128, 128), (128,)
    s["classifier.weight"], s["classifier.bias"] = (7, 128), (7,)
    return s


def synth_pyannote_state_dict(seed: int = 0) -> dict:
    """Seeded PyanNet-shaped weights (float32 numpy, reference keys and layouts).

    sincnet.conv.0 holds real band-passes, as the converted checkpoint does: 80 Hamming-windowed differences of two sincs with mel-spaced
    edges from 40 Hz to 7.6 kHz, unit energy.  The rest is fan-in scaled; the LSTMs carry a forget-gate bias so their state follows the
    0.25 s level pattern of the test clips instead of single frames, and the classifier has a gain of several units so that the
    posteriors move across the thresholds with the input (tests/test_pyannote_cpu.py asserts what the tests need of them)."""
    rng = np.random.default_rng(9111 + seed)
    sd = {"sincnet.wav_norm.weight": np.array([0.9]), "sincnet.wav_norm.bias": np.array([0.02])}
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    edges = hz(np.linspace(mel(40.0), mel(7600.0), 82))
    t = (np.arange(251) - 125) / 16000.0
    ham = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(251) / 250)
    bank = np.zeros((80, 251))
    for c in range(80):
        lo, hi = edges[c], edges[c + 2]
        f = (2 * hi * np.sinc(2 * hi * t) - 2 * lo * np.sinc(2 * lo * t)) * ham
        bank[c] = f / np.sqrt((f * f).sum())
    sd["sincnet.conv.0.weight"] = bank[:, :, None]
    sd["sincnet.conv.0.bias"] = 0.01 * rng.standard_normal(80)
    for i, (co, k, ci) in enumerate([(80, 251, 1), (60, 5, 80), (60, 5, 60)]):
        if i > 0:
            sd[f"sincnet.conv.{i}.weight"] = 1.5 * rng.standard_normal((co, k, ci)) / np.sqrt(k * ci)
            sd[f"sincnet.conv.{i}.bias"] = 0.05 * rng.standard_normal(co)
        sd[f"sincnet.norm.{i}.weight"] = 1.0 + 0.1 * rng.standard_normal(co)
        sd[f"sincnet.norm.{i}.bias"] = 0.1 * rng.standard_normal(co)
    for d in ("lstm_fwd", "lstm_bwd"):
        for l in range(4):
            p, cin = f"{d}.layers.{l}.", (60 if l == 0 else 256)
            sd[p + "Wx"] = 1.2 * rng.standard_normal((512, cin)) / np.sqrt(cin)
            sd[p + "Wh"] = 0.6 * rng.standard_normal((512, 128)) / np.sqrt(128)
            b = 0.1 * rng.standard_normal(512)
            b[128:256] += 1.5                                          # forget gate: the state outlives a frame
            sd[p + "bias"] = b
    sd["linear.0.weight"] = 1.4 * rng.standard_normal((128, 256)) / np.sqrt(256)
    sd["linear.0.bias"] = 0.05 * rng.standard_normal(128)
    sd["linear.1.weight"] = 1.4 * rng.standard_normal((128, 128)) / np.sqrt(128)
    sd["linear.1.bias"] = 0.05 * rng.standard_normal(128)
    sd["classifier.weight"] = PYANNOTE_CLASSIFIER_GAIN * rng.standard_normal((7, 128)) / np.sqrt(128)
    sd["classifier.bias"] = np.zeros(7)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


PYANNOTE_CLASSIFIER_GAIN = 8.0


def write_pyannote_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), extra=(), reshape=None) -> str:
    """Writes `sd` as model_dir/model.safetensors (dtype F32 | F16 | BF16; F64 for the dtype error).  `drop`: keys left out, `extra`:
    (key, array) pairs added (unknown keys), `reshape`: {key: shape} written with a wrong shape.  Returns the file path."""
    return write_wespeaker_safetensors(sd, model_dir, dtype, drop, extra, reshape)


OPENUNMIX_STEMS = ("vocals", "drums", "bass", "other")


def openunmix_tensor_shapes(hidden: int = 512) -> dict:
    """key -> shape of every tensor of one Open-Unmix stem file (OpenUnmixModel.swift:59-85, 229-236)."""
    H = hidden
    s = {"input_mean": (1487,), "input_scale": (1487,), "output_mean": (2049,), "output_scale": (2049,),
         "fc1.weight": (H, 2974), "fc2.weight": (H, 2 * H), "fc3.weight": (4098, H)}
    for i, f in enumerate((H, H, 4098)):
        for k in ("weight", "bias", "running_mean", "running_var"):
            s[f"bn{i + 1}.{k}"] = (f,)
    for l in range(3):
        for d in ("forward", "backward"):
            p = f"lstm.layers.{l}.{d}."
            s[p + "weight_ih"], s[p + "weight_hh"] = (2 * H, H), (2 * H, H // 2)
            s[p + "bias_ih"], s[p + "bias_hh"] = (2 * H,), (2 * H,)
    return s


def synth_openunmix_state_dict(seed: int = 0, hidden: int = 512) -> dict:
    """Seeded Open-Unmix-shaped weights: {stem: {key: float32 array}} in the reference's keys and layouts.

    Fan-in scaled matrices; BatchNorm running statistics away from (0, 1) and affine weights away from (1, 0); input_mean negative and
    input_scale positive of the order of the real checkpoint's (magnitudes of a few units map to O(1) inputs); output_scale positive and
    output_mean about 0.6 so the ReLU mask is neither zero everywhere nor saturated (tests/test_openunmix_cpu.py asserts that)."""
    H = hidden
    out = {}
    for si, stem in enumerate(OPENUNMIX_STEMS):
        rng = np.random.default_rng(77001 + 10 * seed + si)
        sd = {}
        sd["input_mean"] = -1.5 + 0.3 * rng.standard_normal(1487)
        sd["input_scale"] = 0.25 + 0.1 * rng.random(1487)
        sd["output_mean"] = 0.6 + 0.1 * rng.standard_normal(2049)
        sd["output_scale"] = 0.5 + 0.2 * rng.random(2049)
        sd["fc1.weight"] = 1.5 * rng.standard_normal((H, 2974)) / np.sqrt(2974)
        sd["fc2.weight"] = 1.5 * rng.standard_normal((H, 2 * H)) / np.sqrt(2 * H)
        sd["fc3.weight"] = 1.5 * rng.standard_normal((4098, H)) / np.sqrt(H)
        for i, f in enumerate((H, H, 4098)):
            sd[f"bn{i + 1}.weight"] = 1.0 + 0.2 * rng.standard_normal(f)
            sd[f"bn{i + 1}.bias"] = 0.1 * rng.standard_normal(f)
            sd[f"bn{i + 1}.running_mean"] = 0.2 * rng.standard_normal(f)
            sd[f"bn{i + 1}.running_var"] = 0.5 + rng.random(f)
        for l in range(3):
            for d in ("forward", "backward"):
                p = f"lstm.layers.{l}.{d}."
                sd[p + "weight_ih"] = 1.2 * rng.standard_normal((2 * H, H)) / np.sqrt(H)
                sd[p + "weight_hh"] = 0.8 * rng.standard_normal((2 * H, H // 2)) / np.sqrt(H // 2)
                sd[p + "bias_ih"] = 0.1 * rng.standard_normal(2 * H)
                b = 0.1 * rng.standard_normal(2 * H)
                b[H // 2:H] += 1.0                                       # forget gate: the state outlives a frame
                sd[p + "bias_hh"] = b
        out[stem] = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}
    return out


def write_openunmix_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), reshape=None, skip_stems=()) -> str:
    """Writes {stem: state dict} as model_dir/{vocals,drums,bass,other}.safetensors.  For the loader's error tests: `drop` keys are left
    out and `reshape` {key: shape} written with a wrong shape, both in the "drums" file only; `skip_stems` files are not written."""
    import os
    for stem in OPENUNMIX_STEMS:
        if stem in skip_stems or stem not in sd:
            continue
        tweak = stem == "drums"
        path = _write_safetensors(sd[stem], model_dir, dtype, drop if tweak else (), reshape if tweak else None)
        os.replace(path, os.path.join(model_dir, stem + ".safetensors"))
    return model_dir


# ---- Qwen3-TTS speech tokenizer decoder (SpeechTokenizerDecoder.swift, Configuration.swift:128-148) -------------------------------
CODEC_REAL = dict(latent_dim=1024, decoder_dim=1536, hidden_size=512, num_heads=16, head_dim=64, num_layers=8,
                  upsample_rates=(8, 5, 4, 3), upsampling_ratios=(2, 2), num_quantizers=16, semantic_codebook_size=2048,
                  acoustic_codebook_size=2048, codebook_dim=256, rms_norm_eps=1e-8)
CODEC_REDUCED = dict(CODEC_REAL, latent_dim=96, decoder_dim=48, hidden_size=64, num_heads=2, num_layers=2, semantic_codebook_size=64,
                     acoustic_codebook_size=64, codebook_dim=24)


def speech_tokenizer_tensor_shapes(geometry=None) -> dict:
    """key -> shape of every decoder tensor in the checkpoint's names and PyTorch layouts (TTSWeightLoading.swift:190-301, :347-381,
    :458-480).  A codebook appears under its `embed` key; the loader also takes embedding_sum + cluster_usage in its place."""
    g = geometry or CODEC_REAL
    L, H, Dd, D, A = g["latent_dim"], g["hidden_size"], g["decoder_dim"], g["codebook_dim"], g["num_heads"] * g["head_dim"]
    s = {}
    for name, n, size in (("rvq_first", 1, g["semantic_codebook_size"]), ("rvq_rest", g["num_quantizers"] - 1, g["acoustic_codebook_size"])):
        for i in range(n):
            s[f"decoder.quantizer.{name}.vq.layers.{i}._codebook.embed"] = (size, D)
        s[f"decoder.quantizer.{name}.output_proj.weight"] = (H, D, 1)
    s["decoder.pre_conv.conv.weight"], s["decoder.pre_conv.conv.bias"] = (L, H, 3), (L,)
    P = "decoder.pre_transformer."
    s[P + "input_proj.weight"], s[P + "input_proj.bias"] = (H, L), (H,)
    s[P + "output_proj.weight"], s[P + "output_proj.bias"] = (L, H), (L,)
    s[P + "norm.weight"] = (H,)
    for l in range(g["num_layers"]):
        p = P + f"layers.{l}."
        for k in ("q_proj", "k_proj", "v_proj"):
            s[p + f"self_attn.{k}.weight"] = (A, H)
        s[p + "self_attn.o_proj.weight"] = (H, A)
        s[p + "input_layernorm.weight"] = s[p + "post_attention_layernorm.weight"] = (H,)
        s[p + "mlp.gate_proj.weight"] = s[p + "mlp.up_proj.weight"] = (2 * H, H)
        s[p + "mlp.down_proj.weight"] = (H, 2 * H)
        s[p + "self_attn_layer_scale.scale"] = s[p + "mlp_layer_scale.scale"] = (H,)
    for i, r in enumerate(g["upsampling_ratios"]):
        p = f"decoder.upsample.{i}."
        s[p + "0.conv.weight"], s[p + "0.conv.bias"] = (L, L, 2 * r), (L,)
        s[p + "1.dwconv.conv.weight"], s[p + "1.dwconv.conv.bias"] = (L, 1, 7), (L,)
        s[p + "1.norm.weight"] = s[p + "1.norm.bias"] = s[p + "1.gamma"] = s[p + "1.pwconv2.bias"] = (L,)
        s[p + "1.pwconv1.weight"], s[p + "1.pwconv1.bias"] = (4 * L, L), (4 * L,)
        s[p + "1.pwconv2.weight"] = (L, 4 * L)
    s["decoder.decoder.0.conv.weight"], s["decoder.decoder.0.conv.bias"] = (Dd, L, 7), (Dd,)
    c = Dd
    for b, r in enumerate(g["upsample_rates"]):
        p, co = f"decoder.decoder.{b + 1}.block.", c // 2
        s[p + "0.alpha"] = s[p + "0.beta"] = (c,)
        s[p + "1.conv.weight"], s[p + "1.conv.bias"] = (c, co, 2 * r), (co,)
        for j in (2, 3, 4):
            for a in ("act1", "act2"):
                s[p + f"{j}.{a}.alpha"] = s[p + f"{j}.{a}.beta"] = (co,)
            s[p + f"{j}.conv1.conv.weight"], s[p + f"{j}.conv2.conv.weight"] = (co, co, 7), (co, co, 1)
            s[p + f"{j}.conv1.conv.bias"] = s[p + f"{j}.conv2.conv.bias"] = (co,)
        c = co
    s["decoder.decoder.5.alpha"] = s["decoder.decoder.5.beta"] = (c,)
    s["decoder.decoder.6.conv.weight"], s["decoder.decoder.6.conv.bias"] = (1, c, 7), (1,)
    return s


def synth_speech_tokenizer_state_dict(seed: int = 0, geometry=None) -> dict:
    """Seeded decoder weights {key: float32 array}, drawn so that a test can see every layer: layer scales around 0.5 (at the reference's
    initial 0.01 a wrong attention hides under the tolerance), alpha and beta in [-0.5, 0.5], norm weights away from 1, fan-in scaled
    matrices whose gains keep the signal O(1) through the residual chain and the pre-clip output inside (-1, 1)
    (tests/test_codec_cpu.py asserts that).  Even codebooks are stored as `embed`, odd ones as embedding_sum + cluster_usage with
    a few usages below the loader's 1e-7 clamp."""
    g = geometry or CODEC_REAL
    rng = np.random.default_rng(91001 + seed)
    sd = {}
    for key, shape in speech_tokenizer_tensor_shapes(g).items():
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "embed":
            e = rng.standard_normal(shape) * 0.5
            q = int(key.split(".layers.")[1].split(".")[0]) + (0 if "rvq_first" in key else 1)
            if q % 2 == 0:
                sd[key] = e
            else:
                usage = 0.5 + 4.0 * rng.random(shape[0])
                usage[rng.integers(0, shape[0], size=max(2, shape[0] // 16))] = 1e-9
                usage[:2] = 0.0
                sd[key[:-5] + "cluster_usage"] = usage
                sd[key[:-5] + "embedding_sum"] = e * np.maximum(usage, 1e-7)[:, None]
        elif leaf in ("alpha", "beta"):
            sd[key] = rng.uniform(-0.5, 0.5, shape)
        elif leaf in ("scale", "gamma"):
            sd[key] = 0.5 + 0.1 * rng.standard_normal(shape)
        elif leaf == "bias":
            sd[key] = 0.05 * rng.standard_normal(shape)
        elif len(shape) == 1:                                          # norm weights
            sd[key] = 1.0 + 0.2 * rng.standard_normal(shape)
        else:
            if "dwconv" in key:
                fan, gain = shape[2], 1.0
            elif ".block.1.conv" in key or ".0.conv.weight" in key and "upsample" in key:
                fan, gain = 2 * shape[0], 1.0                         # transposed conv: two taps of C_in reach an output
            elif len(shape) == 3:
                fan, gain = shape[1] * shape[2], (0.1 if "decoder.6" in key else 0.6 if ".conv1." in key or ".conv2." in key else 1.0)
            else:
                fan, gain = shape[1], 1.0
            sd[key] = gain * rng.standard_normal(shape) / np.sqrt(fan)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


def write_speech_tokenizer_safetensors(sd: dict, model_dir: str, geometry=None, dtype: str = "F32", drop=(), reshape=None) -> str:
    """Writes `sd` as model_dir/model.safetensors and, for a geometry given, model_dir/config.json with it under "decoder_config".
    `drop` / `reshape`: as write_silero_safetensors (the loader's error tests).  Returns model_dir."""
    import json
    import os
    _write_safetensors(sd, model_dir, dtype, drop, reshape)
    if geometry is not None:
        cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in geometry.items()}
        with open(os.path.join(model_dir, "config.json"), "w") as f:
            json.dump({"decoder_config": cfg}, f)
    return model_dir


# ---- Qwen3-TTS speech tokenizer encoder (SpeechTokenizerEncoder.swift, TTSWeightLoading+Encoder.swift) ----------------------------
def speech_tokenizer_encoder_tensor_shapes(geometry=None) -> dict:
    """key -> shape of every encoder.* tensor in the checkpoint's names and PyTorch layouts (TTSWeightLoading+Encoder.swift).  The channel
    schedule is the decoder's reversed (decoder_dim / 16 .. decoder_dim), the strides upsample_rates reversed then upsampling_ratios
    reversed.  input_proj is the [hidden, codebook_dim, 1] matrix ResidualVectorQuantizer.encode multiplies by.  A codebook appears
    under its `embed` key; the loader also takes embedding_sum + cluster_usage in its place."""
    g = geometry or CODEC_REAL
    L, H, Dd, D, A = g["latent_dim"], g["hidden_size"], g["decoder_dim"], g["codebook_dim"], g["num_heads"] * g["head_dim"]
    strides = tuple(reversed(g["upsample_rates"])) + tuple(reversed(g["upsampling_ratios"]))
    s = {}
    for name, n, size in (("rvq_first", 1, g["semantic_codebook_size"]), ("rvq_rest", g["num_quantizers"] - 1, g["acoustic_codebook_size"])):
        for i in range(n):
            s[f"encoder.quantizer.{name}.vq.layers.{i}._codebook.embed"] = (size, D)
        s[f"encoder.quantizer.{name}.input_proj.weight"] = (H, D, 1)
    c = Dd // 16
    s["encoder.encoder.0.conv.weight"], s["encoder.encoder.0.conv.bias"] = (c, 1, 7), (c,)
    for b in range(4):
        p = f"encoder.encoder.{b + 1}.block."
        for j in range(3):
            for a in ("act1", "act2"):
                s[p + f"{j}.{a}.alpha"] = s[p + f"{j}.{a}.beta"] = (c,)
            s[p + f"{j}.conv1.conv.weight"], s[p + f"{j}.conv2.conv.weight"] = (c, c, 7), (c, c, 1)
            s[p + f"{j}.conv1.conv.bias"] = s[p + f"{j}.conv2.conv.bias"] = (c,)
        s[p + "3.alpha"] = s[p + "3.beta"] = (c,)
        s[p + "4.conv.weight"], s[p + "4.conv.bias"] = (2 * c, c, 2 * strides[b]), (2 * c,)
        c *= 2
    s["encoder.encoder.5.conv.weight"], s["encoder.encoder.5.conv.bias"] = (L, Dd, 7), (L,)
    for i in range(2):
        p = f"encoder.downsample.{i}."
        s[p + "0.dwconv.conv.weight"], s[p + "0.dwconv.conv.bias"] = (L, 1, 7), (L,)
        s[p + "0.norm.weight"] = s[p + "0.norm.bias"] = s[p + "0.gamma"] = s[p + "0.pwconv2.bias"] = (L,)
        s[p + "0.pwconv1.weight"], s[p + "0.pwconv1.bias"] = (4 * L, L), (4 * L,)
        s[p + "0.pwconv2.weight"] = (L, 4 * L)
        s[p + "1.conv.weight"], s[p + "1.conv.bias"] = (L, L, 2 * strides[4 + i]), (L,)
    s["encoder.post_conv.conv.weight"], s["encoder.post_conv.conv.bias"] = (L, L, 3), (L,)
    P = "encoder.pre_transformer."
    s[P + "input_proj.weight"], s[P + "input_proj.bias"] = (H, L), (H,)
    s[P + "output_proj.weight"], s[P + "output_proj.bias"] = (L, H), (L,)
    s[P + "norm.weight"] = (H,)
    for l in range(g["num_layers"]):
        p = P + f"layers.{l}."
        for k in ("q_proj", "k_proj", "v_proj"):
            s[p + f"self_attn.{k}.weight"] = (A, H)
        s[p + "self_attn.o_proj.weight"] = (H, A)
        s[p + "input_layernorm.weight"] = s[p + "post_attention_layernorm.weight"] = (H,)
        s[p + "mlp.gate_proj.weight"] = s[p + "mlp.up_proj.weight"] = (2 * H, H)
        s[p + "mlp.down_proj.weight"] = (H, 2 * H)
        s[p + "self_attn_layer_scale.scale"] = s[p + "mlp_layer_scale.scale"] = (H,)
    return s


def synth_speech_tokenizer_encoder_state_dict(seed: int = 0, geometry=None) -> dict:
    """Seeded encoder weights {key: float32 array} by the decoder's drawing rules (synth_speech_tokenizer_state_dict), from an rng of
    their own: layer scales around 0.5, alpha and beta in [-0.5, 0.5], norm weights away from 1, fan-in scaled matrices (residual-unit
    convs at gain 0.6) that keep the signal O(1) down the chain, even codebooks stored as `embed`, odd ones as embedding_sum +
    cluster_usage with a few usages below the loader's 1e-7 clamp.  The input projections of the quantizers have unit gain, so a
    residual is on the scale of the codebook entries (std 0.5 per coordinate)."""
    g = geometry or CODEC_REAL
    rng = np.random.default_rng(73003 + seed)
    sd = {}
    for key, shape in speech_tokenizer_encoder_tensor_shapes(g).items():
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "embed":
            e = rng.standard_normal(shape) * 0.5
            q = int(key.split(".layers.")[1].split(".")[0]) + (0 if "rvq_first" in key else 1)
            if q % 2 == 0:
                sd[key] = e
            else:
                usage = 0.5 + 4.0 * rng.random(shape[0])
                usage[rng.integers(0, shape[0], size=max(2, shape[0] // 16))] = 1e-9
                usage[:2] = 0.0
                sd[key[:-5] + "cluster_usage"] = usage
                sd[key[:-5] + "embedding_sum"] = e * np.maximum(usage, 1e-7)[:, None]
        elif leaf in ("alpha", "beta"):
            sd[key] = rng.uniform(-0.5, 0.5, shape)
        elif leaf in ("scale", "gamma"):
            sd[key] = 0.5 + 0.1 * rng.standard_normal(shape)
        elif leaf == "bias":
            sd[key] = 0.05 * rng.standard_normal(shape)
        elif len(shape) == 1:                                          # norm weights
            sd[key] = 1.0 + 0.2 * rng.standard_normal(shape)
        else:
            if "dwconv" in key:
                fan, gain = shape[2], 1.0
            elif "quantizer" in key:
                fan, gain = shape[0], 1.0                             # h @ w sums over hidden
            elif len(shape) == 3:
                fan, gain = shape[1] * shape[2], (0.6 if ".conv1." in key or ".conv2." in key else 1.0)
            else:
                fan, gain = shape[1], 1.0
            sd[key] = gain * rng.standard_normal(shape) / np.sqrt(fan)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


def merge_speech_tokenizer_state_dicts(decoder_sd: dict, encoder_sd: dict) -> dict:
    """One state dict holding both halves (decoder.* and encoder.* keys), as the real model.safetensors does; write it with
    write_speech_tokenizer_safetensors."""
    both = dict(decoder_sd)
    for k, v in encoder_sd.items():
        if k in both:
            raise ValueError("key in both halves: " + k)
        both[k] = v
    return both


def tts_speaker_encoder_tensor_shapes(embedding_dim: int = 1024) -> dict:
    """key -> shape of every tensor of the Qwen3-TTS ECAPA-TDNN speaker encoder (SpeakerEncoder.swift:176-209; conv weights
    [out, k, in] as the checkpoint stores them, TTSWeightLoading.swift:436-437), keys without the `speaker_encoder.` prefix."""
    s = {}

    def conv(k, out, taps, cin):
        s[k + ".weight"], s[k + ".bias"] = (out, taps, cin), (out,)

    conv("blocks.0.conv", 512, 5, 128)
    for b in (1, 2, 3):
        p = f"blocks.{b}."
        conv(p + "tdnn1.conv", 512, 1, 512)
        for j in range(7):
            conv(p + f"res2net_block.blocks.{j}.conv", 64, 3, 64)
        conv(p + "tdnn2.conv", 512, 1, 512)
        conv(p + "se_block.conv1", 128, 1, 512)
        conv(p + "se_block.conv2", 512, 1, 128)
    conv("mfa.conv", 1536, 1, 1536)
    conv("asp.tdnn.conv", 128, 1, 4608)
    conv("asp.conv", 1536, 1, 128)
    conv("fc", int(embedding_dim), 1, 3072)
    return s


def synth_tts_speaker_encoder_state_dict(seed: int = 0, embedding_dim: int = 1024) -> dict:
    """Seeded speaker-encoder weights {key: float32 array}: every matrix N(0, 1 / fan_in) times a gain (sqrt 2 in front of a ReLU, 0.25
    for the initial conv, whose input is log-mel of several units), so activations stay O(1) through the three residual blocks, the
    squeeze-excitation gates sit around one half and the attention logits spread over a few units; small biases."""
    rng = np.random.default_rng(88117 + seed)
    sd = {}
    for key, shape in tts_speaker_encoder_tensor_shapes(embedding_dim).items():
        if key.endswith(".bias"):
            sd[key] = 0.05 * rng.standard_normal(shape)
            continue
        fan = shape[1] * shape[2]
        if key.startswith("blocks.0."):
            gain = 0.25
        elif "se_block" in key or key.startswith("asp.") or key.startswith("fc."):
            gain = 1.0
        else:
            gain = math.sqrt(2.0)
        if key.startswith("asp.conv"):
            gain = 3.0                                                 # tanh outputs are below one: logits a few units apart
        sd[key] = gain * rng.standard_normal(shape) / math.sqrt(fan)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


def write_tts_speaker_encoder_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), reshape=None, extra=()) -> str:
    """Writes `sd` under `speaker_encoder.` keys as model_dir/model.safetensors (dtype F32 | F16 | BF16; F64 for the dtype error).
    `drop`: written keys left out, `reshape`: {written key: shape} written with a wrong shape, `extra`: (key, array) pairs added as they
    are (the main checkpoint's other tensors, e.g. talker.*).  Returns model_dir."""
    d = {"speaker_encoder." + k: v for k, v in sd.items()}
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        d[k] = np.asarray(v, dtype=np.float32)
    _write_safetensors(d, model_dir, dtype, drop, reshape)
    return model_dir


# ---- CosyVoice3 HiFT vocoder (qasr_hift_*) ----------------------------------------------------------------------------------------
HIFT_CH, HIFT_UP_K, HIFT_DOWN_K, HIFT_SRC_K, HIFT_RES_K = (512, 256, 128, 64), (16, 11, 7), (30, 6, 1), (7, 7, 11), (3, 7, 11)


def cosyvoice_hifigan_tensor_shapes(ignored: bool = True) -> dict:
    """key -> shape of every tensor of hifigan.safetensors (HiFiGAN.swift:656-749, WeightLoading.swift:214-331; conv weights [out, k, in]
    as the file stores them).  ignored: with the keys the file holds and the reference never loads (every Snake's beta,
    up_activations.*, final_activation.*)."""
    s = {}

    def conv(k, out, taps, cin):
        s[k + ".weight"], s[k + ".bias"] = (out, taps, cin), (out,)

    def resblock(p, C, k):
        for d in range(3):
            conv(f"{p}.convs1.{d}", C, k, C)
            conv(f"{p}.convs2.{d}", C, k, C)
            for a in ("activations1", "activations2"):
                s[f"{p}.{a}.{d}.alpha"] = (C,)
                if ignored:
                    s[f"{p}.{a}.{d}.beta"] = (C,)

    for i in range(5):
        conv(f"f0_predictor.condnet.{2 * i}", 512, 4 if i == 0 else 3, 80 if i == 0 else 512)
    s["f0_predictor.classifier.weight"], s["f0_predictor.classifier.bias"] = (1, 512), (1,)
    s["m_source.l_linear.weight"], s["m_source.l_linear.bias"] = (1, 9), (1,)
    conv("conv_pre", 512, 5, 80)
    for i in range(3):
        C = HIFT_CH[i + 1]
        conv(f"ups.{i}", C, HIFT_UP_K[i], HIFT_CH[i])
        conv(f"source_downs.{i}", C, HIFT_DOWN_K[i], 18)
        resblock(f"source_resblocks.{i}", C, HIFT_SRC_K[i])
        for j in range(3):
            resblock(f"resblocks.{3 * i + j}", C, HIFT_RES_K[j])
        if ignored:
            s[f"up_activations.{i}.alpha"], s[f"up_activations.{i}.beta"] = (HIFT_CH[i],), (HIFT_CH[i],)
    conv("conv_post", 18, 7, 64)
    if ignored:
        s["final_activation.alpha"], s["final_activation.beta"] = (64,), (64,)
    return s


def synth_cosyvoice_hifigan_state_dict(seed: int = 0) -> dict:
    """Seeded HiFT weights {key: float32 array} on the real geometry (21 M parameters).  Every conv is N(0, gain^2 / fan_in): 1.2 in the
    F0 stack (ELU), 0.55 for the two convs that read the mel (its rms is about 1.8), 1.3 for the upsample convs (LeakyReLU), 0.5 inside
    the residual blocks so that three of them in a row leave the signal O(1); Snake alphas are log-normal around 1 (0.5 .. 2).  The
    classifier (deviation about 100 Hz around a bias of 24 Hz, folded by the abs) spreads F0 over roughly 0 .. 400 Hz with about one
    frame in ten under the 10 Hz voicing threshold, so that every test clip of 8 frames or more holds voiced and unvoiced frames; the merge
    weights give a voiced source of amplitude about 0.5; conv_post's outputs stay within +-4 and its magnitude half carries a bias
    of -1.2, so the waveform peaks well above 0.05 and rarely reaches the +-0.99 clamp (tests/test_hift_cpu.py asserts all four).
    The keys the reference ignores hold 1e3: a loader that read them would not go unnoticed."""
    rng = np.random.default_rng(44021 + seed)
    sd = {}
    for key, shape in cosyvoice_hifigan_tensor_shapes().items():
        if key.endswith(".beta") or key.startswith("up_activations.") or key.startswith("final_activation."):
            sd[key] = np.full(shape, 1e3)
        elif key.endswith(".alpha"):
            sd[key] = np.exp(0.3 * rng.standard_normal(shape))
        elif key == "f0_predictor.classifier.weight":
            sd[key] = 160.0 * rng.standard_normal(shape) / math.sqrt(512)
        elif key == "f0_predictor.classifier.bias":
            sd[key] = np.full(shape, 24.0)
        elif key == "m_source.l_linear.weight":
            sd[key] = 3.0 * rng.standard_normal(shape)
        elif key == "conv_post.bias":
            sd[key] = np.concatenate([np.full(9, -1.2), 0.05 * rng.standard_normal(9)])
        elif key.endswith(".bias"):
            sd[key] = 0.05 * rng.standard_normal(shape)
        else:
            fan = shape[1] * shape[2]
            if key.startswith("f0_predictor.condnet.0") or key.startswith("conv_pre"):
                gain = 0.55
            elif key.startswith("f0_predictor."):
                gain = 1.2
            elif key.startswith("ups."):
                gain = 1.3
            elif key.startswith("source_downs."):
                gain = 1.0
            elif key.startswith("conv_post"):
                gain = 0.4
            else:
                gain = 0.5
            sd[key] = gain * rng.standard_normal(shape) / math.sqrt(fan)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


def write_cosyvoice_hifigan_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), reshape=None, extra=()) -> str:
    """Writes `sd` as model_dir/hifigan.safetensors (dtype F32 | F16 | BF16; F64 for the dtype error).  `drop`: keys left out,
    `reshape`: {key: shape} written with a wrong shape, `extra`: (key, array) pairs added as they are.  Returns model_dir."""
    d = dict(sd)
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        d[k] = np.asarray(v, dtype=np.float32)
    _write_safetensors(d, model_dir, dtype, drop, reshape, filename="hifigan.safetensors")
    return model_dir


# ---- Qwen3-TTS Talker + code predictor (qasr_tts_*) ----------------------------------------------------------------------------
TTS_TALKER_REAL = dict(hidden=1024, layers=28, heads=16, kv_heads=8, head_dim=128, inter=3072, text_vocab=151936, text_hidden=2048,
                       codec_vocab=3072, cp_hidden=1024, cp_embedding_dim=1024, cp_layers=5, cp_heads=16, cp_kv_heads=8, cp_head_dim=128,
                       cp_inter=3072, cp_vocab=2048, bits=4, tts_pad=151671, tts_bos=151672, tts_eos=151673)
# reduced test geometries: a text vocabulary of 512 with the three text-side special ids remapped to its end
TTS_TALKER_SMALL = dict(TTS_TALKER_REAL, hidden=256, layers=2, heads=4, kv_heads=2, inter=512, text_vocab=512, text_hidden=128,
                        cp_hidden=256, cp_embedding_dim=256, cp_layers=2, cp_heads=4, cp_kv_heads=2, cp_inter=512,
                        tts_pad=509, tts_bos=510, tts_eos=511)
TTS_TALKER_LARGE_FORM = dict(TTS_TALKER_SMALL, hidden=512, inter=1024, cp_embedding_dim=512)   # embedding_dim != cp_hidden: the projection


def tts_talker_tensor_shapes(geometry=None) -> dict:
    """key -> (shape, quantised?) of every tensor of the Talker and the code predictor in the reference's key names
    (TTSWeightLoading.swift:24-158), with the `talker.` / `talker.code_predictor.` prefixes.  A quantised [out, in] Linear is stored as
    the triplet weight | scales | biases; `.bias` keys are float."""
    g = dict(TTS_TALKER_REAL, **(geometry or {}))
    s = {}

    def net(p, H, heads, kv, hd, inter, layers):
        for l in range(layers):
            q = f"{p}model.layers.{l}."
            s[q + "self_attn.q_proj.weight"] = ((heads * hd, H), True)
            s[q + "self_attn.k_proj.weight"] = ((kv * hd, H), True)
            s[q + "self_attn.v_proj.weight"] = ((kv * hd, H), True)
            s[q + "self_attn.o_proj.weight"] = ((H, heads * hd), True)
            s[q + "self_attn.q_norm.weight"] = ((hd,), False)
            s[q + "self_attn.k_norm.weight"] = ((hd,), False)
            s[q + "input_layernorm.weight"] = ((H,), False)
            s[q + "post_attention_layernorm.weight"] = ((H,), False)
            s[q + "mlp.gate_proj.weight"] = ((inter, H), True)
            s[q + "mlp.up_proj.weight"] = ((inter, H), True)
            s[q + "mlp.down_proj.weight"] = ((H, inter), True)
        s[p + "model.norm.weight"] = ((H,), False)

    t, c = "talker.", "talker.code_predictor."
    s[t + "model.codec_embedding.weight"] = ((g["codec_vocab"], g["hidden"]), False)
    s[t + "model.text_embedding.weight"] = ((g["text_vocab"], g["text_hidden"]), False)
    s[t + "text_projection.linear_fc1.weight"] = ((g["text_hidden"], g["text_hidden"]), True)
    s[t + "text_projection.linear_fc1.bias"] = ((g["text_hidden"],), False)
    s[t + "text_projection.linear_fc2.weight"] = ((g["hidden"], g["text_hidden"]), True)
    s[t + "text_projection.linear_fc2.bias"] = ((g["hidden"],), False)
    s[t + "codec_head.weight"] = ((g["codec_vocab"], g["hidden"]), True)
    net(t, g["hidden"], g["heads"], g["kv_heads"], g["head_dim"], g["inter"], g["layers"])
    net(c, g["cp_hidden"], g["cp_heads"], g["cp_kv_heads"], g["cp_head_dim"], g["cp_inter"], g["cp_layers"])
    for i in range(15):
        s[c + f"model.codec_embedding.{i}.weight"] = ((g["cp_vocab"], g["cp_embedding_dim"]), False)
        s[c + f"lm_head.{i}.weight"] = ((g["cp_vocab"], g["cp_hidden"]), True)
    if g["cp_embedding_dim"] != g["cp_hidden"]:
        s[c + "small_to_mtp_projection.weight"] = ((g["cp_hidden"], g["cp_embedding_dim"]), True)
        s[c + "small_to_mtp_projection.bias"] = ((g["cp_hidden"],), False)
    return s


def synth_tts_talker_state_dict(geometry=None, seed: int = 0, quantized: bool = True) -> dict:
    """Seeded Talker + code-predictor weights in the checkpoint's form: float tensors bf16, every Linear quantised with
    quantize_linear at geometry["bits"] (quantized=False keeps them bf16: the float checkpoint the loader refuses).  Matrices are
    N(0, 1 / fan_in); the heads' rows carry a log-normal gain, which gives the logits a heavy tail (a clear first maximum, as a
    trained model has, so a greedy run does not hang on bf16-sized ties); norms 1 + 0.1 N, embeddings 0.5 N, biases 0.05 N."""
    g = dict(TTS_TALKER_REAL, **(geometry or {}))
    rng = torch.Generator().manual_seed(424242 + seed)
    sd = {}
    for key, (shape, quant) in tts_talker_tensor_shapes(g).items():
        if key.endswith(".bias"):
            w = 0.05 * torch.randn(shape, generator=rng)
        elif "norm" in key:
            w = 1.0 + 0.1 * torch.randn(shape, generator=rng)
        elif "embedding" in key and not quant:
            w = 0.5 * torch.randn(shape, generator=rng)
        else:
            w = torch.randn(shape, generator=rng) / math.sqrt(shape[1])
            if "head" in key:
                w = 2.0 * w * torch.exp(torch.randn((shape[0], 1), generator=rng))
        w = w.to(torch.bfloat16)
        if quant and quantized:
            stem = key[:-len(".weight")]
            sd[key], sd[stem + ".scales"], sd[stem + ".biases"] = quantize_linear(w, g["bits"])
        else:
            sd[key] = w
    return sd


def write_tts_talker_safetensors(sd: dict, model_dir: str, drop=(), extra=(), scales_dtype: str = "BF16") -> str:
    """Writes `sd` (synth_tts_talker_state_dict) as model_dir/model.safetensors: int32 tensors as U32, bf16 as BF16 (scales / biases as
    `scales_dtype`: BF16 | F32 | F16), float32 as F32.  `drop`: keys left out; `extra`: (key, float array) pairs added as F32 (the main
    checkpoint's other tensors).  Returns model_dir."""
    import json
    import os
    os.makedirs(model_dir, exist_ok=True)
    header, blobs, off = {}, [], 0

    def add(key, dtype, shape, raw):
        nonlocal off
        header[key] = {"dtype": dtype, "shape": list(shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)

    for key in sorted(sd):
        if key in drop:
            continue
        v = sd[key]
        if v.dtype == torch.int32:
            add(key, "U32", v.shape, v.contiguous().numpy().astype("<i4").tobytes())
            continue
        dt = scales_dtype if key.endswith((".scales", ".biases")) else ("BF16" if v.dtype == torch.bfloat16 else "F32")
        f = v.to(torch.float32).contiguous().numpy()
        if dt == "BF16":
            raw = (f.view("<u4") >> 16).astype("<u2").tobytes() if v.dtype == torch.bfloat16 else \
                ((f.view("<u4") + 0x7FFF + ((f.view("<u4") >> 16) & 1)) >> 16).astype("<u2").tobytes()
        elif dt == "F16":
            raw = f.astype("<f2").tobytes()
        else:
            raw = f.astype("<f4").tobytes()
        add(key, dt, v.shape, raw)
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        a = np.asarray(v, dtype=np.float32)
        add(k, "F32", a.shape, a.astype("<f4").tobytes())
    h = json.dumps(header).encode()
    h += b" " * ((8 - len(h) % 8) % 8)
    with open(os.path.join(model_dir, "model.safetensors"), "wb") as fh:
        fh.write(len(h).to_bytes(8, "little"))
        fh.write(h)
        for raw in blobs:
            fh.write(raw)
    return model_dir


# ---- CosyVoice3 flow-matching mel decoder (Sources/CosyVoiceTTS/FlowMatching.swift, DiT.swift; keys: WeightLoading.swift:126-212) ----
FLOW_DIM, FLOW_FF, FLOW_MEL, FLOW_SPK, FLOW_VOCAB = 1024, 2048, 80, 192, 6561


def cosyvoice_flow_tensor_shapes(depth: int = 22, vocab: int = FLOW_VOCAB) -> dict:
    """key -> (shape, quantised) of flow.safetensors before quantisation; a quantised `X.weight` [N, K] is stored as X.weight (packed
    uint32), X.scales, X.biases [N, K / 64], beside X.bias [N]."""
    d = "decoder."
    s = {"input_embedding.weight": ((vocab, FLOW_MEL), False),
         "spk_embed_affine_layer.weight": ((FLOW_MEL, FLOW_SPK), False), "spk_embed_affine_layer.bias": ((FLOW_MEL,), False),
         "pre_lookahead_layer.conv1.weight": ((FLOW_DIM, 4, FLOW_MEL), False), "pre_lookahead_layer.conv1.bias": ((FLOW_DIM,), False),
         "pre_lookahead_layer.conv2.weight": ((FLOW_MEL, 3, FLOW_DIM), False), "pre_lookahead_layer.conv2.bias": ((FLOW_MEL,), False),
         d + "input_embed.conv_pos_embed.conv1.0.weight": ((FLOW_DIM, 31, 64), False), d + "input_embed.conv_pos_embed.conv1.0.bias": ((FLOW_DIM,), False),
         d + "input_embed.conv_pos_embed.conv2.0.weight": ((FLOW_DIM, 31, 64), False), d + "input_embed.conv_pos_embed.conv2.0.bias": ((FLOW_DIM,), False),
         d + "proj_out.weight": ((FLOW_MEL, FLOW_DIM), False), d + "proj_out.bias": ((FLOW_MEL,), False)}
    q = [(d + "time_embed.time_mlp.0", FLOW_DIM, 256), (d + "time_embed.time_mlp.2", FLOW_DIM, FLOW_DIM), (d + "input_embed.proj", FLOW_DIM, 4 * FLOW_MEL),
         (d + "norm_out.linear", 2 * FLOW_DIM, FLOW_DIM)]
    for i in range(depth):
        b = d + f"transformer_blocks.{i}."
        q += [(b + "attn_norm.linear", 6 * FLOW_DIM, FLOW_DIM), (b + "attn.to_q", FLOW_DIM, FLOW_DIM), (b + "attn.to_k", FLOW_DIM, FLOW_DIM),
              (b + "attn.to_v", FLOW_DIM, FLOW_DIM), (b + "attn.to_out.0", FLOW_DIM, FLOW_DIM), (b + "ff.ff.0.0", FLOW_FF, FLOW_DIM),
              (b + "ff.ff.2", FLOW_DIM, FLOW_FF)]
    for stem, n, k in q:
        s[stem + ".weight"] = ((n, k), True)
        s[stem + ".bias"] = ((n,), False)
    return s


def synth_cosyvoice_flow_state_dict(seed: int = 0, depth: int = 22, bits: int = 4, vocab: int = FLOW_VOCAB) -> dict:
    """Seeded flow-decoder weights in the checkpoint's form: every QuantizedLinear quantised with quantize_linear (bf16 scales), the rest
    float32.  Matrices are N(0, g / fan_in).  The AdaLN linears give scale and shift of about 0.3 and gates of 0.4 +- 0.15 with a random
    sign (their bias carries the 0.4), so that every gate is of order 0.1 to 1 and depth blocks move the residual stream without
    letting its RMS leave the decade it starts in (tests/test_flow_cpu.py checks both)."""
    rng = torch.Generator().manual_seed(515151 + seed)
    sd = {}
    for key, (shape, quant) in cosyvoice_flow_tensor_shapes(depth, vocab).items():
        if key.endswith(".bias"):
            w = 0.05 * torch.randn(shape, generator=rng)
            if "attn_norm.linear" in key:                   # chunks 2 and 5 are the gates
                sign = torch.where(torch.rand((2, FLOW_DIM), generator=rng) < 0.5, -1.0, 1.0)
                w[2 * FLOW_DIM:3 * FLOW_DIM] += 0.4 * sign[0]
                w[5 * FLOW_DIM:6 * FLOW_DIM] += 0.4 * sign[1]
        elif key == "input_embedding.weight":
            w = 0.5 * torch.randn(shape, generator=rng)
        elif len(shape) == 3:
            w = torch.randn(shape, generator=rng) * math.sqrt(2.0 / (shape[1] * shape[2]))
        else:
            gain = 0.6 if ("attn_norm" in key or "norm_out" in key) else 2.0 if "time_mlp" in key else 10.0 if key.startswith("spk_embed") else 1.0
            w = torch.randn(shape, generator=rng) * (gain / math.sqrt(shape[1]))
        if quant:
            stem = key[:-len(".weight")]
            sd[key], sd[stem + ".scales"], sd[stem + ".biases"] = quantize_linear(w.to(torch.bfloat16), bits)
        else:
            sd[key] = w
    return sd


def write_cosyvoice_flow_safetensors(sd: dict, model_dir: str, drop=(), reshape=None, extra=(), scales_dtype: str = "BF16") -> str:
    """Writes `sd` as model_dir/flow.safetensors: int32 tensors as U32, scales / biases as `scales_dtype`, the rest F32.  `drop`: keys left
    out; `reshape`: key -> shape the tensor is resized to; `extra`: (key, float array) pairs added as F32.  Returns model_dir."""
    import json
    import os
    os.makedirs(model_dir, exist_ok=True)
    header, blobs, off = {}, [], 0

    def add(key, dtype, shape, raw):
        nonlocal off
        header[key] = {"dtype": dtype, "shape": list(shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)

    for key in sorted(sd):
        if key in drop:
            continue
        v = sd[key]
        if v.dtype == torch.int32:
            a = v.contiguous().numpy().astype("<i4")
            if reshape and key in reshape:
                a = np.resize(a, reshape[key])
            add(key, "U32", a.shape, a.tobytes())
            continue
        f = v.to(torch.float32).contiguous().numpy()
        if reshape and key in reshape:
            f = np.resize(f, reshape[key])
        if key.endswith((".scales", ".biases")) and scales_dtype == "BF16":
            u = f.astype("<f4").view("<u4")
            add(key, "BF16", f.shape, ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype("<u2").tobytes())
        elif key.endswith((".scales", ".biases")) and scales_dtype == "F16":
            add(key, "F16", f.shape, f.astype("<f2").tobytes())
        else:
            add(key, "F32", f.shape, f.astype("<f4").tobytes())
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        a = np.asarray(v, dtype=np.float32)
        add(k, "F32", a.shape, a.astype("<f4").tobytes())
    h = json.dumps(header).encode()
    h += b" " * ((8 - len(h) % 8) % 8)
    with open(os.path.join(model_dir, "flow.safetensors"), "wb") as fh:
        fh.write(len(h).to_bytes(8, "little"))
        fh.write(h)
        for raw in blobs:
            fh.write(raw)
    return model_dir


# ---- CosyVoice3 speech tokenizer, S3-Tokenizer-v3 (Sources/CosyVoiceTTS/SpeechTokenizer.swift; keys: WeightLoading.swift:350-398) ----
S3TOK_DIM, S3TOK_HEADS, S3TOK_FF, S3TOK_MELS, S3TOK_FSQ, S3TOK_FSMN_K = 1280, 20, 5120, 128, 8, 31
S3TOK_REAL2 = dict(depth=2)                # the model's widths (the engine knows no others), 2 blocks
S3TOK_REAL12 = dict(depth=12)


def cosyvoice_s3tok_tensor_shapes(geometry=None) -> dict:
    """key -> shape of speech_tokenizer.safetensors; `key` carries no bias."""
    depth = dict(S3TOK_REAL12, **(geometry or {}))["depth"]
    D = S3TOK_DIM
    s = {"encoder.conv1.weight": (D, 3, S3TOK_MELS), "encoder.conv1.bias": (D,), "encoder.conv2.weight": (D, 3, D), "encoder.conv2.bias": (D,)}
    for i in range(depth):
        b = f"encoder.blocks.{i}."
        for n in ("query", "key", "value", "out"):
            s[b + f"attn.{n}.weight"] = (D, D)
            if n != "key":
                s[b + f"attn.{n}.bias"] = (D,)
        s[b + "attn.fsmn_block.weight"] = (D, S3TOK_FSMN_K, 1)
        for n in ("attn_ln", "mlp_ln"):
            s[b + n + ".weight"], s[b + n + ".bias"] = (D,), (D,)
        s[b + "mlp.0.weight"], s[b + "mlp.0.bias"] = (S3TOK_FF, D), (S3TOK_FF,)
        s[b + "mlp.2.weight"], s[b + "mlp.2.bias"] = (D, S3TOK_FF), (D,)
    s["quantizer._codebook.project_down.weight"], s["quantizer._codebook.project_down.bias"] = (S3TOK_FSQ, D), (S3TOK_FSQ,)
    return s


def synth_s3tok_mel(seed: int, frames: int) -> np.ndarray:
    """A seeded [128, frames] stand-in for a Whisper-style log-mel: N(0, 0.6^2), the range (x + 4) / 4 gives speech."""
    return (0.6 * np.random.default_rng(880000 + seed).standard_normal((S3TOK_MELS, frames))).astype(np.float32)


def _s3tok_hidden_f32(sd: dict, mel: np.ndarray, depth: int) -> torch.Tensor:
    """The encoder in torch float32 on one mel, for the calibration of project_down only (the tests' oracle is tests/s3tok_oracle.py)."""
    F = torch.nn.functional
    t = lambda k: torch.from_numpy(sd[k])
    h = torch.from_numpy(mel)[None]
    for c in ("encoder.conv1", "encoder.conv2"):
        h = F.gelu(F.conv1d(h, t(c + ".weight").permute(0, 2, 1), t(c + ".bias"), stride=2, padding=1))
    h = h[0].T
    T, D, H = h.shape[0], S3TOK_DIM, S3TOK_HEADS
    ang = torch.arange(T, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(32, dtype=torch.float32) / 32.0))[None]
    cs, sn = torch.cos(ang)[:, None], torch.sin(ang)[:, None]

    def rope(x):
        a, b = x.view(T, H, 64)[..., :32], x.view(T, H, 64)[..., 32:]
        return torch.cat([a * cs - b * sn, b * cs + a * sn], -1)

    for i in range(depth):
        p = f"encoder.blocks.{i}."
        x = F.layer_norm(h, (D,), t(p + "attn_ln.weight"), t(p + "attn_ln.bias"), 1e-5)
        q, k = rope(x @ t(p + "attn.query.weight").T + t(p + "attn.query.bias")), rope(x @ t(p + "attn.key.weight").T)
        v = x @ t(p + "attn.value.weight").T + t(p + "attn.value.bias")
        mem = F.conv1d(v.T[None], t(p + "attn.fsmn_block.weight").permute(0, 2, 1), None, padding=15, groups=D)[0].T + v
        a = torch.softmax(torch.einsum("thd,shd->hts", q, k) / 8.0, -1)
        o = torch.einsum("hts,shd->thd", a, v.view(T, H, 64)).reshape(T, D)
        h = h + o @ t(p + "attn.out.weight").T + t(p + "attn.out.bias") + mem
        x = F.layer_norm(h, (D,), t(p + "mlp_ln.weight"), t(p + "mlp_ln.bias"), 1e-5)
        h = h + F.gelu(x @ t(p + "mlp.0.weight").T + t(p + "mlp.0.bias")) @ t(p + "mlp.2.weight").T + t(p + "mlp.2.bias")
    return h


def synth_cosyvoice_s3tok_state_dict(seed: int = 0, geometry=None, bf16_values: bool = False) -> dict:
    """Seeded speech-tokenizer weights {key: float32 array} with the loader's key names.  Matrices and convs are N(0, g / fan_in) (g = 2 in
    front of a GELU), the FSMN taps N(0, 0.5 / 31), LayerNorm weights 1 +- 0.1, biases +- 0.05.  project_down is scaled, and its bias set,
    so that the eight projections of synth_s3tok_mel(0, 256) have zero mean and unit standard deviation: tanh then puts roughly 0.29 / 0.42
    / 0.29 of the digits on the three FSQ levels.  bf16_values: every tensor rounded to bf16 values (a file written as BF16 then holds
    exactly what the oracle reads)."""
    depth = dict(S3TOK_REAL12, **(geometry or {}))["depth"]
    rng = np.random.default_rng(660033 + seed)
    sd = {}
    for key, shape in cosyvoice_s3tok_tensor_shapes(dict(depth=depth)).items():
        if "_ln.weight" in key:
            w = 1.0 + 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif key.endswith(".bias"):
            w = 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif "fsmn_block" in key:
            w = rng.standard_normal(shape, dtype=np.float32) * math.sqrt(0.5 / S3TOK_FSMN_K)
        elif len(shape) == 3:
            w = rng.standard_normal(shape, dtype=np.float32) * math.sqrt(2.0 / (shape[1] * shape[2]))
        else:
            gain = 2.0 if "mlp.0" in key else 0.5 if ("mlp.2" in key or "attn.out" in key) else 1.0
            w = rng.standard_normal(shape, dtype=np.float32) * math.sqrt(gain / shape[1])
        sd[key] = np.ascontiguousarray(w, dtype=np.float32)
    if bf16_values:
        sd = {k: torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy() for k, v in sd.items()}
    with torch.no_grad():
        h = _s3tok_hidden_f32(sd, synth_s3tok_mel(0, 256), depth).numpy().astype(np.float64)
    wk, bk = "quantizer._codebook.project_down.weight", "quantizer._codebook.project_down.bias"
    y = h @ sd[wk].astype(np.float64).T
    sd[wk] = (sd[wk] / y.std(0)[:, None]).astype(np.float32)
    sd[bk] = (-(y.mean(0) / y.std(0))).astype(np.float32)
    if bf16_values:
        for k in (wk, bk):
            sd[k] = torch.from_numpy(sd[k]).to(torch.bfloat16).to(torch.float32).numpy()
    return sd


def write_cosyvoice_s3tok_safetensors(sd: dict, model_dir: str, dtype: str = "F32", drop=(), reshape=None, extra=()) -> str:
    """Writes `sd` as model_dir/speech_tokenizer.safetensors (dtype F32 | F16 | BF16; F64 for the dtype error).  `drop`: keys left out,
    `reshape`: {key: shape} written with a wrong shape, `extra`: (key, array) pairs added as they are.  Returns model_dir."""
    d = dict(sd)
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        d[k] = np.asarray(v, dtype=np.float32)
    _write_safetensors(d, model_dir, dtype, drop, reshape, filename="speech_tokenizer.safetensors")
    return model_dir


# ---- CosyVoice3 speech-token LLM (Sources/CosyVoiceTTS/LLM.swift; keys: WeightLoading.swift:18-110) --------------------------------
CVLM_REAL = dict(hidden=896, layers=24, heads=14, kv_heads=2, head_dim=64, inter=4864, text_vocab=151936, speech_tokens=6561,
                 speech_extra=200, bits=4)


def cosyvoice_llm_tensor_shapes(geometry=None) -> dict:
    """key -> (shape, quantised?) of every tensor of llm.safetensors the loader reads, in the reference's key names.  A quantised
    [out, in] Linear is stored as the triplet weight | scales | biases; `.bias` keys (q, k, v) are float."""
    g = dict(CVLM_REAL, **(geometry or {}))
    H, hd, V = g["hidden"], g["head_dim"], g["speech_tokens"] + g["speech_extra"]
    s = {"text_embedding.weight": ((g["text_vocab"], H), False), "speech_embedding.weight": ((V, H), False)}
    for l in range(g["layers"]):
        q = f"layers.{l}."
        for name, n in (("q_proj", g["heads"] * hd), ("k_proj", g["kv_heads"] * hd), ("v_proj", g["kv_heads"] * hd)):
            s[q + f"self_attn.{name}.weight"] = ((n, H), True)
            s[q + f"self_attn.{name}.bias"] = ((n,), False)
        s[q + "self_attn.o_proj.weight"] = ((H, g["heads"] * hd), True)
        s[q + "input_layernorm.weight"] = ((H,), False)
        s[q + "post_attention_layernorm.weight"] = ((H,), False)
        s[q + "mlp.gate_proj.weight"] = ((g["inter"], H), True)
        s[q + "mlp.up_proj.weight"] = ((g["inter"], H), True)
        s[q + "mlp.down_proj.weight"] = ((H, g["inter"]), True)
    s["norm.weight"] = ((H,), False)
    s["speech_head.weight"] = ((V, H), True)
    return s


def synth_cosyvoice_llm_state_dict(geometry=None, seed: int = 0, quantized: bool = True) -> dict:
    """Seeded LLM weights in the checkpoint's form: float tensors bf16, every Linear quantised with quantize_linear at
    geometry["bits"] (quantized=False keeps them bf16: the float checkpoint the loader refuses).  Matrices are N(0, 1 / fan_in); the
    head's rows carry a log-normal gain, which gives the logits a heavy tail (a clear first maximum, as a trained model has); norms
    1 + 0.1 N, embeddings 0.5 N, biases 0.05 N."""
    g = dict(CVLM_REAL, **(geometry or {}))
    rng = torch.Generator().manual_seed(636363 + seed)
    sd = {}
    for key, (shape, quant) in cosyvoice_llm_tensor_shapes(g).items():
        if key.endswith(".bias"):
            w = 0.05 * torch.randn(shape, generator=rng)
        elif "norm" in key:
            w = 1.0 + 0.1 * torch.randn(shape, generator=rng)
        elif "embedding" in key:
            w = 0.5 * torch.randn(shape, generator=rng)
        else:
            w = torch.randn(shape, generator=rng) / math.sqrt(shape[1])
            if "head" in key:
                w = 2.0 * w * torch.exp(torch.randn((shape[0], 1), generator=rng))
        w = w.to(torch.bfloat16)
        if quant and quantized:
            stem = key[:-len(".weight")]
            sd[key], sd[stem + ".scales"], sd[stem + ".biases"] = quantize_linear(w, g["bits"])
        else:
            sd[key] = w
    return sd


def write_cosyvoice_llm_safetensors(sd: dict, model_dir: str, drop=(), extra=(), scales_dtype: str = "BF16", reshape=None) -> str:
    """Writes `sd` (synth_cosyvoice_llm_state_dict) as model_dir/llm.safetensors in the Talker writer's dtypes.  `drop`: keys left out;
    `extra`: (key, float array) pairs added as F32; `reshape`: key -> shape the tensor is resized to.  Returns model_dir."""
    import os
    import tempfile
    if reshape:
        sd = dict(sd)
        for k, shp in reshape.items():
            v = sd[k]
            sd[k] = torch.from_numpy(np.resize(v.to(torch.float32).numpy() if v.dtype != torch.int32 else v.numpy(), shp)).to(v.dtype)
    with tempfile.TemporaryDirectory() as tmp:
        write_tts_talker_safetensors(sd, tmp, drop=drop, extra=extra, scales_dtype=scales_dtype)
        os.makedirs(model_dir, exist_ok=True)
        os.replace(os.path.join(tmp, "model.safetensors"), os.path.join(model_dir, "llm.safetensors"))
    return model_dir


# ---- VoxCPM2 AudioVAE (qasr_avae_*) -------------------------------------------------------------------------------------------
VOXCPM2_AUDIOVAE_REAL = {"encoder_dim": 128, "encoder_rates": [2, 5, 8, 8], "latent_dim": 64, "decoder_dim": 2048,
                         "decoder_rates": [8, 6, 5, 2, 2, 2], "sr_bin_boundaries": [20000, 30000, 40000]}


def voxcpm2_audiovae_tensor_shapes(geom: dict) -> dict:
    """key -> shape of every AudioVAE tensor as the reference's modules hold them (AudioVAE.swift; conv weights [out, k, in / groups],
    alphas [1, 1, C], condition tables [buckets, C]), under the audio_vae. prefix."""
    s = {}

    def conv(k, out, kk, cin):
        s[k + ".weight"], s[k + ".bias"] = (out, kk, cin), (out,)

    def unit(p, C):
        s[p + ".snake1.alpha"], s[p + ".snake2.alpha"] = (1, 1, C), (1, 1, C)
        conv(p + ".conv1", C, 7, 1)
        conv(p + ".conv2", C, 1, C)

    conv("audio_vae.encoder.conv_in", geom["encoder_dim"], 7, 1)
    C = geom["encoder_dim"]
    for i, r in enumerate(geom["encoder_rates"]):
        p = f"audio_vae.encoder.blocks.layers.{i}"
        for u in (1, 2, 3):
            unit(f"{p}.res{u}", C)
        s[p + ".snake.alpha"] = (1, 1, C)
        conv(p + ".conv", 2 * C, 2 * r, C)
        C *= 2
    conv("audio_vae.encoder.fc_mu", geom["latent_dim"], 3, C)
    conv("audio_vae.decoder.conv_in.layers.0", geom["latent_dim"], 7, 1)
    conv("audio_vae.decoder.conv_in.layers.1", geom["decoder_dim"], 1, geom["latent_dim"])
    C, buckets = geom["decoder_dim"], len(geom["sr_bin_boundaries"]) + 1
    for i, r in enumerate(geom["decoder_rates"]):
        p, q = f"audio_vae.decoder.blocks.layers.{i}", f"audio_vae.decoder.sr_cond_layers.{i}"
        s[q + ".scale_embed.weight"], s[q + ".bias_embed.weight"] = (buckets, C), (buckets, C)
        s[p + ".snake.alpha"] = (1, 1, C)
        conv(p + ".conv_t", C // 2, 2 * r, C)
        for u in (1, 2, 3):
            unit(f"{p}.res{u}", C // 2)
        C //= 2
    s["audio_vae.decoder.snake_out.alpha"] = (1, 1, C)
    conv("audio_vae.decoder.conv_out", 1, 7, C)
    return s


def synth_voxcpm2_audiovae_state_dict(geom: dict, seed: int = 0, weight_norm: bool = True, prefixed: bool = True) -> dict:
    """Seeded AudioVAE weights {key: float32 array} as a checkpoint stores them.  Convs are N(0, gain^2 / fan_in): 1 for the convs that
    change the rate and the two conv_in, 0.6 for a unit's depthwise conv and 0.5 for its 1x1, so that the 12 / 18 units in a row leave the
    signal O(1); conv_out 0.6 keeps tanh off its rails.  Snake alphas are log-normal around 1 (drawn positive, 0.4 .. 2.5 in practice); the
    condition tables are 1 + 0.2 N and 0.2 N, a different row per sample-rate bucket.  weight_norm: every second conv weight (in key
    order) is stored as a weight_g [out, 1, 1] / weight_v pair whose fusion is that weight up to rounding; 64-wide condition tables are
    stored [n, 8, 8]; fc_logvar tensors holding 1e3 are added (the loader drops them).  prefixed False: keys start at encoder. /
    decoder., which AudioVAE.sanitize completes."""
    rng, split = np.random.default_rng(77003 + seed), np.random.default_rng(77103 + seed)     # the split draws leave the weights' stream alone
    sd, nth = {}, 0
    for key, shape in voxcpm2_audiovae_tensor_shapes(geom).items():
        if key.endswith(".alpha"):
            v = np.exp(0.35 * rng.standard_normal(shape))
        elif key.endswith("scale_embed.weight"):
            v = 1.0 + 0.2 * rng.standard_normal(shape)
        elif key.endswith("bias_embed.weight"):
            v = 0.2 * rng.standard_normal(shape)
        elif key.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        else:
            fan = shape[1] * shape[2]
            gain = 0.6 if ".conv1." in key or "conv_out" in key else 0.5 if ".conv2." in key else 1.0
            v = gain * rng.standard_normal(shape) / math.sqrt(fan)
        v = np.ascontiguousarray(v, dtype=np.float32)
        if key.endswith("_embed.weight") and shape[1] == 64 and weight_norm:
            v = v.reshape(shape[0], 8, 8)
        if key.endswith(".weight") and len(shape) == 3 and weight_norm:
            nth += 1
            if nth % 2 == 0:
                s = np.exp(0.5 * split.standard_normal((shape[0], 1, 1))).astype(np.float32)
                vv = (v / s).astype(np.float32)
                g = np.sqrt((vv.astype(np.float64).reshape(shape[0], -1) ** 2).sum(axis=1)).reshape(shape[0], 1, 1) * s
                sd[key + "_v"], sd[key + "_g"] = vv, g.astype(np.float32)
                continue
        sd[key] = v
    if weight_norm:
        C = geom["encoder_dim"] << len(geom["encoder_rates"])
        sd["audio_vae.encoder.fc_logvar.weight"] = np.full((geom["latent_dim"], 3, C), 1e3, dtype=np.float32)
        sd["audio_vae.encoder.fc_logvar.bias"] = np.full((geom["latent_dim"],), 1e3, dtype=np.float32)
    if not prefixed:
        sd = {k[len("audio_vae."):]: v for k, v in sd.items()}
    return sd


def write_voxcpm2_audiovae_safetensors(sd: dict, model_dir: str, geom=None, dtype: str = "F32", drop=(), reshape=None, extra=(),
                                       config_extra=None) -> str:
    """Writes `sd` as model_dir/model.safetensors and, for a geometry given, model_dir/config.json with it (and config_extra's fields)
    under "audio_vae_config".  `drop` / `reshape` / `extra`: as write_cosyvoice_hifigan_safetensors.  Returns model_dir."""
    import json
    import os
    d = dict(sd)
    for k, v in (extra.items() if isinstance(extra, dict) else extra):
        d[k] = np.asarray(v, dtype=np.float32)
    _write_safetensors(d, model_dir, dtype, drop, reshape)
    if geom is not None or config_extra:
        cfg = dict(geom or {})
        cfg.update(config_extra or {})
        with open(os.path.join(model_dir, "config.json"), "w") as f:
            json.dump({"architecture": "voxcpm2", "audio_vae_config": cfg}, f)
    return model_dir


# ---- VoxCPM2 local networks (qasr_vloc_*) -------------------------------------------------------------------------------------
# A geometry: {"enc": {hidden_dim, ffn_dim, num_heads, num_layers, kv_channels}, "dit": {...}, "lm": {hidden_size, num_key_value_heads,
# use_mup, scale_depth, rms_norm_eps, rope_theta, max_position_embeddings, rope_scaling}, "patch_size", "feat_dim", "mu_tokens"}.
VLOC_REAL = {
    "enc": {"hidden_dim": 1024, "ffn_dim": 4096, "num_heads": 16, "num_layers": 12, "kv_channels": 128},
    "dit": {"hidden_dim": 1024, "ffn_dim": 4096, "num_heads": 16, "num_layers": 12, "kv_channels": 128},
    "lm": {"hidden_size": 2048, "num_key_value_heads": 2, "use_mup": False, "scale_depth": 1.4, "rms_norm_eps": 1e-5, "rope_theta": 10000.0,
           "max_position_embeddings": 32768},
    "patch_size": 4, "feat_dim": 64, "mu_tokens": 2,
}


def voxcpm2_local_geometry(depth=None, **over) -> dict:
    """VLOC_REAL with both stacks at `depth` layers and top-level or "lm." / "enc." / "dit." fields replaced (e.g. lm__use_mup=True)."""
    import copy
    g = copy.deepcopy(VLOC_REAL)
    if depth is not None:
        g["enc"]["num_layers"] = g["dit"]["num_layers"] = int(depth)
    for k, v in over.items():
        if "__" in k:
            part, field = k.split("__", 1)
            g[part][field] = v
        else:
            g[k] = v
    return g


def voxcpm2_local_tensor_shapes(geom: dict) -> dict:
    """key -> shape of every tensor qasr_vloc_create reads (VoxCPM2TTS.swift:383-440)."""
    s = {}
    F, L = geom["feat_dim"], geom["lm"]["hidden_size"]
    kv = geom["lm"]["num_key_value_heads"]

    def lin(k, out, inn):
        s[k + ".weight"], s[k + ".bias"] = (out, inn), (out,)

    def stack(p, g):
        H, hd = g["hidden_dim"], g["kv_channels"]
        for l in range(g["num_layers"]):
            q = f"{p}.layers.{l}"
            s[q + ".self_attn.q_proj.weight"] = (g["num_heads"] * hd, H)
            s[q + ".self_attn.k_proj.weight"] = (kv * hd, H)
            s[q + ".self_attn.v_proj.weight"] = (kv * hd, H)
            s[q + ".self_attn.o_proj.weight"] = (H, g["num_heads"] * hd)
            s[q + ".mlp.gate_proj.weight"] = (g["ffn_dim"], H)
            s[q + ".mlp.up_proj.weight"] = (g["ffn_dim"], H)
            s[q + ".mlp.down_proj.weight"] = (H, g["ffn_dim"])
            s[q + ".input_layernorm.weight"] = (H,)
            s[q + ".post_attention_layernorm.weight"] = (H,)
        s[p + ".norm.weight"] = (H,)

    He, Hd = geom["enc"]["hidden_dim"], geom["dit"]["hidden_dim"]
    s["feat_encoder.special_token"] = (1, 1, 1, He)
    lin("feat_encoder.in_proj", He, F)
    stack("feat_encoder.encoder", geom["enc"])
    for k in ("in_proj", "cond_proj"):
        lin("feat_decoder.estimator." + k, Hd, F)
    lin("feat_decoder.estimator.out_proj", F, Hd)
    for m in ("time_mlp", "delta_time_mlp"):
        for l in ("linear_1", "linear_2"):
            lin(f"feat_decoder.estimator.{m}.{l}", Hd, Hd)
    stack("feat_decoder.estimator.decoder", geom["dit"])
    lin("enc_to_lm_proj", L, He)
    mu_rows = geom["mu_tokens"] * Hd
    lin("lm_to_dit_proj", mu_rows - mu_rows // 2, L)
    lin("res_to_dit_proj", mu_rows // 2, L)
    return s


def bf16_values(a: np.ndarray) -> np.ndarray:
    """a rounded to the nearest bfloat16 (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def synth_voxcpm2_local_state_dict(geom: dict, seed: int = 0) -> dict:
    """Seeded weights holding bfloat16 values: matrices N(0, 1 / K) so activations stay O(1), norm weights near 1, biases and the special
    token O(0.1 .. 1)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in voxcpm2_local_tensor_shapes(geom).items():
        if key.endswith("norm.weight") or key.endswith("layernorm.weight"):
            v = 1.0 + 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif key.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape, dtype=np.float32)
        elif key.endswith("special_token"):
            v = rng.standard_normal(shape, dtype=np.float32)
        else:
            v = rng.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / math.sqrt(shape[-1]))
        sd[key] = bf16_values(v)
    return sd


def voxcpm2_local_config(geom: dict) -> dict:
    """The config.json of a geometry."""
    cfg = {"architecture": "voxcpm2", "lm_config": dict(geom["lm"]), "encoder_config": dict(geom["enc"]), "dit_config": dict(geom["dit"]),
           "patch_size": geom["patch_size"], "feat_dim": geom["feat_dim"]}
    return cfg


def write_voxcpm2_local_safetensors(sd: dict, model_dir: str, geom=None, dtype: str = "BF16", drop=(), reshape=None, config=None) -> str:
    """Writes `sd` as model_dir/model.safetensors and, for a geometry (or a whole config dict) given, model_dir/config.json.  `drop` /
    `reshape`: as write_silero_safetensors.  Returns model_dir."""
    import json
    import os
    _write_safetensors(sd, model_dir, dtype, drop, reshape)
    if geom is not None or config is not None:
        with open(os.path.join(model_dir, "config.json"), "w") as f:
            json.dump(config if config is not None else voxcpm2_local_config(geom), f)
    return model_dir


def quantize_voxcpm2_local_state_dict(sd: dict, bits: int) -> dict:
    """The MLX 4-bit / 8-bit form of a VoxCPM2 local-network state dict: every Linear weight [out, in] becomes the triplet {weight: packed
    uint32 words (as int32), scales, biases} of quantize_linear with bfloat16 scales (group 64); vectors, and a Linear whose input width is
    no multiple of 64, stay float.  torch tensors."""
    out = {}
    for k, v in sd.items():
        a = np.asarray(v)
        if k.endswith(".weight") and a.ndim == 2 and a.shape[1] % QUANT_GROUP == 0:
            stem = k[:-len(".weight")]
            out[k], out[stem + ".scales"], out[stem + ".biases"] = quantize_linear(torch.from_numpy(a).to(torch.bfloat16), bits)
        else:
            out[k] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return out


def write_voxcpm2_local_quantized_safetensors(qsd: dict, model_dir: str, geom: dict, bits: int, drop=(), reshape=None) -> str:
    """Writes a quantize_voxcpm2_local_state_dict result as model_dir/model.safetensors (U32 words, BF16 scales / biases, F32 vectors) with
    the geometry's config.json and its "quantization" entry.  Returns model_dir."""
    import json
    import os
    write_cosyvoice_flow_safetensors(qsd, model_dir, drop=drop, reshape=reshape)
    os.replace(os.path.join(model_dir, "flow.safetensors"), os.path.join(model_dir, "model.safetensors"))
    cfg = voxcpm2_local_config(geom)
    cfg["quantization"] = {"bits": int(bits), "group_size": QUANT_GROUP}
    with open(os.path.join(model_dir, "config.json"), "w") as f:
        json.dump(cfg, f)
    return model_dir

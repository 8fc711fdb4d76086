"""The Qwen3-TTS speech tokenizer decoder without a GPU: the float64 oracle (tests/codec_oracle.py) against an independent torch
composition, the RoPE convention, chunkedDecode's window table (also through the built library), the observability of the chunking,
the clip condition, the f32 distances that set the GPU bounds, and the host-side argument errors of the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codec_oracle as O
from qasr import synth, _lib

G = O.REDUCED
# the inputs of tests/test_gpu_codec.py on the reduced geometry (seed = T); the real geometry's are listed at their test below
STAGE_T = (1, 2, 11, 35)
DECODE_T = (35, 36, 61)
BATCH_T = (1, 36, 7, 61, 35)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_speech_tokenizer_state_dict(0, G)


@pytest.fixture(scope="module")
def W(sd):
    return O.Weights(sd)


def peak_rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


# ---- an independent torch float64 composition -----------------------------------------------------------------------------------------
def t_(W, k):
    return torch.from_numpy(np.ascontiguousarray(W[k]))


def t_conv(x, W, p, dilation=1, groups=1):
    w = t_(W, p + ".weight")
    return F.conv1d(F.pad(x, ((w.shape[2] - 1) * dilation, 0)), w, t_(W, p + ".bias"), dilation=dilation, groups=groups)


def t_tconv(x, W, p, stride):
    w = t_(W, p + ".weight")
    y = F.conv_transpose1d(x, w, t_(W, p + ".bias"), stride=stride)
    return y[..., :y.shape[-1] - (w.shape[2] - stride)]


def t_snake(x, W, p):
    a, b = t_(W, p + ".alpha")[None, :, None], t_(W, p + ".beta")[None, :, None]
    return x + torch.exp(-b) * torch.sin(torch.exp(a) * x) ** 2


def t_rvq(codes, W, g):
    def cb(p):
        if p + ".embed" in W:
            return t_(W, p + ".embed")
        return t_(W, p + ".embedding_sum") / t_(W, p + ".cluster_usage").clamp(min=1e-7)[:, None]
    c = torch.from_numpy(np.asarray(codes)).long()
    first = F.embedding(c[0], cb("decoder.quantizer.rvq_first.vq.layers.0._codebook"))
    rest = sum(F.embedding(c[1 + i], cb("decoder.quantizer.rvq_rest.vq.layers.%d._codebook" % i)) for i in range(g["num_quantizers"] - 1))
    return (F.conv1d(first.T[None], t_(W, "decoder.quantizer.rvq_first.output_proj.weight"))
            + F.conv1d(rest.T[None], t_(W, "decoder.quantizer.rvq_rest.output_proj.weight")))      # [1, H, T]


def t_rope(x):                                             # [heads, T, 64], rotate-halves
    T, D = x.shape[1], x.shape[2]
    inv = 10000.0 ** (-torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    rot = torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    return x * cos + rot * sin


def t_pre_transformer(x, W, g):                             # x [T, L]
    P = "decoder.pre_transformer."
    nh, hd, eps = g["num_heads"], g["head_dim"], g["rms_norm_eps"]
    rms = lambda v, k: v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * t_(W, k)
    h = F.linear(x, t_(W, P + "input_proj.weight"), t_(W, P + "input_proj.bias"))
    T = h.shape[0]
    for l in range(g["num_layers"]):
        L = P + "layers.%d." % l
        n = rms(h, L + "input_layernorm.weight")
        q, k, v = (F.linear(n, t_(W, L + "self_attn.%s_proj.weight" % s)).view(T, nh, hd).transpose(0, 1) for s in "qkv")
        a = F.scaled_dot_product_attention(t_rope(q)[None], t_rope(k)[None], v[None], is_causal=True)[0]
        a = F.linear(a.transpose(0, 1).reshape(T, nh * hd), t_(W, L + "self_attn.o_proj.weight"))
        h = h + a * t_(W, L + "self_attn_layer_scale.scale")
        n = rms(h, L + "post_attention_layernorm.weight")
        m = F.linear(F.silu(F.linear(n, t_(W, L + "mlp.gate_proj.weight"))) * F.linear(n, t_(W, L + "mlp.up_proj.weight")),
                     t_(W, L + "mlp.down_proj.weight"))
        h = h + m * t_(W, L + "mlp_layer_scale.scale")
    return F.linear(rms(h, P + "norm.weight"), t_(W, P + "output_proj.weight"), t_(W, P + "output_proj.bias"))


def t_upsample(x, W, g):                                    # x [1, L, T]
    for s, ratio in enumerate(g["upsampling_ratios"]):
        p = "decoder.upsample.%d" % s
        x = t_tconv(x, W, p + ".0.conv", ratio)
        h = t_conv(x, W, p + ".1.dwconv.conv", groups=x.shape[1]).transpose(1, 2)
        h = F.layer_norm(h, (h.shape[-1],), t_(W, p + ".1.norm.weight"), t_(W, p + ".1.norm.bias"), 1e-5)
        h = F.linear(F.gelu(F.linear(h, t_(W, p + ".1.pwconv1.weight"), t_(W, p + ".1.pwconv1.bias"))),
                     t_(W, p + ".1.pwconv2.weight"), t_(W, p + ".1.pwconv2.bias"))
        x = x + (h * t_(W, p + ".1.gamma")).transpose(1, 2)
    return x


def t_vocoder(x, W, g):                                     # x [1, L, 4 T] -> [1920 T], before the clip
    h = t_conv(x, W, "decoder.decoder.0.conv")
    for i, s in enumerate(g["upsample_rates"]):
        p = "decoder.decoder.%d.block" % (i + 1)
        h = t_tconv(t_snake(h, W, p + ".0"), W, p + ".1.conv", s)
        for j, d in enumerate((1, 3, 9)):
            u = p + ".%d" % (j + 2)
            r = t_conv(t_snake(h, W, u + ".act1"), W, u + ".conv1.conv", dilation=d)
            h = h + t_conv(t_snake(r, W, u + ".act2"), W, u + ".conv2.conv")
    return t_conv(t_snake(h, W, "decoder.decoder.5"), W, "decoder.decoder.6.conv")[0, 0]


@pytest.mark.parametrize("T", [1, 2, 11, 35])
def test_oracle_matches_torch(W, T):
    """Stage by stage, each fed the oracle's own input, to 1e-9 of the stage's peak."""
    codes = O.make_codes(T, T, G)
    with torch.no_grad():
        q = O.quantizer_decode(codes, W, G)
        assert peak_rel(t_rvq(codes, W, G)[0].T.numpy(), q) < 1e-9
        x = O.pre_conv(q, W)
        assert peak_rel(t_conv(torch.from_numpy(q).T[None], W, "decoder.pre_conv.conv")[0].T.numpy(), x) < 1e-9
        p = O.pre_transformer(x, W, G)
        assert peak_rel(t_pre_transformer(torch.from_numpy(x), W, G).numpy(), p) < 1e-9
        u = O.upsample(p, W, G)
        assert u.shape == (4 * T, G["latent_dim"])
        assert peak_rel(t_upsample(torch.from_numpy(p).T[None], W, G)[0].T.numpy(), u) < 1e-9
        y = O.vocoder(u, W, G, clip=False)
        assert y.shape == (1920 * T,)
        assert peak_rel(t_vocoder(torch.from_numpy(u).T[None].contiguous(), W, G).numpy(), y) < 1e-9
    assert np.array_equal(O.forward(codes, W, G, clip=False), y)
    assert np.array_equal(O.forward(codes, W, G), np.clip(y, -1, 1))


def test_rope_convention():
    """Rotate-halves, written out by hand for one head; the interleaved form is something else."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 1, 64))
    want = np.empty_like(x)
    for t in range(7):
        for i in range(32):
            th = t * 10000.0 ** (-2.0 * i / 64.0)
            a, b = x[t, 0, i], x[t, 0, i + 32]
            want[t, 0, i] = a * math.cos(th) - b * math.sin(th)
            want[t, 0, i + 32] = a * math.sin(th) + b * math.cos(th)
    assert np.abs(O.rope(x) - want).max() < 1e-12
    assert np.abs(O.rope_interleaved(x) - want).max() > 0.1
    assert np.array_equal(O.rope(x)[0], x[0])                                       # position 0 is the identity


def swift_windows(T, chunk=25, left=10):
    """SpeechTokenizerDecoder.chunkedDecode's loop (SpeechTokenizerDecoder.swift:696-733), transcribed line by line."""
    if T <= chunk + left:
        return [(0, 0, T)]
    out = []
    offset = 0
    while offset < T:
        chunk_end = min(offset + chunk, T)
        context_start = max(offset - left, 0)
        actual_context = offset - context_start
        out.append((context_start, actual_context, chunk_end))
        offset = chunk_end
    return out


KNOWN_WINDOWS = {1: [(0, 0, 1)], 35: [(0, 0, 35)], 36: [(0, 0, 25), (15, 10, 36)], 50: [(0, 0, 25), (15, 10, 50)],
                 60: [(0, 0, 25), (15, 10, 50), (40, 10, 60)], 61: [(0, 0, 25), (15, 10, 50), (40, 10, 61)]}


@pytest.mark.parametrize("T", [1, 35, 36, 50, 60, 61, 375])
def test_window_positions(T):
    """The oracle's table, the Swift loop and qasr_codec_window_positions of the built library agree (no GPU involved)."""
    want = swift_windows(T)
    if T in KNOWN_WINDOWS:
        assert want == KNOWN_WINDOWS[T]
    assert len(want) == (1 if T <= 35 else -(-T // 25)) and want[-1][2] == T
    assert sum(e - s - c for s, c, e in want) == T and all(e - s <= 35 for s, c, e in want)
    assert O.window_positions(T) == want
    from qasr import codec
    assert codec.window_positions(T) == want


def test_chunking_is_observable(W):
    """decode equals forward up to 35 frames and differs from an un-chunked pass at 36: the context cut can be seen."""
    for T in (1, 35):
        c = O.make_codes(T, T, G)
        assert np.array_equal(O.decode(c, W, G), O.forward(c, W, G))
    c = O.make_codes(36, 36, G)
    chunked, whole = O.decode(c, W, G, clip=False), O.forward(c, W, G, clip=False)
    assert chunked.shape == whole.shape == (1920 * 36,)
    assert np.abs(chunked[:1920 * 25] - whole[:1920 * 25]).max() < 1e-12 * np.abs(whole).max()      # the first window is causal and complete
    d = float(np.abs(chunked[1920 * 25:] - whole[1920 * 25:]).max() / np.abs(whole).max())
    print("chunked vs un-chunked at T = 36: %.2e of peak" % d)
    assert d > 1e-3


def gpu_inputs():
    return [O.make_codes(T, T, G) for T in sorted(set(STAGE_T + DECODE_T + BATCH_T))]


def test_preclip_inside_unit_interval(W):
    """The clip must not hide a failure: at least 99 % of the oracle's pre-clip samples lie inside (-1, 1) on every GPU test input."""
    for c in gpu_inputs():
        y = O.decode(c, W, G, clip=False)
        inside = float((np.abs(y) < 1.0).mean())
        print("T = %d: %.4f of the pre-clip samples inside (-1, 1), peak %.2f" % (c.shape[1], inside, np.abs(y).max()))
        assert inside >= 0.99


def test_f32_distance(sd, W):
    """max |f32 twin - float64| / peak per stage on the GPU tests' inputs: the figures tests/test_gpu_codec.py's bounds are 10 x of."""
    W32 = O.Weights(sd, np.float32)
    worst = dict(rvq=0.0, pre_transformer=0.0, forward=0.0, decode=0.0)
    for c in gpu_inputs():
        T = c.shape[1]
        if T <= 35:
            q = O.quantizer_decode(c, W, G)
            worst["rvq"] = max(worst["rvq"], peak_rel(O.quantizer_decode(c, W32, G), q))
            x = O.pre_conv(q, W).astype(np.float32)
            worst["pre_transformer"] = max(worst["pre_transformer"],
                                           peak_rel(O.pre_transformer(x, W32, G), O.pre_transformer(x.astype(np.float64), W, G)))
            y32 = O.forward(c, W32, G, clip=False)
            assert y32.dtype == np.float32
            worst["forward"] = max(worst["forward"], peak_rel(y32, O.forward(c, W, G, clip=False)))
        worst["decode"] = max(worst["decode"], peak_rel(O.decode(c, W32, G), O.decode(c, W, G)))
    print("f32 twin vs float64 oracle, reduced geometry, of peak: " + ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert 0 < worst["rvq"] < 1e-5 and 0 < worst["pre_transformer"] < 1e-4 and 0 < worst["forward"] < 1e-3 and 0 < worst["decode"] < 1e-3


REAL_FORWARD = [(100 + T, T) for T in (1, 3, 35)]        # (seed, T) of tests/test_gpu_codec.py's real-geometry inputs, weights seed 1
REAL_PRE_TRANSFORMER, REAL_DECODE = (135, 35), (136, 36)


def test_real_geometry_preclip_and_f32_distance():
    """The two tests above on the real geometry's GPU inputs: the clip condition, and the f32 twin's distances behind the real_* bounds
    of tests/test_gpu_codec.py (forward before the clip, decode after it, as the GPU tests compare them)."""
    R = O.REAL
    sd = synth.synth_speech_tokenizer_state_dict(1, R)
    W, W32 = O.Weights(sd), O.Weights(sd, np.float32)
    del sd
    worst = dict(forward=0.0, pre_transformer=0.0, decode=0.0)

    def inside(y, what):
        frac = float((np.abs(y) < 1.0).mean())
        print("real %s: %.4f of the pre-clip samples inside (-1, 1), peak %.2f" % (what, frac, np.abs(y).max()))
        assert frac >= 0.99

    for seed, T in REAL_FORWARD:
        c = O.make_codes(seed, T, R)
        y = O.forward(c, W, R, clip=False)
        inside(y, "forward T = %d" % T)
        worst["forward"] = max(worst["forward"], peak_rel(O.forward(c, W32, R, clip=False), y))
    c = O.make_codes(*REAL_PRE_TRANSFORMER, R)
    x = O.pre_conv(O.quantizer_decode(c, W, R), W).astype(np.float32)
    worst["pre_transformer"] = peak_rel(O.pre_transformer(x, W32, R), O.pre_transformer(x.astype(np.float64), W, R))
    c = O.make_codes(*REAL_DECODE, R)
    y = O.decode(c, W, R, clip=False)
    inside(y, "decode T = %d" % c.shape[1])
    worst["decode"] = peak_rel(np.clip(O.decode(c, W32, R, clip=False), -1, 1), np.clip(y, -1, 1))
    print("f32 twin vs float64 oracle, real geometry, of peak: " + ", ".join("%s %.2e" % kv for kv in worst.items()))
    assert 0 < worst["forward"] < 1e-3 and 0 < worst["pre_transformer"] < 1e-4 and 0 < worst["decode"] < 1e-3


def test_geometry_must_give_1920_samples_per_frame(tmp_path):
    """Every output buffer of the C ABI is [1920 T]: a config.json whose rates multiply to anything else is refused at create, before
    the weights are opened and before any device call."""
    import json
    lib = _lib.load(strict=True)
    h = C.c_void_p()
    for rates, ratios, product in (((8, 5, 4, 4), (2, 2), 2560), ((8, 5, 4, 3), (2, 1), 960)):
        d = tmp_path / ("g%d" % product)
        d.mkdir()
        (d / "config.json").write_text(json.dumps({"decoder_config": dict(O.REDUCED, upsample_rates=rates, upsampling_ratios=ratios)}))
        assert lib.qasr_codec_create(0, str(d).encode(), 0, None, C.byref(h)) == 1 and not h.value
        msg = lib.qasr_codec_last_error(None).decode()
        assert str(product) in msg and "1920" in msg
    d = tmp_path / "ok"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"decoder_config": dict(O.REDUCED, upsample_rates=(4, 5, 8, 3), upsampling_ratios=(4, 1))}))
    assert lib.qasr_codec_create(0, str(d).encode(), 0, None, C.byref(h)) == 4                      # geometry accepted; no weights there
    assert "model.safetensors" in lib.qasr_codec_last_error(None).decode()


def test_host_argument_errors():
    """What the C ABI refuses without a device: no frames, a table too small, a null handle."""
    lib = _lib.load(strict=True)
    s, c, e = ((C.c_int32 * 4)() for _ in range(3))
    assert lib.qasr_codec_window_positions(0, s, c, e, 4) == -1
    assert lib.qasr_codec_window_positions(375, s, c, e, 4) == -5 and list(s) == [0, 0, 0, 0]
    assert lib.qasr_codec_window_positions(61, s, c, e, 4) == 3
    assert lib.qasr_codec_window_positions(61, None, None, None, 4) == 3
    assert lib.qasr_codec_sample_rate() == 24000 and lib.qasr_codec_samples_per_frame() == 1920
    codes = np.zeros((16, 4), np.int32)
    out = np.zeros(4 * 1920, np.float32)
    ip, fp = codes.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.qasr_codec_forward(None, ip, 1, 4, 1, fp) == 1 and lib.qasr_codec_decode(None, ip, 4, fp) == 1
    assert lib.qasr_codec_num_quantizers(None) == 0 and lib.qasr_codec_memory_footprint(None) == 0 and lib.qasr_codec_is_loaded(None) == 0
    h = C.c_void_p()
    assert lib.qasr_codec_create(0, None, 0, None, C.byref(h)) == 1 and b"model_dir" in lib.qasr_codec_last_error(None)
    assert lib.qasr_codec_create(0, b"/nonexistent-model-dir", 9999, None, C.byref(h)) == 1 and b"max_windows" in lib.qasr_codec_last_error(None)
    assert lib.qasr_codec_create(0, b"/nonexistent-model-dir", 0, None, C.byref(h)) == 4 and not h.value

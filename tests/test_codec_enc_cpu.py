"""CPU checks of the Qwen3-TTS speech tokenizer encoder's oracle (tests/codec_enc_oracle.py) and of the host side of qasr_codec_enc_*.

The float64 oracle is checked stage by stage against a torch f32 twin written independently of it (F.conv1d with stride and left pad,
F.scaled_dot_product_attention without a mask, the expanded distance form).  test_f32_distance measures, on the exact inputs of
tests/test_gpu_codec_enc.py, the twin's distance from the oracle; those figures are that file's F32 table, and each GPU bound is 10 x
its figure.  Measured here (max |d| / peak):
    reduced geometry, n = 1, 1920, 1921, 1920 x 37 + 517, 1920 x 97: conv 1.23e-06, latent 1.03e-06
    real geometry, n = 1920 x 3, 1920 x 33 + 7:                       conv 1.44e-06, latent 1.33e-06
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import codec_enc_oracle as O
from qasr import synth, _lib

G, R = O.REDUCED, O.REAL
LENGTHS = (1, 1920, 1921, 1920 * 37 + 517, 1920 * 97)
REAL_LENGTHS = (1920 * 3, 1920 * 33 + 7)


# ---- the torch f32 twin -------------------------------------------------------------------------------------------------------------
class Twin:
    def __init__(self, sd, g):
        self.w = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
        self.g = g

    def cconv(self, x, key, stride=1, dilation=1, groups=1):
        """x [T, C]: left pad (k - 1) dilation, then F.conv1d."""
        w = self.w[key + ".weight"]
        y = F.conv1d(F.pad(x.T[None], ((w.shape[2] - 1) * dilation, 0)), w, self.w[key + ".bias"], stride=stride, dilation=dilation, groups=groups)
        return y[0].T

    def snake(self, x, key):
        return x + (1.0 / torch.exp(self.w[key + ".beta"])) * torch.sin(torch.exp(self.w[key + ".alpha"]) * x) ** 2

    def conv(self, pcm):
        w, g = self.w, self.g
        st = tuple(reversed(g["upsample_rates"])) + tuple(reversed(g["upsampling_ratios"]))
        h = self.cconv(torch.from_numpy(np.asarray(pcm, dtype=np.float32))[:, None], "encoder.encoder.0.conv")
        for b in range(4):
            p = "encoder.encoder.%d.block." % (b + 1)
            for j, d in enumerate((1, 3, 9)):
                u = self.cconv(self.snake(h, p + "%d.act1" % j), p + "%d.conv1.conv" % j, dilation=d)
                h = self.cconv(self.snake(u, p + "%d.act2" % j), p + "%d.conv2.conv" % j) + h
            h = self.cconv(self.snake(h, p + "3"), p + "4.conv", stride=st[b])
        h = self.cconv(h, "encoder.encoder.5.conv")
        for i in range(2):
            p = "encoder.downsample.%d." % i
            u = self.cconv(h, p + "0.dwconv.conv", groups=h.shape[1])
            u = F.layer_norm(u, (u.shape[1],), w[p + "0.norm.weight"], w[p + "0.norm.bias"], 1e-5)
            u = F.linear(F.gelu(F.linear(u, w[p + "0.pwconv1.weight"], w[p + "0.pwconv1.bias"])), w[p + "0.pwconv2.weight"], w[p + "0.pwconv2.bias"])
            h = self.cconv(u * w[p + "0.gamma"] + h, p + "1.conv", stride=st[4 + i])
        return self.cconv(h, "encoder.post_conv.conv")

    def rms(self, x, key):
        return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + self.g["rms_norm_eps"]) * self.w[key]

    def transformer(self, x):
        w, g = self.w, self.g
        T, nh, hd = x.shape[0], g["num_heads"], g["head_dim"]
        inv = torch.from_numpy((10000.0 ** (-np.arange(hd // 2) / (hd // 2))).astype(np.float32))
        ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
        cos, sin = torch.cos(ang)[None], torch.sin(ang)[None]

        def rot(t):                                                               # [heads, T, hd], rotate-halves
            a, b = t[..., :hd // 2], t[..., hd // 2:]
            return torch.cat([a * cos - b * sin, a * sin + b * cos], dim=-1)

        P = "encoder.pre_transformer."
        h = F.linear(torch.as_tensor(x, dtype=torch.float32), w[P + "input_proj.weight"], w[P + "input_proj.bias"])
        for l in range(g["num_layers"]):
            L = P + "layers.%d." % l
            n = self.rms(h, L + "input_layernorm.weight")
            q, k, v = (F.linear(n, w[L + "self_attn.%s_proj.weight" % c]).reshape(T, nh, hd).transpose(0, 1) for c in "qkv")
            a = F.scaled_dot_product_attention(rot(q), rot(k), v).transpose(0, 1).reshape(T, nh * hd)
            h = h + F.linear(a, w[L + "self_attn.o_proj.weight"]) * w[L + "self_attn_layer_scale.scale"]
            n = self.rms(h, L + "post_attention_layernorm.weight")
            m = F.linear(F.silu(F.linear(n, w[L + "mlp.gate_proj.weight"])) * F.linear(n, w[L + "mlp.up_proj.weight"]), w[L + "mlp.down_proj.weight"])
            h = h + m * w[L + "mlp_layer_scale.scale"]
        return self.rms(h, P + "norm.weight")

    def codebook(self, name, i):
        p = "encoder.quantizer.%s.vq.layers.%d._codebook" % (name, i)
        if p + ".embed" in self.w:
            return self.w[p + ".embed"]
        return self.w[p + ".embedding_sum"] / torch.clamp(self.w[p + ".cluster_usage"], min=1e-7)[:, None]

    def rvq(self, h):
        """The expanded form in f32; the argmin is numpy's (lowest index among equals)."""
        out = []
        for name, _, count in O.chains(self.g):
            r = torch.as_tensor(h, dtype=torch.float32) @ self.w["encoder.quantizer.%s.input_proj.weight" % name][:, :, 0]
            for i in range(count):
                cb = self.codebook(name, i)
                d = ((r * r).sum(dim=-1, keepdim=True) - 2.0 * (r @ cb.T)) + (cb * cb).sum(dim=-1)[None, :]
                c = torch.from_numpy(d.numpy().argmin(axis=-1))
                r = r - cb[c]
                out.append(c.numpy())
        return np.stack(out).astype(np.int32)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def chain_mismatch(got, want):
    """Fraction of (frame, quantizer chain) pairs with any differing code."""
    bad = [(got[0] != want[0]), (got[1:] != want[1:]).any(axis=0)]
    return float(np.concatenate(bad).mean())


@pytest.fixture(scope="module")
def reduced():
    sd = synth.synth_speech_tokenizer_encoder_state_dict(0, G)
    W, twin = O.Weights(sd), Twin(sd, G)
    want = {}
    with torch.no_grad():
        for n in LENGTHS:
            pcm = O.make_pcm(n, n)
            c = O.conv(pcm, W, G)
            tc = twin.conv(pcm)
            want[n] = (c, O.transformer(c, W, G), tc.numpy(), twin.transformer(tc).numpy())
    return sd, W, twin, want


@pytest.fixture(scope="module")
def real():
    """The real geometry on the GPU tests' inputs (tens of seconds of float64: once per module)."""
    sd = synth.synth_speech_tokenizer_encoder_state_dict(1, R)
    W, twin = O.Weights(sd), Twin(sd, R)
    want = {}
    with torch.no_grad():
        for n in REAL_LENGTHS + (1920 * 40,):
            pcm = O.make_pcm(n, n)
            c = O.conv(pcm, W, R)
            tc = twin.conv(pcm)
            want[n] = (c, O.transformer(c, W, R), tc.numpy(), twin.transformer(tc).numpy())
    return sd, W, twin, want


def test_oracle_vs_twin_per_stage(reduced):
    """Each stage of the oracle on its own input against the twin on the same input: two independent statements of the reference."""
    sd, W, twin, want = reduced
    n = 1920 * 37 + 517
    c, h = want[n][0], want[n][1]
    with torch.no_grad():
        d_conv = rel(want[n][2], c)
        d_tr = rel(twin.transformer(torch.from_numpy(c.astype(np.float32))).numpy(), O.transformer(c.astype(np.float32).astype(np.float64), W, G))
        codes_t = twin.rvq(h.astype(np.float32))
    codes_o = O.rvq_encode(h.astype(np.float32).astype(np.float64), W, G)
    print("oracle vs torch f32 twin, 38 frames: conv %.2e, transformer %.2e of peak, rvq chains differing %.4f"
          % (d_conv, d_tr, chain_mismatch(codes_t, codes_o)))
    assert c.shape == (38, G["latent_dim"]) and h.shape == (38, G["hidden_size"]) and codes_o.shape == (16, 38)
    assert d_conv < 1e-4 and d_tr < 1e-4 and chain_mismatch(codes_t, codes_o) <= 0.01
    assert 0.1 < np.abs(c).max() < 100 and len(set(codes_o[0].tolist())) > 8              # the signal is alive down the chain


@pytest.mark.parametrize("n", [1, 1919, 1920, 1921, 5 * 1920 + 1])
def test_frame_counts(n):
    """Ceilings at every rate: ceil(n / 3), / 12, / 60, / 480, / 960, / 1920, from the oracle's own convs and from the library."""
    sd = synth.synth_speech_tokenizer_encoder_state_dict(0, G)
    rows = []
    c = O.conv(O.make_pcm(n, n), O.Weights(sd), G, rows)
    want = [-(-n // r) for r in (1, 3, 12, 60, 480, 960, 1920)]
    assert rows == want == O.lengths(n, G) and c.shape[0] == want[-1]
    with torch.no_grad():
        assert Twin(sd, G).conv(O.make_pcm(n, n)).shape[0] == want[-1]
    lib = _lib.load(strict=True)
    assert lib.qasr_codec_enc_num_frames(n) == want[-1] and lib.qasr_codec_enc_num_frames(0) == 0


def test_acoustic_quantizer_sees_the_latent(reduced):
    """EncoderRVQ.encode gives both quantizers h; SplitResidualVectorQuantizer.encode's form (h minus the decoded first code) gives other
    acoustic codes, and the same semantic ones."""
    sd, W, twin, want = reduced
    h = want[1920 * 97][1]
    a, b = O.rvq_encode(h, W, G), O.rvq_encode_split(h, W, G)
    assert np.array_equal(a[0], b[0]) and (a[1:] != b[1:]).mean() > 0.5
    with torch.no_grad():
        assert chain_mismatch(twin.rvq(h.astype(np.float32)), a) <= 0.01                  # the twin follows the encoder's form


def test_f32_distance(reduced, real):
    """The figures of tests/test_gpu_codec_enc.py's F32 table, on its inputs."""
    fig = {}
    for name, (sd, W, twin, want), lens in (("", reduced, LENGTHS), ("real_", real, REAL_LENGTHS)):
        fig[name + "conv"] = max(rel(want[n][2], want[n][0]) for n in lens)
        fig[name + "latent"] = max(rel(want[n][3], want[n][1]) for n in lens)
    print("torch f32 twin vs float64 oracle, max |d| / peak: " + ", ".join("%s %.2e" % kv for kv in fig.items()))
    assert all(0 < v < 1e-4 for v in fig.values()), fig


def test_rvq_twin(reduced, real):
    """On the GPU tests' latents (the oracle's, cast to f32) the f32 twin's codes are the float64 codes apart from at most half the GPU
    test's cap of 2 % of chains; prints the smallest relative distance gap the f32 form can resolve on these sizes."""
    for name, (sd, W, twin, want), n, g in (("reduced", reduced, 1920 * 97, G), ("real", real, 1920 * 40, R)):
        h = want[n][1].astype(np.float32)
        with torch.no_grad():
            got = twin.rvq(h)
        ref = O.rvq_encode(h.astype(np.float64), W, g)
        res = 0.0
        for cname, _, _ in O.chains(g):                                           # first stage of each chain: eps x the terms / the distance
            r = O.project(h.astype(np.float64), W, cname)
            cb = O.codebook(W, "encoder.quantizer.%s.vq.layers.0._codebook" % cname)
            d = O.distances(r, cb)
            terms = (r * r).sum(-1, keepdims=True) + 2 * np.abs(r @ cb.T) + (cb * cb).sum(-1)[None]
            best = d.argmin(-1)
            res = max(res, float((2.0 ** -24 * terms[np.arange(len(best)), best] / d.min(-1)).max()))
        mis = chain_mismatch(got, ref)
        print("%s rvq, %d frames: f32 twin chains differing from float64 %.4f (allowed 0.01); f32 resolution of the best distance %.1e"
              % (name, h.shape[0], mis, res))
        assert got.shape == ref.shape == (16, h.shape[0]) and mis <= 0.01
        assert res <= 1e-6                                                        # the GPU test's near-tie bound 1e-5 is 10 x this order


def test_f32_twin_end_to_end(reduced):
    """The f32 twin end to end stays under 5 % of chains differing on the GPU test's 38- and 97-frame inputs (its cap is 10 %)."""
    sd, W, twin, want = reduced
    for n in (1920 * 37 + 517, 1920 * 97):
        with torch.no_grad():
            got = twin.rvq(want[n][3])
        mis = chain_mismatch(got, O.rvq_encode(want[n][1], W, G))
        print("n = %d: f32 twin end to end, chains differing from the float64 encode %.4f" % (n, mis))
        assert mis < 0.05


def test_host_errors(tmp_path):
    """Argument and geometry errors that are found before any device call."""
    lib = _lib.load(strict=True)
    h = C.c_void_p()
    err = lambda: lib.qasr_codec_enc_last_error(None).decode()
    assert lib.qasr_codec_enc_create(0, None, 0, None, C.byref(h)) == 1 and "model_dir" in err()
    assert lib.qasr_codec_enc_create(0, str(tmp_path / "none").encode(), 0, None, C.byref(h)) == 4
    assert lib.qasr_codec_enc_create(0, b".", (1 << 24) + 1, None, C.byref(h)) == 1 and "max_samples" in err()
    assert lib.qasr_codec_enc_create(0, b".", 0, None, None) == 1
    sd = synth.synth_speech_tokenizer_encoder_state_dict(0, G)
    key = "encoder.downsample.1.1.conv.weight"
    for kw, code, word in ((dict(drop=(key,)), 4, key), (dict(reshape={key: (96, 96, 3)}), 1, key),
                           (dict(geometry=dict(G, head_dim=32)), 1, "head_dim"), (dict(geometry=dict(G, upsample_rates=(8, 5, 4, 2))), 1, "1920"),
                           (dict(drop=("encoder.pre_transformer.output_proj.bias",)), 4, "output_proj.bias")):
        d = synth.write_speech_tokenizer_safetensors(sd, str(tmp_path / ("m%d" % len(list(tmp_path.iterdir())))), kw.pop("geometry", G), **kw)
        assert lib.qasr_codec_enc_create(0, d.encode(), 0, None, C.byref(h)) == code and word in err() and "speech tokenizer encoder" in err()
    fp, ip = (C.c_float * 4)(), (C.c_int32 * 64)()
    assert lib.qasr_codec_enc_encode(None, fp, 4, ip) == 1 and lib.qasr_codec_enc_quantize(None, fp, 1, ip) == 1
    assert lib.qasr_codec_enc_unload(None) == 1 and lib.qasr_codec_enc_is_loaded(None) == 0 and lib.qasr_codec_enc_memory_footprint(None) == 0
    assert lib.qasr_codec_enc_timing(None, fp) == 1 and lib.qasr_codec_enc_num_quantizers(None) == 0
    # the decoder's synth weights are what they were: the encoder's functions draw from an rng of their own
    a = synth.synth_speech_tokenizer_state_dict(0, G)
    assert not any(k.startswith("encoder.") for k in a) and all(k.startswith("encoder.") for k in sd)
    both = synth.merge_speech_tokenizer_state_dicts(a, sd)
    assert len(both) == len(a) + len(sd) and math.isclose(float(both["decoder.pre_conv.conv.bias"][0]), float(a["decoder.pre_conv.conv.bias"][0]))

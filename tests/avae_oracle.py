"""Float64 NumPy restatement of the VoxCPM2 AudioVAE (Sources/VoxCPM2TTS/AudioVAE.swift) and its torch float32 twin.

One forward, two backends: NP computes in float64 with explicit tap loops, TH in float32 with torch's conv1d / conv_transpose1d (the
weight convention of a transposed conv: torch's weight[in][out][k] = W[out][k][in]).  The distance between the two on the tests'
inputs is what f32 costs on this network; the device bounds are 10 x it (tests/test_gpu_avae.py).  Activations are [rows, channels].
encode() / decode() return (stages, result): stages[0] after conv_in, stages[k] after block k - 1, as qasr_avae_enc_stage / _dec_stage."""
import numpy as np
import torch
import torch.nn.functional as F

from qasr.audiovae import sanitize, sr_index

DILATIONS = (1, 3, 9)


class Weights:
    """The tensors a checkpoint's dict gives after AudioVAE.sanitize, without the audio_vae. prefix."""

    def __init__(self, stored: dict, geom: dict):
        self.geom = geom
        self.f32 = {k[len("audio_vae."):]: v for k, v in sanitize(stored).items() if k.startswith("audio_vae.")}
        self.f64 = {k: v.astype(np.float64) for k, v in self.f32.items()}
        self.th = {k: torch.from_numpy(v) for k, v in self.f32.items()}


class NP:
    name = "float64"

    def __init__(self, W):
        self.w = W.f64

    def array(self, x):
        return np.asarray(x, dtype=np.float64)

    def snake(self, x, key):
        a = self.w[key + ".alpha"].reshape(-1)
        return x + (1.0 / (a + 1e-9)) * np.sin(a * x) ** 2

    def conv(self, x, key, left, stride=1, dil=1):
        """CausalConv1d (:99-111): `left` zeros in front, none behind."""
        w, b = self.w[key + ".weight"], self.w[key + ".bias"]
        out, k, cg = w.shape
        xp = np.concatenate([np.zeros((left, x.shape[1])), x])
        n = (xp.shape[0] - (k - 1) * dil - 1) // stride + 1
        y = np.zeros((n, out))
        for j in range(k):
            seg = xp[j * dil: j * dil + (n - 1) * stride + 1: stride]
            y += seg @ w[:, j, :].T if cg == x.shape[1] else seg * w[:, j, 0]
        return y + b

    def conv_t(self, x, key, s):
        """CausalTransposeConv1d (:147-157): every input row spreads over 2 s output rows, the last s rows are trimmed."""
        w, b = self.w[key + ".weight"], self.w[key + ".bias"]
        L = x.shape[0]
        full = np.zeros(((L + 1) * s, w.shape[0]))
        for j in range(2 * s):
            full[j: j + L * s: s] += x @ w[:, j, :].T
        return full[:L * s] + b

    def affine(self, x, key, idx):
        return x * self.w[key + ".scale_embed.weight"][idx] + self.w[key + ".bias_embed.weight"][idx]

    def tanh(self, x):
        return np.tanh(x)

    def out(self, x):
        return np.asarray(x, dtype=np.float64)


class TH(NP):
    name = "float32"

    def __init__(self, W):
        self.w = W.th

    def array(self, x):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))

    def snake(self, x, key):
        a = self.w[key + ".alpha"].reshape(-1)
        return x + (1.0 / (a + 1e-9)) * torch.sin(a * x) ** 2

    def conv(self, x, key, left, stride=1, dil=1):
        w, b = self.w[key + ".weight"], self.w[key + ".bias"]
        xp = F.pad(x.T[None], (left, 0))
        groups = x.shape[1] // w.shape[2]
        return F.conv1d(xp, w.permute(0, 2, 1).contiguous(), b, stride=stride, dilation=dil, groups=groups)[0].T

    def conv_t(self, x, key, s):
        w, b = self.w[key + ".weight"], self.w[key + ".bias"]
        y = F.conv_transpose1d(x.T[None], w.permute(2, 0, 1).contiguous(), b, stride=s)[0].T
        return y[:x.shape[0] * s]

    def tanh(self, x):
        return torch.tanh(x)

    def out(self, x):
        return x.numpy().astype(np.float64)


def unit(be, x, p, dil):
    """CausalResidualUnit (:266-273)."""
    h = be.conv(be.snake(x, p + ".snake1"), p + ".conv1", 6 * dil, dil=dil)
    return x + be.conv(be.snake(h, p + ".snake2"), p + ".conv2", 0)


def encode(pcm, W, backend=NP):
    """AudioVAE.encode: preprocess (zero samples up to a whole frame), conv_in, the blocks, fc_mu."""
    be, g = backend(W), W.geom
    hop = int(np.prod(g["encoder_rates"]))
    x = np.asarray(pcm, dtype=np.float32)
    x = np.concatenate([x, np.zeros((-x.size) % hop, dtype=np.float32)])
    with torch.no_grad():
        h = be.conv(be.array(x[:, None]), "encoder.conv_in", 6)
        stages = [be.out(h)]
        for i, s in enumerate(g["encoder_rates"]):
            p = f"encoder.blocks.layers.{i}"
            for u, d in enumerate(DILATIONS):
                h = unit(be, h, f"{p}.res{u + 1}", d)
            h = be.conv(be.snake(h, p + ".snake"), p + ".conv", s, stride=s)
            stages.append(be.out(h))
        return stages, be.out(be.conv(h, "encoder.fc_mu", 2))


def output(rows, W, backend=NP):
    """snake_out, conv_out, tanh (:558-560)."""
    be = backend(W)
    with torch.no_grad():
        return be.out(be.tanh(be.conv(be.snake(be.array(rows), "decoder.snake_out"), "decoder.conv_out", 6)))[:, 0]


def decode(z, W, sr_cond=48000, backend=NP):
    """CausalDecoder.callAsFunction (:536-561)."""
    be, g = backend(W), W.geom
    idx = sr_index(sr_cond, g["sr_bin_boundaries"])
    with torch.no_grad():
        h = be.conv(be.conv(be.array(z), "decoder.conv_in.layers.0", 6), "decoder.conv_in.layers.1", 0)
        stages = [be.out(h)]
        for i, s in enumerate(g["decoder_rates"]):
            p = f"decoder.blocks.layers.{i}"
            h = be.affine(h, f"decoder.sr_cond_layers.{i}", idx)
            h = be.conv_t(be.snake(h, p + ".snake"), p + ".conv_t", s)
            for u, d in enumerate(DILATIONS):
                h = unit(be, h, f"{p}.res{u + 1}", d)
            stages.append(be.out(h))
        pcm = be.tanh(be.conv(be.snake(h, "decoder.snake_out"), "decoder.conv_out", 6))
        return stages, be.out(pcm)[:, 0]


def conv_t_two_tap(x, w, b, s):
    """The trimmed transposed conv as the device runs it: y[t s + r] = x[t] W[:, r, :] + x[t - 1] W[:, r + s, :], x[-1] = 0."""
    L, out = x.shape[0], w.shape[0]
    prev = np.concatenate([np.zeros((1, x.shape[1])), x[:-1]])
    y = np.zeros((L, s, out))
    for r in range(s):
        y[:, r] = x @ w[:, r, :].T + prev @ w[:, r + s, :].T
    return y.reshape(L * s, out) + b


def rel(a, b):
    """max |a - b| over the peak of b."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())

"""Float64 restatement of the WeSpeaker speaker embedding (not collected; imported by tests only).

Front end = MelFeatureExtractor.extractRaw (Sources/SpeechVAD/MelFeatureExtractor.swift:120-214), network = WeSpeakerNetwork
(WeSpeakerModel.swift:67-170), in NHWC [F, T, C] with H = frequency, W = time, convolutions written as sums of shifted matmuls.
Two policies:
  REFERENCE  no rounding anywhere
  DEVICE     the points csrc/spk_wespeaker.hip rounds: 3x3 / shortcut weights to bf16, and the stored activations (stem output, each
             block's conv1 output, each block's output) to bf16.  The front end, stem weights, pooling and linear stay unrounded.
"""
import numpy as np
import torch

REFERENCE, DEVICE = "reference", "device"
BLOCKS = (3, 4, 6, 3)
N_FFT, HOP, N_MELS, PAD = 400, 160, 80, 200


def hz_to_mel(hz):
    return 2595.0 * np.log10(1.0 + hz / 700.0)


def mel_to_hz(mel):
    return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)


def mel_bank():
    """[80, 257] HTK triangles on k * 16000 / 512, 20 Hz .. 8 kHz, slaney-normalised (setupMelFilterbank)."""
    pts = mel_to_hz(hz_to_mel(20.0) + np.arange(N_MELS + 2) * (hz_to_mel(8000.0) - hz_to_mel(20.0)) / (N_MELS + 1))
    f = np.arange(257) * 16000.0 / 512.0
    d = np.diff(pts)
    fb = np.zeros((N_MELS, 257))
    for m in range(N_MELS):
        down = (f - pts[m]) / d[m]
        up = (pts[m + 2] - f) / d[m + 1]
        fb[m] = np.maximum(0.0, np.minimum(down, up)) * (2.0 / (pts[m + 2] - pts[m]))
    return fb


def num_frames(n):
    return (n + 2 * PAD - N_FFT) // HOP + 1


def padded(x):
    """pre-emphasis 0.97 (y[0] = x[0]) + the reference's reflect pad with its index clamps"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    e = np.empty(n)
    e[0] = x[0]
    e[1:] = x[1:] - 0.97 * x[:-1]
    left = [e[max(0, min(PAD - i, n - 1))] for i in range(PAD)]
    right = [e[max(0, n - 2 - i)] for i in range(PAD)]
    return np.concatenate([left, e, right])


def fbank(x):
    """post-CMN log-mel [T, 80]"""
    p = padded(x)
    T = num_frames(len(x))
    win = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(N_FFT) / (N_FFT - 1))
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(p[idx] * win, n=512, axis=1)
    power = 4.0 * (spec.real ** 2 + spec.imag ** 2)              # vDSP_fft_zrip returns 2 X
    mel = np.log(np.maximum(power @ mel_bank().T, 1e-10))
    return mel - mel.mean(axis=0, keepdims=True)


def _bf(t, policy):
    return t.to(torch.bfloat16).to(torch.float64) if policy == DEVICE else t


class Weights:
    def __init__(self, sd, policy=REFERENCE):
        self.t = {}
        for k, v in sd.items():
            t = torch.as_tensor(np.asarray(v, dtype=np.float64))
            if k.startswith("layer") and k.endswith(".weight"):
                t = _bf(t, policy)
            self.t[k] = t
        self.policy = policy


def conv(x, w, b, stride):
    """x [F, T, Ci], w [Co, 3, 3, Ci] (or [Co, 1, 1, Ci], no padding), zero padding 1 -> [ceil(F / s), ceil(T / s), Co]"""
    k = w.shape[1]
    F, T = x.shape[0], x.shape[1]
    Fo, To = -(-F // stride), -(-T // stride)
    if k == 1:
        return x[::stride, ::stride, :] @ w[:, 0, 0, :].T + b
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(Fo, To, w.shape[0], dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            out += xp[kh:kh + stride * (Fo - 1) + 1:stride, kw:kw + stride * (To - 1) + 1:stride, :] @ w[:, kh, kw, :].T
    return out + b


def network(feat, W):
    """feat [T, 80] -> (embedding [256], pooled [5120], final activation [10, T', 256])"""
    pol, t = W.policy, W.t
    x = torch.as_tensor(np.asarray(feat, dtype=np.float64)).T.unsqueeze(-1)          # [80, T, 1]
    x = _bf(torch.relu(conv(x, t["conv1.weight"], t["conv1.bias"], 1)), pol)
    for st, nb in enumerate(BLOCKS):
        for i in range(nb):
            p = f"layer{st + 1}.{i}."
            s = 2 if st > 0 and i == 0 else 1
            y = _bf(torch.relu(conv(x, t[p + "conv1.weight"], t[p + "conv1.bias"], s)), pol)
            y = conv(y, t[p + "conv2.weight"], t[p + "conv2.bias"], 1)
            r = conv(x, t[p + "shortcut.weight"], t[p + "shortcut.bias"], 2) if s == 2 else x
            x = _bf(torch.relu(y + r), pol)
    h = x.permute(1, 2, 0).reshape(x.shape[1], -1)                # [T', C * 10 + f] (C*F order)
    mean = h.mean(0)
    var = ((h - mean) ** 2).mean(0)
    pooled = torch.cat([mean, torch.sqrt(var + 1e-10)])
    e = pooled @ t["embedding.weight"].T + t["embedding.bias"]
    e = e / torch.sqrt((e * e).sum() + 1e-10)
    return e.numpy(), pooled.numpy(), x


def embed(pcm, W):
    with torch.no_grad():
        return network(fbank(pcm), W)[0]

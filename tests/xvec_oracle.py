"""float64 numpy restatement of the Qwen3-TTS speaker encoder (reference: Sources/Qwen3TTS/SpeakerEncoder.swift): SpeakerMel.compute
(:245-388) and the ECAPA-TDNN (:10-238).  The oracle of tests/test_xvec_cpu.py and tests/test_gpu_xvec.py.

Where the reference computes a table in Float (the Hann window :282-286, the HTK filterbank :354-387) the table is built here with
float32 arithmetic and then widened; everything that touches the signal is float64.  Weights are the checkpoint's: `.weight`
[out][k][in], `.bias` [out], keys without the `speaker_encoder.` prefix.
"""
import numpy as np

SAMPLE_RATE, N_FFT, HOP, N_MELS, N_BINS = 24000, 1024, 256, 128, 513
CHANNELS, WIDTH, SCALE, SE_DIM, ATT_DIM, CAT = 512, 64, 8, 128, 128, 1536
DILATIONS = (2, 3, 4)
F = np.float32


def num_frames(n):
    return n // HOP + 1 if n > 0 else 0


def make_pcm(seed, n):
    """n samples of a speech-level test signal: two tones under broadband noise, float32, |x| well below 1."""
    rng = np.random.default_rng(9000 + seed)
    t = np.arange(n, dtype=np.float64) / SAMPLE_RATE
    x = 0.05 * rng.standard_normal(n) + 0.05 * np.sin(2 * np.pi * (170.0 + 13.0 * (seed % 7)) * t + 0.3 * seed) \
        + 0.03 * np.sin(2 * np.pi * 2310.0 * t + 1.1)
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- front end ----------------------------------------------------------------------------------------------------------------------
def hann():
    """:282-286 in Float: 0.5 (1 - cos(2 pi i / 1024))."""
    i = np.arange(N_FFT, dtype=F)
    return (F(0.5) * (F(1.0) - np.cos(F(2.0) * F(np.pi) * i / F(N_FFT), dtype=F))).astype(F)


def mel_points():
    """The 130 band edges in Hz (:359-366), Float arithmetic."""
    hz_to_mel = lambda hz: F(2595.0) * np.log10(F(1.0) + hz / F(700.0), dtype=F)
    mel_to_hz = lambda m: F(700.0) * (np.power(F(10.0), m / F(2595.0), dtype=F) - F(1.0))
    lo, hi = hz_to_mel(F(0.0)), hz_to_mel(F(12000.0))
    return np.array([mel_to_hz(lo + F(i) * (hi - lo) / F(N_MELS + 1)) for i in range(N_MELS + 2)], dtype=F)


def filterbank():
    """[513][128] float32 as :354-387 builds it, the >= / <= / > edge rules included."""
    pts = mel_points()
    freqs = (np.arange(N_BINS, dtype=F) * F(SAMPLE_RATE) / F(N_FFT)).astype(F)
    fb = np.zeros((N_BINS, N_MELS), dtype=F)
    for m in range(N_MELS):
        lo, ce, hi = pts[m], pts[m + 1], pts[m + 2]
        for k in range(N_BINS):
            f = freqs[k]
            if f >= lo and f <= ce and ce > lo:
                fb[k, m] = (f - lo) / (ce - lo)
            elif f > ce and f <= hi and hi > ce:
                fb[k, m] = (hi - f) / (hi - ce)
    return fb


_FB64 = None


def filterbank64():
    global _FB64
    if _FB64 is None:
        _FB64 = filterbank().astype(np.float64)
    return _FB64


def padded(x):
    """Reflect pad of 512 with the reference's clamped indices (:294-303)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n, pad = x.size, N_FFT // 2
    i = np.arange(pad)
    left = x[np.minimum(i + 1, n - 1)][::-1]              # padded[pad - 1 - i] = x[min(i + 1, n - 1)]
    right = x[np.maximum(n - 2 - i, 0)]
    return np.concatenate([left, x, right])


def stft_magnitudes(x):
    """[T][513] magnitudes of the plain 1024-point DFT of every Hann-windowed frame, T = n / 256 + 1."""
    p = padded(x)
    T = (p.size - N_FFT) // HOP + 1
    frames = np.stack([p[t * HOP:t * HOP + N_FFT] for t in range(T)]) * hann().astype(np.float64)[None, :]
    return np.abs(np.fft.rfft(frames, axis=1))


def mel(x):
    """SpeakerMel.compute: [T][128] log-mel."""
    return np.log(np.maximum(stft_magnitudes(x) @ filterbank64(), 1e-5))


# ---- network ------------------------------------------------------------------------------------------------------------------------
class Weights:
    def __init__(self, sd):
        self.w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
        self.embedding_dim = int(self.w["fc.weight"].shape[0])

    def __getitem__(self, k):
        return self.w[k]


def conv1d(x, W, key, dilation=1):
    """MLX Conv1d on x [T][in]: weight [out][k][in], zeros of (k - 1) dilation / 2 rows on both sides."""
    w, b = W[key + ".weight"], W[key + ".bias"]
    T, k = x.shape[0], w.shape[1]
    pad = (k - 1) * dilation // 2
    xp = np.zeros((T + 2 * pad, x.shape[1]))
    xp[pad:pad + T] = x
    y = np.tile(b[None, :], (T, 1))
    for j in range(k):
        y += xp[j * dilation:j * dilation + T] @ w[:, j, :].T
    return y


def relu(x):
    return np.maximum(x, 0.0)


def res2net(x, W, prefix, dilation):
    outs = [x[:, :WIDTH]]
    for i in range(1, SCALE):
        chunk = x[:, i * WIDTH:(i + 1) * WIDTH]
        u = chunk if i == 1 else chunk + outs[i - 1]
        outs.append(relu(conv1d(u, W, "%s.blocks.%d.conv" % (prefix, i - 1), dilation)))
    return np.concatenate(outs, axis=1)


def block(x, W, b):
    p, d = "blocks.%d" % b, DILATIONS[b - 1]
    h = relu(conv1d(x, W, p + ".tdnn1.conv"))
    h = res2net(h, W, p + ".res2net_block", d)
    h = relu(conv1d(h, W, p + ".tdnn2.conv"))
    s = h.mean(axis=0, keepdims=True)
    g = 1.0 / (1.0 + np.exp(-conv1d(relu(conv1d(s, W, p + ".se_block.conv1")), W, p + ".se_block.conv2")))
    return h * g + x


def pooling(x, W):
    T = x.shape[0]
    mean = x.mean(axis=0, keepdims=True)
    std = np.sqrt(np.maximum(((x - mean) ** 2).mean(axis=0, keepdims=True), 1e-12))
    a = np.concatenate([x, np.tile(mean, (T, 1)), np.tile(std, (T, 1))], axis=1)
    e = conv1d(np.tanh(conv1d(a, W, "asp.tdnn.conv")), W, "asp.conv")
    e = np.exp(e - e.max(axis=0, keepdims=True))
    alpha = e / e.sum(axis=0, keepdims=True)
    wm = (alpha * x).sum(axis=0)
    wv = (alpha * (x - wm[None, :]) * (x - wm[None, :])).sum(axis=0)
    return np.concatenate([wm, np.sqrt(np.maximum(wv, 1e-12))])


def network(m, W, stages=None):
    """mel [T][128] -> the embedding [E] (not normalised, as the reference leaves it)."""
    h0 = relu(conv1d(np.asarray(m, dtype=np.float64), W, "blocks.0.conv"))
    o1 = block(h0, W, 1)
    o2 = block(o1, W, 2)
    o3 = block(o2, W, 3)
    h = relu(conv1d(np.concatenate([o1, o2, o3], axis=1), W, "mfa.conv"))
    pooled = pooling(h, W)
    if stages is not None:
        stages.update(h0=h0, o1=o1, o2=o2, o3=o3, mfa=h, pooled=pooled)
    return conv1d(pooled[None, :], W, "fc")[0]


def embed(x, W):
    return network(mel(x), W)

"""Float64 numpy restatement of the CosyVoice3 HiFT vocoder (Sources/CosyVoiceTTS/HiFiGAN.swift, Configuration.swift:84-107,
WeightLoading.swift:214-331), the oracle of csrc/voc_cosyvoice.hip.  Channel-last: activations are [rows, channels], conv weights
[out, k, in] as hifigan.safetensors stores them.  The transforms' tables are the reference's Float values (it forms them in Double and
stores Float, :417-433, :539-559); everything else is float64.

The noise is the library's counter stream (include/qasr.h), formed here from the same integers in float64: draw c of a clip is
splitmix64(seed + (c + 1) gamma); u1 = ((r >> 40) + 1) 2^-24, u2 = ((r >> 16) & 0xFFFFFF) 2^-24, uniform = u2, normal = sqrt(-2 ln u1)
cos(2 pi u2).  Counters 0 .. 8: the harmonics' initial phases; 16 + 10 n + h: the unvoiced noise of sample n, harmonic h + 1;
16 + 10 n + 9: the noise added to sample n after the merge."""
import numpy as np

RATE, N_MELS, HARMONICS, N_FFT, HOP, BINS = 24000, 80, 9, 16, 4, 9
RATES, UP_K, CH = (8, 5, 3), (16, 11, 7), (512, 256, 128, 64)
DOWN_STRIDE, DOWN_K, SRC_K, RES_K, DILATIONS = (15, 3, 1), (30, 6, 1), (7, 7, 11), (3, 7, 11), (1, 3, 5)
SAMPLES_PER_FRAME = 480
GAMMA, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def num_samples(T):
    return 480 * T + 16 if T else 0


def make_mel(seed, T):
    """A float32 [T, 80] log-mel-like clip: independent frames around -1 with deviation 1.5."""
    rng = np.random.default_rng(7300 + seed)
    return (1.5 * rng.standard_normal((T, N_MELS)) - 1.0).astype(np.float32)


def clip_mel(T):
    """The clip of T frames both test files use."""
    return make_mel(T, T)


TRACKS = ("voiced", "unvoiced", "alternating", "threshold")


def f0_track(kind, T):
    """A float32 F0 track of T frames.  voiced: 80 .. 380 Hz; unvoiced: 0 .. 10 Hz (the noise path alone); alternating: voiced on even
    frames, 5 Hz on odd ones; threshold: a voiced track whose frames 0, 3, .. are exactly 10.0 (unvoiced: the test is a strict >),
    frames 1, 4, .. exactly 0.0 and frames 2, 5, .. the float32 after 10.0 (voiced)."""
    rng = np.random.default_rng(9100 + T)
    v = (80.0 + 300.0 * rng.random(T)).astype(np.float32)
    if kind == "unvoiced":
        v = (10.0 * rng.random(T)).astype(np.float32)
    elif kind == "alternating":
        v[1::2] = 5.0
    elif kind == "threshold":
        v[0::3], v[1::3], v[2::3] = 10.0, 0.0, np.nextafter(np.float32(10.0), np.float32(11.0))
        v[6::7] = (80.0 + 300.0 * rng.random(len(v[6::7]))).astype(np.float32)
    elif kind != "voiced":
        raise ValueError(kind)
    return v


class Weights:
    def __init__(self, sd):
        self.t = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}

    def __getitem__(self, k):
        return self.t[k]


# ---- the noise stream ---------------------------------------------------------------------------------------------------------------
def draw(seed, counters):
    """splitmix64 at the given counters (any shape) of the stream `seed`: uint64."""
    with np.errstate(over="ignore"):
        c = np.asarray(counters, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (c + np.uint64(1)) * np.uint64(GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        return z ^ (z >> np.uint64(31))


def uniform(r):
    return ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0


def normal(r):
    u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * uniform(r))


# ---- convs --------------------------------------------------------------------------------------------------------------------------
def conv(x, W, key, dilation=1, lpad=None, rpad=0, stride=1):
    """Conv1d of x [rows, in] with zeros of lpad rows in front (default (k - 1) dilation: causal) and rpad rows behind."""
    w, b = W[key + ".weight"], W[key + ".bias"]
    out, k, cin = w.shape
    lpad = (k - 1) * dilation if lpad is None else lpad
    xp = np.concatenate([np.zeros((lpad, cin)), x, np.zeros((rpad, cin))], axis=0)
    n = (xp.shape[0] - (k - 1) * dilation - 1) // stride + 1
    cols = np.concatenate([xp[j * dilation: j * dilation + (n - 1) * stride + 1: stride] for j in range(k)], axis=1)
    return cols @ w.reshape(out, k * cin).T + b


def snake(x, alpha):
    s = np.sin(alpha * x)
    return x + (1.0 / (alpha + 1e-9)) * (s * s)


def resblock(x, W, p, k):
    h = x
    for d, dil in enumerate(DILATIONS):
        xt = conv(snake(h, W["%s.activations1.%d.alpha" % (p, d)]), W, "%s.convs1.%d" % (p, d), dilation=dil)
        xt = conv(snake(xt, W["%s.activations2.%d.alpha" % (p, d)]), W, "%s.convs2.%d" % (p, d))
        h = h + xt
    return h


# ---- stages -------------------------------------------------------------------------------------------------------------------------
def f0(mel, W):
    """F0Predictor (:361-373): mel [T, 80] -> [T]."""
    h = np.asarray(mel, dtype=np.float64)
    for i in range(5):
        h = conv(h, W, "f0_predictor.condnet.%d" % (2 * i), lpad=0, rpad=3) if i == 0 else conv(h, W, "f0_predictor.condnet.%d" % (2 * i))
        h = np.where(h > 0, h, np.exp(np.minimum(h, 0.0)) - 1.0)
    return np.abs(h @ W["f0_predictor.classifier.weight"].T + W["f0_predictor.classifier.bias"])[:, 0]


def source(f0_track, seed, W):
    """interpolateF0 and SourceModuleHnNSF (:383-395, :253-289, :323-328): f0 [T] -> [480 T]."""
    f = np.repeat(np.asarray(f0_track, dtype=np.float64), SAMPLES_PER_FRAME)
    n = np.arange(f.size, dtype=np.uint64)
    h = np.arange(1, HARMONICS + 1, dtype=np.float64)
    uv = (f > 10.0)[:, None]
    cycles = np.cumsum(f[:, None] * h[None, :] / RATE * uv, axis=0) + uniform(draw(seed, np.arange(HARMONICS)))[None, :]
    sines = 0.1 * np.sin(2.0 * np.pi * (cycles - np.floor(cycles)))
    noise = 0.003 * normal(draw(seed, np.uint64(16) + np.uint64(10) * n[:, None] + np.arange(HARMONICS, dtype=np.uint64)[None, :]))
    waves = np.where(uv, sines, noise)
    merged = np.tanh(waves @ W["m_source.l_linear.weight"].T + W["m_source.l_linear.bias"])[:, 0]
    return merged + 0.003 * normal(draw(seed, np.uint64(16) + np.uint64(10) * n + np.uint64(9)))


def hann():
    return np.array([np.float32(0.5 * (1.0 - np.cos(2.0 * np.pi * n / N_FFT))) for n in range(N_FFT)], dtype=np.float64)


def stft(x):
    """:410-486: x [n] -> [n / 4 + 1, 18] (9 real | 9 imaginary), reflect padding 8."""
    x = np.asarray(x, dtype=np.float64)
    p = np.concatenate([x[8:0:-1], x, x[-2:-10:-1]])
    frames = (p.size - N_FFT) // HOP + 1
    fr = np.stack([p[HOP * f: HOP * f + N_FFT] for f in range(frames)]) * hann()[None, :]
    ang = 2.0 * np.pi * np.outer(np.arange(BINS), np.arange(N_FFT)) / N_FFT
    re = np.cos(ang).astype(np.float32).astype(np.float64)
    im = (-np.sin(ang)).astype(np.float32).astype(np.float64)
    return np.concatenate([fr @ re.T, fr @ im.T], axis=1)


def istft(mag, ph):
    """:502-620: mag, ph [F, 9] -> [4 F + 12]; the centre padding stays."""
    F = mag.shape[0]
    re, im = mag * np.cos(ph), mag * np.sin(ph)
    full_re = np.concatenate([re, re[:, BINS - 2:0:-1]], axis=1)
    full_im = np.concatenate([im, -im[:, BINS - 2:0:-1]], axis=1)
    ang = 2.0 * np.pi * np.outer(np.arange(N_FFT), np.arange(N_FFT)) / N_FFT
    ct = (np.cos(ang) / N_FFT).astype(np.float32).astype(np.float64)
    st = (np.sin(ang) / N_FFT).astype(np.float32).astype(np.float64)
    w = hann()
    t = (full_re @ ct.T - full_im @ st.T) * w[None, :]
    out, wsum = np.zeros(4 * F + 12), np.zeros(4 * F + 12)
    for s in range(4):
        out[4 * s: 4 * s + 4 * F] += t[:, 4 * s: 4 * s + 4].reshape(-1)
        wsum[4 * s: 4 * s + 4 * F] += np.tile(w[4 * s: 4 * s + 4] ** 2, F)
    return out / np.maximum(wsum, 1e-8)


def decode_source(mel, src, W, st=None):
    """:777-857 on a given source: mel [T, 80], src [480 T] -> [480 T + 16].  st: a dict that receives the row counts on both sides of
    every source add and conv_post's output."""
    mel = np.asarray(mel, dtype=np.float64)
    spec = stft(src)
    x = conv(mel, W, "conv_pre", lpad=0, rpad=4)
    for i in range(3):
        x = np.maximum(x, 0.1 * x)
        x = conv(np.repeat(x, RATES[i], axis=0), W, "ups.%d" % i)
        if i == 2:
            x = np.concatenate([x[1:2], x], axis=0)
        s = conv(spec, W, "source_downs.%d" % i, lpad=DOWN_STRIDE[i] - 1, stride=DOWN_STRIDE[i])
        s = resblock(s, W, "source_resblocks.%d" % i, SRC_K[i])
        if st is not None:
            st["rows%d" % i] = (x.shape[0], s.shape[0])
        rows = min(x.shape[0], s.shape[0])                                            # the reference's trim; it trims nothing
        assert rows == x.shape[0] == s.shape[0]
        x = x[:rows] + s[:rows]
        fused = resblock(x, W, "resblocks.%d" % (3 * i), RES_K[0])
        for j in (1, 2):
            fused = fused + resblock(x, W, "resblocks.%d" % (3 * i + j), RES_K[j])
        x = fused / 3.0
    x = np.maximum(x, 0.01 * x)
    x = conv(x, W, "conv_post")
    if st is not None:
        st["post"] = x
    audio = istft(np.exp(x[:, :BINS]), np.sin(x[:, BINS:]))
    return np.clip(audio, -0.99, 0.99)


def decode(mel, seed, W):
    """HiFiGANGenerator.callAsFunction (:755-858) with the library's noise stream."""
    return decode_source(mel, source(f0(mel, W), seed, W), W)

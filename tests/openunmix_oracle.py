"""NumPy restatement of the reference's Open-Unmix source separation (Sources/SourceSeparation), in float64 (the oracle) or, with
dtype=np.float32, as its f32 twin: the same code on f32 arrays, which measures what f32 arithmetic alone costs.

STFT.swift:40-102 (stft, magnitude), OpenUnmixModel.swift:91-127 and 175-301 (stem_forward, bilstm), WienerFilterMLX.swift:139-261
(wiener), STFT.swift:183-231 (istft), :240-260 (phase_apply), SourceSeparation.swift:45-175 (separate).
"""
import numpy as np

N_FFT, N_HOP, N_BINS, MAX_BIN, PAD = 4096, 1024, 2049, 1487, 2048
STEMS = ("vocals", "drums", "bass", "other")
BN_EPS = 1e-5          # MLXNN.BatchNorm's default; OpenUnmixModel.swift:71 passes none


def num_frames(n: int) -> int:
    return n // N_HOP + 1


def hann(dtype=np.float64):
    """Periodic Hann (STFT.swift:25-27)."""
    i = np.arange(N_FFT, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * i / N_FFT))).astype(dtype)


def pad_indices(n: int) -> np.ndarray:
    """Source index of every sample of the centre-padded signal (STFT.swift:43-58): left audio[max(0, min(2048 - i, n - 1))], right
    audio[max(0, n - 2 - i)].  A reflect pad only when n > 2048."""
    i = np.arange(PAD)
    left = np.maximum(0, np.minimum(PAD - i, n - 1))
    right = np.maximum(0, n - 2 - i)
    return np.concatenate([left, np.arange(n), right])


def stft(audio, dtype=np.float64):
    """audio [2, n] -> re, im, magnitude [T, 2, 2049]."""
    a = np.asarray(audio, dtype=dtype)
    n = a.shape[1]
    T = num_frames(n)
    idx = pad_indices(n)
    frames = idx[np.arange(T)[:, None] * N_HOP + np.arange(N_FFT)[None, :]]        # [T, 4096] source indices
    w = hann(dtype)
    re = np.zeros((T, 2, N_BINS), dtype=dtype)
    im = np.zeros((T, 2, N_BINS), dtype=dtype)
    for c in range(2):
        z = np.fft.rfft(a[c][frames] * w, axis=-1)
        re[:, c], im[:, c] = z.real.astype(dtype), z.imag.astype(dtype)
    return re, im, np.sqrt(re * re + im * im)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _bn(x, sd, p, dtype):
    g = lambda k: np.asarray(sd[p + "." + k], dtype=dtype)
    return (x - g("running_mean")) / np.sqrt(g("running_var") + dtype(BN_EPS)) * g("weight") + g("bias")


def lstm_direction(x, sd, p, reverse, dtype):
    """One LSTMCell over time (OpenUnmixModel.swift:275-301): gates i, f, g, o; h0 = c0 = 0; reverse walks T-1 .. 0 and returns its
    outputs in forward time order."""
    g = lambda k: np.asarray(sd[p + k], dtype=dtype)
    wih, whh, bih, bhh = g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh")
    hs = whh.shape[1]
    pre = x @ wih.T + bih
    h, c = np.zeros(hs, dtype=dtype), np.zeros(hs, dtype=dtype)
    out = np.zeros((x.shape[0], hs), dtype=dtype)
    whhT = np.ascontiguousarray(whh.T)
    for t in (range(x.shape[0] - 1, -1, -1) if reverse else range(x.shape[0])):
        gates = pre[t] + h @ whhT + bhh
        i, f = _sigmoid(gates[:hs]), _sigmoid(gates[hs:2 * hs])
        gg, o = np.tanh(gates[2 * hs:3 * hs]), _sigmoid(gates[3 * hs:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[t] = h
    return out


def bilstm(x, sd, dtype):
    for l in range(3):
        p = f"lstm.layers.{l}."
        x = np.concatenate([lstm_direction(x, sd, p + "forward.", False, dtype), lstm_direction(x, sd, p + "backward.", True, dtype)], axis=-1)
    return x


def stem_forward(mag, sd, dtype=np.float64):
    """mag [T, 2, 2049] -> masked magnitude [T, 2, 2049] (OpenUnmixModel.swift:91-127)."""
    g = lambda k: np.asarray(sd[k], dtype=dtype)
    mix = np.asarray(mag, dtype=dtype)
    T = mix.shape[0]
    h = (mix[:, :, :MAX_BIN] + g("input_mean")) * g("input_scale")
    h = h.reshape(T, 2 * MAX_BIN)
    h = np.tanh(_bn(h @ g("fc1.weight").T, sd, "bn1", dtype))
    skip = h
    h = np.concatenate([skip, bilstm(h, sd, dtype)], axis=-1)
    h = np.maximum(_bn(h @ g("fc2.weight").T, sd, "bn2", dtype), 0)
    h = _bn(h @ g("fc3.weight").T, sd, "bn3", dtype).reshape(T, 2, N_BINS)
    h = np.maximum(h * g("output_scale") + g("output_mean"), 0)
    return (h * mix).astype(dtype)


def wiener(masked, re, im, iterations=1, window=300, dtype=np.float64):
    """masked [J, T, 2, F], mixture re / im [T, 2, F] -> refined (re, im) [J, T, 2, F] (WienerFilterMLX.swift:26-84, 139-261)."""
    m, re, im = (np.asarray(a, dtype=dtype) for a in (masked, re, im))
    J, T = m.shape[0], m.shape[1]
    ore, oim = np.zeros_like(m), np.zeros_like(m)
    eps = dtype(1e-10)
    half = dtype(0.5)
    for pos in range(0, T, window):
        sl = slice(pos, min(T, pos + window))
        tL, tR = m[:, sl, 0], m[:, sl, 1]
        mRL, mIL, mRR, mIR = re[sl, 0], im[sl, 0], re[sl, 1], im[sl, 1]
        mLmag, mRmag = np.sqrt(mRL * mRL + mIL * mIL), np.sqrt(mRR * mRR + mIR * mIR)
        scale_div = dtype(max(1.0, float(max(mLmag.max(), mRmag.max())) / 10.0))
        s = dtype(1.0) / scale_div
        cosL, sinL = mRL / np.maximum(mLmag, eps), mIL / np.maximum(mLmag, eps)
        cosR, sinR = mRR / np.maximum(mRmag, eps), mIR / np.maximum(mRmag, eps)
        yLR, yLI, yRR, yRI = tL * cosL * s, tL * sinL * s, tR * cosR * s, tR * sinR * s
        xLR, xLI, xRR, xRI = mRL * s, mIL * s, mRR * s, mIR * s
        for _ in range(iterations):
            v = half * (yLR * yLR + yLI * yLI + yRR * yRR + yRI * yRI)
            sumV = v.sum(axis=1) + eps
            R00 = ((yLR * yLR + yLI * yLI).sum(axis=1) / sumV)[:, None]
            R01re = ((yLR * yRR + yLI * yRI).sum(axis=1) / sumV)[:, None]
            R01im = ((yLI * yRR - yLR * yRI).sum(axis=1) / sumV)[:, None]
            R11 = ((yRR * yRR + yRI * yRI).sum(axis=1) / sumV)[:, None]
            g0r, g1r, g1i, g3r = v * R00, v * R01re, v * R01im, v * R11
            c00, c01re, c01im, c11 = g0r.sum(axis=0) + eps, g1r.sum(axis=0), g1i.sum(axis=0), g3r.sum(axis=0) + eps
            c10re, c10im = c01re, -c01im
            detRe = (c00 * c11) - (c01re * c10re - c01im * c10im)
            detIm = -(c01re * c10im + c01im * c10re)
            detMag2 = detRe * detRe + detIm * detIm + eps * eps
            idR, idI = detRe / detMag2, -detIm / detMag2
            i0r, i0i = c11 * idR, c11 * idI
            i1r, i1i = -(c01re * idR - c01im * idI), -(c01re * idI + c01im * idR)
            i2r, i2i = -(c10re * idR - c10im * idI), -(c10re * idI + c10im * idR)
            i3r, i3i = c00 * idR, c00 * idI
            g2r, g2i = g1r, -g1i
            w0r = (g0r * i0r) + (g1r * i2r - g1i * i2i)
            w0i = (g0r * i0i) + (g1r * i2i + g1i * i2r)
            w1r = (g0r * i1r) + (g1r * i3r - g1i * i3i)
            w1i = (g0r * i1i) + (g1r * i3i + g1i * i3r)
            w2r = (g2r * i0r - g2i * i0i) + (g3r * i2r)
            w2i = (g2r * i0i + g2i * i0r) + (g3r * i2i)
            w3r = (g2r * i1r - g2i * i1i) + (g3r * i3r)
            w3i = (g2r * i1i + g2i * i1r) + (g3r * i3i)
            yLR, yLI, yRR, yRI = (w0r * xLR - w0i * xLI + w1r * xRR - w1i * xRI, w0r * xLI + w0i * xLR + w1r * xRI + w1i * xRR,
                                  w2r * xLR - w2i * xLI + w3r * xRR - w3i * xRI, w2r * xLI + w2i * xLR + w3r * xRI + w3i * xRR)
        ore[:, sl, 0], oim[:, sl, 0], ore[:, sl, 1], oim[:, sl, 1] = yLR * scale_div, yLI * scale_div, yRR * scale_div, yRI * scale_div
    return ore, oim


def phase_apply(masked, re, im, dtype=np.float64):
    """Without Wiener (STFT.swift:240-260): mag * cos / sin(atan2(im, re))."""
    m, re, im = (np.asarray(a, dtype=dtype) for a in (masked, re, im))
    ph = np.arctan2(im, re)
    return (m * np.cos(ph)).astype(dtype), (m * np.sin(ph)).astype(dtype)


def istft(re, im, length, dtype=np.float64):
    """re / im [..., T, 2, 2049] -> [..., 2, length]: irfft (1 / N), window, overlap-add, / max(sum w^2, 1e-8), trim 2048."""
    re, im = np.asarray(re, dtype=dtype), np.asarray(im, dtype=dtype)
    T = re.shape[-3]
    w = hann(dtype)
    z = (re + 1j * im)
    z[..., 0].imag = 0          # irfft reads the real part of bins 0 and 2048, as the mirrored full DFT's real output does
    z[..., N_BINS - 1].imag = 0
    frames = (np.fft.irfft(z, n=N_FFT, axis=-1).astype(dtype) * w)                  # [..., T, 2, 4096]
    frames = np.moveaxis(frames, -3, -2)                                               # [..., 2, T, 4096]
    out = np.zeros(frames.shape[:-2] + ((T + 3) * N_HOP,), dtype=dtype)
    wsum = np.zeros((T + 3) * N_HOP, dtype=dtype)
    for t in range(T):
        out[..., t * N_HOP:t * N_HOP + N_FFT] += frames[..., t, :]
        wsum[t * N_HOP:t * N_HOP + N_FFT] += w * w
    out = out / np.maximum(wsum, dtype(1e-8))
    return out[..., PAD:PAD + length]


def separate(audio, sds, targets=STEMS, use_wiener=True, iterations=1, window=300, dtype=np.float64):
    """audio [2, n] (or [n] / [1, n]: mono, duplicated) -> {target: [2, n]} (SourceSeparation.swift:45-175)."""
    a = np.asarray(audio, dtype=dtype)
    if a.ndim == 1:
        a = a[None]
    if a.shape[0] == 1:
        a = np.concatenate([a, a])
    names = [t for t in STEMS if t in targets]
    re, im, mag = stft(a, dtype)
    masked = np.stack([stem_forward(mag, sds[t], dtype) for t in names])
    if use_wiener and len(names) > 1:
        yre, yim = wiener(masked, re, im, iterations, window, dtype)
    else:
        yre, yim = phase_apply(masked, re, im, dtype)
    out = istft(yre, yim, a.shape[1], dtype)
    return {t: out[i] for i, t in enumerate(names)}


def clip(seed: int, n: int) -> np.ndarray:
    """Stereo test audio [2, n] float32: a few partials with slow envelopes, panned differently, over a noise floor in each channel, so
    that no bin is silent in every source (the Wiener stage divides by |det|^2 + eps^2)."""
    rng = np.random.default_rng(31000 + seed)
    t = np.arange(n) / 44100.0
    out = np.zeros((2, n))
    for k in range(6):
        f = 80.0 * (1.9 ** k) * (1.0 + 0.05 * rng.standard_normal())
        env = 0.5 + 0.5 * np.sin(2 * np.pi * (0.7 + 0.4 * k) * t + rng.uniform(0, 6.28))
        tone = 0.12 * env * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))
        pan = rng.uniform(0.2, 0.8)
        out[0] += pan * tone
        out[1] += (1.0 - pan) * tone
    out += 0.02 * rng.standard_normal((2, n))
    return np.ascontiguousarray(out, dtype=np.float32)

"""Float64 restatement of the CosyVoice3 speech tokenizer and voice-profile front ends, and its "twin": the same arithmetic in float32
with the device's bf16 rounding points.  Reference: Sources/CosyVoiceTTS/SpeechTokenizer.swift,
WhisperMelExtractor.swift, FlowMelExtractor.swift, VoiceCloning.swift:69-158, :329-345.  Independent of the device code: torch / numpy only.
"""
import math

import numpy as np
import torch

DIM, HEADS, HD, FF, MELS, FSQ, FSMN_K = 1280, 20, 64, 5120, 128, 8, 31
FSQ_SCALE = float(np.float32(0.9990000128746033))
FSQ_EDGE = math.atanh(0.5 / FSQ_SCALE)                 # |projection| at which a digit changes level
F = torch.nn.functional


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


# ---- lengths ------------------------------------------------------------------------------------------------------------------------
def whisper_frames(n):
    return (n + 400 - 400) // 160 + 1 - 1 if n > 0 else 0          # reflect pad 200 each side, frames of 400 at hop 160, last dropped


def conv_len(T):
    return (T + 2 - 3) // 2 + 1


def tokens_of(T):
    return conv_len(conv_len(T)) if T > 0 else 0


def flow_frames(n):
    N = n + 1440
    return (N - 1920) // 480 + 1 if n > 0 and N >= 1920 else 0


def resampled_length(n, src, dst):
    return n if src == dst else int(math.floor(float(n) * (float(dst) / float(src))))


def resample(x, src, dst):
    """VoiceCloning.swift:329-345: position in float64, fraction and interpolation in float32."""
    x = np.asarray(x, dtype=np.float32)
    if src == dst:
        return x.copy()
    ratio = float(dst) / float(src)
    n_out = int(math.floor(float(x.size) * ratio))
    step = 1.0 / ratio
    pos = np.arange(n_out, dtype=np.float64) * step
    idx = pos.astype(np.int64)
    frac = (pos - idx.astype(np.float64)).astype(np.float32)
    a = x[idx]
    b = np.where(idx + 1 < x.size, x[np.minimum(idx + 1, x.size - 1)], a)
    return (a * (np.float32(1.0) - frac) + b * frac).astype(np.float32)


def profile_cut(n_tokens, frames):
    return min(n_tokens, frames // 2)


# ---- mel front ends: dt = np.float64 is the oracle, np.float32 the twin ------------------------------------------------------------------
def _slaney(dt, core_form):
    """(hz_to_mel, mel_to_hz) in dt; core_form: csrc/mel_core.h's way of writing them, else the reference's."""
    f_sp, log_step = dt(200.0) / dt(3.0), np.log(dt(6.4)) / dt(27.0)
    if core_form:
        h2m = lambda hz: dt(3.0) * hz / dt(200.0) if hz < dt(1000.0) else dt(15.0) + np.log(hz / dt(1000.0)) * (dt(27.0) / np.log(dt(6.4)))
        m2h = lambda m: dt(200.0) * m / dt(3.0) if m < dt(15.0) else dt(1000.0) * np.exp((m - dt(15.0)) * (np.log(dt(6.4)) / dt(27.0)))
    else:
        h2m = lambda hz: hz / f_sp if hz < dt(1000.0) else dt(1000.0) / f_sp + np.log(hz / dt(1000.0)) / log_step
        m2h = lambda m: f_sp * m if m < dt(1000.0) / f_sp else dt(1000.0) * np.exp(log_step * (m - dt(1000.0) / f_sp))
    return h2m, m2h


def filterbank(n_mels, sr, padded, dt, core_form=False):
    """[n_mels, padded / 2 + 1] Slaney-scale, Slaney-norm triangles on the padded FFT's bin grid."""
    h2m, m2h = _slaney(dt, core_form)
    npts, nb = n_mels + 2, padded // 2 + 1
    lo, hi = h2m(dt(0.0)), h2m(dt(sr) / dt(2.0))
    if core_form:
        pts = np.array([m2h(lo + dt(i) * (hi - lo) / dt(npts - 1)) for i in range(npts)], dtype=dt)
    else:
        pts = np.array([m2h(lo + (hi - lo) * (dt(i) / dt(npts - 1))) for i in range(npts)], dtype=dt)
    hz = np.arange(nb).astype(dt) * dt(sr) / dt(padded)
    fb = np.zeros((n_mels, nb), dtype=dt)
    for m in range(n_mels):
        l, c, r = pts[m], pts[m + 1], pts[m + 2]
        if core_form:
            v = np.maximum(dt(0.0), np.minimum((hz - l) / (c - l), (r - hz) / (r - c)))
        else:
            up, dn = (hz - l) / max(c - l, dt(1e-12)), (r - hz) / max(r - c, dt(1e-12))
            v = np.where((hz >= l) & (hz <= c), up, np.where((hz > c) & (hz <= r), dn, dt(0.0)))
        fb[m] = v.astype(dt) * (dt(2.0) / (r - l))
    return fb


def _frames(x, n_fft, hop, pad, n_frames, padded, dt):
    """Reflect pad with the reference's clamps, windowed frames zero-padded to the FFT length, and their spectrum by a plain DFT in dt."""
    x = np.asarray(x, dtype=np.float32).astype(dt)
    n = x.size
    i = np.arange(pad)
    left = x[np.maximum(0, np.minimum(pad - i, n - 1))]
    right = x[np.maximum(0, n - 2 - i)]
    p = np.concatenate([left, x, right])
    win = (dt(0.5) * (dt(1.0) - np.cos(dt(2.0) * dt(np.float32(np.pi) if dt is np.float32 else np.pi) * np.arange(n_fft).astype(dt) / dt(n_fft)))).astype(dt)
    fr = np.stack([p[f * hop:f * hop + n_fft] for f in range(n_frames)]) * win if n_frames else np.zeros((0, n_fft), dtype=dt)
    ang = 2.0 * np.pi * np.outer(np.arange(n_fft), np.arange(padded // 2 + 1)) / padded
    return fr.astype(dt) @ np.cos(ang).astype(dt), -(fr.astype(dt) @ np.sin(ang).astype(dt))


def whisper_mel(pcm, twin=False):
    """WhisperMelExtractor.extract: [128, n // 160].  twin: float32, the filterbank by csrc/mel_core.h's arithmetic."""
    dt = np.float32 if twin else np.float64
    T = whisper_frames(len(pcm))
    re, im = _frames(pcm, 400, 160, 200, T, 512, dt)
    mel = (re * re + im * im) @ filterbank(128, 16000, 512, dt, core_form=twin).T
    lg = np.log10(np.maximum(mel, dt(1e-10)))
    lg = np.maximum(lg, lg.max() - dt(8.0))
    return np.ascontiguousarray(((lg + dt(4.0)) / dt(4.0)).T)


def flow_mel(pcm, twin=False):
    """FlowMelExtractor.extract: [80, n // 480]."""
    dt = np.float32 if twin else np.float64
    T = flow_frames(len(pcm))
    re, im = _frames(pcm, 1920, 480, 720, T, 2048, dt)
    mel = np.sqrt(re * re + im * im + dt(1e-9)) @ filterbank(80, 24000, 2048, dt).T
    return np.ascontiguousarray(np.log(np.maximum(mel, dt(1e-5))).T)


# ---- the tokenizer -------------------------------------------------------------------------------------------------------------------
def fsq_digits(proj):
    """[rows, 8] projections -> digits in {0, 1, 2} (SpeechTokenizer.swift:78-80), float32 as the reference."""
    h = torch.tanh(torch.as_tensor(np.array(proj, dtype=np.float32))) * torch.tensor(FSQ_SCALE, dtype=torch.float32)
    return (torch.round(h) + 1.0).to(torch.int64).numpy()


def fsq_codes(proj):
    return (fsq_digits(proj) * (3 ** np.arange(FSQ))[None]).sum(1).astype(np.int32)


def digits_of(codes):
    c = np.asarray(codes, dtype=np.int64)[:, None]
    return (c // (3 ** np.arange(FSQ))[None]) % 3


class S3Oracle:
    """SpeechTokenizerModel on one clip.  twin: float32 with bf16 GEMM operands (weights, LayerNorm outputs, stem inputs, q and k after
    RoPE, v, the attention probabilities and output, the GELU output), everything else as the device keeps it in f32."""

    def __init__(self, sd, twin=False):
        self.twin = twin
        self.dt = torch.float32 if twin else torch.float64
        self.sd = {k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(self.dt) for k, v in sd.items()}
        self.depth = 0
        while f"encoder.blocks.{self.depth}.attn.query.weight" in self.sd:
            self.depth += 1

    def r(self, x):
        return bf16(x) if self.twin else x

    def lin(self, x, stem, bias=True):
        y = self.r(x) @ self.r(self.sd[stem + ".weight"]).T
        return y + self.sd[stem + ".bias"] if bias else y

    def rope(self, x):
        T = x.shape[0]
        inv = torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(32, dtype=torch.float64) / 32.0)
        ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None]
        cs, sn = torch.cos(ang).to(self.dt)[:, None], torch.sin(ang).to(self.dt)[:, None]
        a, b = x.view(T, HEADS, HD)[..., :32], x.view(T, HEADS, HD)[..., 32:]              # split-half pairs (i, i + 32) on every head
        return torch.cat([a * cs - b * sn, b * cs + a * sn], -1)

    def stem(self, x, name):
        w = self.r(self.sd[name + ".weight"]).permute(0, 2, 1)                             # [out][k][in] -> torch's [out][in][k]
        return F.gelu(F.conv1d(self.r(x).T[None], w, self.sd[name + ".bias"], stride=2, padding=1))[0].T

    def hidden(self, mel):
        with torch.no_grad():
            h = torch.as_tensor(np.asarray(mel, dtype=np.float32)).to(self.dt).T           # [T, 128]
            h = self.stem(h, "encoder.conv1")
            h = self.stem(h, "encoder.conv2")
            T = h.shape[0]
            for i in range(self.depth):
                p = f"encoder.blocks.{i}."
                x = F.layer_norm(h, (DIM,), self.sd[p + "attn_ln.weight"], self.sd[p + "attn_ln.bias"], 1e-5)
                q, k = self.r(self.rope(self.lin(x, p + "attn.query"))), self.r(self.rope(self.lin(x, p + "attn.key", bias=False)))
                v = self.r(self.lin(x, p + "attn.value"))
                w = self.sd[p + "attn.fsmn_block.weight"].permute(0, 2, 1)                 # [1280][31][1] -> [1280][1][31]
                mem = F.conv1d(v.T[None], w, None, padding=15, groups=DIM)[0].T + v        # over the un-rotated v before the head split
                s = torch.einsum("thd,shd->hts", q, k) / 8.0
                e = torch.exp(s - s.max(-1, keepdim=True).values)
                o = torch.einsum("hts,shd->thd", self.r(e), v.view(T, HEADS, HD)) / e.sum(-1).T[..., None]
                h = h + mem
                h = h + self.lin(o.reshape(T, DIM), p + "attn.out")
                x = F.layer_norm(h, (DIM,), self.sd[p + "mlp_ln.weight"], self.sd[p + "mlp_ln.bias"], 1e-5)
                h = h + self.lin(F.gelu(self.lin(x, p + "mlp.0")), p + "mlp.2")
            return h

    def project(self, mel=None, hidden=None):
        h = self.hidden(mel) if hidden is None else hidden
        with torch.no_grad():
            y = h @ self.sd["quantizer._codebook.project_down.weight"].T + self.sd["quantizer._codebook.project_down.bias"]
        return y.numpy().astype(np.float64)

    def both(self, mel):
        h = self.hidden(mel)
        return h.numpy().astype(np.float64), self.project(hidden=h)

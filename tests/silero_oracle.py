"""Float64 numpy restatement of Silero VAD v5 (helper for the VAD tests; not collected, not imported by the product).

Reference: Sources/SpeechVAD/SileroModel.swift (network), SileroVAD.swift (processChunk, resetState, detectSpeech) and
VADPipeline.swift:117-181 (binarize + filterDurations).  Weights as synth.synth_silero_state_dict returns them (reference layouts).
The front end is vectorised over chunks and the recurrence over rows, so 32 x 30 s runs in seconds.
"""
import numpy as np

CHUNK, CTX = 512, 64
f32 = np.float32


def reflection_pad_right(x, padding=64):
    """SileroModel.swift reflectionPadRight: indices T-2 ... T-1-padding appended (last axis)."""
    T = x.shape[-1]
    if padding <= 0 or T <= padding:
        return x
    return np.concatenate([x, x[..., np.arange(T - 2, T - 2 - padding, -1)]], axis=-1)


def _conv(x, w, b, stride):
    """MLX Conv1d, channels-last x [N, T, Cin], w [out, k, in], zero padding 1 (SileroModel.swift:48-53)."""
    N, T, _ = x.shape
    xp = np.concatenate([np.zeros((N, 1, x.shape[2])), x, np.zeros((N, 1, x.shape[2]))], axis=1)
    T_out = (T + 2 - 3) // stride + 1
    out = np.empty((N, T_out, w.shape[0]))
    for t in range(T_out):
        acc = np.zeros((N, w.shape[0]))
        for k in range(3):
            acc += xp[:, t * stride + k] @ w[:, k, :].T
        out[:, t] = acc + b
    return out


class Weights:
    def __init__(self, sd):
        self.t = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}


def front(W, x576):
    """[N, 576] inputs (context ++ chunk) -> LSTM pre-gates [N, 512] = x Wx^T + bias (SileroModel.swift forward up to lstmForward)."""
    x = reflection_pad_right(np.asarray(x576, dtype=np.float64), 64)                 # [N, 640]
    frames = np.stack([x[:, f * 128:f * 128 + 256] for f in range(4)], axis=1)       # STFT Conv1d(1 -> 258, k 256, stride 128)
    s = frames @ W.t["stft.weight"][:, :, 0].T                                       # [N, 4, 258]
    h = np.sqrt(s[..., :129] ** 2 + s[..., 129:] ** 2)                               # magnitude [N, 4, 129]
    for i, stride in enumerate((1, 2, 2, 1)):                                        # encoder: Conv1d + ReLU
        h = np.maximum(_conv(h, W.t[f"encoder.{i}.weight"], W.t[f"encoder.{i}.bias"], stride), 0.0)
    return h[:, 0] @ W.t["lstm.Wx"].T + W.t["lstm.bias"]                             # addMM(bias, x, Wx^T)


def cell(W, pre, h, c):
    """lstmForward one step, gates split i, f, g, o; a nil state is the zero state."""
    ifgo = pre + h @ W.t["lstm.Wh"].T
    i, f, g, o = np.split(ifgo, 4, axis=-1)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    c = sig(f) * c + sig(i) * np.tanh(g)
    h = sig(o) * np.tanh(c)
    return h, c


def decode(W, h):
    """sigmoid(decoder(relu(h))), decoder = Conv1d(128 -> 1, k 1) with bias."""
    z = np.maximum(h, 0.0) @ W.t["decoder.weight"][0, 0] + W.t["decoder.bias"][0]
    return 1.0 / (1.0 + np.exp(-z))


def chunk_inputs(pcm, context=None):
    """detectSpeech's walk: whole 512-sample chunks, the last one zero-padded; each prefixed with the previous chunk's last 64 samples
    (zeros, or `context`, for the first).  -> [n_chunks, 576], final context [64]."""
    pcm = np.asarray(pcm, dtype=np.float32)
    nc = -(-pcm.shape[0] // CHUNK)
    padded = np.zeros(nc * CHUNK, dtype=np.float32)
    padded[:pcm.shape[0]] = pcm
    chunks = padded.reshape(nc, CHUNK)
    ctx0 = np.zeros(CTX, dtype=np.float32) if context is None else np.asarray(context, dtype=np.float32)
    ctxs = np.concatenate([ctx0[None], chunks[:-1, -CTX:]], 0) if nc else np.zeros((0, CTX), dtype=np.float32)
    final = chunks[-1, -CTX:].copy() if nc else ctx0.copy()
    return np.concatenate([ctxs, chunks], 1), final


def probs_rows(W, rows):
    """Whole buffers from the zero state: list of pcm -> (list of probs [n_chunks], list of (h, c, context) after the last chunk)."""
    ins = [chunk_inputs(r) for r in rows]
    ncs = [x.shape[0] for x, _ in ins]
    pre_all = front(W, np.concatenate([x for x, _ in ins], 0)) if sum(ncs) else np.zeros((0, 512))
    base = np.concatenate([[0], np.cumsum(ncs)])
    B, T = len(rows), max(ncs) if ncs else 0
    h, c = np.zeros((B, 128)), np.zeros((B, 128))
    probs = [np.zeros(n) for n in ncs]
    for t in range(T):
        live = np.array([t < n for n in ncs])
        idx = np.nonzero(live)[0]
        pre = pre_all[[base[b] + t for b in idx]]
        hn, cn = cell(W, pre, h[idx], c[idx])
        h[idx], c[idx] = hn, cn
        p = decode(W, hn)
        for j, b in enumerate(idx):
            probs[b][t] = p[j]
    return probs, [(h[b].copy(), c[b].copy(), ins[b][1]) for b in range(B)]


class Stream:
    """One SileroVADModel's streaming state: processChunk / resetState."""

    def __init__(self, W):
        self.W = W
        self.reset()

    def reset(self):
        self.h, self.c, self.context = np.zeros(128), np.zeros(128), np.zeros(CTX, dtype=np.float32)

    def process_chunk(self, chunk):
        chunk = np.asarray(chunk, dtype=np.float32)
        assert chunk.shape == (CHUNK,)
        x = np.concatenate([self.context, chunk])[None]
        self.context = chunk[-CTX:].copy()
        self.h, self.c = (v[0] for v in cell(self.W, front(self.W, x), self.h[None], self.c[None]))
        return float(decode(self.W, self.h[None])[0])


def binarize(probs, onset=0.5, offset=0.35, min_speech=0.25, min_silence=0.1):
    """VADPipeline.binarize + filterDurations with detectSpeech's frame duration, every step in f32 as in Swift."""
    n = len(probs)
    if n == 0:
        return []
    frame = (f32(n) * (f32(512) / f32(16000))) / f32(n)
    onset, offset, min_speech, min_silence = f32(onset), f32(offset), f32(min_speech), f32(min_silence)
    segs, inside, start = [], False, f32(0)
    for i, p in enumerate(np.asarray(probs, dtype=np.float32)):
        t = f32(i) * frame
        if not inside and p >= onset:
            inside, start = True, t
        elif inside and p < offset:
            inside = False
            segs.append((start, t))
    if inside:
        segs.append((start, f32(n) * frame))
    kept = [s for s in segs if f32(s[1] - s[0]) >= min_speech]
    if not kept:
        return []
    merged, cur = [], kept[0]
    for nxt in kept[1:]:
        if f32(nxt[0] - cur[1]) < min_silence:
            cur = (cur[0], nxt[1])
        else:
            merged.append(cur)
            cur = nxt
    merged.append(cur)
    return [(float(a), float(b)) for a, b in merged]

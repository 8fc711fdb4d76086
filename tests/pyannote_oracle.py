"""Float64 numpy statement of the pyannote PyanNet segmentation network and of the host logic of the two pipelines built on it, after the
reference (paths under Sources/SpeechVAD/).  The host logic takes the float type as a parameter: np.float64 is the plain statement,
np.float32 repeats every time and index expression in the reference's own precision and operation order (the device's segment tests
compare against that one: sample ranges and threshold decisions depend on f32 rounding)."""
import numpy as np

RATE, WINDOW, FRAMES = 16000, 160000, 589


def num_frames(n):
    """SincNet.swift:52-67 with maxPool1d :109-111: conv k 251 s 10, pool 3, conv k 5, pool 3, conv k 5, pool 3 (floors)."""
    if n < 251:
        return -1
    L0 = (n - 251) // 10 + 1
    L1 = L0 // 3 - 4
    L2 = (L1 // 3 if L1 > 0 else 0) - 4
    F = L2 // 3 if L2 > 0 else 0
    return F if F >= 1 else -1


def leaky(x):
    return np.maximum(x, 0.01 * x)                                     # SincNet.swift:127-129


def instance_norm(x, w, b):
    """x [L, C] over L: population variance, eps 1e-5, affine (SincNet.swift:89-97)."""
    m = x.mean(0, keepdims=True)
    v = ((x - m) ** 2).mean(0, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * w + b


def conv1d(x, w, b, stride=1):
    """x [L, Cin], w [Cout, K, Cin] (MLX layout), b [Cout] -> [L', Cout]."""
    K = w.shape[1]
    L = (x.shape[0] - K) // stride + 1
    idx = np.arange(L)[:, None] * stride + np.arange(K)[None, :]
    return x[idx].reshape(L, -1) @ w.reshape(w.shape[0], -1).T + b


def max_pool3(x):
    L = x.shape[0] // 3                                                # SincNet.swift:109-124: the L mod 3 tail is dropped
    return x[:3 * L].reshape(L, 3, -1).max(1)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_layer(x, wx, wh, bias):
    """BiLSTM.swift:27-59: projected = bias + x Wx^T; gates i, f, g, o; nil initial state = zeros."""
    H = wh.shape[1]
    pre = bias + x @ wx.T
    h, c = np.zeros(H), np.zeros(H)
    out = np.zeros((x.shape[0], H))
    for t in range(x.shape[0]):
        z = pre[t] + wh @ h
        i, f, g, o = sigmoid(z[:H]), sigmoid(z[H:2 * H]), np.tanh(z[2 * H:3 * H]), sigmoid(z[3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        out[t] = h
    return out


def sincnet(x, sd):
    """SincNet.swift:45-71 on one window [n] -> [F, 60]."""
    W = lambda k: np.asarray(sd[k], np.float64)
    y = instance_norm(np.asarray(x, np.float64)[:, None], W("sincnet.wav_norm.weight"), W("sincnet.wav_norm.bias"))
    for i in range(3):
        y = conv1d(y, W(f"sincnet.conv.{i}.weight"), W(f"sincnet.conv.{i}.bias"), 10 if i == 0 else 1)
        if i == 0:
            y = np.abs(y)
        y = leaky(instance_norm(max_pool3(y), W(f"sincnet.norm.{i}.weight"), W(f"sincnet.norm.{i}.bias")))
    return y


def forward(x, sd):
    """Segmentation.swift:63-84 on one window: posteriors [F, 7]."""
    W = lambda k: np.asarray(sd[k], np.float64)
    y = sincnet(x, sd)
    for l in range(4):                                                 # runBiLSTM, BiLSTM.swift:81-99
        f = lstm_layer(y, W(f"lstm_fwd.layers.{l}.Wx"), W(f"lstm_fwd.layers.{l}.Wh"), W(f"lstm_fwd.layers.{l}.bias"))
        b = lstm_layer(y[::-1], W(f"lstm_bwd.layers.{l}.Wx"), W(f"lstm_bwd.layers.{l}.Wh"), W(f"lstm_bwd.layers.{l}.bias"))[::-1]
        y = np.concatenate([f, b], 1)
    for l in range(2):
        y = leaky(y @ W(f"linear.{l}.weight").T + W(f"linear.{l}.bias"))
    z = y @ W("classifier.weight").T + W("classifier.bias")
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def speaker_probabilities(p):
    """PowersetDecoder.swift:23-31."""
    return np.stack([p[..., 1] + p[..., 4] + p[..., 5], p[..., 2] + p[..., 4] + p[..., 6], p[..., 3] + p[..., 5] + p[..., 6]], -1)


def speech_probability(p):
    return 1.0 - p[..., 0]                                             # Segmentation.swift:93-96


# ---- host logic (T = np.float64 or np.float32) ---------------------------------------------------------------------------------------
def window_positions(n, window=WINDOW, step=WINDOW // 2):
    """VADPipeline.swift:37-60 = DiarizationPipeline.swift:319-332."""
    if n <= 0:
        return []
    if n <= window:
        return [(0, n)]
    pos, s = [], 0
    while s + window <= n:
        pos.append((s, s + window))
        s += step
    if not pos or pos[-1][1] < n:
        pos.append((n - window, n))
    return pos


def aggregate_frames(window_probs, positions, n, rate=RATE, frame_duration=None, T=np.float32):
    """VADPipeline.swift:74-106."""
    fd = T(frame_duration)
    total = T(n) / T(rate)
    num = int(np.ceil(total / fd))
    if num <= 0:
        return np.zeros(0, T)
    s, c = np.zeros(num, T), np.zeros(num, T)
    for probs, (start, _) in zip(window_probs, positions):
        t0 = T(start) / T(rate)
        for f, p in enumerate(probs):
            g = int((t0 + T(f) * fd) / fd)
            if 0 <= g < num:
                s[g] = s[g] + T(p)
                c[g] = c[g] + T(1)
    return np.where(c > 0, s / np.maximum(c, T(1)), T(0)).astype(T)


def binarize(probs, onset, offset, frame_duration, T=np.float32):
    """PowersetDecoder.swift:44-72 (no duration filter)."""
    fd, on, off = T(frame_duration), T(onset), T(offset)
    segs, inside, start = [], False, T(0)
    for i, p in enumerate(probs):
        t = T(i) * fd
        if not inside and T(p) >= on:
            inside, start = True, t
        elif inside and T(p) < off:
            inside = False
            segs.append((start, t))
    if inside:
        segs.append((start, T(len(probs)) * fd))
    return segs


def filter_durations(segs, min_speech, min_silence, T=np.float32):
    """VADPipeline.swift:150-180."""
    kept = [s for s in segs if T(s[1]) - T(s[0]) >= T(min_speech)]
    if not kept:
        return []
    out, cur = [], kept[0]
    for nx in kept[1:]:
        if T(nx[0]) - T(cur[1]) < T(min_silence):
            cur = (cur[0], nx[1])
        else:
            out.append(cur)
            cur = nx
    out.append(cur)
    return out


VAD_DEFAULT = dict(onset=0.767, offset=0.377, min_speech_duration=0.136, min_silence_duration=0.067, window_duration=10.0, step_ratio=0.1)
DIAR_DEFAULT = dict(onset=0.5, offset=0.3, min_speech_duration=0.3, min_silence_duration=0.15, clustering_threshold=0.715)


def detect_speech(speech_windows, positions, n, cfg=VAD_DEFAULT, T=np.float32):
    """SpeechVAD.swift:89-140 after the model: aggregate, binarize, filter (frame duration windowDuration / 589)."""
    fd = T(cfg["window_duration"]) / T(FRAMES)
    agg = aggregate_frames(speech_windows, positions, n, RATE, fd, T)
    return filter_durations(binarize(agg, cfg["onset"], cfg["offset"], fd, T), cfg["min_speech_duration"], cfg["min_silence_duration"], T)


def cosine_distance(a, b, T=np.float32):
    """DiarizationHelpers.swift:168-182: sums in index order."""
    n = min(len(a), len(b))
    if n == 0:
        return T(2)
    dot = na = nb = T(0)
    for i in range(n):
        x, y = T(a[i]), T(b[i])
        dot = dot + x * y
        na = na + x * x
        nb = nb + y * y
    den = np.sqrt(na) * np.sqrt(nb)
    if not den > T(1e-10):
        return T(2)
    return T(1) - dot / den


def cluster(embeddings, windows, threshold, T=np.float32):
    """DiarizationHelpers.swift:83-164 -> (assignment, centroids)."""
    n = len(embeddings)
    if n == 0:
        return [], []
    cen = [np.asarray(e, T).copy() for e in embeddings]
    if n == 1:
        return [0], cen
    of, members, wins, active = list(range(n)), [[i] for i in range(n)], [{int(w)} for w in windows], set(range(n))
    while len(active) > 1:
        best, bi, bj = T(np.finfo(np.float32).max), -1, -1
        lst = sorted(active)
        for ai in range(len(lst)):
            for aj in range(ai + 1, len(lst)):
                ci, cj = lst[ai], lst[aj]
                if wins[ci] & wins[cj]:
                    continue
                d = cosine_distance(cen[ci], cen[cj], T)
                if d < best:
                    best, bi, bj = d, ci, cj
        if not (best < T(threshold)) or bi < 0:
            break
        si, sj = T(len(members[bi])), T(len(members[bj]))
        tot = T(len(members[bi]) + len(members[bj]))
        cen[bi] = ((cen[bi] * si + cen[bj] * sj) / tot).astype(T)
        for m in members[bj]:
            of[m] = bi
        members[bi] += members[bj]
        wins[bi] |= wins[bj]
        active.remove(bj)
    lst = sorted(active)
    cmap = {old: new for new, old in enumerate(lst)}
    return [cmap[of[i]] for i in range(n)], [cen[o] for o in lst]


def merge_segments(segs, min_silence, T=np.float32):
    """DiarizationHelpers.swift:11-45; speakers in ascending id, stable sorts (segs: (start, end, speaker))."""
    if not segs:
        return []
    out = []
    for spk in sorted({s[2] for s in segs}):
        v = sorted([s for s in segs if s[2] == spk], key=lambda s: s[0])
        cur = v[0]
        for nx in v[1:]:
            if T(nx[0]) - T(cur[1]) < T(min_silence):
                cur = (cur[0], nx[1], spk)
            else:
                out.append(cur)
                cur = nx
        out.append(cur)
    return sorted(out, key=lambda s: s[0])


def compact_speaker_ids(segs):
    """DiarizationHelpers.swift:48-58."""
    m = {old: new for new, old in enumerate(sorted({s[2] for s in segs}))}
    return [(s[0], s[1], m[s[2]]) for s in segs]


def trim_to_speech_mask(start, end, mask, min_duration, T=np.float32):
    """DiarizationPipeline.swift:540-565."""
    dur = T(end) - T(start)
    if not dur > 0:
        return None
    overlap, ts, te = T(0), T(end), T(start)
    for vs, ve in mask:
        os_, oe = max(T(start), T(vs)), min(T(end), T(ve))
        if os_ < oe:
            overlap = overlap + (oe - os_)
            ts, te = min(ts, os_), max(te, oe)
    if not (overlap / dur >= T(0.5)) or not (te - ts >= T(min_duration)):
        return None
    return ts, te


def solo_clips(samples, positions, tracks, cfg=DIAR_DEFAULT, T=np.float32):
    """DiarizationPipeline.swift:369-428 up to the embed call: [(window, local speaker, clip)] and the per-track binarisation.
    tracks [W, F, 3]."""
    fd = T(10.0) / T(FRAMES)
    off = T(cfg["offset"])
    clips, binar = [], {}
    for w, (start, _) in enumerate(positions):
        tr = np.asarray(tracks[w])
        for ls in range(3):
            bs = binarize(tr[:, ls], cfg["onset"], cfg["offset"], fd, T)
            binar[(w, ls)] = bs
            if not bs:
                continue
            parts = []
            for s0, s1 in bs:
                f0, f1 = int(s0 / fd), min(int(s1 / fd), tr.shape[0])
                for f in range(f0, f1):
                    if any(T(tr[f, o]) >= off for o in range(3) if o != ls):
                        continue
                    a = start + int(T(f) * fd * T(RATE))
                    b = min(start + int(T(f + 1) * fd * T(RATE)), len(samples))
                    if b > a:
                        parts.append(samples[a:b])
            clip = np.concatenate(parts) if parts else np.zeros(0, np.float32)
            if len(clip) >= RATE // 2:
                clips.append((w, ls, clip))
    return clips, binar


def diarize(samples, positions, tracks, embed_batch, mask=None, cfg=DIAR_DEFAULT, T=np.float32):
    """DiarizationPipeline.swift:301-537 given the windows' speaker tracks [W, F, 3]; embed_batch(list of clips) -> [C, 256];
    mask: the pre-filter's (start, end) list or None.  -> (segments [(start, end, speaker)], num_speakers, centroids [k, 256])."""
    empty = ([], 0, np.zeros((0, 256), np.float32))
    n = len(samples)
    if (mask is not None and not mask) or n == 0:
        return empty
    clips, binar = solo_clips(samples, positions, tracks, cfg, T)
    if not clips:
        return empty
    emb = np.asarray(embed_batch([c for _, _, c in clips]))
    assign, cents = cluster(list(emb), [w for w, _, _ in clips], cfg["clustering_threshold"], T)
    l2g = {(w, ls): a for (w, ls, _), a in zip(clips, assign)}
    segs = []
    R = T(RATE)
    for w, (start, end) in enumerate(positions):
        ws, we = T(start) / R, T(end) / R
        prev_end = T(positions[w - 1][1]) / R if w > 0 else T(0)
        next_start = T(positions[w + 1][0]) / R if w + 1 < len(positions) else T(n) / R
        own_start = (ws + prev_end) / T(2) if w > 0 else T(0)
        own_end = (we + next_start) / T(2) if w + 1 < len(positions) else T(n) / R
        for ls in range(3):
            if (w, ls) not in l2g:
                continue
            for s0, s1 in binar[(w, ls)]:
                cs, ce = max(ws + s0, own_start), min(min(ws + s1, we), own_end)
                if not (ce - cs >= T(cfg["min_speech_duration"])):
                    continue
                if mask is not None:
                    t = trim_to_speech_mask(cs, ce, mask, cfg["min_speech_duration"], T)
                    if t is not None:
                        segs.append((t[0], t[1], l2g[(w, ls)]))
                else:
                    segs.append((cs, ce, l2g[(w, ls)]))
    segs = compact_speaker_ids(sorted(segs, key=lambda s: s[0]))
    merged = merge_segments(segs, cfg["min_silence_duration"], T)
    k = len({s[2] for s in merged})
    out = np.zeros((k, 256), np.float32)
    for i in range(min(k, len(cents))):
        out[i] = cents[i]
    return merged, k, out


# ---- test clips ----------------------------------------------------------------------------------------------------------------------
def turns_clip(seed, seconds):
    """Speech-like test audio: turns of 1.5 .. 3 s taken in rotation from three synthetic voices (synth_waveform 3, 11, 23), each with a
    level that changes every 0.25 s, separated by pauses of 0.1 .. 0.5 s of digital silence."""
    from qasr import synth
    n = int(round(seconds * RATE))
    rng = np.random.default_rng(seed)
    parts, have, k = [], 0, 0
    while have < n:
        x = synth.synth_waveform([3, 11, 23][k % 3], float(rng.uniform(1.5, 3.0))).astype(np.float64)
        x *= np.repeat(rng.uniform(0.2, 1.0, len(x) // 4000 + 1), 4000)[:len(x)]
        gap = np.zeros(int(rng.uniform(0.1, 0.5) * RATE))
        parts += [x, gap]
        have += len(x) + len(gap)
        k += 1
    return np.concatenate(parts)[:n].astype(np.float32)

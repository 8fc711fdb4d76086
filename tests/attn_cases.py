"""Float64 references, inputs and bounds for the text decoder's attention and the kernels that write its K / V cache (csrc/dec_attention.hip,
csrc/dec_prefill.hip, EpiQkHeads of csrc/dec_kernels.h), shared by tests/test_attn_cases_cpu.py and tests/test_gpu_attn_cases.py.  All
arithmetic is float64 on bf16-valued inputs with the kernels' rounding points and nothing else.

Fragment-major V image (KVLayout::vf), per (slot, kv head): [key / 32][d / 16][lane 64][8] with lane = d % 16 + 16 g and element
half * 4 + j for key % 32 = half * 16 + g * 4 + j (the layout comment of vfrag_index and of decoder.hip), i.e. the key axis split as
(block, half, g, j) and the head dim as (tile, dl), stored in the order (block, tile, g, dl, half, j).

Norm + rope (norm_rope_pair of dec_rope.h): n = bf16(x * inv), y = bf16(w * n), o1 = bf16(y1 c - y2 s), o2 = bf16(y1 s + y2 c) over the
pairs (i, i + hd / 2), inv = 1 / sqrt(mean x^2 + eps).  The cos / sin tables are the engine's f32 tables, rebuilt here with the C library's
expf / cosf / sinf in the same f32 steps.  Writer bound: the device forms inv and the products in f32 (relative error below REL = 2^-18:
at most 22 f32 additions for the sum of squares, rsqrtf, one product), so an inner rounding can only land on the other neighbour where
the float64 value lies within REL of a rounding tie; such an element may move n by one ulp, y by |w| ulp(n) + ulp(y), and that is carried
through the rotation (the EpiResidBf16 candidate argument of tests/gemm_cases.py).  The rotation itself is two f32 products and one f32
sum, an ABSOLUTE error rot <= 3 * 2^-24 (|y1 c| + |y2 s|) < 2^-22 (|y1 c| + |y2 s|): where the two products cancel (|o| of 1e-6 beside
terms of 1) that is many ulps of o, so it enters the bound as a term of its own; the f32 twin (norm_rope_twin) needs it at such elements.
The final rounding is granted one ulp.  Hence
    |got - o| <= ulp_bf16(|o| + prop + rot) + prop + rot,   prop = |c| dy1 + |s| dy2  (o1),  |s| dy1 + |c| dy2  (o2),  dy = 0 away from ties.
V is copied, so it is bit-exact.

Attention.  Decode: scores s_k = scale q.k_k over the cached keys k < pos and the token's own key; P_k = bf16(exp(s_k - m)) for the
cached keys, the token's own weight exp(s_new - m) unrounded, one division: v = (sum P_k V_k + p_new v_new) / (sum P_k + p_new).  Prompt:
causal per clip, P rounded, the sum over the rounded P.  (m is the global maximum here; the kernels round P against a running maximum,
which the 2^-7 term below covers.)  For one output element with normalised weights w_k, A = sum_k w_k |V[k][d]|:
    |got - v| <= (0.5 + 2^-6) ulp_bf16(|v| + e) + e,    e = 2^-7 A + c.
2^-7 A: every P_k may round the other way than in the reference, half a bf16 ulp (at most 2^-8 of P_k) in the numerator and the same
in the denominator.  c = A * (expm1(2 ds) + 2 e_exp + 2 e_sum):
    ds     error of a score: 2^-23 (hd * max_k scale sum_d |q_d k_kd| + max |s|) for the f32 MFMA accumulation of hd exact products, the
           f32 scale and its product, plus (decode) scale * sum_d (dq_d |k_kd| + |q_d| dk_d) with dq, dk the flips the writer analysis
           above allows for the token's own q and k (zero away from ties).  A score error ds changes every weight by at most a factor
           exp(+-2 ds) after normalisation.
    e_exp  2^-21 + R 2^-22 for __expf / exp2 of an argument of magnitude up to R = the score range of the row (argument rounding and the
           hardware exp2's 1 ulp).
    e_sum  (K + 64) 2^-23 for the f32 sums over K keys (numerator and denominator), the rescales of the online softmax, the merge and the
           division.
At hd 128, K = 1055 and Gaussian inputs c is about 3e-4 A, against 7.8e-3 A for the 2^-7 term.  The honest f32 twins below (decode_twin:
per-wave online maxima, 32-key chunks, cross-wave merge; prompt_twin: 64-key tiles, one running maximum per query row) must stay inside
the bound: tests/test_attn_cases_cpu.py.

Inputs.  Beside Gaussian inputs every case runs a readout set (V[k][d] = 1 where k % hd == d) and spike sets that give one edge key a
weight of at least 0.2 (decode_inputs, prompt_inputs), so that a dropped or wrongly admitted edge key moves an output by >= 10 x the bound:
asserted on the CPU for every decode and prompt case.
"""
import ctypes
import ctypes.util
import functools
import numpy as np
from gemm_cases import bf16_round, bf16_bits, bf16_from_bits, ulp_bf16, randn_bf16

REL = 2.0 ** -18
NAN_BITS = np.array([0x7FC0, 0xFFC1, 0x7FFF, 0xFF81], np.uint16)    # quiet and signalling NaN patterns for rows past the context
SENTINEL = 0x4B4B                                                       # slots outside the batch
PROMPT, DECODE = 0, 1


# ---- fragment-major V ------------------------------------------------------------------------------------------------------------------
def vfrag_pack(V):
    """V [keys, hd] (keys % 32 == 0) -> the flat fragment image of one (slot, kv head)"""
    keys, hd = V.shape
    return np.ascontiguousarray(V.reshape(keys // 32, 2, 4, 4, hd // 16, 16).transpose(0, 4, 2, 5, 1, 3)).reshape(-1)


def vfrag_unpack(img, hd):
    keys = img.size // hd
    return np.ascontiguousarray(img.reshape(keys // 32, hd // 16, 4, 16, 2, 4).transpose(0, 4, 2, 5, 1, 3)).reshape(keys, hd)


# ---- rope tables, norm + rope -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rope_tables(theta, half, n_pos):
    """the engine's table builder (decoder.hip rope_tables_host) step for step in f32 with the C library's expf / cosf / sinf -> float64"""
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (m.expf, m.cosf, m.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    k = np.float32(-np.log(np.float64(np.float32(theta))) / half)
    cos, sin = np.empty((n_pos, half)), np.empty((n_pos, half))
    for i in range(half):
        inv = np.float32(m.expf(np.float32(i) * k))
        for p in range(n_pos):
            ang = np.float32(p) * inv
            cos[p, i], sin[p, i] = m.cosf(ang), m.sinf(ang)
    return cos, sin


def _tie_gap(t):
    """distance of t from the nearest bf16 rounding tie"""
    return 0.5 * ulp_bf16(t) - np.abs(t - bf16_round(t))


def norm_rope_ref(x, w, cos, sin, eps):
    """x [..., hd], w [hd], cos / sin [..., hd / 2] (rows of the tables) -> (o, bound, flip): the float64 value, the writer bound of the
    module docstring, and the distance an element may lie from o through a rounding flip (0 where no rounding is near a tie)"""
    half = x.shape[-1] // 2
    inv = 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + np.float64(np.float32(eps)))
    t = x * inv
    n = bf16_round(t)
    dn = np.where(_tie_gap(t) <= REL * np.abs(t), ulp_bf16(n), 0.0)
    y = bf16_round(w * n)                                   # bf16 x bf16 is exact in f32: no tie of its own
    dy = np.where(dn > 0, np.abs(w) * dn + ulp_bf16(y), 0.0)
    y1, y2, d1, d2 = y[..., :half], y[..., half:], dy[..., :half], dy[..., half:]
    r = np.concatenate([y1 * cos - y2 * sin, y1 * sin + y2 * cos], -1)
    mag = np.concatenate([np.abs(y1 * cos) + np.abs(y2 * sin), np.abs(y1 * sin) + np.abs(y2 * cos)], -1)
    prop = np.concatenate([np.abs(cos) * d1 + np.abs(sin) * d2, np.abs(sin) * d1 + np.abs(cos) * d2], -1)
    o = bf16_round(r)
    rot = 2.0 ** -22 * mag                                  # two f32 products and their f32 sum: absolute, so it counts where they cancel
    bound = ulp_bf16(np.abs(o) + prop + rot) + prop + rot
    flip = np.where((prop > 0) | (_tie_gap(r) <= rot), bound, 0.0)
    return o, bound, flip


def norm_rope_twin(x, w, cos, sin, eps):
    """an honest f32 realisation of norm_rope_pair (f32 sum of squares, f32 products, no fused multiply-add) -> bf16 values"""
    f = np.float32
    x, w, cos, sin = (np.asarray(a, f) for a in (x, w, cos, sin))
    half = x.shape[-1] // 2
    inv = (f(1) / np.sqrt((x * x).sum(-1, keepdims=True, dtype=f) / f(x.shape[-1]) + f(eps))).astype(f)
    y = _bf16_f32(w * _bf16_f32(x * inv))
    y1, y2 = y[..., :half], y[..., half:]
    return bf16_round(np.concatenate([y1 * cos - y2 * sin, y1 * sin + y2 * cos], -1).astype(np.float64))


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def _finish(v, A, ds, R, K):
    c = A * (np.expm1(2.0 * ds) + 2.0 * (2.0 ** -21 + R * 2.0 ** -22) + 2.0 * (K + 64) * 2.0 ** -23)
    e = 2.0 ** -7 * A + c
    return (0.5 + 2.0 ** -6) * ulp_bf16(np.abs(v) + e) + e


def decode_ref(q, Kc, Vc, k_new, v_new, dq=None, dk=None, drop=None, admit=False):
    """q [R, hd] query heads of one kv head, Kc / Vc [pos, hd] cached, the token's own k_new / v_new [hd] -> (v [R, hd], bound [R, hd]).
    drop = key index to leave out (pos = the token itself), admit = also count the row at `pos` (the appended key) as a cached key: the
    two defects of the mutation condition."""
    R, hd = q.shape
    pos, scale = Kc.shape[0], 1.0 / np.sqrt(hd)
    s = np.concatenate([Kc @ q.T, (q @ k_new)[None]], 0) * scale                     # [pos + 1, R]; the last row is the token itself
    keys = np.concatenate([Kc, k_new[None]], 0)
    vals = np.concatenate([Vc, v_new[None]], 0)
    rounded = np.ones(pos + 1, bool)
    rounded[pos] = False
    if admit:
        s, keys, vals, rounded = (np.concatenate([a, a[pos:pos + 1]], 0) for a in (s, keys, vals, rounded))
        rounded[-1] = True
    if drop is not None:
        keep = np.arange(s.shape[0]) != drop
        s, keys, vals, rounded = s[keep], keys[keep], vals[keep], rounded[keep]
    if s.shape[0] == 0:
        return np.full((R, hd), np.nan), np.zeros((R, hd))
    p = np.exp(s - s.max(0))
    p = np.where(rounded[:, None], bf16_round(p), p)
    den = p.sum(0)
    v = (p.T @ vals) / den[:, None]
    A = (p.T @ np.abs(vals)) / den[:, None]
    sabs = scale * (np.abs(keys) @ np.abs(q).T).max(0)
    ds = 2.0 ** -23 * (hd * sabs + np.abs(s).max(0))
    if dq is not None:
        ds = ds + scale * ((np.abs(keys) @ dq.T).max(0) + np.abs(q) @ (dk if dk is not None else 0.0 * k_new))
    return v, _finish(v, A, ds[:, None], (s.max(0) - s.min(0))[:, None], s.shape[0])


def prompt_ref(q, K, V, drop=None, admit=False):
    """q, K, V [T, hd] of one (clip, head) -> (v [T, hd], bound [T, hd]); causal.  The defects of the mutation condition: drop = a key index
    to leave out of every row, or "own" for each row's own key (a mask `key < qpos`); admit = row t also sees key t + 1 (a mask one too wide).
    A row left without a key comes out as NaN."""
    T, hd = q.shape
    scale = 1.0 / np.sqrt(hd)
    s = (q @ K.T) * scale
    vis = np.tril(np.ones((T, T), bool))
    if admit:
        vis |= np.eye(T, k=1, dtype=bool)
    if isinstance(drop, str):
        vis &= ~np.eye(T, dtype=bool)
    elif drop is not None:
        vis[:, drop] = False
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = np.where(vis, s, -np.inf)
        p = np.where(vis, bf16_round(np.exp(sm - sm.max(1, keepdims=True))), 0.0)
        den = p.sum(1, keepdims=True)
        v, A = (p @ V) / den, (p @ np.abs(V)) / den
        sabs = scale * np.where(vis, np.abs(q) @ np.abs(K).T, 0.0).max(1, keepdims=True)
        ds = 2.0 ** -23 * (hd * sabs + np.where(vis, np.abs(s), 0.0).max(1, keepdims=True))
        R = sm.max(1, keepdims=True) - np.where(vis, s, np.inf).min(1, keepdims=True)
        return v, _finish(v, A, ds, R, vis.sum(1, keepdims=True))


def prompt_twin(q, K, V, tile=64):
    """an honest f32 realisation of the prompt kernels' schedule for one (clip, head): 64-key tiles, one running maximum per query row, P
    rounded to bf16 against it, f32 sums of the rounded P, the rescale per tile, one reciprocal at the end -> bf16 values [T, hd]"""
    f = np.float32
    T, hd = q.shape
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    sc = f(1.0 / np.sqrt(f(hd)))
    m, l, o = np.full(T, -np.inf, f), np.zeros(T, f), np.zeros((T, hd), f)
    rows = np.arange(T)
    for k0 in range(0, T, tile):
        k1 = min(k0 + tile, T)
        act = rows >= k0                                        # the rows that see a key of this tile
        s = np.where(np.arange(k0, k1)[None, :] <= rows[act][:, None], (q[act] @ K[k0:k1].T).astype(f) * sc, f(-np.inf))
        mn = np.maximum(m[act], s.max(1))
        a = np.exp(m[act] - mn, dtype=f)
        p = _bf16_f32(np.exp(s - mn[:, None], dtype=f))
        l[act] = l[act] * a + p.sum(1, dtype=f)
        o[act] = o[act] * a[:, None] + (p @ V[k0:k1]).astype(f)
        m[act] = mn
    return bf16_round((o * (f(1) / l)[:, None]).astype(np.float64))


def _bf16_f32(x):
    return bf16_round(np.asarray(x, np.float64)).astype(np.float32)


def decode_twin(q, Kc, Vc, k_new, v_new, waves=8):
    """an honest f32 realisation of the decode kernel's schedule for one query head: per-wave online maxima over 32-key chunks, P rounded
    to bf16 against the running maximum, cross-wave merge with the token's own term, one division -> bf16 values [hd]"""
    f = np.float32
    hd, pos = q.shape[0], Kc.shape[0]
    q, Kc, Vc, k_new, v_new = (np.asarray(a, f) for a in (q, Kc, Vc, k_new, v_new))
    sc = f(1.0 / np.sqrt(f(hd)))
    stats = []
    for w in range(waves):
        m, l, o = f(-np.inf), f(0), np.zeros(hd, f)
        for c in range(w, (pos + 31) // 32, waves):
            k0, k1 = c * 32, min(c * 32 + 32, pos)
            s = (Kc[k0:k1] @ q).astype(f) * sc
            mn = max(m, s.max())
            a = np.exp(f(m - mn), dtype=f)
            p = _bf16_f32(np.exp(s - mn, dtype=f))
            l = f(l * a + p.sum(dtype=f))
            o = (o * a + (p @ Vc[k0:k1]).astype(f)).astype(f)
            m = mn
        stats.append((m, l, o))
    s_new = f((q @ k_new) * sc)
    mm = max([s_new] + [m for m, _, _ in stats])
    pn = np.exp(f(s_new - mm), dtype=f)
    num, den = (pn * v_new).astype(f), pn
    for m, l, o in stats:
        if m != -np.inf:
            a = np.exp(f(m - mm), dtype=f)
            num, den = (num + o * a).astype(f), f(den + l * a)
    return bf16_round((num / den).astype(np.float64))


# ---- decode cases -------------------------------------------------------------------------------------------------------------------------
CTX_LENS = (0, 1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 545)


def decode_batches(max_ctx):
    """three rows with three different context lengths per launch, over the issue's list: 0 leaves the token alone, 256 = 8 waves x 32,
    512 = the first request round at two chunks per wave, 513 / 545 start the second, max_ctx - 1 sits against the clamp"""
    lens = [n for n in CTX_LENS if n < max_ctx - 1] + [max_ctx - 1]
    while len(lens) % 3:
        lens.append(lens[len(lens) % 3 + 3])
    return [tuple(lens[i:i + 3]) for i in range(0, len(lens), 3)]


def edge_keys(pos):
    """0, pos - 1, the first and last key of the last 32-key chunk, the last key of the chunk before it, and the token itself (= pos)"""
    if pos == 0:
        return [0]
    first = (pos - 1) // 32 * 32
    return sorted({0, pos - 1, first, first - 1 if first else 0, pos})


INPUT_SETS = ("readout", "gauss", "spike")


def decode_inputs(hd, kv_heads, max_ctx, n_slots, lens, kind, spike=0, seed=0, theta=10000.0, eps=1e-6):
    """One DECODE launch.  kind: readout (V[k][d] = 1 where k % hd == d: the output reads the weights out in groups), gauss, spike (gauss
    with edge key edge_keys(pos)[spike % n] of every row aligned with query head 0 of its kv head at a weight near one half).
    -> dict with the probe's arrays (qkv, qn_w, kn_w as bf16 values; K / VF images as bits) and the float64 view of the caches"""
    rng = np.random.default_rng([seed, hd, kv_heads, max_ctx, sum(lens), INPUT_SETS.index(kind), spike])
    B, heads, half = len(lens), 2 * kv_heads, hd // 2
    nh = heads + 2 * kv_heads
    cos, sin = rope_tables(theta, half, max_ctx)
    qkv = randn_bf16(rng, (B, nh, hd))
    qn_w, kn_w = bf16_round(1.0 + 0.1 * rng.standard_normal(hd)), bf16_round(1.0 + 0.1 * rng.standard_normal(hd))
    Kf = randn_bf16(rng, (B, kv_heads, max_ctx, hd))
    Vf = randn_bf16(rng, (B, kv_heads, max_ctx, hd))
    if kind == "readout":
        Vf[:] = (np.arange(max_ctx)[:, None] % hd == np.arange(hd)[None, :]).astype(np.float64)
        for b, pos in enumerate(lens):
            qkv[b, heads + kv_heads:] = (np.arange(hd) == pos % hd).astype(np.float64)
    if kind == "spike":
        for b, pos in enumerate(lens):
            ek = edge_keys(pos)
            e = ek[spike % len(ek)]
            q, _, _ = norm_rope_ref(qkv[b, :heads], qn_w, cos[pos], sin[pos], eps)
            for kvh in range(kv_heads):
                q0 = q[2 * kvh]
                s = (Kf[b, kvh, :pos] @ q0) / np.sqrt(hd)
                if e == pos:                 # the token's own key: the k input row leans on the q input row (k = 1.5 q at full alignment, see
                    xq = qkv[b, 2 * kvh]     # kn_w below) by the cosine that puts its weight near one half
                    rho = min(1.0, max(np.log(np.exp(s).sum() + 1.0), 1.0) * np.sqrt(hd) / (1.5 * (q0 @ q0)))
                    g = rng.standard_normal(hd)
                    g -= xq * (g @ xq) / (xq @ xq)
                    qkv[b, heads + kvh] = bf16_round(rho * xq + np.sqrt(1.0 - rho * rho) * g * np.sqrt((xq @ xq) / (g @ g)))
                    continue
                s[e] = -np.inf
                target = np.log(np.exp(s - 0.0).sum() + 1.0) if pos > 1 else 1.0
                Kf[b, kvh, e] = bf16_round(q0 * (max(target, 1.0) * np.sqrt(hd) / (q0 @ q0)))
    if kind == "spike" and any(edge_keys(p)[spike % len(edge_keys(p))] == p for p in lens):
        kn_w = bf16_round(qn_w * 1.5)        # weight of the token's own key well above 0.2 at every context of the list
    Kbits = np.full((n_slots, kv_heads, max_ctx, hd), SENTINEL, np.uint16)
    VFbits = np.full((n_slots, kv_heads, max_ctx * hd), SENTINEL, np.uint16)
    nan = NAN_BITS[np.arange(max_ctx * hd).reshape(max_ctx, hd) % 4]
    for b, pos in enumerate(lens):
        for kvh in range(kv_heads):
            kb, vb = bf16_bits(Kf[b, kvh]), bf16_bits(Vf[b, kvh])
            kb[pos:], vb[pos:] = nan[pos:], nan[pos:]
            Kbits[b, kvh], VFbits[b, kvh] = kb, vfrag_pack(vb)
    return dict(hd=hd, kv_heads=kv_heads, heads=heads, max_ctx=max_ctx, n_slots=n_slots, lens=tuple(lens), theta=theta, eps=eps,
                qkv=qkv, qn_w=qn_w, kn_w=kn_w, K=Kf, V=Vf, Kbits=Kbits, VFbits=VFbits)


def decode_expect(inp, drop_edge=None, admit=False):
    """-> (v, bound [B, heads, hd], k_new, k_bound [B, kv_heads, hd], v_new [B, kv_heads, hd]); drop_edge = index into every row's edge list"""
    hd, heads, kvh_n, lens = inp["hd"], inp["heads"], inp["kv_heads"], inp["lens"]
    cos, sin = rope_tables(inp["theta"], hd // 2, inp["max_ctx"])
    B = len(lens)
    v, bound = np.empty((B, heads, hd)), np.empty((B, heads, hd))
    pos = np.asarray(lens)
    q, _, dq = norm_rope_ref(inp["qkv"][:, :heads], inp["qn_w"], cos[pos][:, None], sin[pos][:, None], inp["eps"])
    k, kb, dk = norm_rope_ref(inp["qkv"][:, heads:heads + kvh_n], inp["kn_w"], cos[pos][:, None], sin[pos][:, None], inp["eps"])
    v_new = inp["qkv"][:, heads + kvh_n:]
    for b, p in enumerate(lens):
        ek = edge_keys(p)
        drop = None if drop_edge is None else ek[drop_edge % len(ek)]
        for h in range(kvh_n):
            sl = slice(2 * h, 2 * h + 2)
            v[b, sl], bound[b, sl] = decode_ref(q[b, sl], inp["K"][b, h, :p], inp["V"][b, h, :p], k[b, h], v_new[b, h], dq[b, sl], dk[b, h],
                                                drop=drop, admit=admit)
    return v, bound, k, kb, v_new


def decode_sets(lens):
    """the input sets of one case: readout, gauss and one spike run per edge key of its longest edge list"""
    n = max(len(edge_keys(p)) for p in lens)
    return [("readout", 0), ("gauss", 0)] + [("spike", i) for i in range(n)]


# ---- prompt cases -------------------------------------------------------------------------------------------------------------------------
PROMPT_CLIPS = ((1, 2, 63), (64, 65, 127), (128, 129, 200))
SLOT_OF_CLIP = (2, 0, 1)


def prompt_edge_keys(T):
    """key 0, the first key of the clip's last 64-key tile and the last key of the tile before it (the clip's last key, T - 1, is the last
    row's own key: the first spike set)"""
    first = (T - 1) // 64 * 64
    return sorted({0, first, first - 1 if first else 0})


def prompt_sets(clips):
    """the input sets of one case: readout, gauss, and the spike sets 0 (every row's own key), 1 (the key after every row), 2 + i (edge key i
    of every clip)"""
    return [("readout", 0), ("gauss", 0)] + [("spike", i) for i in range(2 + max(len(prompt_edge_keys(T)) for T in clips))]


def prompt_inputs(hd, kv_heads, clips, kind, spike=0, max_ctx=256, n_slots=4, seed=0, theta=10000.0, eps=1e-6):
    """One PROMPT launch.  kind: readout, gauss, spike.  The spikes are set in the packed input rows, ahead of norm + rope:
      0  the k row of every position = the q row of its kv head's first query head, and kn_w = 1.5 qn_w: the rotation of q and k at one
         position cancels, so every row's own key scores 1.5 sqrt(hd) against Gaussian neighbours (weight > 0.8);
      1  the k row of position t + 1 = that q row of position t: one position of relative rotation keeps > 0.9 of that score, so the key
         one past the causal edge would take most of the weight if it were admitted;
      2 + i  edge key prompt_edge_keys(T)[i] of every clip: every q row carries a constant in the 8 dims of the 4 slowest rope pairs (which
         turn by < 0.25 rad over 200 positions), the edge key's row is that direction alone, every other k row is zero there, and kn_w is 2
         in those dims: the edge key scores about 8 (hd 32) to 10 (hd 128) against Gaussian neighbours, for every row that sees it."""
    rng = np.random.default_rng([seed, hd, kv_heads, sum(clips), INPUT_SETS.index(kind)] + ([spike] if kind == "spike" else []))
    heads, half = 2 * kv_heads, hd // 2
    nh, n_pos = heads + 2 * kv_heads, sum(clips)
    qkv = randn_bf16(rng, (n_pos, nh, hd))
    cu = np.concatenate([[0], np.cumsum(clips)]).astype(np.int32)
    pos = np.concatenate([np.arange(T) for T in clips]).astype(np.int32)
    slot = np.concatenate([np.full(T, s) for T, s in zip(clips, SLOT_OF_CLIP)]).astype(np.int32)
    if kind == "readout":
        qkv[:, heads + kv_heads:] = (pos[:, None] % hd == np.arange(hd)[None, :]).astype(np.float64)[:, None, :]
    qn_w, kn_w = bf16_round(1.0 + 0.1 * rng.standard_normal(hd)), bf16_round(1.0 + 0.1 * rng.standard_normal(hd))
    if kind == "spike" and spike == 0:
        qkv[:, heads:heads + kv_heads] = qkv[:, 0:heads:2]
        kn_w = bf16_round(1.5 * qn_w)
    elif kind == "spike" and spike == 1:
        for c in range(len(clips)):
            qkv[cu[c] + 1:cu[c + 1], heads:heads + kv_heads] = qkv[cu[c]:cu[c + 1] - 1, 0:heads:2]
        kn_w = bf16_round(1.5 * qn_w)
    elif kind == "spike":
        D = np.r_[half - 4:half, hd - 4:hd]
        qkv[:, :heads, D] = 2.0
        qkv[:, heads:heads + kv_heads, D] = 0.0
        for c, T in enumerate(clips):
            ek = prompt_edge_keys(T)
            row = cu[c] + ek[(spike - 2) % len(ek)]
            qkv[row, heads:heads + kv_heads] = 0.0
            qkv[row, heads:heads + kv_heads, D] = 1.0
        kn_w[D] = 2.0
    return dict(hd=hd, kv_heads=kv_heads, heads=heads, max_ctx=max_ctx, n_slots=n_slots, clips=tuple(clips), theta=theta, eps=eps, qkv=qkv,
                qn_w=qn_w, kn_w=kn_w, cu=cu, pos=pos, slot=slot, slot_of_clip=np.asarray(SLOT_OF_CLIP[:len(clips)], np.int32))


def prompt_writer_expect(inp, qkv=None):
    """-> (q, q_bound [n_pos, heads, hd], k, k_bound [n_pos, kv_heads, hd], v [n_pos, kv_heads, hd])"""
    hd, heads, kvh_n = inp["hd"], inp["heads"], inp["kv_heads"]
    qkv = inp["qkv"] if qkv is None else qkv
    cos, sin = rope_tables(inp["theta"], hd // 2, inp["max_ctx"])
    c, s = cos[inp["pos"]][:, None], sin[inp["pos"]][:, None]
    q, qb, _ = norm_rope_ref(qkv[:, :heads], inp["qn_w"], c, s, inp["eps"])
    k, kb, _ = norm_rope_ref(qkv[:, heads:heads + kvh_n], inp["kn_w"], c, s, inp["eps"])
    return q, qb, k, kb, qkv[:, heads + kvh_n:]


def prompt_attn_expect(inp, q, k, v, drop_edge=None, admit=False):
    """q [n_pos, heads, hd], k / v [n_pos, kv_heads, hd] as WRITTEN (the device's bits, or the reference's) -> (out, bound [n_pos, heads, hd]);
    drop_edge = "own", or an index into every clip's prompt_edge_keys"""
    out, bound = np.empty_like(q), np.empty_like(q)
    rep = inp["heads"] // inp["kv_heads"]
    for c, T in enumerate(inp["clips"]):
        r = slice(inp["cu"][c], inp["cu"][c + 1])
        ek = prompt_edge_keys(T)
        drop = drop_edge if drop_edge is None or isinstance(drop_edge, str) else ek[drop_edge % len(ek)]
        for h in range(inp["heads"]):
            out[r, h], bound[r, h] = prompt_ref(q[r, h], k[r, h // rep], v[r, h // rep], drop=drop, admit=admit)
    return out, bound


# ---- hand-over -----------------------------------------------------------------------------------------------------------------------------
HANDOVER_CLIPS = (33, 64)


def handover_prompt(hd):
    """the PROMPT half: clips of 33 and 64 keys in slots 0 and 1 of a 2-slot, 128-key cache"""
    inp = prompt_inputs(hd, 2, HANDOVER_CLIPS, "gauss", max_ctx=128, n_slots=2)
    inp["slot_of_clip"] = np.array([0, 1], np.int32)
    inp["slot"] = np.concatenate([np.full(T, c) for c, T in enumerate(HANDOVER_CLIPS)]).astype(np.int32)
    return inp


def handover_decode(inp, K_written):
    """the DECODE half at ctx_len = T over the cache of handover_prompt: K_written [n_pos, kv_heads, hd] = the key rows the prompt wrote (the
    device's values, or the reference's), V = the V rows it was given.  Kbits / VFbits are the caller's to replace with the device's images."""
    hd, heads, kv = inp["hd"], inp["heads"], inp["kv_heads"]
    dec = decode_inputs(hd, kv, inp["max_ctx"], inp["n_slots"], HANDOVER_CLIPS, "gauss", seed=7)
    dec["qn_w"], dec["kn_w"] = inp["qn_w"], inp["kn_w"]
    for b, T in enumerate(HANDOVER_CLIPS):
        rows = slice(inp["cu"][b], inp["cu"][b + 1])
        dec["K"][b, :, :T] = K_written[rows].transpose(1, 0, 2)
        dec["V"][b, :, :T] = inp["qkv"][rows, heads + kv:].transpose(1, 0, 2)
    return dec

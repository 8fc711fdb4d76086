"""Float64 references, inputs and bounds for the attention kernels of the speech-synthesis stacks, shared by
tests/test_syn_attn_cases_cpu.py and tests/test_gpu_syn_attn_cases.py: cvlm_rope_append_kernel + cvlm_attention_kernel
(csrc/llm_cosyvoice.hip), tts_cp_attn_kernel (csrc/tts_talker.hip) and vl_attention_kernel (csrc/loc_voxcpm.hip), each run alone through
qasr_syn_attn_case_probe.  All arithmetic is float64 on the inputs' exact values with the kernels' rounding points and nothing else.  No
bar comes from a device run.

Writers.  cvlm append: split-half RoPE without a norm, o1 = bf16(x1 c - x2 s), o2 = bf16(x1 s + x2 c) over the pairs (d, d + 32); the
products and their sum are f32, an ABSOLUTE error rot <= 2^-22 (|x1 c| + |x2 s|) (the rot term of tests/attn_cases.py), then one bf16
rounding granted one ulp: |got - o| <= ulp_bf16(|o| + rot) + rot (rope_ref).  V is copied: bit-exact.  The code predictor's k (and its
q, which never leaves the registers) goes through norm_rope_pair of dec_rope.h: attn_cases.norm_rope_ref and its three-rounding bound.
norm_rope_pair ROUNDS its two outputs to bf16 (bf16_round in f32), so the code predictor's q is a bf16 value exactly as if it had gone
through memory; its possible rounding flips (the `flip` of norm_rope_ref) enter the score error below as dq.  The key the launch appends
is read back from the cache, so the attention reference runs over the bits the device wrote (q of cvlm: the qr it wrote).

Attention with f32 probabilities (cvlm, cp).  Unlike the text decoder's kernels these keep p = expf(s - m) in f32: there is no 2^-7 term.
For one output element with normalised weights w_k, A = sum_k w_k |V[k][d]|, v = sum_k w_k V[k][d]:
    |got - v| <= (0.5 + 2^-6) ulp_bf16(|v| + c) + c,     c = A (expm1(2 ds) + 2 e_exp + 2 e_sum)
    ds     error of a score: 2^-23 (hd max_k scale sum_d |q_d k_kd| + max |s|) for the f32 sum of hd exact bf16 x bf16 products (64 ascending
           terms in cvlm, a pair sum and a 64-lane tree in cp) and the scale, plus scale sum_d dq_d |k_kd| for the flips of cp's q.  A score
           error ds changes every weight by at most a factor exp(+-2 ds) after normalisation.
    e_exp  2^-22 + R 2^-23: expf within two ulp, its argument s - m rounded once (R = the score range of the row).
    e_sum  (K + 64) 2^-23: the f32 sums over K keys (numerator and denominator: cvlm four per lane, a wave tree, then one term per round;
           cp ascending), the products p v, cvlm's rescales alpha = expf(m_old - m_new) of o and l once per 256-key round, the division.
The one bf16 rounding of the output is the first term.  (attn_f32p; `decode_ref` of tests/attn_cases.py rounds P to bf16, which these
kernels do not, so only its structure is reused, not its 2^-7 term.)

vl attention: f32 throughout, nothing is rounded to bf16.  RoPE at the load, q' = q1 c - q2 s | q2 c + q1 s: two f32 products and a sum,
|dq'_d| <= 2^-23 (|q1 c| + |q2 s|) per element (dk' alike); the score is one lane's fmaf chain over 128 terms and the f32 scale
1 / sqrtf(128) (granted 2^-22 relative):
    ds = scale sum_d (dq'_d |k'_d| + |q'_d| dk'_d + dq'_d dk'_d) + 2^-23 (128 scale sum_d |q'_d k'_d| + |s|) + 2^-22 |s|,
propagated through the softmax as above (every weight within exp(+-2 ds)), e_exp as above, e_sum = (S + 8) 2^-23 for the wave tree of
the denominator, the division p = e / sum and the fmaf chain over the S keys:  |got - v| <= c + 2^-23 |v|.

Inputs.  Per case: Gaussian; readout (a score that selects ONE edge key at a weight of 1 - 1e-5, V rows that name their key, so the output
is that key's V row); edge spike (an edge key at a weight of 0.2 or more over Gaussian values).  The keys past the admitted set hold NaN
patterns where the cache is untouched, and real finite data where the product has it there: the later rows of the prompt-shaped cvlm
launch, the next sequence of a vl launch.  tests/test_syn_attn_cases_cpu.py proves on every case's inputs that a dropped edge key, a key
admitted past the set, the wrong K/V head, a wrong wave's running maximum, a missing rescale, a wrong RoPE pairing, swapped cos / sin,
a misplaced append and a neighbour's norm statistics each move an output by >= 10 x the bound or break an exact check.
"""
import functools
import math
import numpy as np
import attn_cases as A
from gemm_cases import bf16_round, bf16_bits, bf16_from_bits, ulp_bf16, randn_bf16

CVLM, CP, VL = 0, 1, 2
NAN_BITS, SENTINEL = A.NAN_BITS, A.SENTINEL
F32_SENTINEL = np.float32(-7.5e7)
KINDS = ("gauss", "readout", "spike")
CVLM_THETA, CP_THETA, CP_EPS = 1e6, 1e6, 1e-6
ROUND, CHUNK = 256, 64                 # keys of one round of the cvlm sweep, and of one wave in it


def frac(got, v, bound):
    """the largest |got - v| / bound; where the bound is 0 (an output that is a sum of zeros) only an exact match counts as inside"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    d = np.abs(got - v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf)).max())


def nan_rows(n, hd):
    return NAN_BITS[np.arange(n * hd).reshape(n, hd) % 4]


def readout_v(n, hd):
    """V rows that name their key: 1 at d = k % hd, 0.5 more at d = (k / hd + hd / 2) % hd"""
    k, d = np.arange(n)[:, None], np.arange(hd)[None, :]
    return (k % hd == d) * 1.0 + ((k // hd + hd // 2) % hd == d) * 0.5


# ---- writers -------------------------------------------------------------------------------------------------------------------------------
def rope_ref(x, cos, sin, mut=None):
    """x [..., hd] bf16 values, cos / sin [..., hd / 2] -> (o, bound): the split-half rotation, one bf16 rounding.  mut: "pair" rotates
    d with d + 1, "swap_hi" swaps cos and sin in the high half"""
    half = x.shape[-1] // 2
    if mut == "pair":
        x1, x2 = x[..., 0::2], x[..., 1::2]
        r = np.empty_like(x)
        r[..., 0::2], r[..., 1::2] = x1 * cos - x2 * sin, x1 * sin + x2 * cos
        return bf16_round(r), None
    x1, x2 = x[..., :half], x[..., half:]
    hi = x1 * cos + x2 * sin if mut == "swap_hi" else x1 * sin + x2 * cos
    r = np.concatenate([x1 * cos - x2 * sin, hi], -1)
    mag = np.concatenate([np.abs(x1 * cos) + np.abs(x2 * sin), np.abs(x1 * sin) + np.abs(x2 * cos)], -1)
    o, rot = bf16_round(r), 2.0 ** -22 * mag
    return o, ulp_bf16(np.abs(o) + rot) + rot


def rope_twin(x, cos, sin):
    f = np.float32
    x, cos, sin = (np.asarray(a, f) for a in (x, cos, sin))
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return bf16_round(np.concatenate([x1 * cos - x2 * sin, x1 * sin + x2 * cos], -1).astype(np.float64))


def norm_rope_mut(x, w, cos, sin, eps, mut):
    """the code predictor's writer with a defect, float64 with the three roundings: x [..., heads, hd]; "neighbour" takes the statistics
    of the next head (cyclically; a single head has no neighbour and is exempt)"""
    ms = (x * x).mean(-1, keepdims=True)
    if mut == "neighbour":
        ms = np.roll(ms, -1, -2)
    y = bf16_round(w * bf16_round(x / np.sqrt(ms + np.float64(np.float32(eps)))))
    return rope_ref(y, cos, sin, mut if mut in ("pair", "swap_hi") else None)[0]


# ---- attention with f32 probabilities ---------------------------------------------------------------------------------------------------------
def attn_f32p(q, K, V, scale, dq=None):
    """q [R, hd], K / V [n, hd] the admitted keys -> (v, bound) [R, hd]: the module docstring's bound for f32 scores and probabilities and one
    bf16 rounding of the output"""
    hd, n = q.shape[1], K.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = (q @ K.T) * scale
        p = np.exp(s - s.max(1, keepdims=True))
        den = p.sum(1, keepdims=True)
        v, Aabs = (p @ V) / den, (p @ np.abs(V)) / den
        ds = 2.0 ** -23 * (hd * scale * (np.abs(q) @ np.abs(K).T).max(1) + np.abs(s).max(1))
        if dq is not None:
            ds = ds + scale * (dq @ np.abs(K).T).max(1)
        R = s.max(1) - s.min(1)
        c = Aabs * (np.expm1(2.0 * ds) + 2.0 * (2.0 ** -22 + R * 2.0 ** -23) + 2.0 * (n + 64) * 2.0 ** -23)[:, None]
        return v, (0.5 + 2.0 ** -6) * ulp_bf16(np.abs(v) + c) + c


def _f32(x):
    return np.asarray(x, np.float32)


def _tree(x, adjacent=False):
    """f32 sum over the last axis (64 lanes) as a butterfly: halves folded (wave_sum), or neighbours first (lane_sum)"""
    x = _f32(x)
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = (x[..., 0::2] + x[..., 1::2]) if adjacent else (x[..., :h] + x[..., h:])
    return x[..., 0]


def cvlm_twin(q, K, V, mut=None, dtype=np.float32):
    """the schedule of cvlm_attention_kernel for the rep heads of one (row, kv head): q [rep, 64], K / V [pos + 1, 64].  Rounds of 256 keys;
    a score is the sum over d ascending of the f32 products, times 1 / 8; per round and head the maximum, alpha = exp(m_old - m_new),
    p = exp(s - m), the sum of the p as the lane's four, then the wave's tree; o = o alpha + the p V in key order; o / l, one bf16 rounding.
    dtype float64 with mut: the defects of the mutation condition, "wave" (head h rescales with head h + 4's running maximum), "no_o" /
    "no_l" (o / l not rescaled at a round change); float64 without mut is the plain softmax up to summation order."""
    f = dtype
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    rep, n = q.shape[0], K.shape[0]
    m, l, o = np.full(rep, -np.inf, f), np.zeros(rep, f), np.zeros((rep, 64), f)
    with np.errstate(invalid="ignore"):
        for j0 in range(0, n, ROUND):
            Kr, Vr = K[j0:j0 + ROUND], V[j0:j0 + ROUND]
            nk = Kr.shape[0]
            s = np.zeros((rep, nk), f)
            for d in range(64):
                s = (s + (q[:, d:d + 1] * Kr[None, :, d]).astype(f)).astype(f)
            s = np.concatenate([s * f(0.125), np.full((rep, ROUND - nk), -np.inf, f)], 1)
            m_old = m.copy()
            if mut == "wave":
                m_old[:-4] = m[4:] if rep > 4 else m_old[:-4]
            m_new = np.maximum(m_old, s.max(1))
            p = np.exp(s - m_new[:, None]).astype(f)
            alpha = np.where(np.isinf(m_old), f(0), np.exp(m_old - m_new)).astype(f)
            lanes = ((p[:, 0:64] + p[:, 64:128]) + (p[:, 128:192] + p[:, 192:256])).astype(f)
            tot = _tree(lanes) if f is np.float32 else lanes.sum(1)
            l = (l * (f(1) if mut == "no_l" and j0 else alpha) + tot).astype(f)
            o = (o * (f(1) if mut == "no_o" and j0 else alpha[:, None])).astype(f)
            for jj in range(nk):
                o = (o + (p[:, jj:jj + 1] * Vr[jj][None, :]).astype(f)).astype(f)
            m = m_new
    res = (o / l[:, None]).astype(np.float64)
    return bf16_round(res) if f is np.float32 else res


def cp_twin(q, K, V):
    """tts_cp_attn_kernel for one query head: q [128], K / V [pos + 1, 128]: lane d owns the pair (d, d + 64), the score a 64-lane tree times
    the f32 scale, the global maximum, p = exp(s - m), l and o in ascending key order, o / l, one bf16 rounding"""
    f = np.float32
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    sc = f(1) / np.sqrt(f(128))
    s = (_tree((q[None, :64] * K[:, :64]).astype(f) + (q[None, 64:] * K[:, 64:]).astype(f), adjacent=True) * sc).astype(f)
    p = np.exp(s - s.max()).astype(f)
    l, o = f(0), np.zeros(128, f)
    for j in range(K.shape[0]):
        l = f(l + p[j])
        o = (o + (p[j] * V[j]).astype(f)).astype(f)
    return bf16_round((o / l).astype(np.float64))


# ---- cvlm cases ---------------------------------------------------------------------------------------------------------------------------------
CVLM_GEOMS = ((14, 2), (6, 2), (16, 1), (2, 2))       # rep 7: wave 3 serves one head; rep 3: wave 3 idle; rep 16: the limit; rep 1
CVLM_POS = {320: (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 319),
            544: (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 319, 511, 512, 513, 543)}
CHUNK_GEOM, CHUNK_CTX, CHUNK_POS = (14, 2), 320, tuple(range(224, 288))     # the product's prompt chunk: 64 rows of one slot
CHUNK_EDGES = ("own", "next", 0, 255, 256)
SLOW = np.r_[28:32, 60:64]             # the 4 slowest RoPE pairs of head_dim 64: < 2e-3 rad over 320 positions at theta 1e6


def cvlm_batches(max_ctx):
    """the positions of the list in launches of six to eight rows"""
    pos = CVLM_POS[max_ctx]
    n = -(-len(pos) // 8)
    return [tuple(pos[i::n]) for i in range(n)]


def cvlm_edge_keys(pos):
    """key 0, pos - 1, the row's own key (= pos), the first key of the 64-key chunk and of the 256-key round that hold pos, and the last
    key of the chunk and of the round before"""
    c0, r0 = pos // CHUNK * CHUNK, pos // ROUND * ROUND
    return sorted({0, pos, max(pos - 1, 0), c0, max(c0 - 1, 0), r0, max(r0 - 1, 0)})


def cvlm_sets(poss):
    n = max(len(cvlm_edge_keys(p)) for p in poss)
    return [("gauss", 0)] + [(k, i) for i in range(n) for k in ("readout", "spike")]


def chunk_sets():
    return [("gauss", 0)] + [(k, i) for i in range(len(CHUNK_EDGES)) for k in ("readout", "spike")]


def _slots(rng, rows, n_slots):
    while True:
        s = rng.permutation(n_slots)[:rows]
        if rows == 1 or not np.array_equal(s, np.sort(s)):
            return s.astype(np.int32)


def cvlm_inputs(heads, kv, max_ctx, poss, kind, edge=0, seed=0):
    """One launch of three to nine rows in slots permuted against row order (one spare slot).  readout / spike: edge key
    cvlm_edge_keys(pos)[edge % n] of every row is aligned with query head (row + edge) % rep of each kv head."""
    rng = np.random.default_rng([seed, heads, kv, max_ctx, sum(poss), len(poss), KINDS.index(kind), edge])
    rows, rep, nh = len(poss), heads // kv, heads + 2 * kv
    n_slots = rows + 1
    slot = _slots(rng, rows, n_slots)
    cos, sin = A.rope_tables(CVLM_THETA, 32, max_ctx)
    qkv = randn_bf16(rng, (rows, nh, 64))
    Kf, Vf = randn_bf16(rng, (rows, kv, max_ctx, 64)), randn_bf16(rng, (rows, kv, max_ctx, 64))
    if kind == "readout":
        Vf[:] = readout_v(max_ctx, 64)
        for r, pos in enumerate(poss):
            qkv[r, heads + kv:] = readout_v(max_ctx, 64)[pos]
    if kind != "gauss":
        boost = 12.0 if kind == "readout" else 0.0
        for r, pos in enumerate(poss):
            ek = cvlm_edge_keys(pos)
            e = ek[edge % len(ek)]
            q = rope_ref(qkv[r, :heads], cos[pos], sin[pos])[0]
            k_own = rope_ref(qkv[r, heads:heads + kv], cos[pos], sin[pos])[0]
            for g in range(kv):
                h = g * rep + (r + edge) % rep
                s = np.concatenate([Kf[r, g, :pos] @ q[h], [k_own[g] @ q[h]]]) * 0.125
                s[e] = -np.inf
                target = max(np.log(np.exp(s).sum()), 1.0) + boost if pos else 1.0 + boost
                if e == pos:             # k = a q in the input row: the rotation at one position cancels in the score
                    qkv[r, heads + g] = bf16_round(qkv[r, h] * (target * 8.0 / (qkv[r, h] @ qkv[r, h])))
                else:
                    Kf[r, g, e] = bf16_round(q[h] * (target * 8.0 / (q[h] @ q[h])))
    return _cvlm_pack(heads, kv, max_ctx, n_slots, slot, np.asarray(poss, np.int32), qkv, Kf, Vf, np.asarray(poss), cos, sin)


def _cvlm_pack(heads, kv, max_ctx, n_slots, slot, pos, qkv, Kf, Vf, filled, cos, sin, owner=None):
    """cache images: slot of row r holds Kf[r] / Vf[r] below filled[r] and NaN patterns from there up; every other slot the sentinel"""
    rows = len(pos)
    Kbits = np.full((n_slots, kv, max_ctx, 64), SENTINEL, np.uint16)
    Vbits = Kbits.copy()
    nan = nan_rows(max_ctx, 64)
    for r in (range(rows) if owner is None else owner):
        for img, src in ((Kbits, Kf), (Vbits, Vf)):
            img[slot[r]] = bf16_bits(src[r])
            img[slot[r], :, filled[r]:] = nan[filled[r]:]
    return dict(heads=heads, kv_heads=kv, max_ctx=max_ctx, n_slots=n_slots, slot=slot, pos=pos, qkv=qkv, Kbits=Kbits, Vbits=Vbits,
                cos=cos, sin=sin, out_rows=rows + 2)


def chunk_inputs(kind, edge=0, seed=0):
    """The launch shaped like the product's prompt chunk: 64 rows of ONE slot (1 of 2) at positions 224 .. 287 over 224 cached keys.  The keys
    behind a row's own position are the later rows' appends: real, finite data that must not be admitted.  readout / spike on CHUNK_EDGES:
    "own" the k row of every position = a x its first query head's q row; "next" the k row of position t + 1 = a x that q row of position t
    (one position of relative rotation keeps > 0.9 of the score); a key index: every q row carries a constant in the 8 dims of the 4 slowest
    RoPE pairs, that key's row (in the cache, or the input row that appends it) is that direction alone and every other key is zero there."""
    heads, kv = CHUNK_GEOM
    rng = np.random.default_rng([seed, 64, KINDS.index(kind), edge, 99])
    rows, rep, nh, max_ctx, p0 = len(CHUNK_POS), heads // kv, heads + 2 * kv, CHUNK_CTX, CHUNK_POS[0]
    cos, sin = A.rope_tables(CVLM_THETA, 32, max_ctx)
    qkv = randn_bf16(rng, (rows, nh, 64))
    Kf, Vf = randn_bf16(rng, (1, kv, max_ctx, 64)), randn_bf16(rng, (1, kv, max_ctx, 64))
    if kind == "readout":
        Vf[0] = readout_v(max_ctx, 64)
        qkv[:, heads + kv:] = readout_v(max_ctx, 64)[p0:p0 + rows][:, None, :]
    if kind != "gauss":
        e = CHUNK_EDGES[edge]
        amp = 2.5 if kind == "readout" else 0.75
        if e in ("own", "next"):
            src = qkv[:, 0:heads:rep] * amp                    # [rows, kv, 64]: |q|^2 / 8 = 8 on average, so a score near 8 amp
            if e == "own":
                qkv[:, heads:heads + kv] = bf16_round(src)
            else:
                qkv[1:, heads:heads + kv] = bf16_round(src[:-1])
        else:
            b = 10.0 if kind == "readout" else 4.0             # the edge key scores 8 * 2 * b / 8 = 2 b against N(0, 7 / 8)
            qkv[:, :heads, SLOW] = 2.0
            qkv[:, heads:heads + kv, SLOW] = 0.0
            Kf[0][:, :, SLOW] = 0.0
            if e < p0:
                Kf[0, :, e] = 0.0
                Kf[0, :, e, 28:32] = b
                Kf[0, :, e, 60:64] = b
            else:
                qkv[e - p0, heads:heads + kv] = 0.0
                qkv[e - p0, heads:heads + kv, 28:32] = b
                qkv[e - p0, heads:heads + kv, 60:64] = b
    slot = np.ones(rows, np.int32)
    return _cvlm_pack(heads, kv, max_ctx, 2, slot, np.asarray(CHUNK_POS, np.int32), qkv, Kf, Vf, [p0], cos, sin, owner=[0])


def cvlm_writer_expect(inp, mut=None):
    """-> (q, q_bound [rows, heads, 64], k, k_bound [rows, kv, 64], v [rows, kv, 64])"""
    heads, kv = inp["heads"], inp["kv_heads"]
    c, s = inp["cos"][inp["pos"]][:, None], inp["sin"][inp["pos"]][:, None]
    q, qb = rope_ref(inp["qkv"][:, :heads], c, s, mut)
    k, kb = rope_ref(inp["qkv"][:, heads:heads + kv], c, s, mut)
    return q, qb, k, kb, inp["qkv"][:, heads + kv:]


def cvlm_cache_expect(inp, K, V, at=None):
    """the caches after the append with the device's own K rows let through: (wantK, wantV) images to compare whole, and the written K rows
    [rows, kv, 64] as values.  at = (slot, pos) arrays: where a defective append would have put the rows instead."""
    wantK, wantV = inp["Kbits"].copy(), inp["Vbits"].copy()
    heads, kv = inp["heads"], inp["kv_heads"]
    slot, pos = (inp["slot"], inp["pos"]) if at is None else at
    got = np.empty((len(pos), kv, 64))
    flatK, flatV = wantK.reshape(-1, 64), wantV.reshape(-1, 64)
    for r in range(len(pos)):
        for g in range(kv):
            i = (slot[r] * kv + g) * inp["max_ctx"] + pos[r]
            got[r, g] = bf16_from_bits(K.reshape(-1, 64)[i])
            flatK[i] = K.reshape(-1, 64)[i]
            flatV[i] = bf16_bits(inp["qkv"][r, heads + kv + g])
    return wantK, wantV, got


def cvlm_attn_expect(inp, q, K, V, drop=None, admit=False, kvmap=None, mut=None, rows=None):
    """q [rows, heads, 64] and the caches K / V [n_slots, kv, max_ctx, 64] as WRITTEN (values) -> (out, bound [rows, heads, 64]).  The
    defects: drop = index into every row's edge list (or a list of key indices per row, None = none), admit = the cache row after the
    row's own is a key too, kvmap "mod" = head h reads K/V head h % kv_heads, mut = the round defects of cvlm_twin."""
    heads, kv, mc = inp["heads"], inp["kv_heads"], inp["max_ctx"]
    rep = heads // kv
    flatK, flatV = K.reshape(-1, 64), V.reshape(-1, 64)
    out, bound = np.full(q.shape, np.nan), np.zeros(q.shape)
    for r in (range(len(inp["pos"])) if rows is None else rows):
        pos, sl = int(inp["pos"][r]), int(inp["slot"][r])
        keys = np.arange(pos + 1)
        if drop is not None:
            d = drop[r] if isinstance(drop, (list, tuple)) else cvlm_edge_keys(pos)[drop % len(cvlm_edge_keys(pos))]
            keys = keys if d is None else keys[keys != d]
        for h0 in range(0, heads, 1 if kvmap else rep):
            hs = slice(h0, h0 + (1 if kvmap else rep))
            g = h0 % kv if kvmap else h0 // rep
            idx = (sl * kv + g) * mc + keys
            if admit:
                idx = np.append(idx, (sl * kv + g) * mc + pos + 1)
                if idx[-1] >= flatK.shape[0]:
                    continue
            if len(idx) == 0:
                continue
            if mut:
                out[r, hs] = cvlm_twin(q[r, hs], flatK[idx], flatV[idx], mut, np.float64)
            else:
                out[r, hs], bound[r, hs] = attn_f32p(q[r, hs], flatK[idx], flatV[idx], 0.125)
    return out, bound


# ---- code predictor cases -----------------------------------------------------------------------------------------------------------------------
CP_GEOMS = ((2, 2), (4, 2), (4, 1))                   # rep 1, 2, 4
CP_B = (1, 3, 17)
CP_ALONE_POS = (0, 5, 15)                             # positions at which every row is also launched alone


def cp_edge_keys(pos):
    return sorted({0, pos, max(pos - 1, 0)})


def cp_sets(pos):
    return [("gauss", 0)] + [(k, i) for i in range(len(cp_edge_keys(pos))) for k in ("readout", "spike")]


@functools.lru_cache(maxsize=None)
def cp_tables():
    return A.rope_tables(CP_THETA, 64, 16)


def _cp_scales(B, nh):
    """rows and heads 40 x apart (the norm is per head): 40 where row + head is odd"""
    b, h = np.arange(B)[:, None], np.arange(nh)[None, :]
    return np.where((b + h) % 2 == 1, 40.0, 1.0)[:, :, None]


def cp_inputs(heads, kv, B, pos, kind, edge=0, seed=0, fresh=False):
    """One launch at position pos.  The cache of row b holds Gaussian entries below pos and NaN patterns from pos up (fresh: NaN everywhere,
    the start of the product's own sequence); one spare cache row holds the sentinel.  readout / spike: edge key cp_edge_keys(pos)[edge % n]
    (edge "own": the row's own key) aligned with a query head of each kv head; the row's own key through its input row (k leaning on q
    before the norm)."""
    rng = np.random.default_rng([seed, heads, kv, B, pos, KINDS.index(kind), 7 if edge == "own" else edge, int(fresh)])
    rep, nh = heads // kv, heads + 2 * kv
    cos, sin = cp_tables()
    qn_w, kn_w = bf16_round(1.0 + 0.1 * rng.standard_normal(128)), bf16_round(1.0 + 0.1 * rng.standard_normal(128))
    qkv = bf16_round(rng.standard_normal((B, nh, 128)) * _cp_scales(B, nh))
    Kf = randn_bf16(rng, (B, kv, 16, 128), 1.0)
    Vf = bf16_round(rng.standard_normal((B, kv, 16, 128)) * _cp_scales(B, kv)[:, :, None])
    if kind == "readout":
        Vf[:] = readout_v(16, 128)
        qkv[:, heads + kv:] = readout_v(16, 128)[pos]
    if kind != "gauss":
        boost = 12.0 if kind == "readout" else 0.0
        ek = cp_edge_keys(pos)
        e = pos if edge == "own" else ek[edge % len(ek)]
        sc = 1.0 / math.sqrt(128.0)
        q = A.norm_rope_ref(qkv[:, :heads], qn_w, cos[pos], sin[pos], CP_EPS)[0]
        k_own = A.norm_rope_ref(qkv[:, heads:heads + kv], kn_w, cos[pos], sin[pos], CP_EPS)[0]
        for b in range(B):
            for g in range(kv):
                h = g * rep + (b + (0 if edge == "own" else edge)) % rep
                s = np.concatenate([Kf[b, g, :pos] @ q[b, h], [k_own[b, g] @ q[b, h]]]) * sc
                s[e] = -np.inf
                target = max(np.log(np.exp(s).sum()), 1.0) + boost if pos else 1.0 + boost
                if e == pos:             # the normed k is kn_w / qn_w x the normed q: a score near sqrt(128) at full alignment
                    xq = qkv[b, h]
                    full = (qn_w * kn_w * xq * xq).sum() / (xq * xq).mean() * sc
                    rho = min(1.0, target / full)
                    gg = rng.standard_normal(128)
                    gg -= xq * (gg @ xq) / (xq @ xq)
                    qkv[b, heads + g] = bf16_round(rho * xq + math.sqrt(1.0 - rho * rho) * gg * math.sqrt((xq @ xq) / (gg @ gg)))
                else:
                    Kf[b, g, e] = bf16_round(q[b, h] * (target / sc / (q[b, h] @ q[b, h])))
    Kbits = np.full((B + 1, kv, 16, 128), SENTINEL, np.uint16)
    Vbits = Kbits.copy()
    nan = nan_rows(16, 128)
    lo = 0 if fresh else pos
    for img, src in ((Kbits, Kf), (Vbits, Vf)):
        img[:B] = bf16_bits(src)
        img[:B, :, lo:] = nan[lo:]
    return dict(heads=heads, kv_heads=kv, B=B, pos=pos, qkv=qkv, qn_w=qn_w, kn_w=kn_w, Kbits=Kbits, Vbits=Vbits, cos=cos, sin=sin,
                eps=CP_EPS, out_rows=B + 1)


def cp_writer_expect(inp, mut=None):
    """-> (k, k_bound [B, kv, 128], v [B, kv, 128]) of cache entry pos"""
    heads, kv, pos = inp["heads"], inp["kv_heads"], inp["pos"]
    x = inp["qkv"][:, heads:heads + kv]
    k, kb, _ = A.norm_rope_ref(x, inp["kn_w"], inp["cos"][pos], inp["sin"][pos], inp["eps"])
    if mut:
        k = norm_rope_mut(x, inp["kn_w"], inp["cos"][pos], inp["sin"][pos], inp["eps"], mut)
    return k, kb, inp["qkv"][:, heads + kv:]


def cp_attn_expect(inp, K, V, drop=None, admit=False, kvmap=None, qmut=None, rows=None):
    """the caches K / V [>= B, kv, 16, 128] as WRITTEN (values) -> (out, bound [B, heads, 128]); q is the float64 norm + rope of the input row
    with its flips as dq.  drop = index into the edge list, admit = entry pos + 1 too, kvmap "mod", qmut = a defect of the q writer."""
    heads, kv, pos, B = inp["heads"], inp["kv_heads"], inp["pos"], inp["B"]
    rep = heads // kv
    q, _, dq = A.norm_rope_ref(inp["qkv"][:, :heads], inp["qn_w"], inp["cos"][pos], inp["sin"][pos], inp["eps"])
    if qmut:
        q = norm_rope_mut(inp["qkv"][:, :heads], inp["qn_w"], inp["cos"][pos], inp["sin"][pos], inp["eps"], qmut)
    keys = np.arange(pos + 1)
    if drop is not None:
        keys = keys[keys != cp_edge_keys(pos)[drop % len(cp_edge_keys(pos))]]
    if admit:
        keys = np.append(keys, pos + 1)
    out, bound = np.full((B, heads, 128), np.nan), np.zeros((B, heads, 128))
    if len(keys) == 0 or keys[-1] > 15:
        return out, bound
    for b in (range(B) if rows is None else rows):
        for h in range(heads):
            g = h % kv if kvmap else h // rep
            out[b, h:h + 1], bound[b, h:h + 1] = attn_f32p(q[b, h:h + 1], K[b, g, keys], V[b, g, keys], 1.0 / math.sqrt(128.0), dq[b, h:h + 1])
    return out, bound


# ---- vl cases -----------------------------------------------------------------------------------------------------------------------------------
VL_GEOMS = ((4, 4), (8, 2), (8, 1), (4, 2))
VL_NSEQ = (1, 3, 9)
VL_SLOW = np.r_[60:64, 124:128]        # the 4 slowest RoPE pairs of head_dim 128: < 6e-3 rad over 32 positions at theta 1e4
VL_LONG = dict(max_pos=131072, orig=8192, long_factor=[1.0 + 3.0 * i / 63.0 for i in range(64)])
VL_SCALE = np.float32(1.0) / np.sqrt(np.float32(128.0))
VL_SETS = (("gauss", 0), ("readout", 0), ("readout", 1), ("spike", 0), ("spike", 1), ("spike", 2))      # edge 0: key 0, 1: key S - 1, 2: outside


@functools.lru_cache(maxsize=None)
def vl_tables(long):
    """MiniCPMLongRoPE as csrc/loc_voxcpm.hip vloc_rope_table documents it, in double with the C library's functions, rounded to f32:
    inv_i = exp(i / 64 * -ln theta), angle = p * (1 / factor_i) * inv_i, amplitude sqrt(1 + ln(max(max_pos / 32768, 1)) / ln 32768);
    both halves of a row hold the same 64 values.  -> (cos, sin) float32 [32, 128].  long: VL_LONG, else the plain table."""
    fac = VL_LONG["long_factor"] if long else [1.0] * 64
    ratio = (VL_LONG["max_pos"] if long else 32768) / 32768.0
    amp = math.sqrt(1.0 + math.log(max(ratio, 1.0)) / math.log(32768.0))
    cos, sin = np.empty((32, 128), np.float32), np.empty((32, 128), np.float32)
    for p in range(32):
        for i in range(64):
            inv = math.exp(float(i) / 64.0 * -math.log(float(np.float32(10000.0))))
            ang = float(p) * (1.0 / float(np.float32(fac[i]))) * inv
            cos[p, i] = cos[p, 64 + i] = np.float32(math.cos(ang) * amp)
            sin[p, i] = sin[p, 64 + i] = np.float32(math.sin(ang) * amp)
    return cos, sin


def vl_inputs(S, heads, kv, n_seq, kind, edge=0, seed=0):
    """One launch: qkv f32 [n_seq, S, heads + 2 kv, 128].  readout / spike: every q row carries a constant in the 8 slow dims, the edge key's
    row is that direction alone and every other key is zero there: edge 0 key 0, edge 1 key S - 1 of every sequence; edge 2 (outside): rows
    0 and S - 1 of the EVEN sequences only, so that an odd sequence has the spikes just past both of its ends and none inside."""
    rng = np.random.default_rng([seed, S, heads, kv, n_seq, KINDS.index(kind), edge])
    nh = heads + 2 * kv
    qkv = rng.standard_normal((n_seq, S, nh, 128)).astype(np.float32)
    if kind == "readout":
        qkv[:, :, heads + kv:] = readout_v(S, 128)[None, :, None, :]
    if kind != "gauss":
        b = 10.0 if kind == "readout" else 4.0
        qkv[:, :, :heads, VL_SLOW] = 3.0
        qkv[:, :, heads:heads + kv, VL_SLOW] = 0.0
        seqs = slice(0, n_seq, 2) if edge == 2 else slice(None)
        for j in ((0, S - 1) if edge == 2 else (0,) if edge == 0 else (S - 1,)):
            qkv[seqs, j, heads:heads + kv] = 0.0
            qkv[seqs, j, heads:heads + kv, 60:64] = b
            qkv[seqs, j, heads:heads + kv, 124:128] = b
    cos, sin = vl_tables(bool((S + heads + kv) % 2))
    return dict(S=S, heads=heads, kv_heads=kv, n_seq=n_seq, qkv=qkv, cos=cos, sin=sin, out_rows=n_seq * S + 2)


def _vl_rope(x, cos, sin, mut=None):
    """x [n, S, h, 128] float64, tables [S, 128] -> (rotated, per-element error bound of the f32 rotation)"""
    c, s = cos[None, :, None, :64], sin[None, :, None, :64]
    if mut == "pair":
        x1, x2 = x[..., 0::2], x[..., 1::2]
        r = np.empty_like(x)
        r[..., 0::2], r[..., 1::2] = x1 * c - x2 * s, x2 * c + x1 * s
        return r, None
    x1, x2 = x[..., :64], x[..., 64:]
    hi = x2 * s + x1 * c if mut == "swap_hi" else x2 * c + x1 * s
    r = np.concatenate([x1 * c - x2 * s, hi], -1)
    mag = np.concatenate([np.abs(x1 * c) + np.abs(x2 * s), np.abs(x2 * c) + np.abs(x1 * s)], -1)
    return r, 2.0 ** -23 * mag


def vl_expect(inp, drop=None, admit=False, kvmap=None, rope_mut=None):
    """-> (out, bound [n_seq, S, heads, 128]) in float64.  The defects: drop = a key index left out of every row, admit = the next sequence's
    row 0 is a key too (the last sequence: exempt, NaN), kvmap "mod", rope_mut "pair" / "swap_hi" on q and k."""
    S, heads, kv, n = inp["S"], inp["heads"], inp["kv_heads"], inp["n_seq"]
    x = inp["qkv"].astype(np.float64)
    cos, sin = inp["cos"][:S].astype(np.float64), inp["sin"][:S].astype(np.float64)
    q, dq = _vl_rope(x[:, :, :heads], cos, sin, rope_mut)
    k, dk = _vl_rope(x[:, :, heads:heads + kv], cos, sin, rope_mut)
    v = x[:, :, heads + kv:]
    if rope_mut == "pair":
        dq, dk = np.zeros_like(q), np.zeros_like(k)
    if admit:
        nxt = lambda a: np.concatenate([a, np.concatenate([a[1:, :1], np.full_like(a[:1, :1], np.nan)], 0)], 1)
        k, dk, v = nxt(k), nxt(dk), nxt(v)
    if drop is not None:
        keep = np.arange(k.shape[1]) != drop
        k, dk, v = k[:, keep], dk[:, keep], v[:, keep]
    if k.shape[1] == 0:
        return np.full(q.shape, np.nan), np.zeros(q.shape)
    hmap = np.arange(heads) % kv if kvmap else np.arange(heads) // (heads // kv)
    k, dk, v = k[:, :, hmap], dk[:, :, hmap], v[:, :, hmap]                    # [n, keys, heads, 128]
    sc = float(VL_SCALE)
    with np.errstate(invalid="ignore"):
        qk = lambda a, b: np.matmul(a.transpose(0, 2, 1, 3), b.transpose(0, 2, 3, 1))             # [n, i, h, d] x [n, j, h, d] -> [n, h, i, j]
        s = qk(q, k) * sc
        sabs = qk(np.abs(q), np.abs(k)) * sc
        ds = sc * (qk(dq, np.abs(k)) + qk(np.abs(q) + dq, dk))
        ds = (ds + 2.0 ** -23 * (128 * sabs + np.abs(s)) + 2.0 ** -22 * np.abs(s)).max(-1)          # [n, h, i]
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out = np.matmul(p, v.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
        Aabs = np.matmul(p, np.abs(v).transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
        R = s.max(-1) - s.min(-1)
        c = Aabs * (np.expm1(2.0 * ds) + 2.0 * (2.0 ** -22 + R * 2.0 ** -23) + 2.0 * (k.shape[1] + 8) * 2.0 ** -23).transpose(0, 2, 1)[..., None]
        return out, c + 2.0 ** -23 * np.abs(out)


def _fma32(a, b, c):
    """fmaf on float32 arrays through float64: the product is exact there, the sum rounds twice (to 53 bits, then to 24)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def vl_twin(inp, n_max=None):
    """vl_attention_kernel in f32 for the launch's first n_max sequences (default all): the rotation as two products and a sum, a score as ONE lane's fmaf chain over
    d = 0 .. 127 times the f32 scale, exp(s - max), the denominator as a tree, p = e / sum, an output element as one lane's fmaf chain over
    the keys in order -> float32 [n_seq, S, heads, 128]"""
    f = np.float32
    S, heads, kv = inp["S"], inp["heads"], inp["kv_heads"]
    x = inp["qkv"][:n_max]
    c, s = inp["cos"][None, :S, None, :64], inp["sin"][None, :S, None, :64]
    rot = lambda a: np.concatenate([(a[..., :64] * c).astype(f) - (a[..., 64:] * s).astype(f), (a[..., 64:] * c).astype(f) + (a[..., :64] * s).astype(f)], -1).astype(f)
    hmap = np.arange(heads) // (heads // kv)
    q, k, v = rot(x[:, :, :heads]), rot(x[:, :, heads:heads + kv])[:, :, hmap], x[:, :, heads + kv:][:, :, hmap]
    qt, kt = q.transpose(0, 2, 1, 3), k.transpose(0, 2, 1, 3)                  # [n, h, S, 128]
    acc = np.zeros(qt.shape[:3] + (S,), f)
    for d in range(128):
        acc = _fma32(qt[:, :, :, None, d], kt[:, :, None, :, d], acc)
    sc = (acc * VL_SCALE).astype(f)
    e = np.exp(sc - sc.max(-1, keepdims=True)).astype(f)
    pad = np.concatenate([e, np.zeros(e.shape[:3] + (64 - S,), f)], -1)
    p = (e / _tree(pad)[..., None]).astype(f)
    vt = v.transpose(0, 2, 1, 3)                                               # [n, h, keys, 128]
    o = np.zeros(qt.shape, f)
    for j in range(S):
        o = _fma32(p[:, :, :, j:j + 1], vt[:, :, None, j, :], o)
    return o.transpose(0, 2, 1, 3)

"""Float64 references, inputs, bounds and f32 twins for the encoder-side kernels that are not the GEMM (csrc/ctc_attention.hip,
csrc/enc_kernels.hip, csrc/ctc_kernels.hip), shared by tests/test_enc_cases_cpu.py and tests/test_gpu_enc_cases.py.  All arithmetic is
float64 on bf16- / f32-valued inputs with each kernel's own rounding points and nothing else.  No term of any bound comes from a device run.

ATTENTION (unmasked inside a clip / window; q, K, V rows of one (clip, head), s_k = q.k_k / sqrt(hd), m = max_k s_k).  The three kernels
round at different points, so there are three references:
    window_attention_kernel   P_k = bf16(e_k / sum e), e_k = exp(s_k - m) (expf), the sum unrounded; v = sum P_k V_k, stored as bf16(v)
    mha_attention_kernel      P_k = bf16(exp(s_k - m)); v = sum P_k V_k / sum P_k (the ROUNDED P), one division
    mha64_attention_kernel    p_k = exp2(s_k c - m c), c = log2(e) / sqrt(hd); v = sum bf16(p_k) V_k / sum p_k (the UNROUNDED p), one division
The bound is the one of tests/attn_cases.py: with A = sum_k w_k |V[k][d]| (w = the normalised weights of the reference),
    |got - v| <= (0.5 + 2^-6) ulp_bf16(|v| + e) + e,    e = 2^-7 A + c,    c = A (expm1(2 ds) + 2 e_exp + 2 e_sum).
2^-7 A  every P_k may round the other way than in the reference (the mha kernels round against a running maximum, the window kernel after
        an f32 division): half a bf16 ulp, at most 2^-8 of P_k, on either side.
ds      error of a score: q and k are INPUTS here (no writer terms): 2^-23 (hd max_k sum_d |q_d k_kd| / sqrt(hd) + max_k |s_k|) for the f32
        MFMA accumulation of hd exact products, the f32 scale and its product.  It moves every weight by at most exp(+-2 ds).
e_exp   relative error of one exponential, R = m - min_k s_k the score range of the row, M = max_k |s_k|:
          window  expf of an f32 difference: 2^-24 R for the subtraction, under 2 ulp for expf: <= 2^-21 + R 2^-22
          mha     __expf(x) = exp2(x log2 e): the subtraction, the product (2^-24 R each) and the hardware exp2's ulp: <= 2^-21 + R 2^-22
          mha64   exp2(fma(s_raw, c, -(m_raw c))): c is an f32 constant (2^-24 relative on an argument of R log2 e), m_raw c is rounded
                  (2^-24 |m| log2 e, and |m| <= M is NOT bounded by R), the fma rounds once (2^-24 R log2 e), exp2 one ulp; times ln 2
                  for the relative error of p: <= 2^-23 + R 2^-23 + M 2^-24 <= 2^-21 + (R + M) 2^-22
e_sum   relative error of the f32 sums, K keys, T = ceil(K / 64) tiles.  A factor the kernel applies to numerator and denominator alike
        (the rescale alpha of the online softmax) cancels, only its roundings count:
          window  numerator: K f32 MFMA additions; denominator: 8 in-lane + 4 shuffle additions, the reciprocal, the product: (K + 14) 2^-24
          mha     per tile 4 in-lane + 4 lane additions and l alpha + rs (2), o alpha (1), 64 MFMA additions; the reciprocal and the
                  product at the end: (K + 11 T + 2) 2^-24
          mha64   per tile and lane 16 pair sums + 16 accumulations, one rescale of l and one of o; the half swap sum, the reciprocal and
                  the product at the end: (K + 34 T + 3) 2^-24
At 513 keys c is below 2e-4 A against 7.8e-3 A for the 2^-7 term.
Inputs per batch of packed clips: Gaussian; a readout set (V[k][d] = 1 where k % hd == d); spike sets: every q row holds 2.0 in the last 8
head dims, every K row 0 there, and ONE edge key per clip is that direction alone with a score of ln L + 1.5 (weight near 0.7 for every
query of the clip): key 0, the last key, the keys either side of every 64-key tile start (window: every 16-key boundary, which holds the
32-key ones).  The first row of the NEXT packed clip is that clip's key 0, so the key-0 set also arms the key that must not be admitted;
after the last clip the rows are NaN patterns.

ROW KERNELS.  The float64 value and a bound counted from the kernel's f32 operations (-ffp-contract=off: every product and sum rounds, an
fmaf once), u = 2^-24:
layernorm_f32p (two-pass)  a term passes through nr = ceil(D / 256) + 9 roundings on its way into a row sum (two levels inside a
    float4, one accumulation per float4 of the lane, 6 across the wave, the 1 / D):  dmean = nr u mean|x|;  the deviation d_i carries
    eta_i = dmean + u |d_i|.  The TRUE deviations sum to zero, so an error of the mean enters the sum of squares only in second order:
    dvar = dmean^2 + (nr + 4) u (var + dmean^2) + 2 u dmean mean|d|  (two roundings per square, nr for the sum);
    rho = dvar / (2 (var + eps)) + 4 u (the sum with eps, rsqrtf);  e_y = |g| rstd (eta_i + |d_i| (rho + 3 u)) + u (|g d_i rstd| + |y|).
    At mean 100 and unit deviation e_y is 1e-4 |g|, nearly all of it the shift dmean; a one-pass variance is off by 1e4 u per rounding
    RELATIVE to a variance of 1, which moves the tails of a row by tens of that bound (tests/test_enc_cases_cpu.py).
    bf16 out: (0.5 + 2^-6) ulp_bf16(|v| + e) + e, e = e_y; through GELU e = 1.13 e_y + 2^-21 |y| (1.13 = the largest slope of GELU;
    gelu_erf is Abramowitz-Stegun 7.1.26, |erfc error| <= 1.5e-7, i.e. 0.75e-7 |y|, plus under 10 f32 ulps of a factor <= 1 for its
    evaluation, 3e-7 |y|: together below 2^-21 |y|).  f32 out: e + u |v|.
w2v_conv0  xs = (x - mean) inv: 2 u |xs|;  v_c = fma chain of 10 from the bias: e_v = 13 u (|bias| + sum |w xs|);  LayerNorm over the C
    channels with the ONE-PASS variance E[v^2] - mu^2, as the reference computes it: dmu = mean e_v + 24 u mean|v|,
    dE2 = mean(2 |v| e_v) + 25 u E2,  dvar = dE2 + 2 |mu| dmu + 2 u (E2 + mu^2): the conditioning E2 / var of that formula times the f32
    sum error;  rho = dvar / (2 (var + eps)) + 4 u;  e_y = |g| rstd (e_v + dmu + |v - mu| (rho + 3 u)) + u (|g (v - mu) rstd| + |y|);
    bf16 through GELU as above.  The inputs keep dvar / var below 2^-10 (asserted), where first order in rho is enough.
wave_stats  mean and 1 / sqrt(max(0, E[x^2] - mean^2) + eps) from f32 sums of depth ceil(n / 1024) + 23: dmean = depth u mean|x|,
    dE2 = (depth + 1) u E2, dvar = dE2 + 2 |mean| dmean + 2 u (E2 + mean^2); inv_std lies between the values at var -+ dvar (clamped at 0),
    plus 3 u of it for the sum with eps, sqrtf and the division.  A DC offset of 50 deviations makes E2 / var = 2501 and the bound that
    much wider.
conv1  fma chain of 9 from the bias: e = 10 u (|bias| + sum |w x|), bf16 through GELU as above; columns ow >= w1 are +0.
argmax, cast, conv rows, frame info are exact.
"""
import functools
import math
import numpy as np
from gemm_cases import bf16_round, bf16_bits, bf16_from_bits, ulp_bf16, randn_bf16, gelu, GELU_SLOPE
from attn_cases import NAN_BITS, SENTINEL, _bf16_f32

U = 2.0 ** -24
(MHA, WINDOW, LN_BF16, LN_GELU_BF16, LN_GELU_F32, CONV0, WAVE_STATS, CONV1, ARGMAX, CAST, CONV_ROWS, FRAME_INFO) = range(12)
SENTINEL_F32 = np.float32(-7.25e9)
HEADS = 3

# ---- attention: cases --------------------------------------------------------------------------------------------------------------------
# every length of the issue's list once, short clips beside long ones, unaligned cu offsets; max_len = the longest clip of the batch
MHA_BATCHES = ((1, 513, 15, 64, 17), (300, 16, 257, 31, 33), (256, 63, 129, 32, 65), (127, 255, 128, 191, 192))
WINDOW_BATCHES = ((1, 128, 15, 97, 17), (104, 16, 65, 31, 33), (96, 63, 127, 32, 64))
ENCODER_WINDOWS = (104, 104, 98)                    # what the Qwen3 encoder launches for 2350 mel frames
PAIRS8 = (2, (33, 64, 17, 129))                     # heads, clips: exactly 8 (clip, head) pairs
PAIRS9 = (3, (65, 1, 130))                          # exactly 9
KINDS = ("window", "mha", "mha64")


def mha_kind(hd, form):
    return "mha64" if hd == 64 and form >= 1 else "mha"


def query_group(kind, form=1):
    """rows of one wave's query group"""
    return 32 if kind == "mha64" else 16


def edge_keys(L, tile):
    return sorted({0, L - 1} | {k for t in range(tile, L, tile) for k in (t - 1, t)})


def attn_sets(clips, tile):
    n = max(len(edge_keys(L, tile)) for L in clips)
    return [("readout", 0), ("gauss", 0)] + [("spike", i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def attn_inputs(clips, heads, hd, kind, spike, tile, extra=3, seed=0):
    """-> (qkv values [rows, 3, heads, hd] float64, bits [rows + extra, 3 * heads * hd] with NaN patterns past the last clip, cu)"""
    rng = np.random.default_rng([seed, hd, heads, sum(clips), len(clips), ("readout", "gauss", "spike").index(kind), spike])
    rows = sum(clips)
    cu = np.concatenate([[0], np.cumsum(clips)]).astype(np.int32)
    qkv = randn_bf16(rng, (rows, 3, heads, hd))
    if kind == "readout":
        for c, L in enumerate(clips):
            qkv[cu[c]:cu[c + 1], 2] = (np.arange(L)[:, None] % hd == np.arange(hd)[None, :]).astype(np.float64)[:, None, :]
    if kind == "spike":
        D8 = np.arange(hd - 8, hd)
        qkv[:, 0][..., D8] = 2.0
        qkv[:, 1][..., D8] = 0.0
        for c, L in enumerate(clips):
            ek = edge_keys(L, tile)
            row = cu[c] + ek[spike % len(ek)]
            qkv[row, 1] = 0.0
            qkv[row, 1][..., D8] = bf16_round((math.log(L) + 1.5) * math.sqrt(hd) / 16.0)
    bits = np.empty((rows + extra, 3 * heads * hd), np.uint16)
    bits[:rows] = bf16_bits(qkv).reshape(rows, -1)
    bits[rows:] = NAN_BITS[np.arange(extra * 3 * heads * hd).reshape(extra, -1) % 4]
    qkv.setflags(write=False)
    bits.setflags(write=False)
    return qkv, bits, cu


# ---- attention: reference, bound, mutations --------------------------------------------------------------------------------------------------
def attn_ref(q, K, V, kind, vis=None):
    """q [L, hd], K / V [Lk, hd] of one (clip, head), vis [L, Lk] = the keys each row sees (None: all) -> (v, bound) [L, hd]"""
    L, hd = q.shape
    Lk = K.shape[0]
    scale = 1.0 / math.sqrt(hd)
    vis = np.ones((L, Lk), bool) if vis is None else vis
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = (q @ K.T) * scale
        sm = np.where(vis, s, -np.inf)
        m = sm.max(1, keepdims=True)
        p = np.where(vis, np.exp(sm - m), 0.0)
        if kind == "window":
            P, den = bf16_round(p / p.sum(1, keepdims=True)), 1.0
        elif kind == "mha":
            P = bf16_round(p)
            den = P.sum(1, keepdims=True)
        else:
            P, den = bf16_round(p), p.sum(1, keepdims=True)
        v, A = (P @ V) / den, (P @ np.abs(V)) / den
        sabs = scale * np.where(vis, np.abs(q) @ np.abs(K).T, 0.0).max(1, keepdims=True)
        M = np.where(vis, np.abs(s), 0.0).max(1, keepdims=True)
        ds = 2.0 ** -23 * (hd * sabs + M)
        R = m - np.where(vis, s, np.inf).min(1, keepdims=True)
        Kn = vis.sum(1, keepdims=True)
        T = -(-Kn // 64)
        e_exp = 2.0 ** -21 + (R + (M if kind == "mha64" else 0.0)) * 2.0 ** -22
        e_sum = U * {"window": Kn + 14, "mha": Kn + 11 * T + 2, "mha64": Kn + 34 * T + 3}[kind]
        e = A * (2.0 ** -7 + np.expm1(2.0 * ds) + 2.0 * e_exp + 2.0 * e_sum)
        return v, (0.5 + 2.0 ** -6) * ulp_bf16(np.abs(v) + e) + e


MUTATIONS = ("last_key", "admit_next", "last_tile", "tile2_first", "ragged_group")


def mutation_vis(name, L, tile, group):
    """the keys each row of a clip of L sees under a defect, [L, L + 1] (column L = the row after the clip), or None where the defect
    does not exist at this length"""
    vis = np.ones((L, L + 1), bool)
    vis[:, L] = False
    if name == "last_key":
        vis[:, L - 1] = False
    elif name == "admit_next":
        vis[:, L] = True
    elif name == "last_tile":
        if L <= tile or L % tile == 0:
            return None
        vis[:, L // tile * tile:L] = False
    elif name == "tile2_first":
        if L <= tile:
            return None
        vis[:, tile] = False
    elif name == "ragged_group":
        if L % group == 0:
            return None
        vis[(L - 1) // group * group:, L - 1] = False
    if not vis.any(1).all():
        return None                                     # a row left without a key (L = 1, its only key dropped): nothing to compare
    return vis


def attn_expect(qkv, cu, kind, mutation=None, tile=64, group=16, nan_row=None):
    """the whole packed batch -> (v, bound [rows, heads, hd]); under a mutation the defective value (NaN where a NaN row was admitted)"""
    rows, _, heads, hd = qkv.shape
    v, b = np.empty((rows, heads, hd)), np.empty((rows, heads, hd))
    for c in range(len(cu) - 1):
        r = slice(cu[c], cu[c + 1])
        L = cu[c + 1] - cu[c]
        for h in range(heads):
            q, K, V = qkv[r, 0, h], qkv[r, 1, h], qkv[r, 2, h]
            if mutation is None:
                v[r, h], b[r, h] = attn_ref(q, K, V, kind)
                continue
            vis = mutation_vis(mutation, L, tile, group)
            if vis is None:
                v[r, h], b[r, h] = attn_ref(q, K, V, kind)
                continue
            if not vis[:, L].any():
                v[r, h], b[r, h] = attn_ref(q, K, V, kind, vis[:, :L])
                continue
            nxt = qkv[cu[c + 1]] if cu[c + 1] < rows else np.full((3, heads, hd), np.nan)
            v[r, h], b[r, h] = attn_ref(q, np.concatenate([K, nxt[1, h][None]]), np.concatenate([V, nxt[2, h][None]]), kind, vis)
    return v, b


@functools.lru_cache(maxsize=None)
def attn_expect_cached(clips, heads, hd, set_kind, spike, tile, kind):
    qkv, _, cu = attn_inputs(clips, heads, hd, set_kind, spike, tile)
    v, b = attn_expect(qkv, cu, kind)
    v.setflags(write=False)
    b.setflags(write=False)
    return v, b


# ---- attention: honest f32 twins --------------------------------------------------------------------------------------------------------------
def _tree16(x):
    """sum over the last axis (16 lanes) as four butterfly steps"""
    while x.shape[-1] > 1:
        x = (x[..., 0::2] + x[..., 1::2]).astype(np.float32)
    return x[..., 0]


def window_twin(q, K, V):
    """window_attention_kernel: all scores of a row in registers, expf, in-lane sums over the 16-key tiles then over the 16 lanes, one
    reciprocal, P = bf16(e * (1 / sum)), f32 MFMA sum, bf16 store"""
    f = np.float32
    L, hd = q.shape
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    s = (q @ K.T).astype(f) * f(1.0 / np.sqrt(f(hd)))
    e = np.exp(s - s.max(1, keepdims=True), dtype=f)
    pad = np.zeros((L, 128), f)
    pad[:, :L] = e
    lanes = np.zeros((L, 16), f)
    for kt in range(8):
        lanes = (lanes + pad[:, kt * 16:kt * 16 + 16]).astype(f)
    inv = (f(1) / _tree16(lanes)).astype(f)
    P = _bf16_f32((e * inv[:, None]).astype(f))
    return bf16_round((P @ V).astype(f).astype(np.float64))


def mha_twin(q, K, V):
    """mha_attention_kernel: 64-key tiles, a running maximum per row, P = bf16(__expf(s - m)), the row sum over the ROUNDED P, rescale
    per tile, one reciprocal"""
    f = np.float32
    L, hd = q.shape
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    sc = f(1.0 / np.sqrt(f(hd)))
    m, l, o = np.full(L, -np.inf, f), np.zeros(L, f), np.zeros((L, hd), f)
    for k0 in range(0, L, 64):
        s = (q @ K[k0:k0 + 64].T).astype(f) * sc
        mn = np.maximum(m, s.max(1))
        a = np.exp(m - mn, dtype=f)
        p = _bf16_f32(np.exp(s - mn[:, None], dtype=f))
        l = (l * a + p.sum(1, dtype=f)).astype(f)
        o = (o * a[:, None] + (p @ V[k0:k0 + 64]).astype(f)).astype(f)
        m = mn
    return bf16_round((o * (f(1) / l)[:, None]).astype(f).astype(np.float64))


def mha64_twin(q, K, V):
    """mha64_attention_kernel: 64-key tiles, the running maximum in RAW score units, p = exp2(fma(s_raw, c, -(m c))) with the f32 constant
    c = scale * log2(e), the row sum over the UNROUNDED p, P = bf16(p) for the product, one reciprocal"""
    f = np.float32
    L, hd = q.shape
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    c = f(f(1.0 / np.sqrt(f(hd))) * f(1.4426950408889634))
    m, l, o = np.full(L, -np.inf, f), np.zeros(L, f), np.zeros((L, hd), f)
    for k0 in range(0, L, 64):
        s = (q @ K[k0:k0 + 64].T).astype(f)
        mn = np.maximum(m, s.max(1))
        with np.errstate(invalid="ignore"):
            a = np.where(m == -np.inf, f(0), np.exp2(((m - mn) * c).astype(f), dtype=f)).astype(f)
        mc = (mn * c).astype(f)
        arg = (s.astype(np.float64) * np.float64(c) - mc[:, None].astype(np.float64)).astype(f)        # one rounding: the fma
        p = np.exp2(arg, dtype=f)
        l = (l * a + p.sum(1, dtype=f)).astype(f)
        o = (o * a[:, None] + (_bf16_f32(p) @ V[k0:k0 + 64]).astype(f)).astype(f)
        m = mn
    return bf16_round((o * (f(1) / l)[:, None]).astype(f).astype(np.float64))


TWINS = {"window": window_twin, "mha": mha_twin, "mha64": mha64_twin}


# ---- f32 GELU of the device (common.h gelu_erf), for the twins ------------------------------------------------------------------------------------
def gelu_erf_f32(x):
    f = np.float32
    x = np.asarray(x, f)
    z = (np.abs(x) * f(0.70710678118654752440)).astype(f)
    t = (f(1) / (f(0.3275911) * z + f(1)).astype(f)).astype(f)
    p = (f(1.061405429) * t + f(-1.453152027)).astype(f)
    for cst in (1.421413741, -0.284496736, 0.254829592):
        p = (p * t + f(cst)).astype(f)
    erfc = ((p * t).astype(f) * np.exp2(((f(-1.4426950408889634) * z).astype(f) * z).astype(f), dtype=f)).astype(f)
    return ((f(0.5) * x).astype(f) * np.where(x >= 0, f(2) - erfc, erfc).astype(f)).astype(f)


def _out_bound(v, y, e_y, form):
    """form 0: bf16(y); 1: bf16(gelu(y)); 2: f32 gelu(y)"""
    if form == 0:
        return (0.5 + 2.0 ** -6) * ulp_bf16(np.abs(v) + e_y) + e_y
    e = GELU_SLOPE * e_y + 2.0 ** -21 * np.abs(y)
    if form == 1:
        return (0.5 + 2.0 ** -6) * ulp_bf16(np.abs(v) + e) + e
    return e + U * np.abs(v) + 1e-30


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (4, 64, 252, 256, 260, 512, 896, 1024, 1280, 2044, 2048)
LN_FORMS = {LN_BF16: 0, LN_GELU_BF16: 1, LN_GELU_F32: 2}
LN_EPS = 1e-5


def ln_rpw(D):
    """rows per wave of the width's instantiation (layernorm_f32p_rows_kernel: 8 / (D / 256); the generic kernel: 1)"""
    return {256: 8, 512: 4, 1024: 2, 2048: 1}.get(D, 1)


def ln_row_counts(D):
    r = ln_rpw(D)
    return sorted({1, 3, 4, 5, 4 * r - 1, 4 * r, 4 * r + 1})


@functools.lru_cache(maxsize=None)
def ln_inputs(D, rows, kind, seed=0):
    """kind "mixed": row r has mean (r % 3 - 1) * 2 and deviation 0.5 + r % 4; "mean100": mean 100, unit deviation.
    -> x f32 [rows + 1, D] (the row after the last is NaN), gamma, beta f32 [D]"""
    rng = np.random.default_rng([seed, D, rows, kind == "mean100"])
    r = np.arange(rows)[:, None]
    x = rng.standard_normal((rows, D))
    x = 100.0 + x if kind == "mean100" else (r % 3 - 1) * 2.0 + (0.5 + r % 4) * x
    x = np.concatenate([x, np.full((1, D), np.nan)]).astype(np.float32)
    g = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    b = (0.3 * rng.standard_normal(D)).astype(np.float32)
    for a in (x, g, b):
        a.setflags(write=False)
    return x, g, b


def ln_ref(x, g, b, form, eps=LN_EPS, div=None, shift_stats=False):
    """x [rows, D] -> (v, bound).  Defects: div = divide the sums by this width instead of D; shift_stats = row r takes the statistics of
    row min(r + 1, rows - 1) (the clamped duplicate of layernorm_f32p_rows_kernel leaking into a stored row)"""
    x, g, b = (np.asarray(a, np.float64) for a in (x, g, b))
    D = x.shape[1]
    n = float(div or D)
    eps = float(np.float32(eps))
    mean = x.sum(1, keepdims=True) / n
    d = x - mean
    var = (d * d).sum(1, keepdims=True) / n
    if shift_stats:
        idx = np.minimum(np.arange(x.shape[0]) + 1, x.shape[0] - 1)
        mean, var = mean[idx], var[idx]
        d = x - mean
    rstd = 1.0 / np.sqrt(var + eps)
    y = d * rstd * g + b
    nr = -(-D // 256) + 9
    dmean = nr * U * np.abs(x).mean(1, keepdims=True)
    eta = dmean + U * np.abs(d)
    dvar = dmean ** 2 + (nr + 4) * U * (var + dmean ** 2) + 2 * U * dmean * np.abs(d).mean(1, keepdims=True)
    rho = dvar / (2.0 * (var + eps)) + 4 * U
    e_y = np.abs(g) * rstd * (eta + np.abs(d) * (rho + 3 * U)) + U * (np.abs(g * d * rstd) + np.abs(y))
    v = y if form == 0 else gelu(y)
    return v, _out_bound(v, y, e_y, form)


def _lane_sum64(s):
    """[rows, 64] f32 -> [rows]: six butterfly steps"""
    while s.shape[-1] > 1:
        s = (s[..., 0::2] + s[..., 1::2]).astype(np.float32)
    return s[..., 0]


def ln_twin(x, g, b, form, eps=LN_EPS, one_pass=False):
    """the kernels in numpy f32: lane l holds the float4 l + 64 i, ((x + y) + (z + w)) per float4, sequential over i, a butterfly over the
    64 lanes, two passes (one_pass = the defect: E[x^2] - mean^2 from the same order of sums)"""
    f = np.float32
    x, g, b = (np.asarray(a, f) for a in (x, g, b))
    rows, D = x.shape
    nv = -(-D // 256)
    pad = np.zeros((rows, nv * 256), f)
    pad[:, :D] = x
    valid = np.zeros(nv * 256, bool)
    valid[:D] = True
    valid = valid.reshape(nv, 64, 4)

    def total(a):
        a = a.reshape(rows, nv, 64, 4)
        s = np.zeros((rows, 64), f)
        for i in range(nv):
            s = (s + ((a[:, i, :, 0] + a[:, i, :, 1]).astype(f) + (a[:, i, :, 2] + a[:, i, :, 3]).astype(f)).astype(f)).astype(f)
        return _lane_sum64(s)

    rows_kernel = D in (256, 512, 1024, 2048)
    scale = (lambda t: (t * f(1.0 / D)).astype(f)) if rows_kernel else (lambda t: (t / f(D)).astype(f))
    mean = scale(total(pad))[:, None]
    if one_pass:
        var = (scale(total((pad * pad).astype(f))) - (mean[:, 0] * mean[:, 0]).astype(f)).astype(f)
    else:
        d = np.where(valid.reshape(-1)[None, :], (pad - mean).astype(f), f(0))
        var = scale(total((d * d).astype(f)))
    rstd = (f(1) / np.sqrt((var + f(eps)).astype(f), dtype=f)).astype(f)[:, None]
    y = ((((x - mean).astype(f) * rstd).astype(f) * g).astype(f) + b).astype(f)
    if form == 0:
        return bf16_round(y.astype(np.float64))
    o = gelu_erf_f32(y).astype(np.float64)
    return bf16_round(o) if form == 1 else o


# ---- w2v conv0 ----------------------------------------------------------------------------------------------------------------------------------
CONV0_CASES = ((512, (130, 17, 64)), (64, (1, 65, 16)), (40, (15, 63, 130)), (1024, (16, 1, 17)))      # channels, frames of three clips
CONV0_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def conv0_inputs(C, frames, seed=0):
    """three ragged clips at unaligned pcm offsets, their output rows packed with a gap of 2 sentinel rows after the FIRST clip (whose
    n_out is far below max_out in the first case); stats are given, not computed.  Samples past a clip's 5 n + 5 are NaN."""
    rng = np.random.default_rng([seed, C, sum(frames)])
    B = len(frames)
    ns = [5 * n + 5 for n in frames]
    pcm_off = np.cumsum([3] + [n + 3 for n in ns[:-1]]).astype(np.int64)
    n_in = int(pcm_off[-1] + ns[-1] + 7)
    pcm = np.full(n_in, np.nan, np.float32)
    stats = np.empty((B, 2), np.float32)
    for b in range(B):
        pcm[pcm_off[b]:pcm_off[b] + ns[b]] = (0.02 * (b + 1) + 0.1 * (b + 1) * rng.standard_normal(ns[b])).astype(np.float32)
        stats[b] = (0.02 * (b + 1), 1.0 / (0.1 * (b + 1)))
    frame_off = np.array([0, frames[0] + 2, frames[0] + 2 + frames[1]], np.int32)
    rows = int(frame_off[-1] + frames[-1])
    w = (rng.standard_normal((C, 10)) / np.sqrt(10.0)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(C)).astype(np.float32)
    g = (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    be = (0.3 * rng.standard_normal(C)).astype(np.float32)
    out = dict(C=C, frames=frames, pcm=pcm, pcm_off=pcm_off, stats=stats, frame_off=frame_off, n_out=np.asarray(frames, np.int32), rows=rows,
               w=w, bias=bias, g=g, be=be)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def conv0_ref(inp, tap_shift=False, div=None):
    """-> (v, bound [rows, C], written [rows] bool).  Defects: tap_shift = tap 0 reads the sample after its own; div = the LayerNorm sums
    divided by this width instead of C (the padded thread count)"""
    C, eps = inp["C"], float(np.float32(CONV0_EPS))
    w, bias, g, be = (np.asarray(inp[k], np.float64) for k in ("w", "bias", "g", "be"))
    v, bound = np.zeros((inp["rows"], C)), np.zeros((inp["rows"], C))
    written = np.zeros(inp["rows"], bool)
    n = float(div or C)
    for b, nf in enumerate(inp["frames"]):
        x = np.asarray(inp["pcm"][inp["pcm_off"][b]:inp["pcm_off"][b] + 5 * nf + 5], np.float64)
        mean, inv = (float(t) for t in inp["stats"][b])
        xs = (x - mean) * inv
        win = xs[5 * np.arange(nf)[:, None] + np.arange(10)[None, :]]                       # [nf, 10]
        if tap_shift:
            win = win.copy()
            win[:, 0] = xs[5 * np.arange(nf) + 1]
        pre = win @ w.T + bias
        mag = np.abs(win) @ np.abs(w).T + np.abs(bias)
        e_v = 13 * U * mag
        mu = pre.sum(1, keepdims=True) / n
        E2 = (pre * pre).sum(1, keepdims=True) / n
        var = np.maximum(E2 - mu * mu, 0.0)
        dmu = e_v.mean(1, keepdims=True) + 24 * U * np.abs(pre).mean(1, keepdims=True)
        dE2 = (2.0 * np.abs(pre) * e_v).mean(1, keepdims=True) + 25 * U * E2
        dvar = dE2 + 2.0 * np.abs(mu) * dmu + 2 * U * (E2 + mu * mu)
        if div is None and not tap_shift:
            assert (dvar / var < 2.0 ** -10).all(), "conv0 inputs: the one-pass variance is badly conditioned"
        rstd = 1.0 / np.sqrt(var + eps)
        rho = dvar / (2.0 * (var + eps)) + 4 * U
        y = (pre - mu) * rstd * g + be
        e_y = np.abs(g) * rstd * (e_v + dmu + np.abs(pre - mu) * (rho + 3 * U)) + U * (np.abs(g * (pre - mu) * rstd) + np.abs(y))
        r = slice(inp["frame_off"][b], inp["frame_off"][b] + nf)
        v[r] = gelu(y)
        bound[r] = _out_bound(v[r], y, e_y, 1)
        written[r] = True
    return v, bound, written


def conv0_twin(inp):
    f = np.float32
    C = inp["C"]
    out = np.zeros((inp["rows"], C))
    wave = C == 512
    for b, nf in enumerate(inp["frames"]):
        x = inp["pcm"][inp["pcm_off"][b]:inp["pcm_off"][b] + 5 * nf + 5]
        mean, inv = inp["stats"][b]
        xs = ((x - mean).astype(f) * inv).astype(f)
        win = xs[5 * np.arange(nf)[:, None] + np.arange(10)[None, :]]
        v = np.broadcast_to(inp["bias"], (nf, C)).astype(np.float64)
        for k in range(10):                                                                    # fmaf: one rounding per tap
            v = (win[:, k:k + 1].astype(np.float64) * inp["w"][None, :, k].astype(np.float64) + v).astype(f).astype(np.float64)
        v = v.astype(f)
        pad = np.zeros((nf, -(-C // 64) * 64), f)
        pad[:, :C] = v
        sq = (pad * pad).astype(f)
        if wave:                                                                                # a lane sums its 8 channels, then the butterfly
            s = _lane_sum64(pad.reshape(nf, 64, 8).astype(f).cumsum(2, dtype=f)[..., -1])
            ss = _lane_sum64(sq.reshape(nf, 64, 8).cumsum(2, dtype=f)[..., -1])
            mu = (s * f(1.0 / C)).astype(f)
            var = np.maximum(((ss * f(1.0 / C)).astype(f) - (mu * mu).astype(f)).astype(f), f(0))
        else:                                                                                   # a butterfly per wave, then the waves in order
            s = _lane_sum64(pad.reshape(nf, -1, 64)).cumsum(1, dtype=f)[:, -1]
            ss = _lane_sum64(sq.reshape(nf, -1, 64)).cumsum(1, dtype=f)[:, -1]
            mu = (s / f(C)).astype(f)
            var = np.maximum(((ss / f(C)).astype(f) - (mu * mu).astype(f)).astype(f), f(0))
        rstd = (f(1) / np.sqrt((var + f(CONV0_EPS)).astype(f), dtype=f)).astype(f)
        y = ((((v - mu[:, None]).astype(f) * rstd[:, None]).astype(f) * inp["g"]).astype(f) + inp["be"]).astype(f)
        out[inp["frame_off"][b]:inp["frame_off"][b] + nf] = bf16_round(gelu_erf_f32(y).astype(np.float64))
    return out


# ---- wave stats -----------------------------------------------------------------------------------------------------------------------------------
WAVE_NS = (0, 1, 63, 64, 1023, 1024, 1025, 40001, 4000)      # the last one is the DC-offset clip
WAVE_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def wave_inputs(seed=0):
    rng = np.random.default_rng([seed, 77])
    off, clips, cur = [], [], 1
    for i, n in enumerate(WAVE_NS):
        x = 0.1 * rng.standard_normal(n) + (0.01 if i < len(WAVE_NS) - 1 else 5.0)          # DC clip: offset = 50 deviations
        off.append(cur)
        clips.append(x.astype(np.float32))
        cur += n + 1 + i % 3                                                                  # unaligned offsets, a NaN sample between clips
    pcm = np.full(cur + 3, np.nan, np.float32)
    for o, x in zip(off, clips):
        pcm[o:o + x.size] = x
    pcm.setflags(write=False)
    return pcm, np.asarray(off, np.int64), np.asarray(WAVE_NS, np.int32)


def wave_ref(pcm, off, ns, eps=WAVE_EPS):
    """-> (stats [B, 2], bound [B, 2])"""
    eps = float(np.float32(eps))
    v, bound = np.zeros((len(ns), 2)), np.zeros((len(ns), 2))
    for b, (o, n) in enumerate(zip(off, ns)):
        if n == 0:
            v[b], bound[b] = (0.0, 1.0 / math.sqrt(eps)), (0.0, 3 * U / math.sqrt(eps))
            continue
        x = np.asarray(pcm[o:o + n], np.float64)
        depth = -(-n // 1024) + 23
        mean, E2 = x.mean(), (x * x).mean()
        var = max(E2 - mean * mean, 0.0)
        dmean = depth * U * np.abs(x).mean()
        dvar = (depth + 1) * U * E2 + 2.0 * abs(mean) * dmean + 2 * U * (E2 + mean * mean)
        inv = 1.0 / math.sqrt(var + eps)
        lo, hi = 1.0 / math.sqrt(var + dvar + eps), 1.0 / math.sqrt(max(var - dvar, 0.0) + eps)
        v[b] = (mean, inv)
        bound[b] = (dmean + U * abs(mean), max(inv - lo, hi - inv) + 3 * U * hi)
    return v, bound


def wave_twin(pcm, off, ns, eps=WAVE_EPS):
    f = np.float32
    out = np.zeros((len(ns), 2))
    for b, (o, n) in enumerate(zip(off, ns)):
        if n == 0:
            out[b] = (0.0, f(1) / np.sqrt(f(eps)))
            continue
        pad = np.zeros(-(-n // 1024) * 1024, f)
        pad[:n] = pcm[o:o + n]
        s, ss = np.zeros(1024, f), np.zeros(1024, f)
        for row in pad.reshape(-1, 1024):
            s = (s + row).astype(f)
            ss = (row.astype(np.float64) * row.astype(np.float64) + ss).astype(f)           # fmaf
        ts = _lane_sum64(s.reshape(16, 64)).cumsum(dtype=f)[-1]
        tss = _lane_sum64(ss.reshape(16, 64)).cumsum(dtype=f)[-1]
        mean = f(ts / f(n))
        var = max(f(0), f(f(tss / f(n)) - f(mean * mean)))
        out[b] = (mean, f(1) / np.sqrt(f(var + f(eps))))
    return out


# ---- conv1 ------------------------------------------------------------------------------------------------------------------------------------------
CONV1_CASES = ((8, 128), (64, 11), (480, 12))        # channels, mel bins (H1 = (n_mels + 1) / 2: the odd count ends on a padding row)
CONV1_W1, CONV1_STRIDE = 50, 208
# (clip, t0, clen, w0): a full chunk, a second chunk at t0 = 100 whose last frame is missing, a single short chunk, a single frame
CONV1_IMAGES = ((0, 0, 100, 100), (0, 100, 99, 100), (1, 0, 51, 51), (2, 7, 1, 1))


def conv_len(w):
    return (w - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def conv1_inputs(C, n_mels, seed=0):
    """mel f32 [3 clips][n_mels][stride 208]; every frame no image may read is NaN.  -> dict with the 9-int ChunkMeta records"""
    rng = np.random.default_rng([seed, C, n_mels])
    mel = np.full((3, n_mels, CONV1_STRIDE), np.nan, np.float32)
    meta = np.zeros((len(CONV1_IMAGES), 9), np.int32)
    for i, (clip, t0, clen, w0) in enumerate(CONV1_IMAGES):
        mel[clip, :, t0:t0 + clen] = rng.standard_normal((n_mels, clen)).astype(np.float32)
        w1 = conv_len(w0)
        meta[i] = (clip, t0, clen, w0, w1, conv_len(w1), conv_len(conv_len(w1)), 13 * i, conv_len(conv_len(conv_len(clen))))
    w = randn_bf16(rng, (C, 9), 1.0 / 3.0)
    bias = (0.2 * rng.standard_normal(C)).astype(np.float32)
    out = dict(C=C, n_mels=n_mels, H1=(n_mels + 1) // 2, mel=mel, meta=meta, w=w, bias=bias)
    for a in (mel, meta, w, bias):
        a.setflags(write=False)
    return out


def conv1_ref(inp, tap_shift=False, pad_as_data=False, mask_shift=0):
    """-> (v, bound [img, H1, W1, C]); masked columns are exactly 0.  Defects: tap_shift = tap kw 2 reads one sample further; pad_as_data =
    the columns iw >= clen are read from the array instead of taken as zero; mask_shift = the width mask ow < w1 + mask_shift"""
    C, n_mels, H1, W1 = inp["C"], inp["n_mels"], inp["H1"], CONV1_W1
    w, bias = np.asarray(inp["w"], np.float64).reshape(C, 3, 3), np.asarray(inp["bias"], np.float64)
    n = len(CONV1_IMAGES)
    v, bound = np.zeros((n, H1, W1, C)), np.zeros((n, H1, W1, C))
    for i, (clip, t0, clen, w0) in enumerate(CONV1_IMAGES):
        xin = np.zeros((n_mels + 2, 2 * W1 + 4))                                              # row 0 = ih -1, column 0 = iw -1
        have = min(CONV1_STRIDE - t0, 2 * W1 + 3) if pad_as_data else min(clen, 2 * W1 + 1)
        xin[1:n_mels + 1, 1:1 + have] = inp["mel"][clip, :, t0:t0 + have]
        pre, mag = np.zeros((H1, W1, C)) + bias, np.zeros((H1, W1, C)) + np.abs(bias)
        for kh in range(3):
            for kw in range(3):
                sh = 1 if tap_shift and kw == 2 else 0
                x = xin[kh:kh + 2 * H1:2, kw + sh:kw + sh + 2 * W1:2][:H1, :W1]
                pre += x[..., None] * w[:, kh, kw]
                mag += np.abs(x[..., None] * w[:, kh, kw])
        v[i] = gelu(pre)
        bound[i] = _out_bound(v[i], pre, 10 * U * mag, 1)
        w1 = inp["meta"][i, 4] + mask_shift
        v[i, :, w1:], bound[i, :, w1:] = 0.0, 0.0
    return v, bound


def conv1_twin(inp):
    f = np.float32
    C, n_mels, H1, W1 = inp["C"], inp["n_mels"], inp["H1"], CONV1_W1
    w = np.asarray(inp["w"], np.float64).reshape(C, 3, 3)
    out = np.zeros((len(CONV1_IMAGES), H1, W1, C))
    for i, (clip, t0, clen, w0) in enumerate(CONV1_IMAGES):
        xin = np.zeros((n_mels + 2, 2 * W1 + 4))
        have = min(clen, 2 * W1 + 1)
        xin[1:n_mels + 1, 1:1 + have] = inp["mel"][clip, :, t0:t0 + have]
        acc = (np.zeros((H1, W1, C)) + inp["bias"].astype(np.float64))
        for kh in range(3):
            for kw in range(3):
                x = xin[kh:kh + 2 * H1:2, kw:kw + 2 * W1:2][:H1, :W1]
                acc = (x[..., None] * w[:, kh, kw] + acc).astype(f).astype(np.float64)       # fmaf
        out[i] = bf16_round(gelu_erf_f32(acc.astype(f)).astype(np.float64))
        out[i, :, inp["meta"][i, 4]:] = 0.0
    return out


# ---- exact kernels ------------------------------------------------------------------------------------------------------------------------------------
def cast_ref_bits(x):
    """f32 -> bf16 bits, round to nearest even (finite and infinite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def conv_rows_ref(in_off, out_off, n_out, total, stride, C):
    out = np.zeros(total, np.int64)
    B = len(in_off)
    for m in range(total):
        b = 0
        while b + 1 < B and m >= out_off[b + 1]:
            b += 1
        t = m - out_off[b]
        out[m] = (int(in_off[b]) + stride * t) * C if t < n_out[b] else 0
    return out


def frame_info_ref(frame_off, n_frames, total):
    out = np.zeros((total, 2), np.int32)
    B = len(frame_off)
    for m in range(total):
        b = 0
        while b + 1 < B and m >= frame_off[b + 1]:
            b += 1
        out[m] = (m - frame_off[b], n_frames[b])
    return out


def argmax_ref(x):
    """first index of the maximum over the non-NaN entries of every row, 0 for an all-NaN row; err = any NaN or infinity"""
    ids = np.zeros(x.shape[0], np.int32)
    for r, row in enumerate(x):
        ok = ~np.isnan(row)
        if ok.any():
            ids[r] = int(np.flatnonzero(ok & (row == row[ok].max()))[0])
    return ids, int(not np.isfinite(x).all())

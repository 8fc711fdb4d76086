"""Float64 references, inputs, bounds, f32 twins and wrong-kernel models for the kernels that stream the weights of a decode step
(csrc/dec_gemv.hip, csrc/dec_gemv_wide.hip, csrc/dec_quant.hip, csrc/dec_lmhead.hip, rmsnorm_rows of csrc/dec_prefill.hip), shared by
tests/test_dec_cases_cpu.py and tests/test_gpu_dec_cases.py.  All arithmetic is float64 on bf16- / f32-valued inputs with each kernel's own
rounding points and nothing else.  No term of any bound comes from a device run; the bounds are those of tests/gemm_cases.py.

BF16 LINEAR (decode_gemv_kernel, decode_gemv2_kernel, decode_gemv_wide_kernel).  s = the staged activation row (X, or the RMSNorm of X, below),
v = sum_k s_k W[n][k], mag = sum_k |s_k W[n][k]|, e = F32_REL mag (gemm_cases: f32 accumulation over K <= 8192 in MFMA order; 6144 is inside).
    BF16     bound_bf16(v, mag)
    LOGITS   f32 values that are bf16 values: the same bound
    RESID    out = bf16(r + bf16(acc)): the inner rounding is of the device's acc, within e of v, so the result lies between
             r + bf16(v - e) and r + bf16(v + e) (gemm_cases.resid_bf16_candidates); the BF16 bound with mag + |r| applies outside the two
    SWIGLU   weight rows in blocks of 16 gate + 16 up; gemm_cases.swiglu_ref.  Coherent inputs (x >= 0, every weight row of one sign): within
             three bf16 ulps.  Gaussian inputs: the share of outputs not bit-equal to the reference is at most 3 x the share of the f32 twin
             on the same inputs (the twin-share method of tests/test_gpu_gemm_cases.py).

RMSNORM PROLOGUE and rmsnorm_rows: s_k = bf16(w_k bf16(x_k inv)), inv = rsqrt(mean(x^2) + eps).  w t is the product of two bf16 values, exact in
f32, so only the first rounding depends on the device's inv.  Its relative distance from the float64 inv, u = 2^-24 per rounding:
    the sum of squares: an fmaf chain of n = K / (threads per row) terms per thread (<= 128: K = 2048 on 16 threads, the two-tile image), every
    partial sum <= the total, so <= n u; log2(threads) <= 6 shuffle additions: (n + 6) u <= 134 u, halved by the square root: 67 u
    ss / K and + eps: 2 u, halved: u;  rsqrtf: two f32 ulps = 4 u;  the product x inv: u           together INV_REL = 73 u = 4.4e-6
An element is AMBIGUOUS when bf16(x inv (1 - INV_REL)) != bf16(x inv (1 + INV_REL)).  About 0.1 % of Gaussian elements are (0.117 % of the
plain rows of 1024 elements, a fifth of which hold one); so the activation rows behind a norm are drawn by rejection (norm_rows: a candidate row with an ambiguous element is
drawn again) and NO row of any case has one -- tests/test_dec_cases_cpu.py asserts it for every case (the issue's condition is 90 % of the
rows).  gemv_expect still adds sum over ambiguous k of |W[n][k]| ulp_bf16(s_k) to e, so the reference stays right for rows that are not
drawn that way (rmsnorm_rows is also run on plain Gaussian rows and checked element by element against the two candidates).

QUANTISED LINEAR (decode_gemvq_kernel, gemvq_generic_kernel; MLX affine, group 64).  The kernels evaluate sum_g (s_g A_g + b'_g S_g) with
A_g = sum q'_k x_k, S_g = sum x_k over the group.  The tuned kernels at 4 bit multiply by q' = 16 + q (dec_quant_dev.h frag_q4) and use
b' = fmaf(-16, s, b) rounded to f32 (eff_bias); at 8 bit and in the generic kernel q' = q, b' = b.  The reference is that sum in float64 with
that q' and that (f32) b'.  mag = sum_g (|s_g| sum q'_k |x_k| + |b'_g| sum |x_k|): the magnitude of what the f32 arithmetic adds up.  The two
terms cancel (b is near -s 2^(bits-1)), so sum |w x| of the dequantised weight understates the f32 error by their ratio, most on all-positive x
(kind "positive").  Bounds from v and mag as for the bf16 linear.

LM HEADS (lm_head_kernel, lm_head_q_kernel, the generic head): logits under the LOGITS bound; the argmax partials are exact against the
device's own logits (partials_defects).

INPUTS, seeded, per case (64 rows; a launch of B rows takes the first B and a NaN row after them):
    gauss     Gaussian X (behind a norm: row r scaled by 2^(r % 3 - 1)) and W (quantised: uniform q, scales near 2 / (2^bits sqrt K), biases near -s 2^(bits-1))
    coherent  SWIGLU: x >= 0, every weight row of one sign, gate / up values over +-[0.25, 4]; with the spikes below
    positive  quantised: x >= 0
    spike     row r holds 8.0 at column spike_ks(K)[r % len] and every weight row +-0.5 there (quantised: the largest q, a weight near
              1 / sqrt K): one product of 4 (quantised: 0.1 .. 0.4) on a slot boundary -- column
              0, the last k-step of wave 0 at 8 waves and at 4, column 3072 of K = 6144 (the first of the second phase), the first column of
              the last 64-column group, the last column.  Row B - 1 of every B holds one; row B is NaN.
    readout   (no norm, BF16 / RESID) X one-hot: row r holds 1.0 at column readout_k(K, r, shift); out[r][n] is then W[n][k] bit for bit
              (quantised: s q' + b' in the kernel's f32 order).  Over the shifts every (k-step, half fragment) is read by some row.
              W one-hot ("wreadout", bf16): weight row n holds 1.0 at readout_k(K, n, shift), X Gaussian; out[r][n] = X[r][k] bit for bit at
              every B.
"""
import functools
import math
import numpy as np
import gemm_cases as G
from gemm_cases import bf16_round, bf16_bits, bf16_from_bits, ulp_bf16, randn_bf16, F32_REL

U = 2.0 ** -24
INV_REL = 73 * U
EPS = float(np.float32(1e-6))
GEMV, GEMVQ, LMHEAD, LMHEADQ, RMSNORM_ROWS = range(5)
BF16, RESID, SWIGLU, LOGITS = range(4)
EPI_NAMES = ("bf16", "resid", "swiglu", "logits")
SENTINEL = np.uint16(0xc3c2)
SENTINEL_F32 = np.float32(-7.25e9)
NAN_BITS = np.array([0x7fc0, 0xffc0, 0x7fff, 0xffa5], np.uint16)
SENTINEL_VALUE = float(bf16_from_bits(np.array([SENTINEL]))[0])
ROWS = 64
BS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 49, 64)
BS_Q = (1, 7, 8, 16, 17, 33, 64)


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gemv_cases():
    """(epi, K, N, norm, generic) of the bf16 linear"""
    c = []
    for K in (1024, 2048, 3072, 6144):
        c += [(BF16, K, 144, 0, 0), (RESID, K, 144, 0, 0)]
    for K in (1024, 2048):
        c += [(BF16, K, 144, 1, 0), (SWIGLU, K, 288, 1, 0)]
    c += [(LOGITS, 1024, 320, 1, 0), (LOGITS, 2048, 320, 1, 0)]     # N % 64 == 0: the tuned four-tile form, 5 partials per row
    for K in (96, 1056):
        c += [(BF16, K, 144, 0, 1), (RESID, K, 144, 0, 1), (SWIGLU, K, 288, 1, 1), (LOGITS, K, 272, 1, 1)]
    return tuple(c)


@functools.lru_cache(maxsize=None)
def gemvq_cases():
    """(epi, K, N, norm, generic, bits, sb_f32) of the quantised linear"""
    c = []
    for bits in (4, 8):
        for sbf in (0, 1):
            for K in (1024, 2048, 3072, 6144):
                c += [(RESID, K, 144, 0, 0, bits, sbf)]
            for K in (1024, 2048):
                c += [(BF16, K, 144, 1, 0, bits, sbf), (SWIGLU, K, 288, 1, 0, bits, sbf)]
            c += [(BF16, 192, 144, 0, 1, bits, sbf), (RESID, 192, 144, 0, 1, bits, sbf), (SWIGLU, 192, 288, 1, 1, bits, sbf)]
    c += [(BF16, 1024, 4096, 1, 0, 4, 0), (SWIGLU, 1024, 6144, 1, 0, 4, 0), (BF16, 2048, 4096, 1, 0, 8, 1), (SWIGLU, 2048, 6144, 1, 0, 8, 0)]
    return tuple(c)


def gemv_route(epi, K, N, norm, generic, wide=1, B=1):
    """1 where decode_gemv_dense_launch has a tuned instantiation (dec_gemv.hip gemv2_k, dec_gemv_wide.hip), read from the dispatch.  The
    four-tile LOGITS form at K = 2048 has none above 48 rows: gemv2_lds<4, 4, 8, 8, false> is 16 x 4112 + 7 x 16 x 1024 = 176 KiB, over the
    156 KiB gemv2_go takes, so those launches run the generic kernel (no product launch reaches that form: lm_head_launch hands the fused
    launcher no fragment-major image)"""
    if generic or (epi == LOGITS and K == 2048 and B > 48):
        return 0
    if K == 6144:
        return int(bool(wide) and not norm and epi in (BF16, RESID))
    if norm:
        return int(K in (1024, 2048) and (epi in (BF16, SWIGLU) or (epi == LOGITS and N % 64 == 0)))
    return int(K in (1024, 2048, 3072) and epi in (BF16, RESID))


def gemvq_route(epi, K, N, norm, generic, wide=1):
    """1 where decode_gemv_q_launch has a tuned instantiation (dec_quant.hip gemvq_epi / gemvq_k)"""
    if generic:
        return 0
    if norm:
        return int(K in (1024, 2048) and epi in (BF16, SWIGLU))
    return int(epi == RESID and (K in (1024, 2048, 3072) or (K == 6144 and bool(wide))))


def gemv_knob_runs(epi, K, N, norm, generic):
    """(knob, value, batch sizes, bit-equal to the defaults?) where the setting changes the instantiation of this case (dec_gemv.hip gemv2_nb /
    gemv2_go).  Every setting but gemv_w1024 and gemv_wide keeps the (wave -> k-steps, reduction order) map: it changes the order of the
    requests (earlyw, xbar), the cache policy (nt), what dead rows cost (partial) or which workgroup holds a row (splitb: 16 rows per
    workgroup, two tiles resident, or 16 rows per phase against the same weights) -- each output is still wave w's k-steps w, w + WAVES, ...
    in ascending order, then wave 0 + 1 + ... in order."""
    if generic or K == 6144:
        return [("gemv_wide", 0, (1, 17, 64), False)] if K == 6144 and not generic else []
    if epi == LOGITS:               # the dispatch keeps LOGITS out of the row groups, the non-temporal form and every small-batch form
        return []
    runs = [("gemv_splitb", 0, (17, 32, 33, 49, 64), True), ("gemv_nt", 1, (1, 16, 33), True)]
    runs += [("gemv_splitb", 1, (17, 33, 64), True), ("gemv_earlyw", 0, (1, 8), True), ("gemv_earlyw", 2, (9, 16, 33), True),
             ("gemv_earlyw", 3, (16, 33), True)]
    runs += [("gemv_xbar", x, (9, 16, 17, 33), True) for x in (0, 1, 2, 3)]
    if norm:
        runs += [("gemv_partial", 0, (1, 7, 9, 15), True)]
    if K == 1024:
        runs += [("gemv_w1024", 4, (1, 16, 33, 64), False)]
    return runs


def gemvq_knob_runs(epi, K, N, norm, generic):
    if generic:
        return []
    if K == 6144:
        return [("gemv_wide", 0, (1, 17, 64), False)]
    return [("gemv_xbar", x, (1, 8, 16, 17, 33), True) for x in (0, 1, 2, 3)]


# ---- RMSNorm staging -------------------------------------------------------------------------------------------------------------------------
def rms_stage(x, w, eps=EPS):
    """x [rows, K], w [K] -> (s = bf16(w bf16(x inv)), ambiguous [rows, K], the two candidates of s)"""
    K = x.shape[-1]
    inv = 1.0 / np.sqrt((x * x).sum(-1, keepdims=True) / K + eps)
    y = x * inv
    lo, hi = bf16_round(y * (1.0 - INV_REL)), bf16_round(y * (1.0 + INV_REL))
    return bf16_round(w * bf16_round(y)), lo != hi, (bf16_round(w * lo), bf16_round(w * hi))


def norm_rows(rng, rows, K, make):
    """rows of make(rng, n) [n, K] drawn again until none holds an ambiguous element"""
    out = np.empty((rows, K))
    need = np.arange(rows)
    while need.size:
        cand = make(rng, need)
        ok = ~rms_stage(cand, 1.0)[1].any(1)
        out[need[ok]] = cand[ok]
        need = need[~ok]
    return out


def spike_ks(K):
    ks = {0, K - 1, K - 64, K - 32 * 8, K - 32 * 4}
    if K == 6144:
        ks |= {3072, 3071}
    return sorted(k for k in ks if 0 <= k < K)


def readout_k(K, r, shift):
    """row r of launch `shift`: half fragment (r + shift) % 2 of k-step (r // 2 + shift * 32) % (K / 32), a lane column that walks with r"""
    step = (r // 2 + shift * 32) % (K // 32)
    return step * 32 + ((r + shift) % 2) * 16 + (r * 5) % 16


def readout_shifts(K, rows):
    return range(max(1, -(-(K // 32 * 2) // rows)))


@functools.lru_cache(maxsize=None)
def x_rows(K, kind, norm):
    """[ROWS, K] float64 bf16 values, read-only"""
    rng = np.random.default_rng([K, ("gauss", "coherent", "positive", "spike").index(kind), norm])
    ks = spike_ks(K)

    def make(rng, rows):
        x = randn_bf16(rng, (len(rows), K))
        if kind in ("coherent", "positive"):
            x = np.abs(x)
        if kind in ("coherent", "spike"):
            x[np.arange(len(rows)), [ks[r % len(ks)] for r in rows]] = 8.0
        if norm:                                            # rows of three scales: the neighbour's inv is off by a factor of two
            x = x * 2.0 ** (np.asarray(rows) % 3 - 1)[:, None]
        return x
    x = norm_rows(rng, ROWS, K, make) if norm else make(rng, np.arange(ROWS))
    x.setflags(write=False)
    return x


def x_bits(x, B, extra=1):
    """the first B rows and `extra` NaN rows"""
    K = x.shape[1]
    b = np.empty((B + extra, K), np.uint16)
    b[:B] = bf16_bits(x[:B])
    b[B:] = NAN_BITS[np.arange(extra * K).reshape(extra, K) % 4]
    return b


@functools.lru_cache(maxsize=None)
def norm_weight(K):
    w = bf16_round(1.0 + 0.1 * np.random.default_rng(K + 5).standard_normal(K))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def gemv_inputs(epi, K, N, norm, kind):
    """-> dict(X [ROWS, K], W [N, K], nw [K] or None, r [ROWS, N] residual or None)"""
    rng = np.random.default_rng([epi, K, N, norm, ("gauss", "coherent", "spike").index(kind)])
    X = x_rows(K, kind, norm)
    if kind == "coherent":
        row = rng.choice([-1.0, 1.0], N) * 2.0 ** rng.uniform(-2, 2, N) / (0.6366 * K)
        W = bf16_round(np.abs(rng.standard_normal((N, K))) * row[:, None])
        sgn = np.sign(row)
    else:
        W = randn_bf16(rng, (N, K), 1.0 / math.sqrt(K))
        sgn = rng.choice([-1.0, 1.0], N)
    if kind in ("coherent", "spike"):
        W[:, spike_ks(K)] = (0.5 if kind == "spike" else 0.125) * sgn[:, None]
    d = dict(X=X, W=W, nw=norm_weight(K) if norm else None, r=bf16_round(rng.standard_normal((ROWS, N))) if epi == RESID else None)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def gemv_kinds(epi, norm):
    return ("coherent", "gauss") if epi == SWIGLU else ("gauss", "spike")


# ---- bf16 linear: reference, bounds -------------------------------------------------------------------------------------------------------------
def stage(d):
    """-> (staged rows, extra error per output from ambiguous elements [ROWS, N] or 0)"""
    if d["nw"] is None:
        return d["X"], 0.0
    s, amb, _ = rms_stage(d["X"], d["nw"])
    return s, (amb * ulp_bf16(s)) @ np.abs(d["W"]).T if amb.any() else 0.0


@functools.lru_cache(maxsize=None)
def gemv_expect(epi, K, N, norm, kind):
    """-> dict: BF16 / LOGITS: v, mag;  RESID: lo, hi, mag;  SWIGLU: ref (gemm_cases.swiglu_ref on the staged rows)"""
    d = gemv_inputs(epi, K, N, norm, kind)
    s, e_amb = stage(d)
    if epi == SWIGLU:
        return dict(ref=G.swiglu_ref(s, d["W"]))
    acc = s @ d["W"].T
    mag = np.abs(s) @ np.abs(d["W"]).T + e_amb / F32_REL
    if epi == RESID:
        lo, hi, m = G.resid_bf16_candidates(dict(acc=acc, mag=mag, resid_bf16=d["r"]))
        return dict(lo=lo, hi=hi, mag=m)
    return dict(v=acc, mag=mag)


def frac_bf16(got, v, mag, v_hi=None):
    """worst distance as a fraction of the BF16 bound, below v and above v_hi (v where there is one candidate)"""
    hi = v if v_hi is None else v_hi
    assert np.isfinite(got).all(), "a value that is not finite"
    return float(np.maximum((v - got) / G.bound_bf16(v, mag), (got - hi) / G.bound_bf16(hi, mag)).max())


def gemv_frac(epi, exp, got, B):
    """got [B, cols] float64 against the first B rows of gemv_expect -> fraction of the bound (SWIGLU: bf16 ulps)"""
    if epi == SWIGLU:
        assert np.isfinite(got).all()
        return float(G.ulps_bf16(got, exp["ref"][:B]).max())
    if epi == RESID:
        return frac_bf16(got, exp["lo"][:B], exp["mag"][:B], exp["hi"][:B])
    return frac_bf16(got, exp["v"][:B], exp["mag"][:B])


def gemv_twin(epi, d):
    """an honest f32 realisation: numpy f32 on the reversed K axis, the kernel's rounding points -> what the device would return"""
    s = stage(d)[0]
    if epi == SWIGLU:
        return G.swiglu_twin_f32(s, d["W"])
    acc = (np.ascontiguousarray(s[:, ::-1], np.float32) @ np.ascontiguousarray(d["W"][:, ::-1], np.float32).T).astype(np.float64)
    if epi == RESID:
        return bf16_round(f32(d["r"] + bf16_round(acc)))
    return bf16_round(acc)


def readout_expect(epi, W, k, r=None):
    """X one-hot at k [rows] -> out [rows, N] exactly: the accumulator IS the weight"""
    acc = W[:, k].T
    return acc if epi != RESID else bf16_round(f32(r + acc))


# ---- wrong kernels of the bf16 linear ------------------------------------------------------------------------------------------------------------
GEMV_MUTATIONS = ("drop_kstep", "double_kstep", "drop_phase2", "admit_row_B", "drop_last_row", "group_read_0", "group_write_0", "resid_row0",
                  "resid_no_inner_round", "up_tile_shift", "inv_neighbour", "inv_half_K", "norm_w_chunk")


def gemv_model(epi, d, B, mut=None, waves=8):
    """float64 model of the launch on B rows with one defect -> out [B, cols], or None where the defect does not exist for this case.
    NaN marks an output that took the NaN row in; a row that was not written holds the sentinel's value."""
    X, W, nw, r = d["X"][:B].copy(), d["W"], d["nw"], None if d["r"] is None else d["r"][:B]
    K, N = X.shape[1], W.shape[0]
    rows = np.arange(B)
    if mut in ("inv_neighbour", "inv_half_K", "norm_w_chunk") and nw is None:
        return None
    if mut in ("resid_row0", "resid_no_inner_round") and epi != RESID:
        return None
    if mut == "up_tile_shift" and (epi != SWIGLU or N < 64):
        return None
    if mut in ("group_read_0", "group_write_0") and B <= 16:
        return None
    if mut == "drop_phase2" and K != 6144:
        return None
    if nw is not None:
        inv = 1.0 / np.sqrt((X * X).sum(-1, keepdims=True) / K + EPS)
        if mut == "inv_neighbour":
            if B == 1:
                return None
            inv = np.roll(inv, 1, 0)
        if mut == "inv_half_K":
            inv = 1.0 / np.sqrt((X[:, :K // 2] ** 2).sum(-1, keepdims=True) / K + EPS)
        s = bf16_round((np.roll(nw, 8) if mut == "norm_w_chunk" else nw) * bf16_round(X * inv))
    else:
        s = X
    if mut == "group_read_0":
        s = s[rows % 16]
    P = np.matmul(s.reshape(B, K // 32, 32).transpose(1, 0, 2), W.reshape(N, K // 32, 32).transpose(1, 2, 0)).transpose(1, 2, 0)   # [B, N, k-step]
    acc = P.sum(-1)
    step = K // 32 - waves                                  # the last k-step of wave 0
    if mut == "drop_kstep":
        acc = acc - P[:, :, step]
    if mut == "double_kstep":
        acc = acc + P[:, :, step]
    if mut == "drop_phase2":
        acc = P[:, :, :96].sum(-1)
    if mut == "admit_row_B":
        acc[B - 1] = np.nan                                 # row B (NaN) taken for row B - 1: whatever takes it in is NaN
    if epi == SWIGLU:
        g, u = G.swiglu_split(acc)
        if mut == "up_tile_shift":
            u = np.roll(u, 16, 1)
        g, u = bf16_round(g), bf16_round(u)
        out = bf16_round(bf16_round(g / (1.0 + np.exp(-g))) * u)
    elif epi == RESID:
        rr = r[np.zeros(B, int)] if mut == "resid_row0" else r
        out = bf16_round(rr + (acc if mut == "resid_no_inner_round" else bf16_round(acc)))
    else:
        out = bf16_round(acc)
    if mut == "drop_last_row":
        out[B - 1] = SENTINEL_VALUE
    if mut == "group_write_0":
        out[16:] = SENTINEL_VALUE          # rows of the later groups land on group 0's rows and are never written
    return out


# ---- quantised linear ------------------------------------------------------------------------------------------------------------------------------
def quant_words(q, bits):
    """q [N, K] integers -> uint32 [N, K bits / 32]: element i of a row in word i / (32 / bits), LSB first"""
    per = 32 // bits
    N, K = q.shape
    sh = (np.arange(per, dtype=np.uint64) * bits)[None, None, :]
    return (q.reshape(N, K // per, per).astype(np.uint64) << sh).sum(-1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def quant_matrix(K, N, bits, sb_f32, coherent=False, spike=False):
    """-> dict(q [N, K] float64 integers, s, b [N, K / 64] float64 values of the stored dtype, words uint32).  coherent: every row's
    dequantised weights of one sign (SWIGLU three-ulp premise).  spike: the largest q at the columns spike_ks(K), i.e. the largest weight a
    row can hold there (near 1 / sqrt K), against 8.0 in x"""
    rng = np.random.default_rng([K, N, bits, sb_f32, int(coherent)])
    top = 2 ** bits - 1
    q = rng.integers(0, top + 1, (N, K)).astype(np.float64)
    if spike or coherent:
        q[:, spike_ks(K)] = top
    s = (0.5 + rng.random((N, K // 64))) * 2.0 / (top * math.sqrt(K))
    b = -s * (top + 1) / 2 * (1.0 + 0.05 * rng.standard_normal(s.shape))
    if coherent:                                            # w = s (q + 0.5): E sum w x = K 0.8 s top / 2 = +-2^U(-2, 2)
        s = rng.choice([-1.0, 1.0], N)[:, None] * 2.0 ** rng.uniform(-2, 2, (N, 1)) / (0.4 * K * top) * (0.5 + rng.random((N, K // 64)))
        b = 0.5 * s
    rnd = f32 if sb_f32 else bf16_round
    d = dict(q=q, s=rnd(s), b=rnd(b), words=quant_words(q, bits))
    for v in d.values():
        v.setflags(write=False)
    return d


def quant_eff(m, bits, tuned):
    """-> (q', b') the kernel multiplies by: 16 + q and fmaf(-16, s, b) in the tuned 4-bit kernels"""
    if bits == 4 and tuned:
        return m["q"] + 16.0, f32(-16.0 * m["s"] + m["b"])
    return m["q"], m["b"]


def quant_dot(x, m, bits, tuned, dtype=np.float64, mut=None):
    """the factored sum in `dtype` -> (value [rows, N], mag [rows, N])"""
    qe, be = quant_eff(m, bits, tuned)
    s = m["s"]
    N, K = qe.shape
    Gn = K // 64
    if mut == "neighbour_scale":
        s = np.roll(s, 1, 1)
    if mut == "neighbour_bias":
        be = np.roll(be, 1, 1)
    if mut == "no_bias":
        be = be * 0.0
    if mut == "no_offset":
        be = m["b"]
    if mut == "swap":                                       # nibbles of a byte (4 bit) / bytes of a halfword (8 bit) exchanged
        qe = qe.reshape(N, K // 2, 2)[:, :, ::-1].reshape(N, K)
    keep = np.ones(Gn)                                      # how often a 64-column group is added
    if mut == "drop_block":                                 # the last k-block of a wave: the last group (both bit widths)
        keep[Gn - 1] = 0.0
    if mut == "double_block":
        keep[Gn - 1] = 2.0
    if mut == "drop_phase2":                                # K = 6144: the columns from 3072
        keep[Gn // 2:] = 0.0
    xg = np.ascontiguousarray(x.reshape(-1, Gn, 64).transpose(1, 0, 2), dtype)              # [group, rows, 64]
    qg = np.ascontiguousarray(qe.reshape(N, Gn, 64).transpose(1, 2, 0), dtype)              # [group, 64, N]
    sg, bg = s.T.astype(dtype)[:, None, :], be.T.astype(dtype)[:, None, :]                  # [group, 1, N]
    v = ((sg * np.matmul(xg, qg) + bg * xg.sum(-1)[:, :, None]) * keep.astype(dtype)[:, None, None]).sum(0)
    if dtype != np.float64:
        return v.astype(np.float64), None
    return v, (np.abs(sg) * np.matmul(np.abs(xg), qg) + np.abs(bg) * np.abs(xg).sum(-1)[:, :, None]).sum(0)


QUANT_MUTATIONS = ("neighbour_scale", "neighbour_bias", "no_bias", "swap", "no_offset", "drop_block", "double_block", "drop_phase2",
                   "admit_row_B", "drop_last_row", "group_read_0", "group_write_0")


def gemvq_kinds(epi):
    return ("coherent", "gauss") if epi == SWIGLU else ("gauss", "positive", "spike")


@functools.lru_cache(maxsize=None)
def gemvq_inputs(epi, K, N, norm, bits, sb_f32, kind):
    rng = np.random.default_rng([epi, K, N, norm, bits, sb_f32, 77])
    m = quant_matrix(K, N, bits, sb_f32, coherent=kind == "coherent", spike=kind == "spike")
    d = dict(X=x_rows(K, kind, norm), m=m, nw=norm_weight(K) if norm else None,
             r=bf16_round(rng.standard_normal((ROWS, N))) if epi == RESID else None)
    if d["r"] is not None:
        d["r"].setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def gemvq_expect(epi, K, N, norm, bits, sb_f32, kind, tuned):
    d = gemvq_inputs(epi, K, N, norm, bits, sb_f32, kind)
    s = d["X"]
    if norm:
        s, amb, _ = rms_stage(d["X"], d["nw"])
        assert not amb.any()
    acc, mag = quant_dot(s, d["m"], bits, tuned)
    if epi == SWIGLU:
        g, u = G.swiglu_split(acc)
        g, u = bf16_round(g), bf16_round(u)
        return dict(ref=bf16_round(bf16_round(g / (1.0 + np.exp(-g))) * u))
    if epi == RESID:
        lo, hi, mm = G.resid_bf16_candidates(dict(acc=acc, mag=mag, resid_bf16=d["r"]))
        return dict(lo=lo, hi=hi, mag=mm)
    return dict(v=acc, mag=mag)


def gemvq_twin(epi, d, bits, tuned, mut=None):
    """the factored sum in numpy f32 -> what the device would return (mut: a wrong kernel, in float64; the row defects as in gemv_model, on
    all ROWS rows: the kernels take 16 rows per workgroup)"""
    s = d["X"] if d["nw"] is None else rms_stage(d["X"], d["nw"])[0]
    if mut == "group_read_0":
        s = s[np.arange(ROWS) % 16]
    acc = quant_dot(s, d["m"], bits, tuned, np.float64 if mut else np.float32, mut)[0]
    if mut == "admit_row_B":
        acc[ROWS - 1] = np.nan
    out = _quant_epilogue(epi, d, acc)
    if mut == "drop_last_row":
        out[ROWS - 1] = SENTINEL_VALUE
    if mut == "group_write_0":
        out[16:] = SENTINEL_VALUE
    return out


def _quant_epilogue(epi, d, acc):
    if epi == SWIGLU:
        g, u = G.swiglu_split(acc)
        g, u = bf16_round(g).astype(np.float32), bf16_round(u).astype(np.float32)
        sg = bf16_round(g / (np.float32(1.0) + np.exp(-g))).astype(np.float32)
        return bf16_round(sg * u)
    if epi == RESID:
        return bf16_round(f32(d["r"] + bf16_round(acc)))
    return bf16_round(acc)


def quant_readout_expect(epi, m, bits, tuned, k, r=None):
    """X one-hot (1.0) at k [rows]: every group but k's adds s 0 + b' 0; k's adds fl(fl(s q') + fl(b' 1)), all in f32 -> out [rows, N]"""
    qe, be = quant_eff(m, bits, tuned)
    g = np.asarray(k) // 64
    t = (m["s"][:, g].astype(np.float32) * qe[:, k].astype(np.float32) + be[:, g].astype(np.float32)).T.astype(np.float64)
    return bf16_round(t) if epi != RESID else bf16_round(f32(r + bf16_round(t)))


# ---- LM heads -----------------------------------------------------------------------------------------------------------------------------------------
def partials_defects(logits, pv, pi, tiles_of_part=None):
    """logits [B, N] f32 of the device, pv / pi [B, parts] -> list of defects (empty = exact): every partial names a logit of its value,
    reducing the partials by "larger value, else lower index" gives the FIRST maximum of the row, and (tiles_of_part given) every partial is
    the first maximum of the 16-row tiles its part owns"""
    bad = []
    B, N = logits.shape
    if ((pi < 0) | (pi >= N)).any():
        return ["a partial index outside the row"]
    if not (np.take_along_axis(logits, pi, 1) == pv).all():
        bad.append("a partial's value is not the logit at its index")
    best = pv.max(1)
    win = np.where(pv == best[:, None], pi, N).min(1)
    if not (win == logits.argmax(1)).all():
        bad.append("the partials do not reduce to the first maximum of the row")
    if tiles_of_part is not None:
        mv, mi = head_partials_model(logits, tiles_of_part)
        if not (np.array_equal(mv, pv) and np.array_equal(mi, pi)):
            bad.append("a partial is not the first maximum of its part's tiles")
    return bad


def head_partials_model(logits, tiles_of_part, mut=None):
    """model of a head's argmax: part p owns the 16-row tiles tiles_of_part[p] -> (pv, pi) [B, parts]; mut: skip_tail (the last tile of every
    part is dropped unless it holds the part's maximum -- it is simply never compared), tie_high (ties go to the higher index)"""
    B, N = logits.shape
    pv, pi = np.empty((B, len(tiles_of_part)), np.float32), np.empty((B, len(tiles_of_part)), np.int32)
    for p, tiles in enumerate(tiles_of_part):
        tiles = tiles[:-1] if mut == "skip_tail" and len(tiles) > 1 else tiles
        cols = (np.asarray(tiles)[:, None] * 16 + np.arange(16)[None]).reshape(-1)
        sub = logits[:, cols]
        j = sub.shape[1] - 1 - sub[:, ::-1].argmax(1) if mut == "tie_high" else sub.argmax(1)
        pv[:, p], pi[:, p] = sub[np.arange(B), j], cols[j]
    return pv, pi


def persistent_tiles(N, grid, waves=8, wg_fastest=1):
    """tiles of every workgroup of the persistent heads: wave gw takes tiles gw, gw + grid * waves, ..."""
    total = grid * waves
    parts = []
    for wg in range(grid):
        t = []
        for w in range(waves):
            gw = w * grid + wg if wg_fastest else wg * waves + w
            t += list(range(gw, N // 16, total))
        parts.append(sorted(t))
    return parts


# ---- LM heads: cases, inputs, reference ---------------------------------------------------------------------------------------------------------------
N_HEAD, N_HEADQ = 65616, 32848          # 4101 / 2053 tiles: 5 more than 2 / 1 per wave of 256 workgroups x 8 waves, so 5 waves own a tail tile
HEAD_GRID, HEAD_WAVES = 256, 8
# (K, N, generic, batch sizes); the generic head has one partial per block of 16 (N % 32 != 0) or 64 rows: 17 and 257 per row
HEAD_CASES = ((1024, N_HEAD, 0, (1, 16, 17, 33, 49, 64)), (2048, N_HEAD, 0, (1, 17, 32)), (1024, 272, 1, (1, 17, 64)), (1024, 16448, 1, (1, 33, 64)))
# (K, N, generic, bits, sb_f32, batch sizes); the generic quantised head (one partial per row) at N = 272
HEADQ_CASES = ((1024, N_HEADQ, 0, 4, 0, (1, 16, 17, 33, 49, 64)), (1024, N_HEADQ, 0, 4, 1, (1, 17, 33)), (1024, N_HEADQ, 0, 8, 0, (16, 32, 64)),
               (1024, N_HEADQ, 0, 8, 1, (1, 49)), (2048, N_HEADQ, 0, 4, 0, (1, 17, 32)), (2048, N_HEADQ, 0, 8, 1, (16, 32)),
               (1024, 272, 1, 4, 0, (1, 17, 64)), (1024, 272, 1, 8, 1, (33,)))


def tie_pairs(N, persistent):
    """(lower copy, higher copy) of planted equal weight rows; pair i is scaled to be the maximum of batch row i"""
    if not persistent:
        return ((20, 21), (35, N - 45), (3, N // 2 + 16 + 3), (63, 64), (N - 2, N - 1))
    total = HEAD_GRID * HEAD_WAVES
    tail3 = 3 + N // 16 // total * total                            # wave 3's tail tile
    return ((7 * 16 + 4, 7 * 16 + 5),                               # two of one lane's four outputs (bf16 head; quantised: two lanes)
            (3 * 16 + 3, tail3 * 16 + 3),                           # the first and the tail tile of one wave
            (11 * 16 + 8, (11 + HEAD_GRID) * 16 + 8),               # two waves of one workgroup (workgroup-fastest order)
            (13 * 16 + 15, 14 * 16),                                # neighbouring workgroups
            (2 * 16 + 1, (N // 16 - 1) * 16 + 1))                   # the last tail tile against a first-round tile of another wave


def head_tiles(N, persistent, order=1):
    """16-row tiles of every partial: the persistent heads' workgroups, or the generic head's blocks of 1 / 2 / 4 tiles"""
    if persistent:
        return persistent_tiles(N, HEAD_GRID, HEAD_WAVES, order)
    nt = 4 if N % 64 == 0 else 2 if N % 32 == 0 else 1
    return [list(range(p * nt, (p + 1) * nt)) for p in range(N // (16 * nt))]


def _bf16_f32(a):
    """round f32 values to bf16 values (f32 storage), ties to even"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).view(np.float32)


@functools.lru_cache(maxsize=2)
def head_inputs(K, N, persistent):
    """-> dict(X [ROWS, K] float64, nw, s = the staged rows, W float32 [N, K] of bf16 values with planted ties); read-only"""
    rng = np.random.default_rng([K, N, 31])
    X, nw = x_rows(K, "gauss", 1), norm_weight(K)
    s, amb, _ = rms_stage(X, nw)
    assert not amb.any()
    W = _bf16_f32(rng.standard_normal((N, K), np.float32) * np.float32(1.0 / math.sqrt(K)))
    for i, (lo, hi) in enumerate(tie_pairs(N, persistent)):
        W[lo] = W[hi] = _bf16_f32((4.0 / math.sqrt(K) * s[i]).astype(np.float32))
    for v in (s, W):
        v.setflags(write=False)
    return dict(X=X, nw=nw, s=s, W=W)


@functools.lru_cache(maxsize=2)
def head_expect(K, N, persistent):
    """-> (v, mag) [ROWS, N] float64, in chunks of weight rows"""
    d = head_inputs(K, N, persistent)
    v, mag = np.empty((ROWS, N)), np.empty((ROWS, N))
    sa = np.abs(d["s"])
    for n0 in range(0, N, 8192):
        Wc = d["W"][n0:n0 + 8192].astype(np.float64).T
        v[:, n0:n0 + 8192], mag[:, n0:n0 + 8192] = d["s"] @ Wc, sa @ np.abs(Wc)
    return v, mag


def head_twin(d):
    """f32 logits of an honest f32 head (numpy f32, reversed K), bf16-rounded -> float32 [ROWS, N]"""
    return _bf16_f32(np.ascontiguousarray(d["s"][:, ::-1], np.float32) @ np.ascontiguousarray(d["W"][:, ::-1]).T)


@functools.lru_cache(maxsize=2)
def headq_inputs(K, N, bits, sb_f32, persistent):
    """-> dict(X, nw, s, m = quant_matrix with planted ties: pair i = two copies of the row that is batch row i's maximum, scales and biases
    doubled)"""
    base = quant_matrix(K, N, bits, sb_f32)
    X, nw = x_rows(K, "gauss", 1), norm_weight(K)
    s, amb, _ = rms_stage(X, nw)
    assert not amb.any()
    m = {k: v.copy() for k, v in base.items()}
    pairs = tie_pairs(N, persistent)
    w = (np.repeat(m["s"], 64, 1) * m["q"] + np.repeat(m["b"], 64, 1)).astype(np.float32)
    src = (s[:len(pairs)].astype(np.float32) @ w.T).argmax(1)
    for i, (lo, hi) in enumerate(pairs):
        for n in (lo, hi):
            m["q"][n], m["s"][n], m["b"][n] = base["q"][src[i]], 2.0 * base["s"][src[i]], 2.0 * base["b"][src[i]]
    m["words"] = quant_words(m["q"], bits)
    for v in m.values():
        v.setflags(write=False)
    return dict(X=X, nw=nw, s=s, m=m)


@functools.lru_cache(maxsize=2)
def headq_expect(K, N, bits, sb_f32, persistent):
    """the persistent quantised head multiplies like the tuned linear (q' = 16 + q at 4 bit), the generic one like gemvq_generic_kernel"""
    d = headq_inputs(K, N, bits, sb_f32, persistent)
    v, mag = np.empty((ROWS, N)), np.empty((ROWS, N))
    for n0 in range(0, N, 4096):
        mc = {k: a[n0:n0 + 4096] for k, a in d["m"].items()}
        v[:, n0:n0 + 4096], mag[:, n0:n0 + 4096] = quant_dot(d["s"], mc, bits, persistent)
    return v, mag


def headq_twin(d, bits, persistent):
    N = d["m"]["q"].shape[0]
    out = np.empty((ROWS, N), np.float32)
    for n0 in range(0, N, 4096):
        mc = {k: a[n0:n0 + 4096] for k, a in d["m"].items()}
        out[:, n0:n0 + 4096] = bf16_round(quant_dot(d["s"], mc, bits, persistent, np.float32)[0])
    return out


# ---- greedy tail and embedding lookups: exact restatements -------------------------------------------------------------------------------------------
FINALIZE, EMBED = 5, 6
NO_WINNER = 0x7fffffff
FINALIZE_MUTATIONS = ("append_finished", "ctx_not_advanced", "rope_current", "no_clamp")


def dequant_rows(m, rows):
    """dequantized(row) as quant_dequant_chunk computes it: bf16(fmaf(scale, q, bias)) -- the fma rounds to f32 (the float64 sum below is exact:
    24 x 8 bits plus a bias within 2^9 of the product), the store to bf16; with f32 scales the two roundings differ from one rounding of the
    exact value at about one element in 2^16 -> [len(rows), K]"""
    return bf16_round(f32(np.repeat(m["s"][rows], 64, 1) * m["q"][rows] + np.repeat(m["b"][rows], 64, 1)))


def table_rows(table, rows):
    """rows of a bf16 table (array) or of a quantised one (quant_matrix dict)"""
    return dequant_rows(table, rows) if isinstance(table, dict) else table[rows]


def finalize_inputs(B, n_parts, vocab, max_new, scenario, seed=0):
    """-> dict(pv f32 [B, n_parts], pi int32, tokens [B, max_new + 1], lens, finished, ctx_len, n_active, eos).  Partials are bf16-valued; every
    row's maximum stands in two parts, the lower index in the LATER part; rows 3 k + 1 are finished; row 0's winner is eos; row 2 (if any) is
    one token short of max_tokens = max_new - 1.  scenario "insane": unfinished rows 0 .. 5 hold +inf | NaN everywhere | -inf everywhere | a
    winner at index vocab | a negative index | NaN beside finite values (this last one is sane); "insane_finished": the same on finished rows"""
    rng = np.random.default_rng([B, n_parts, vocab, seed])
    pv = bf16_round(rng.standard_normal((B, n_parts)) * 4.0).astype(np.float32)
    pi = rng.integers(0, vocab, (B, n_parts)).astype(np.int32)
    top = np.float32(32.0)
    for b in range(B):
        p = rng.permutation(n_parts)[:2]
        pv[b, p] = top
        if n_parts > 1:
            lo, hi = sorted(p)
            pi[b, hi], pi[b, lo] = rng.integers(0, vocab // 2), rng.integers(vocab // 2, vocab)
    finished = (np.arange(B) % 3 == 1).astype(np.int32)
    eos = int(pi[0][pv[0] == top].min())
    lens = rng.integers(0, max_new - 3, B).astype(np.int32)
    if B > 2:
        lens[2] = max_new - 2
    if scenario != "plain":
        rows = [b for b in range(B) if finished[b] == (scenario == "insane_finished")][:6]
        for j, b in enumerate(rows):
            if j == 0:
                pv[b, n_parts // 2] = np.inf
            elif j == 1:
                pv[b] = np.nan
            elif j == 2:
                pv[b] = -np.inf
            elif j == 3:
                pi[b][pv[b] == top] = vocab
            elif j == 4:
                pi[b][pv[b] == top] = -5
            else:
                pv[b, 0 if pv[b, 0] != top else n_parts - 1] = np.nan
    tokens = rng.integers(0, vocab, (B, max_new + 1)).astype(np.int32)
    return dict(pv=pv, pi=pi, tokens=tokens, lens=lens, finished=finished, ctx_len=rng.integers(0, 40, B).astype(np.int32),
                n_active=int((finished == 0).sum()), eos=eos, max_tokens=max_new - 1, vocab=vocab, max_new=max_new)


def finalize_ref(d, table, rope_cos, rope_sin, advance_ctx, ignore_eos, mut=None):
    """greedy_finalize_kernel restated -> dict(tokens, lens, finished, ctx_len, n_active, err, x [B, H], cos_rows, sin_rows)"""
    B = d["pv"].shape[0]
    o = {k: d[k].copy() for k in ("tokens", "lens", "finished", "ctx_len")}
    o["n_active"], o["err"] = d["n_active"], 0
    toks = np.zeros(B, np.int64)
    o["cos_rows"], o["sin_rows"] = np.empty((B, rope_cos.shape[1]), np.float32), np.empty((B, rope_cos.shape[1]), np.float32)
    for b in range(B):
        best, bidx = -np.inf, NO_WINNER
        for v, n in zip(d["pv"][b], d["pi"][b]):
            if v > best or (v == best and n < bidx):
                best, bidx = float(v), int(n)
        in_vocab = 0 <= bidx < d["vocab"]
        sane = in_vocab and abs(best) <= 3.0e38
        tok = bidx if in_vocab or mut == "no_clamp" else 0
        fin, n = int(d["finished"][b]), int(d["lens"][b])
        if not sane and not fin:
            o["err"] = 1
        if advance_ctx and mut != "ctx_not_advanced":
            o["ctx_len"][b] += 1
        if not fin or mut == "append_finished":
            o["tokens"][b, n] = tok
            o["lens"][b] = n + 1
            if (tok == d["eos"] and not ignore_eos) or n + 1 >= d["max_tokens"]:
                if not fin:
                    o["n_active"] -= 1
                o["finished"][b] = 1
        pos = int(d["ctx_len"][b]) + (advance_ctx if mut != "rope_current" else 0)
        o["cos_rows"][b], o["sin_rows"][b] = rope_cos[pos], rope_sin[pos]
        toks[b] = tok
    o["x"] = table_rows(table, np.clip(toks, 0, (table["q"] if isinstance(table, dict) else table).shape[0] - 1))
    o["tok"] = toks
    return o

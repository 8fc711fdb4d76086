"""Float64 restatements, in plain numpy, of every operand gather and fused epilogue of the bf16 MFMA GEMM (csrc/gemm.h and the
epilogues of csrc/{ctc,enc,dec}_kernels.h), the deterministic inputs the CPU and GPU case tests share, and the bounds of
tests/test_gpu_gemm_cases.py.  All arithmetic is on the bf16-rounded inputs, so a reference differs from the device only by the
device's f32 accumulation, its f32 activation and the output rounding.

Bounds (each derived from the number formats, none from a device run):
  F32   |got - v| <= 2e-6 * mag + 1e-30, mag = sum_k |a_k w_k| + |bias| (+ |residual| or |position term|): the project's GEMM bound
        (tests/test_gpu_gemm.py: f32 accumulation over K <= 8192 in MFMA order); the extra f32 additions of an epilogue are 6e-8 of terms
        that mag already holds.  EpiPosConv: mag * 1.13 (the largest slope of GELU: d/dx x Phi(x) <= 1.129, at x = sqrt 2) plus
        2^-20 |v| for the device's f32 erf (eight f32 ulps).
  BF16  |got - v| <= (0.5 + 2^-6) ulp_bf16(|v| + e) + 1.13 e with e the F32 bound of the pre-activation value: round-to-nearest of an
        f32 value within 1.13 e of v; 2^-6 ulp (6e-5 relative) covers the f32 activation.
"""
import functools
import math
import numpy as np

F32_REL = 2e-6
GELU_SLOPE = 1.13

# case ids of include/qasr.h
(CONV, CONV_PLAIN, ROWTABLE, GROUPCONV, GROUPCONV_PLAIN, BIAS_BF16, BIAS_BF16_GELU, BIASF_BF16, BIASF_BF16_GELU, STORE_BF16, RESID_F32,
 RESID_F32F, RESID_BF16, POS_F32, SWIGLU) = range(15)


# ---- bf16 on float64 ---------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """nearest bf16 value (8 significant bits, ties to even) of float64 x, as float64; normal range only"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def bf16_bits(x):
    """bit patterns (uint16) of values that ARE bf16 values"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_from_bits(u):
    return (np.ascontiguousarray(u, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def ulp_bf16(x):
    """spacing of bf16 at |x| (the subnormal spacing 2^-133 below the normal range)"""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.maximum(np.where(x == 0, -125, e), -125) - 8)


def randn_bf16(rng, shape, scale=1.0):
    return bf16_round(rng.standard_normal(shape) * scale)


_erfc = np.frompyfunc(math.erfc, 1, 1)


def gelu(x):
    """exact GELU x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2 (no cancellation in the left tail)"""
    x = np.asarray(x, np.float64)
    return 0.5 * x * _erfc(-x / math.sqrt(2.0)).astype(np.float64)


def bound_f32(mag, v=None, gelu_out=False):
    if gelu_out:
        return F32_REL * GELU_SLOPE * mag + 2.0 ** -20 * np.abs(v) + 1e-30
    return F32_REL * mag + 1e-30


def bound_bf16(v, mag):
    e = F32_REL * mag + 1e-30
    return (0.5 + 2.0 ** -6) * ulp_bf16(np.abs(v) + e) + GELU_SLOPE * e


# ---- 3x3 / stride 2 / pad 1 convolution as a GEMM (AConv3x3s2, AConv3x3s2W, EpiConvGelu) ----------------------------------------------
def conv_out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def conv_im2col(x, hw_major):
    """x [n, H, W, C] -> [n * OH * OW, 9 C]: K index (kh * 3 + kw) * C + ci, zeros at padding taps; rows (img, oh, ow) or (img, ow, oh)"""
    n, H, W, C = x.shape
    OH, OW = conv_out_hw(H, W)
    xp = np.zeros((n, H + 2, W + 2, C))
    xp[:, 1:H + 1, 1:W + 1] = x
    cols = np.empty((n, OH, OW, 9, C))
    for kh in range(3):
        for kw in range(3):
            cols[:, :, :, kh * 3 + kw] = xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][:, :OH, :OW]
    if not hw_major:
        cols = cols.transpose(0, 2, 1, 3, 4)
    return np.ascontiguousarray(cols.reshape(n * OH * OW, 9 * C))


def conv_row_ow(n, H, W, hw_major):
    """output column ow and image of every GEMM row"""
    OH, OW = conv_out_hw(H, W)
    img, oh, ow = np.meshgrid(np.arange(n), np.arange(OH), np.arange(OW), indexing="ij")
    if not hw_major:
        img, ow = img.transpose(0, 2, 1), ow.transpose(0, 2, 1)
    return ow.reshape(-1), img.reshape(-1)


def conv_ref(x, w, bias, valid, hw_major):
    """-> (pre-activation acc + bias, gelu of it with zeros at ow >= valid[img], mag, masked rows)"""
    A = conv_im2col(x, hw_major)
    pre = A @ w.T + bias
    mag = np.abs(A) @ np.abs(w).T + np.abs(bias)
    ow, img = conv_row_ow(x.shape[0], x.shape[1], x.shape[2], hw_major)
    masked = ow >= np.asarray(valid)[img]
    v = gelu(pre)
    v[masked] = 0.0
    return pre, v, mag, masked


# ---- grouped Conv1d of the wav2vec2 positional encoder (AGroupConv1d, EpiPosConv) ----------------------------------------------------
def frame_info(lens):
    """per packed frame (t, L) of its clip, int32 [frames, 2]"""
    return np.array([(t, L) for L in lens for t in range(L)], np.int32).reshape(-1, 2)


def groupconv_im2col(x, lens, KP, cpg, g):
    """x [frames, D] -> [frames, KP * cpg] of group g: K index tap * cpg + ci, source frame t - KP / 2 + tap of the SAME clip or zero"""
    info = frame_info(lens)
    M = info.shape[0]
    t, L = info[:, 0], info[:, 1]
    A = np.zeros((M, KP, cpg))
    for tap in range(KP):
        src = t - KP // 2 + tap
        ok = (src >= 0) & (src < L)
        A[ok, tap] = x[(np.arange(M) - KP // 2 + tap)[ok], g * cpg:(g + 1) * cpg]
    return A.reshape(M, KP * cpg)


def groupconv_ref(x, w, bias, lens, KP, cpg, groups):
    """w [groups, cpg, KP * cpg] -> (acc + bias [frames, D], mag): kernel KP, padding KP / 2, the trailing frame trimmed"""
    pre = np.empty((x.shape[0], groups * cpg))
    mag = np.empty_like(pre)
    for g in range(groups):
        A = groupconv_im2col(x, lens, KP, cpg, g)
        sl = slice(g * cpg, (g + 1) * cpg)
        pre[:, sl] = A @ w[g].T + bias[sl]
        mag[:, sl] = np.abs(A) @ np.abs(w[g]).T + np.abs(bias[sl])
    return pre, mag


# ---- SwiGLU mode (gemm_nt_swiglu, gemm_swiglu) ---------------------------------------------------------------------------------------
def swiglu_split(acc):
    """[M, N] with weight rows in blocks of 16 gate + 16 up -> (gate, up), each [M, N / 2]"""
    M, N = acc.shape
    b = acc.reshape(M, N // 32, 2, 16)
    return b[:, :, 0].reshape(M, N // 2), b[:, :, 1].reshape(M, N // 2)


def swiglu_ref(A, W):
    """the kernel's rounding points in float64: g = bf16(g), u = bf16(u), sg = bf16(g sigmoid(g)), out = bf16(sg u)"""
    g, u = swiglu_split(A @ W.T)
    g, u = bf16_round(g), bf16_round(u)
    sg = bf16_round(g / (1.0 + np.exp(-g)))
    return bf16_round(sg * u)


def swiglu_twin_f32(A, W):
    """the same with np.float32 accumulation over the REVERSED K axis and an f32 sigmoid: a second honest f32 realisation"""
    a32 = np.ascontiguousarray(A[:, ::-1], np.float32)
    w32 = np.ascontiguousarray(W[:, ::-1], np.float32)
    g, u = swiglu_split(a32 @ w32.T)
    g, u = bf16_round(g).astype(np.float32), bf16_round(u).astype(np.float32)
    sg = bf16_round(g / (np.float32(1.0) + np.exp(-g))).astype(np.float32)
    return bf16_round(sg * u)


SWIGLU_SHAPES = [(M, N, K) for M in (1, 129, 257) for N in (32, 96, 1056) for K in (64, 1000)]


@functools.lru_cache(maxsize=None)
def swiglu_inputs(M, N, K, coherent=False):
    """Two input sets per shape, each for the check whose premise it meets.
    coherent=False: Gaussian operands like every other case -- the mismatch SHARE is measured on these (device against 3 x the f32 twin).
    coherent=True: A >= 0 and every weight row of one sign, scaled so that gate and up values spread over +-[0.25, 4]: every accumulator
    is +-sum |a w|, free of cancellation, so its f32 error (2e-6 relative) is far below half a bf16 ulp (2e-3) of ITSELF -- the premise of
    the THREE-ULP bound (each of the three roundings may flip by one ulp of its own value).  With Gaussian operands a gate or up value
    that cancels to 1e-6 of sum |a w| moves by many of its own ulps under any f32 summation order: the f32 twin leaves the three ulps
    at 2 of the 458 208 Gaussian outputs (35 ulps at an up value of 3e-7 under sum |a w| = 5)."""
    rng = np.random.default_rng(M * 11 + N * 5 + K)
    if not coherent:
        return randn_bf16(rng, (M, K)), randn_bf16(rng, (N, K), 1.0 / math.sqrt(K))
    A = np.abs(randn_bf16(rng, (M, K)))
    row = rng.choice([-1.0, 1.0], N) * 2.0 ** rng.uniform(-2, 2, N) / (0.6366 * K)        # E|a| E|w| = 2 / pi
    return A, bf16_round(np.abs(rng.standard_normal((N, K))) * row[:, None])


def ulps_bf16(a, b):
    """distance in bf16 ulps (of the larger magnitude)"""
    return np.abs(a - b) / ulp_bf16(np.maximum(np.abs(a), np.abs(b)))


@functools.lru_cache(maxsize=None)
def swiglu_twin_share():
    """share of the Gaussian outputs, pooled over SWIGLU_SHAPES, where the f32 twin is not bit-equal to the float64 reference"""
    diff = total = 0
    for s in SWIGLU_SHAPES:
        A, W = swiglu_inputs(*s)
        ref = swiglu_ref(A, W)
        diff += int((swiglu_twin_f32(A, W) != ref).sum())
        total += ref.size
    return diff / total


# ---- dense x epilogue ---------------------------------------------------------------------------------------------------------------
DENSE_SHAPES = [(1, 4, 8), (1, 16, 64), (17, 20, 72), (129, 260, 1000), (256, 256, 64), (257, 512, 128), (300, 1028, 192), (511, 100, 4320)]


@functools.lru_cache(maxsize=None)
def dense_inputs(M, N, K):
    """-> dict of the shared operands of one shape and their float64 product; never modified by a test"""
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A, W = randn_bf16(rng, (M, K)), randn_bf16(rng, (N, K), 1.0 / math.sqrt(K))
    d = dict(A=A, W=W, acc=A @ W.T, mag=np.abs(A) @ np.abs(W).T, bias_bf16=randn_bf16(rng, N),
             bias_f32=rng.standard_normal(N).astype(np.float32).astype(np.float64),
             resid_f32=rng.standard_normal((M, N)).astype(np.float32).astype(np.float64), resid_bf16=randn_bf16(rng, (M, N)),
             n_t=13, tok_t=rng.integers(0, 13, M).astype(np.int32), pe=rng.standard_normal((13, N)).astype(np.float32).astype(np.float64))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def dense_ref(which, d, with_bias=True):
    """-> (v, mag) of an f32-output epilogue, (v, mag of the pre-activation value) of a bf16-output one; RESID_BF16: see resid_bf16_candidates"""
    acc, mag = d["acc"], d["mag"]
    if which in (BIAS_BF16, BIAS_BF16_GELU, BIASF_BF16, BIASF_BF16_GELU):
        b = (d["bias_bf16"] if which in (BIAS_BF16, BIAS_BF16_GELU) else d["bias_f32"]) if with_bias else np.zeros(acc.shape[1])
        pre = acc + b
        return (gelu(pre) if which in (BIAS_BF16_GELU, BIASF_BF16_GELU) else pre), mag + np.abs(b)
    if which == STORE_BF16:
        return acc, mag
    if which in (RESID_F32, RESID_F32F):
        b = d["bias_bf16"] if which == RESID_F32 else d["bias_f32"]
        return d["resid_f32"] + acc + b, mag + np.abs(b) + np.abs(d["resid_f32"])
    if which == POS_F32:
        p = d["pe"][d["tok_t"]]
        return acc + p, mag + np.abs(p)
    raise ValueError(which)


def resid_bf16_candidates(d):
    """EpiResidBf16: x = bf16(x + bf16(acc)).  The inner rounding is of the device's f32 acc, which lies within e = 2e-6 mag of the float64
    acc; rounding is monotonic, so bf16(acc_dev) lies in [bf16(acc - e), bf16(acc + e)] (one value, or two neighbours when acc is within e
    of a rounding tie) -> the float64 values x + that, low and high, and the magnitude for the outer BF16 bound"""
    e = F32_REL * d["mag"] + 1e-30
    return d["resid_bf16"] + bf16_round(d["acc"] - e), d["resid_bf16"] + bf16_round(d["acc"] + e), d["mag"] + np.abs(d["resid_bf16"])

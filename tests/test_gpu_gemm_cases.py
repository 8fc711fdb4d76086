"""Every operand gather and fused epilogue of the bf16 MFMA GEMM by itself, through qasr_gemm_case_probe (csrc/gemm_cases.hip: the
product's own functor types through the product's own launch entries), against the float64 restatements of tests/gemm_cases.py.

  a. gathers, no tolerance: AConv3x3s2 / AConv3x3s2W / ARowTable / AGroupConv1d with EpiBiasF32 are BIT-EQUAL to qasr_gemm_probe on the
     operand materialised in numpy (im2col with zeros at the padding taps, gathered rows, per-group im2col: same k order, same zeros);
     AConv3x3s2 == AConv3x3s2W; every form (128x128 double / single buffer, 256x256 ping-pong, the engine's pick) == every other, per case.
  b. f32 outputs: |got - v| <= 2e-6 mag + 1e-30 (gemm_cases.bound_f32; EpiPosConv: 1.13 mag and + 2^-20 |v|).
  c. bf16 outputs: |got - v| <= (0.5 + 2^-6) ulp_bf16(|v| + e) + 1.13 e (gemm_cases.bound_bf16).  EpiResidBf16 rounds twice,
     bf16(x + bf16(acc)): the inner rounding is monotonic in acc, so the value lies between the two float64 values formed with
     bf16(acc - e) and bf16(acc + e) (gemm_cases.resid_bf16_candidates; they coincide unless acc is within e of a rounding tie) and the
     bound applies below the lower and above the upper one.
  d. EpiConvGelu's masked columns are +0 bit patterns; rows >= M of an oversized, sentinel-filled output are untouched (every dense case).
  e. SwiGLU: within 3 bf16 ulps of the float64 reference with the kernel's rounding points on cancellation-free inputs; on Gaussian
     inputs the share of outputs not bit-equal to it is at most 3 x the share of the f32 twin (gemm_cases.swiglu_twin_share, 0.0166 %,
     measured on the CPU by tests/test_gemm_cases_cpu.py on the same inputs; see gemm_cases.swiglu_inputs for why two input sets).
Derivations: the docstring of tests/gemm_cases.py.  No bar comes from a device run.

Measured distances: every test prints its worst distance as a fraction of its bound (pytest -s).  On the CPU, an honest f32
realisation (numpy f32 products with the K axis reversed, put through these same tests in place of the device) sits at <= 0.07 of the
F32 bound and <= 0.97 of the BF16 bound (the half ulp of the output rounding is most of that bound), 2 bf16 ulps and 1.0 x the twin's
share in SwiGLU.  No MI355X figure is recorded here yet: this module was written while no GPU could be had.
"""
import ctypes as C
import numpy as np
import pytest
import gemm_cases as G
import gpu_util
from qasr import _lib

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2, -1)
P16 = C.POINTER(C.c_uint16)
BF16_OUT = {G.CONV, G.BIAS_BF16, G.BIAS_BF16_GELU, G.BIASF_BF16, G.BIASF_BF16_GELU, G.STORE_BF16, G.RESID_BF16, G.SWIGLU}
BF16_BIAS = {G.BIAS_BF16, G.BIAS_BF16_GELU, G.RESID_F32}


@pytest.fixture(scope="module")
def eng():
    e = gpu_util.Engine("tiny", max_audio_seconds=2)
    yield e
    e.close()


def _probe(eng, which, form, a_op, w_op, bias, out, aux_i=None, aux_l=None, aux_f=None, expect_ok=True, **geom):
    """a_op, w_op, bias as float64 arrays of bf16 / f32 values; `out` is the [rows, ld] buffer in its device dtype (uint16 bits or float32), updated in
    place.  -> the status when expect_ok is False"""
    g = _lib.QasrGemmCase(**geom)
    A16, W16 = G.bf16_bits(a_op), G.bf16_bits(w_op)
    b = None if bias is None else (G.bf16_bits(bias) if which in BF16_BIAS else np.ascontiguousarray(bias, np.float32))
    ai = None if aux_i is None else np.ascontiguousarray(aux_i, np.int32)
    al = None if aux_l is None else np.ascontiguousarray(aux_l, np.int64)
    af = None if aux_f is None else np.ascontiguousarray(aux_f, np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rc = eng.lib.qasr_gemm_case_probe(eng.h, which, form, C.byref(g), ptr(A16, P16), ptr(W16, P16), ptr(b, C.c_void_p),
                                      ptr(ai, C.POINTER(C.c_int32)), ptr(al, C.POINTER(C.c_int64)), ptr(af, C.POINTER(C.c_float)),
                                      ptr(out, C.c_void_p))
    if expect_ok:
        eng.check(rc)
    return rc


def _dense_probe(eng, A, W, bias, form=1):
    """qasr_gemm_probe on a materialised operand: the yardstick of part a"""
    M, K = A.shape
    N = W.shape[0]
    out = np.empty((M, N), np.float32)
    A16, W16, b = G.bf16_bits(A), G.bf16_bits(W), np.ascontiguousarray(bias, np.float32)
    eng.check(eng.lib.qasr_gemm_probe(eng.h, A16.ctypes.data_as(P16), W16.ctypes.data_as(P16), b.ctypes.data_as(C.POINTER(C.c_float)), M, N, K,
                                      form, 1, out.ctypes.data_as(C.POINTER(C.c_float)), None))
    return out


def _same_bits(outs, what):
    first = outs[0][1]
    for key, o in outs[1:]:
        assert np.array_equal(first.view(np.uint8), o.view(np.uint8)), (what, outs[0][0], key)


def _check_f32(got, v, mag, what, **kw):
    bound = G.bound_f32(mag, v, **kw)
    frac = float((np.abs(got.astype(np.float64) - v) / bound).max())
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


def _check_bf16(bits, v, mag, what, v_hi=None):
    got = G.bf16_from_bits(bits)
    hi = v if v_hi is None else v_hi
    over = np.maximum((v - got) / G.bound_bf16(v, mag), (got - hi) / G.bound_bf16(hi, mag))
    frac = float(over.max())
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


# ---- conv ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4), (16, 25), (32, 13)])
@pytest.mark.parametrize("Cc", [8, 64, 72, 480])
def test_conv(eng, Cc, H, W, n_img):
    rng = np.random.default_rng(Cc * 131 + H * 17 + W * 3 + n_img)
    N, K = Cc, 9 * Cc
    x, w = G.randn_bf16(rng, (n_img, H, W, Cc)), G.randn_bf16(rng, (N, K), K ** -0.5)
    bias = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    OH, OW = G.conv_out_hw(H, W)
    M = n_img * OH * OW
    valid = [max(OW - 1, 0)] if n_img == 1 else [0, min(1, OW), OW]
    wides = (0, 1) if Cc >= 64 else (0,)
    worst_b = worst_c = 0.0
    for hw_major in (1, 0):
        geom = dict(M=M, N=N, K=K, n_img=n_img, H=H, W=W, C=Cc, hw_major=hw_major, level=2 if hw_major else 3)
        pre, v, mag, masked = G.conv_ref(x, w, bias, valid, bool(hw_major))
        plain, act = [], []
        for wide in wides:
            for form in FORMS:
                o = np.full((M, N), np.nan, np.float32)
                _probe(eng, G.CONV_PLAIN, form, x, w, bias, o, wide=wide, **geom)
                plain.append(((wide, form), o))
                o = np.full((M, N), 0x7fc1, np.uint16)
                _probe(eng, G.CONV, form, x, w, bias, o, aux_i=valid, wide=wide, **geom)
                act.append(((wide, form), o))
        plain.append(("materialised", _dense_probe(eng, G.conv_im2col(x, bool(hw_major)), w, bias)))
        _same_bits(plain, ("conv-plain", hw_major))
        _same_bits(act, ("conv", hw_major))
        worst_b = max(worst_b, _check_f32(plain[0][1], pre, mag, ("conv-plain", hw_major)))
        worst_c = max(worst_c, _check_bf16(act[0][1], v, mag, ("conv", hw_major)))
        assert (act[0][1][masked] == 0).all(), "masked columns must be +0"
    print(f"conv C={Cc} {H}x{W} x{n_img}: plain {worst_b:.3f} of the F32 bound, gelu {worst_c:.3f} of the BF16 bound")


# ---- rowtable ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 132])
@pytest.mark.parametrize("M", [1, 129, 300])
@pytest.mark.parametrize("K", [8, 72, 2560])
def test_rowtable(eng, K, M, N):
    rng = np.random.default_rng(K + M * 5 + N)
    stride = {8: 8, 72: 16, 2560: 24}[K]                     # rows overlap (stride < K) wherever 16-byte alignment allows it
    a = G.randn_bf16(rng, (M - 1) * stride + K + 40)
    off = (((np.arange(M) * 7 + 3) % M) * stride).astype(np.int64) if M % 7 else np.arange(M)[::-1] * stride   # non-monotonic
    off[M // 2] += 40                                        # and not an arithmetic sequence
    assert M < 3 or (np.diff(off) < 0).any()
    w, bias = G.randn_bf16(rng, (N, K), K ** -0.5), rng.standard_normal(N).astype(np.float32).astype(np.float64)
    A = a[off[:, None] + np.arange(K)[None, :]]
    outs = []
    for form in FORMS:
        o = np.full((M, N), np.nan, np.float32)
        _probe(eng, G.ROWTABLE, form, a, w, bias, o, aux_l=off, M=M, N=N, K=K, a_len=a.size)
        outs.append((form, o))
    outs.append(("materialised", _dense_probe(eng, A, w, bias)))
    _same_bits(outs, "rowtable")
    frac = _check_f32(outs[0][1], A @ w.T + bias, np.abs(A) @ np.abs(w).T + np.abs(bias), "rowtable")
    print(f"rowtable {M}x{N}x{K}: {frac:.3f} of the F32 bound")


# ---- groupconv -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["edges", "rows>128"])
@pytest.mark.parametrize("groups", [2, 4])
@pytest.mark.parametrize("KP,cpg", [(4, 8), (8, 16), (128, 64), (128, 80)])
def test_groupconv(eng, KP, cpg, groups, batch):
    rng = np.random.default_rng(KP + cpg * 3 + groups)
    # every tap range clips at a clip border with another clip's frames right behind it
    lens = [L for L in (KP // 2 + 1, 1, KP + 3, 2, KP // 2 - 1, KP // 2) if L > 0] if batch == "edges" else [67, 3, KP // 2 + 2, 64]
    M, D, K = sum(lens), groups * cpg, KP * cpg
    assert batch == "edges" or M > 128
    x = G.randn_bf16(rng, (M, D))
    w = G.randn_bf16(rng, (groups, cpg, K), K ** -0.5)
    bias = rng.standard_normal(D).astype(np.float32).astype(np.float64)
    resid = rng.standard_normal((M, D)).astype(np.float32).astype(np.float64)
    info = G.frame_info(lens)
    geom = dict(M=M, N=cpg, K=K, KP=KP, cpg=cpg, groups=groups)
    plain, pos = [], []
    for form in (-1, 1):
        o = np.full((M, D), np.nan, np.float32)
        _probe(eng, G.GROUPCONV_PLAIN, form, x, w, bias, o, aux_i=info, **geom)
        plain.append((form, o))
        o = np.full((M, D), np.nan, np.float32)
        _probe(eng, G.GROUPCONV, form, x, w, bias, o, aux_i=info, aux_f=resid, **geom)
        pos.append((form, o))
    mat = np.concatenate([_dense_probe(eng, G.groupconv_im2col(x, lens, KP, cpg, g), w[g], bias[g * cpg:(g + 1) * cpg])
                          for g in range(groups)], axis=1)
    plain.append(("materialised", mat))
    _same_bits(plain, "groupconv-plain")
    _same_bits(pos, "groupconv")
    pre, mag = G.groupconv_ref(x, w, bias, lens, KP, cpg, groups)
    fb = _check_f32(plain[0][1], pre, mag, "groupconv-plain")
    v = G.gelu(pre) + resid
    fp = _check_f32(pos[0][1], v, mag + np.abs(resid), "groupconv", gelu_out=True)
    print(f"groupconv KP={KP} cpg={cpg} x{groups} {batch}: plain {fb:.3f}, EpiPosConv {fp:.3f} of the F32 bound")


# ---- dense x epilogue ----------------------------------------------------------------------------------------------------------------
DENSE_CASES = [("bias_bf16", G.BIAS_BF16, True), ("bias_bf16_nobias", G.BIAS_BF16, False), ("bias_bf16_gelu", G.BIAS_BF16_GELU, True),
               ("bias_bf16_gelu_nobias", G.BIAS_BF16_GELU, False), ("biasf_bf16", G.BIASF_BF16, True), ("biasf_bf16_gelu", G.BIASF_BF16_GELU, True),
               ("store_bf16", G.STORE_BF16, True), ("resid_f32", G.RESID_F32, True), ("resid_f32f", G.RESID_F32F, True),
               ("resid_bf16", G.RESID_BF16, True), ("pos_f32", G.POS_F32, True)]


@pytest.mark.parametrize("M,N,K", G.DENSE_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in G.DENSE_SHAPES])
@pytest.mark.parametrize("name,which,with_bias", DENSE_CASES, ids=[c[0] for c in DENSE_CASES])
def test_dense_epilogue(eng, name, which, with_bias, M, N, K):
    d = G.dense_inputs(M, N, K)
    ld = N + 12 if M % 2 else N                              # 1, 17, 129, 257, 511 rows: a row stride larger than N
    rows = M + 3                                             # rows >= M must come back as they went in
    bf16_out = which in BF16_OUT
    if which in (G.RESID_F32, G.RESID_F32F):
        init = np.full((rows, ld), -777.25, np.float32)
        init[:M, :N] = d["resid_f32"]
    elif which == G.RESID_BF16:
        init = np.full((rows, ld), 0xc3c2, np.uint16)
        init[:M, :N] = G.bf16_bits(d["resid_bf16"])
    else:
        init = np.full((rows, ld), 0xc3c2, np.uint16) if bf16_out else np.full((rows, ld), -777.25, np.float32)
    bias = None
    if with_bias and which in (G.BIAS_BF16, G.BIAS_BF16_GELU, G.RESID_F32):
        bias = d["bias_bf16"]
    elif which in (G.BIASF_BF16, G.BIASF_BF16_GELU, G.RESID_F32F):
        bias = d["bias_f32"]
    aux_i = aux_f = None
    geom = dict(M=M, N=N, K=K, ld=ld, out_rows=rows)
    if which == G.POS_F32:
        pe = np.zeros((d["n_t"], ld), np.float32)
        pe[:, :N] = d["pe"]
        aux_i, aux_f, geom["n_t"] = d["tok_t"], pe, d["n_t"]
    outs = []
    for form in FORMS:
        o = init.copy()
        _probe(eng, which, form, d["A"], d["W"], bias, o, aux_i=aux_i, aux_f=aux_f, **geom)
        outs.append((form, o))
    _same_bits(outs, name)
    got = outs[0][1]
    assert np.array_equal(got[M:], init[M:]) and np.array_equal(got[:, N:], init[:, N:]), "wrote outside [M, N]"
    if which == G.RESID_BF16:
        lo, hi, mag = G.resid_bf16_candidates(d)
        frac = _check_bf16(got[:M, :N], lo, mag, name, v_hi=hi)
    else:
        v, mag = G.dense_ref(which, d, with_bias)
        frac = _check_bf16(got[:M, :N], v, mag, name) if bf16_out else _check_f32(got[:M, :N], v, mag, name)
    print(f"{name} {M}x{N}x{K}: {frac:.3f} of the {'BF16' if bf16_out else 'F32'} bound")


# ---- swiglu --------------------------------------------------------------------------------------------------------------------------
def _swiglu_run(eng, A, W, M, N, K, what):
    outs = []
    for form in FORMS:
        o = np.full((M + 1, N // 2 + 4), 0xc3c2, np.uint16)
        _probe(eng, G.SWIGLU, form, A, W, None, o, M=M, N=N, K=K, ld=N // 2 + 4, out_rows=M + 1)
        outs.append((form, o))
    _same_bits(outs, what)
    assert (outs[0][1][M:] == 0xc3c2).all() and (outs[0][1][:, N // 2:] == 0xc3c2).all(), "wrote outside [M, N / 2]"
    return G.bf16_from_bits(outs[0][1][:M, :N // 2])


def test_swiglu(eng):
    worst = 0.0
    diff = total = beyond = 0
    for M, N, K in G.SWIGLU_SHAPES:
        A, W = G.swiglu_inputs(M, N, K, coherent=True)
        got = _swiglu_run(eng, A, W, M, N, K, ("swiglu coherent", M, N, K))
        ulps = float(G.ulps_bf16(got, G.swiglu_ref(A, W)).max())
        assert ulps <= 3, (M, N, K, ulps)
        worst = max(worst, ulps)
        A, W = G.swiglu_inputs(M, N, K)
        got, ref = _swiglu_run(eng, A, W, M, N, K, ("swiglu gaussian", M, N, K)), G.swiglu_ref(A, W)
        diff += int((got != ref).sum())
        beyond += int((G.ulps_bf16(got, ref) > 3).sum())
        total += ref.size
    share, twin = diff / total, G.swiglu_twin_share()
    print(f"swiglu: cancellation-free inputs worst {worst:.0f} bf16 ulps; Gaussian inputs {share * 100:.4f} % of {total} outputs differ "
          f"({beyond} by more than 3 ulps), f32 twin {twin * 100:.4f} %")
    assert share <= 3 * twin, (share, twin)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(eng):
    z = np.zeros(4096)
    o = np.zeros(4096, np.float32)
    bad = lambda which, form=-1, **kw: _probe(eng, which, form, z, z, kw.pop("bias", z), o, expect_ok=False,
                                              aux_i=kw.pop("aux_i", np.zeros(64, np.int32)), aux_l=kw.pop("aux_l", np.zeros(64, np.int64)),
                                              aux_f=kw.pop("aux_f", np.zeros(4096, np.float32)), **kw)
    conv = dict(M=2, N=8, K=72, n_img=1, H=2, W=3, C=8, hw_major=1, level=2)
    assert bad(G.CONV, **conv) == 0 and bad(G.CONV_PLAIN, **conv) == 0
    assert bad(G.CONV, **{**conv, "C": 12, "K": 108}) != 0                       # C % 8
    assert bad(G.CONV, **{**conv, "wide": 1}) != 0                               # AConv3x3s2W with C < 64
    assert bad(G.CONV, **{**conv, "N": 6}) != 0                                  # N % 4
    assert bad(G.CONV, **{**conv, "M": 3}) != 0 and bad(G.CONV, **{**conv, "level": 1}) != 0 and bad(G.CONV, form=3, **conv) != 0
    assert bad(G.SWIGLU, M=4, N=32, K=8) == 0 and bad(G.SWIGLU, M=4, N=48, K=8) != 0 and bad(G.SWIGLU, M=4, N=16, K=8) != 0
    grp = dict(M=2, N=8, K=32, KP=4, cpg=8, groups=2)
    info = np.array([0, 2, 1, 2], np.int32)
    assert bad(G.GROUPCONV, aux_i=info, **grp) == 0 and bad(G.GROUPCONV, form=1, aux_i=info, **grp) == 0
    assert bad(G.GROUPCONV, form=2, aux_i=info, **grp) != 0 and bad(G.GROUPCONV_PLAIN, form=2, aux_i=info, **grp) != 0   # no_p8
    assert bad(G.GROUPCONV, aux_i=np.array([0, 2, 1, 3], np.int32), **grp) != 0   # a clip that ends outside the packed frames
    assert bad(G.GROUPCONV, aux_i=info, **{**grp, "cpg": 4, "N": 4, "K": 16}) != 0
    row = dict(M=2, N=4, K=8, a_len=16)
    assert bad(G.ROWTABLE, aux_l=np.array([8, 0], np.int64), **row) == 0
    assert bad(G.ROWTABLE, aux_l=np.array([8, 9], np.int64), **row) != 0 and bad(G.ROWTABLE, aux_l=np.array([4, 0], np.int64), **row) != 0
    assert bad(G.ROWTABLE, aux_l=np.array([-8, 0], np.int64), **row) != 0
    assert bad(G.POS_F32, aux_i=np.array([0, 1], np.int32), M=2, N=4, K=8, n_t=2) == 0
    assert bad(G.POS_F32, aux_i=np.array([0, 2], np.int32), M=2, N=4, K=8, n_t=2) != 0
    assert bad(G.STORE_BF16, M=2, N=4, K=8, ld=6) != 0 and bad(G.STORE_BF16, M=2, N=4, K=8, out_rows=1) != 0
    assert bad(G.STORE_BF16, M=2, N=4, K=12) != 0 and bad(G.BIASF_BF16, bias=None, M=2, N=4, K=8) != 0 and bad(15, M=2, N=4, K=8) != 0
    assert bad(G.BIAS_BF16, bias=None, M=2, N=4, K=8) == 0
    assert b"gemm case" in eng.lib.qasr_last_error(eng.h)

"""Float64 references, inputs, bounds and cases for the f32 kernels the waveform codecs share (csrc/codec_shared.h), each run alone through
qasr_codec_case_probe: codec_gemm_kernel<Rows, SNAKE, EPI> behind its four row locators (TILE), codec_rms_kernel (RMS) and
codec_dwln_kernel<Rows> (DWLN); and for codec_out_kernel (OUT), cenc_in_kernel (CENC_IN), codec_gather_kernel (GATHER), cenc_vq_kernel
(VQ), codec_attn_kernel (ATTN_DEC), cenc_attn_kernel (ATTN_ENC), vae_dw_kernel (VAE_DW) and vae_unit_kernel (VAE_UNIT), whose sections
below say what is checked.  Shared by tests/test_codec_cases_cpu.py and tests/test_gpu_codec_cases.py.  No bar comes from a device run.

References are written from the operation, window by window: a window's (clip's) input rows are cut out, the SnakeBeta map
x + b sin^2(a x) is applied, (taps - 1) dil rows of zeros are put in front, and output row t is sum_j Xpad[last(t) + j dil] W[:, :, j]^T
with the weight in its textbook layout W [N][C_in][taps]; last(t) = t for a conv, t stride for the encoder's strided conv, (t + 1) s - 1
for the AudioVAE's strided conv (k = 2 s).  The packing Wt[j C_in + c][n] = W[n][c][j] is done here, so it is part of what is checked;
conv_ref / tconv_ref are the textbook strided and transposed convs (torch conv1d / an explicit scatter in float64) that the CPU module
holds the window reference to.  tile_eval is a second float64 evaluation that walks the LOCATOR ARRAYS row by row as the launch is told
about them; the CPU module holds the two to each other and uses tile_eval's `mut` for the mutation condition.

Bounds.  u = 2^-24.  An output of the tile is one thread's fmaf chain over k = 0 .. K - 1 (absent rows and the K tail add exact zeros):
    d_acc = (K + 1) u (S + |bias|) + dS (1 + 2^-10),   S = sum |a w|, dS = sum |da| |w|
the + 1 is the bias add; da is the error of an operand that went through the snake load, from its five f32 operations and sinf:
    da = |b| (2 |s| ds + 2 u s^2) + u |snake|,   ds = u |a x| + T_sin 2^-23 |s|      (cos <= 1; s = sin(a x))
d_acc is carried through each epilogue's derivative and the epilogue's own operations are added (e of the issue's (K + e)):
    E_LIN     nothing more
    E_GELU    g(v) = 0.5 v (1 + erf(v c)): |g'| d_acc + |0.5 v| (d_erf + u |1 + erf|) + u |g|, d_erf = (2 / sqrt(pi)) exp(-(v c)^2) 2 u |v c|
              + T_erf 2^-23 |erf| (the product v c and the rounding of the constant c)
    E_RES     d_acc + u |v + R|
    E_LSRES   |ls| d_acc + u |v ls| + u |v ls + R|
    E_SWIGLU  silu(g) up: |up| d_silu + |silu| d_up + u |out|, d_silu = |silu'| d_g + |silu| ((T_exp 2^-23 e + u (1 + e)) / (1 + e) + DIV),
              e = exp(-g)
    E_RESMAP  t = (v [+ R]) [ls + ls2], out = snake(t): (1 + |a b|) d_t + the snake's own error as da above
DIV = 5 u is granted to each f32 division and sqrtf: HIP's default is the correctly rounded form (u); 2.5 ulp is what the inexact forms
the compiler may choose instead are specified to.  The row kernels (RMS, DWLN) reduce a row as codec_shared.h states: a thread's
sequential partial over c = tid, tid + 256, .. (P = ceil(C / 256) terms, a product and an add each), then an 8-level tree; see rms_ref
and dwln_ref for the propagation.

The one ingredient not derived here is the error of the device's sinf, expf and erff.  ULP_CPU is the largest distance, in ulps of the f32
result, of torch's f32 functions from float64 over the arguments the twins of EVERY op form on their cases: the snakes of the tile, of
OUT, VAE_DW and VAE_UNIT, the expf of E_SWIGLU and of both attention kernels, the erff of E_GELU (measured and asserted by the CPU module); the
device's math library is a different implementation and is granted T = 4 x that per call.  |a x| of every snake stays below 8 by
construction (SNAKE_A).

Cases are the smallest shapes at which each guard of the kernels is live, never a model's geometry; every (Rows, SNAKE, EPI) of
CODEC_TILE_COMBOS (csrc/codec_launch.h) is launched with M and N off the 64-wide tile.  Under TailRows a wholly dead LAST PARTIAL tile
cannot exist: a window's last row is always live (kept lies inside its window), which is what the kernel's skip relies on; the case
tail_lead1 holds a last partial tile of which only the last three rows are live.
"""
import functools
import math
import re
import os
import numpy as np
import torch

TILE, RMS, DWLN, GATHER, OUT, CENC_IN, VQ, ATTN_DEC, ATTN_ENC, VAE_DW, VAE_UNIT = range(11)
WINDOW, TAIL, CLIP, VSTRIDE = 0, 1, 2, 3
ROWS_NAMES = {"WindowRows": WINDOW, "TailRows": TAIL, "ClipRows": CLIP, "VaeStrideRows": VSTRIDE}
E_LIN, E_GELU, E_RES, E_LSRES, E_SWIGLU, E_RESMAP = range(6)
EPI_NAMES = {"E_LIN": E_LIN, "E_GELU": E_GELU, "E_RES": E_RES, "E_LSRES": E_LSRES, "E_SWIGLU": E_SWIGLU, "E_RESMAP": E_RESMAP}
U = 2.0 ** -24
DIV = 5 * U
SENTINEL = np.float32(-7.5e7)
POISON = np.array([1e30, -1e30, np.nan, 1e30], np.float32)
ULP_CPU = dict(sin=0.60, exp=0.55, erf=0.55)          # measured: test_transcendental_ulps_of_the_cpu (MEASURED_CPU of the CPU module)
T_ULP = {k: 4.0 * v for k, v in ULP_CPU.items()}
SNAKE_A = 1.6                                          # a = exp(alpha) in (1 / 1.6, 1.6): |a x| < 8 for |x| < 5
RMS_EPS = 1e-8
CG_T = 64
EXTRA = 2                                              # sentinel rows the GPU module puts after every launch's rows


def combos_of_the_dispatch():
    """the (rows, snake, epi) of CODEC_TILE_COMBOS, read from csrc/codec_launch.h"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "qwen3-asr-swift_amd", "csrc", "codec_launch.h")).read()
    body = text[text.index("#define CODEC_TILE_COMBOS(X)"):]
    body = body[:body.index("\n\n")]
    found = re.findall(r"X\((\w+), (true|false), (E_\w+)\)", body)
    return [(ROWS_NAMES[r], s == "true", EPI_NAMES[e]) for r, s, e in found]


def frac(got, v, bound):
    """the largest |got - v| / bound; where the bound is 0 only an exact match counts as inside"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "a non-finite output"
    d = np.abs(got - v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf)).max())


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
W5 = (1, 70, 2, 1, 55)                                 # reach (taps - 1) dil exceeds a window; tile 1 holds three windows; M = 129


def _c(name, kind, snake, epi, segs, Cin, taps, N, dil=1, rate=1, stride=1, bmod=None, ldc_extra=0, kept=None, lead=0, tconv=0, in_place=False,
       bias=True, resid=True, affine=True, indep=False):
    return dict(name=name, kind=kind, snake=snake, epi=epi, segs=tuple(segs), Cin=Cin, taps=taps, N=N, dil=dil, rate=rate, stride=stride,
                bmod=bmod if bmod else N, ldc_extra=ldc_extra, kept=kept, lead=lead, tconv=tconv, in_place=in_place, bias=bias, resid=resid,
                affine=affine, indep=indep, K=taps * Cin)


TAIL_SEGS = (200, 30, 20, 50)                          # rows 0..199 | 200..229 | 230..249 | 250..299: tiles of 64 end at 64, 128, 192, 256, 300
TILE_CASES = [
    # WindowRows, plain load, E_LIN: the M, K, N tails, dilations, rates, the repeating bias, ldc > N
    _c("w_m1", WINDOW, False, E_LIN, (1,), 5, 7, 2),                                                   # K = 35: a tap across a K step
    _c("w_m63", WINDOW, False, E_LIN, (1, 60, 2), 5, 3, 6, dil=3, bmod=3, ldc_extra=2),                # K = 15
    _c("w_m64", WINDOW, False, E_LIN, (1, 61, 2), 16, 1, 62, ldc_extra=3),
    _c("w_m65", WINDOW, False, E_LIN, (1, 62, 2), 24, 2, 64, bias=False),
    _c("w_m129", WINDOW, False, E_LIN, W5, 5, 7, 66, dil=9, bmod=6),
    _c("w_rate2", WINDOW, False, E_LIN, (1, 3, 2, 1, 26), 16, 3, 130, dil=3, rate=2),                  # M = 66
    _c("w_rate8", WINDOW, False, E_LIN, (1, 5, 2, 1), 5, 7, 6, dil=9, rate=8, bmod=3, ldc_extra=1),    # M = 72
    _c("w_tconv_s2", WINDOW, False, E_LIN, W5, 5, 2, 6, bmod=3, tconv=2),                              # N = s C_out = 2 x 3
    _c("w_tconv_s11", WINDOW, False, E_LIN, (1, 3, 2, 1, 26), 24, 2, 66, rate=2, bmod=6, tconv=11),    # N = 11 x 6
    # WindowRows, the other instantiations
    _c("w_gelu", WINDOW, False, E_GELU, (1, 62, 2), 16, 1, 66),
    _c("w_res", WINDOW, False, E_RES, W5, 24, 1, 62, bmod=31),
    _c("w_lsres", WINDOW, False, E_LSRES, (1, 62, 2), 24, 1, 130, in_place=True),
    _c("w_swiglu", WINDOW, False, E_SWIGLU, (1, 62, 2), 16, 1, 62, bias=False),
    _c("w_swiglu_n2", WINDOW, False, E_SWIGLU, (1,), 5, 1, 2, bias=False, ldc_extra=2),
    _c("w_swiglu_n130", WINDOW, False, E_SWIGLU, (1, 60, 2), 24, 1, 130, bias=False),
    _c("w_resmap", WINDOW, False, E_RESMAP, W5, 24, 1, 66),
    _c("w_resmap_no_r", WINDOW, False, E_RESMAP, (1, 62, 2), 16, 1, 6, resid=False),
    _c("w_resmap_no_affine", WINDOW, False, E_RESMAP, (1, 62, 2), 16, 1, 62, affine=False),
    _c("w_snake_lin", WINDOW, True, E_LIN, W5, 5, 7, 66, dil=3),
    _c("w_snake_lin_rate2", WINDOW, True, E_LIN, (1, 3, 2, 1, 26), 5, 7, 6, dil=9, rate=2, bmod=3),
    _c("w_snake_tconv", WINDOW, True, E_LIN, (1, 62, 2), 16, 2, 64, bmod=8, tconv=8),
    _c("w_snake_res", WINDOW, True, E_RES, (1, 62, 2), 24, 1, 62, in_place=True),
    # TailRows: `live` of window 0 on a tile edge and one row either side (kept 130, 129, 131 at lead 66), nothing dead (window 1), a lead
    # that clamps to the window start (window 2), a straddling tile and a last partial tile whose only live rows are their last
    _c("tail_edge", TAIL, False, E_LIN, TAIL_SEGS, 5, 7, 66, dil=3, kept=(130, 200, 231, 298), lead=66),
    _c("tail_edge_m1", TAIL, False, E_LIN, TAIL_SEGS, 5, 7, 66, dil=3, kept=(129, 200, 231, 298), lead=66),
    _c("tail_edge_p1", TAIL, False, E_LIN, TAIL_SEGS, 5, 7, 66, dil=3, kept=(131, 200, 231, 298), lead=66),
    _c("tail_lead1", TAIL, True, E_LIN, TAIL_SEGS, 5, 7, 6, dil=9, kept=(130, 200, 231, 298), lead=1, bmod=3),
    _c("tail_rate2", TAIL, True, E_LIN, (40, 10), 16, 3, 62, dil=3, rate=2, kept=(35, 40), lead=6),    # live = 64 of M = 100
    _c("tail_res", TAIL, True, E_RES, TAIL_SEGS, 24, 1, 62, kept=(130, 200, 231, 298), lead=2, in_place=True),
    # ClipRows: strides 1, 2, 8, clips of one output row; independent rows
    _c("c_s1", CLIP, False, E_LIN, W5, 5, 7, 66, dil=3),
    _c("c_s2", CLIP, False, E_LIN, W5, 5, 4, 6, stride=2, ldc_extra=2),
    _c("c_s8", CLIP, False, E_LIN, (1, 62, 2), 5, 16, 62, stride=8),
    _c("c_rows", CLIP, False, E_LIN, (65,), 24, 1, 130, indep=True),
    _c("c_gelu", CLIP, False, E_GELU, (65,), 16, 1, 66, indep=True),
    _c("c_lsres", CLIP, False, E_LSRES, (65,), 24, 1, 62, indep=True, in_place=True),
    _c("c_swiglu", CLIP, False, E_SWIGLU, (65,), 16, 1, 66, indep=True, bias=False),
    _c("c_snake_lin", CLIP, True, E_LIN, W5, 5, 7, 66, dil=9),
    _c("c_snake_s2", CLIP, True, E_LIN, (1, 62, 2), 5, 4, 6, stride=2),
    _c("c_snake_res", CLIP, True, E_RES, W5, 24, 1, 62, in_place=True),
    # VaeStrideRows: k = 2 s
    _c("v_s2", VSTRIDE, False, E_LIN, (1, 20, 2, 1, 12), 5, 4, 66, rate=2, stride=2),                  # M = 72
    _c("v_s5", VSTRIDE, False, E_LIN, (1, 62, 2), 5, 10, 6, stride=5, ldc_extra=1),                    # M = 65, K = 50
]
TILE_BY_NAME = {c["name"]: c for c in TILE_CASES}
ROW_C = (4, 255, 256, 257, 4096)
ROW_SEGS = (1, 8, 2)                                   # DWLN: a row at a window start (six taps absent), one and six rows after it


def layout(c):
    """-> dict(M, a_rows, segs [(o0, o1, i0, i1)], loc_a, loc_b, n_clips): the rows of every window / clip and the locator's arrays"""
    kind, rate, stride = c["kind"], c["rate"], c["stride"]
    segs, la, lb = [], None, None
    if kind in (WINDOW, TAIL, VSTRIDE):
        f0, fs, kp = 0, [], []
        in_rate = rate * (stride if kind == VSTRIDE else 1)
        for i, n in enumerate(c["segs"]):
            segs.append((f0 * rate, (f0 + n) * rate, f0 * in_rate, (f0 + n) * in_rate))
            fs += [f0] * n
            if kind == TAIL:
                kp += [c["kept"][i]] * n
            f0 += n
        la = np.array(fs, np.int32)
        lb = np.array(kp, np.int32) if kind == TAIL else None
    else:
        o0 = i0 = 0
        for n in c["segs"]:
            segs.append((o0, o0 + n, i0, i0 + n * stride))
            o0, i0 = o0 + n, i0 + n * stride
        if not c["indep"]:
            la = np.array([s[0] for s in segs] + [o0], np.int32)
            lb = np.array([s[2] for s in segs] + [i0], np.int32)
    return dict(M=segs[-1][1], in_rows=segs[-1][3], a_rows=segs[-1][3] + 2, segs=segs, loc_a=la, loc_b=lb,
                n_clips=len(segs) if kind == CLIP and not c["indep"] else 0)


def _last_local(c, t):
    if c["kind"] == CLIP:
        return t * c["stride"]
    if c["kind"] == VSTRIDE:
        return (t + 1) * c["stride"] - 1
    return t


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def pack_conv(W):
    """W [N][C_in][taps] -> Wt [taps C_in][N]: Wt[j C_in + c][n] = W[n][c][j]"""
    N, Cin, taps = W.shape
    return _f32(W.transpose(2, 1, 0).reshape(taps * Cin, N))


def pack_tconv(Wt3, s):
    """a transposed conv [C_in][C_out][2 s] as two taps: tap 0 (x[t - 1]) holds W[:, :, ph + s], tap 1 (x[t]) holds W[:, :, ph]; column
    n = ph C_out + co -> the same W [N][C_in][2] the conv reference takes"""
    Cin, Cout, k = Wt3.shape
    W = np.zeros((s * Cout, Cin, 2), Wt3.dtype)
    for ph in range(s):
        W[ph * Cout:(ph + 1) * Cout, :, 0] = Wt3[:, :, ph + s].T
        W[ph * Cout:(ph + 1) * Cout, :, 1] = Wt3[:, :, ph].T
    return W


@functools.lru_cache(maxsize=None)
def _tile_inputs(name):
    c = TILE_BY_NAME[name]
    L = layout(c)
    r = np.random.default_rng(_seed(name))
    Cin, taps, N, K = c["Cin"], c["taps"], c["N"], c["K"]
    A = r.standard_normal((L["a_rows"], Cin)).clip(-4.5, 4.5).astype(np.float32)
    A[L["in_rows"]:] = POISON[np.arange(2 * Cin).reshape(2, Cin) % 4]
    inp = dict(case=c, L=L, A=A)
    if c["tconv"]:
        s = c["tconv"]
        assert taps == 2 and N % s == 0 and c["bmod"] == N // s
        inp["Wt3"] = (r.standard_normal((Cin, N // s, 2 * s)) / math.sqrt(K)).astype(np.float32)
        inp["W"] = pack_tconv(inp["Wt3"], s)
    else:
        inp["W"] = (r.standard_normal((N, Cin, taps)) / math.sqrt(K)).astype(np.float32)
    inp["Wt"] = pack_conv(inp["W"])
    repeats = c["kind"] in (WINDOW, TAIL)
    inp["bias"] = ((0.2 if "clip" in c else 1.0) * r.standard_normal(c["bmod"] if repeats else N)).astype(np.float32) if c["bias"] else None
    n_s = N if c["epi"] == E_RESMAP else Cin
    if c["snake"] or c["epi"] == E_RESMAP:
        inp["sa"] = np.exp(r.uniform(-math.log(SNAKE_A), math.log(SNAKE_A), n_s)).astype(np.float32)
        inp["sb"] = (1.0 / np.exp(r.uniform(-0.7, 0.7, n_s))).astype(np.float32)
    else:
        inp["sa"] = inp["sb"] = None
    inp["ls"] = None
    if c["epi"] == E_LSRES:
        inp["ls"] = r.standard_normal(N).astype(np.float32)
    if c["epi"] == E_RESMAP and c["affine"]:
        inp["ls"] = np.concatenate([r.uniform(0.4, 0.9, N), 0.3 * r.standard_normal(N)]).astype(np.float32)
    ncols = N // 2 if c["epi"] == E_SWIGLU else N
    inp["ncols"], inp["ldc"] = ncols, ncols + c["ldc_extra"] if c["epi"] == E_SWIGLU else N + c["ldc_extra"]
    has_r = c["epi"] in (E_RES, E_LSRES) or (c["epi"] == E_RESMAP and c["resid"])
    inp["R"] = ((0.5 if c["epi"] == E_RESMAP else 1.0) * r.standard_normal((L["M"], N))).astype(np.float32) if has_r else None
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp


def tile_inputs(c):
    return _tile_inputs(c["name"])


# ---- the float64 pieces ------------------------------------------------------------------------------------------------------------------
def snake64(x, a, b):
    """-> (x + b sin^2(a x), the error of the five f32 operations and sinf)"""
    x, a, b = np.asarray(x, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.sin(a * x)
    v = x + b * s * s
    ds = U * np.abs(a * x) + T_ULP["sin"] * 2 * U * np.abs(s)
    return v, np.abs(b) * (2 * np.abs(s) * ds + 2 * U * s * s) + U * np.abs(v)


def _erf64(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def epilogue64(c, inp, acc, dacc):
    """acc, dacc [M][N] float64 (before the bias) -> (out [M][ncols], bound)"""
    N, epi = c["N"], c["epi"]
    v = acc
    if inp["bias"] is not None:
        v = v + inp["bias"].astype(np.float64)[np.arange(N) % len(inp["bias"])]
    R = None if inp["R"] is None else inp["R"].astype(np.float64)
    if epi == E_LIN:
        return v, dacc
    if epi == E_GELU:
        cc = 0.70710678118654752440
        e = _erf64(v * cc)
        out = 0.5 * v * (1.0 + e)
        dg = np.abs(0.5 * (1.0 + e) + v * np.exp(-0.5 * v * v) / math.sqrt(2 * math.pi))
        derf = (2 / math.sqrt(math.pi)) * np.exp(-(v * cc) ** 2) * 2 * U * np.abs(v * cc) + T_ULP["erf"] * 2 * U * np.abs(e)
        return out, dg * dacc + np.abs(0.5 * v) * (derf + U * np.abs(1.0 + e)) + U * np.abs(out)
    if epi == E_RES:
        return v + R, dacc + U * np.abs(v + R)
    if epi == E_LSRES:
        ls = inp["ls"].astype(np.float64)
        return v * ls + R, np.abs(ls) * dacc + U * np.abs(v * ls) + U * np.abs(v * ls + R)
    if epi == E_SWIGLU:
        g, up, dg, dup = v[:, 0::2], v[:, 1::2], dacc[:, 0::2], dacc[:, 1::2]
        e = np.exp(-g)
        sig = 1.0 / (1.0 + e)
        silu = g * sig
        dsilu = np.abs(sig * (1.0 + g * (1.0 - sig))) * dg + np.abs(silu) * ((T_ULP["exp"] * 2 * U * e + U * (1.0 + e)) / (1.0 + e) + DIV)
        out = silu * up
        return out, np.abs(up) * dsilu + np.abs(silu) * dup + U * np.abs(out)
    assert epi == E_RESMAP
    t, dt = v, dacc
    if R is not None:
        t = t + R
        dt = dt + U * np.abs(t)
    if inp["ls"] is not None:
        ls = inp["ls"].astype(np.float64)
        t0 = t
        t = t0 * ls[:N] + ls[N:]
        dt = np.abs(ls[:N]) * dt + U * np.abs(t0 * ls[:N]) + U * np.abs(t)
    a, b = inp["sa"].astype(np.float64), inp["sb"].astype(np.float64)
    out, own = snake64(t, a, b)
    return out, (1.0 + np.abs(a * b)) * dt * (1.0 + 2.0 ** -10) + own


def _d_acc(c, inp, S, dS):
    """the chain's bound with the bias add, [M][N]"""
    b = 0.0 if inp["bias"] is None else np.abs(inp["bias"].astype(np.float64))[np.arange(c["N"]) % len(inp["bias"])]
    return (c["K"] + 1) * U * (S + b) + dS * (1.0 + 2.0 ** -10)


def tile_ref(c, A=None):
    """the window-by-window reference -> (out [M][ncols], bound)"""
    inp = tile_inputs(c)
    L = inp["L"]
    A = inp["A"] if A is None else A
    taps, dil, Cin, N = c["taps"], c["dil"], c["Cin"], c["N"]
    W = inp["W"].astype(np.float64)
    acc, S, dS = (np.zeros((L["M"], N)) for _ in range(3))
    pad = (taps - 1) * dil
    for o0, o1, i0, i1 in L["segs"]:
        X = A[i0:i1].astype(np.float64)
        dX = np.zeros_like(X)
        if c["snake"]:
            X, dX = snake64(X, inp["sa"], inp["sb"])
        Xp, dXp = np.concatenate([np.zeros((pad, Cin)), X]), np.concatenate([np.zeros((pad, Cin)), dX])
        last = _last_local(c, np.arange(o1 - o0))
        assert last.max() < i1 - i0
        for j in range(taps):
            acc[o0:o1] += Xp[last + j * dil] @ W[:, :, j].T
            S[o0:o1] += np.abs(Xp[last + j * dil]) @ np.abs(W[:, :, j]).T
            dS[o0:o1] += dXp[last + j * dil] @ np.abs(W[:, :, j]).T
    return epilogue64(c, inp, acc, _d_acc(c, inp, S, dS))


def conv_ref(c):
    """the accumulator (no bias, no epilogue) of a plain-load case as torch's strided, dilated conv1d in float64, clip by clip, left-padded"""
    inp = tile_inputs(c)
    L, taps, dil = inp["L"], c["taps"], c["dil"]
    stride = c["stride"] if c["kind"] in (CLIP, VSTRIDE) else 1
    W = torch.from_numpy(inp["W"].astype(np.float64))
    out = np.zeros((L["M"], c["N"]))
    for o0, o1, i0, i1 in L["segs"]:
        x = torch.from_numpy(inp["A"][i0:i1].astype(np.float64)).T[None]
        # the last tap of output 0 sits on input row last(0): pad so that it does
        left = (taps - 1) * dil - _last_local(c, 0)
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(x, (left, 0)), W, stride=stride, dilation=dil)
        out[o0:o1] = y[0].T.numpy()[:o1 - o0]
    return out


def tconv_ref(c):
    """the accumulator of a transposed-conv case from the unpacked weight [C_in][C_out][2 s]: y_full[t s + i] += x[t] W[:, :, i], the first
    T s rows kept (the causal trim), as rows [T][s C_out]"""
    inp = tile_inputs(c)
    L, s = inp["L"], c["tconv"]
    W = inp["Wt3"].astype(np.float64)
    Cout = W.shape[1]
    out = np.zeros((L["M"], c["N"]))
    for o0, o1, i0, i1 in L["segs"]:
        x = inp["A"][i0:i1].astype(np.float64)
        T = i1 - i0
        full = np.zeros((T * s + s, Cout))
        for t in range(T):
            for i in range(2 * s):
                full[t * s + i] += x[t] @ W[:, :, i]
        out[o0:o1] = full[:T * s].reshape(T, s * Cout)
    return out


def spans(c, L, mut=None):
    """(first, last) of every output row, from the locator ARRAYS as the launch is told about them.  mut "clip": the clip search off by one
    at a clip's last row; "stride": stride + 1"""
    m = np.arange(L["M"])
    kind, rate = c["kind"], c["rate"]
    stride = c["stride"] + (1 if mut == "stride" else 0)
    if kind in (WINDOW, TAIL):
        return L["loc_a"][m // rate].astype(np.int64) * rate, m
    if kind == VSTRIDE:
        return L["loc_a"][m // rate].astype(np.int64) * rate * stride, (m + 1) * stride - 1
    if L["loc_a"] is None:
        return np.zeros_like(m), m
    clip = np.searchsorted(L["loc_a"], m + (1 if mut == "clip" else 0), side="right") - 1
    clip = np.minimum(clip, L["n_clips"] - 1)
    first = L["loc_b"][clip].astype(np.int64)
    return first, first + (m - L["loc_a"][clip]) * stride


def live_rows(c, L):
    """TailRows: the first live row of each row's window, clamped to the window's first row"""
    f = np.arange(L["M"]) // c["rate"]
    return np.maximum(L["loc_b"][f].astype(np.int64) * c["rate"] - c["lead"], L["loc_a"][f].astype(np.int64) * c["rate"])


def tile_eval(c, mut=None, A=None):
    """a second float64 evaluation, row by row over the locator arrays -> out [M][ncols].  mut names a defect of one guard:
    leak (a tap admitted before `first`), drop_first (the tap on `first` dropped), dil (dil + 1), ktail (the operand's k < K guard gone: the
    elements k = K .. up to the 16-wide step are read, against a weight of 1), swiglu (the pair shifted by one column), bias (bias[n] for
    bias[n % bmod]: past the array, 1e30), clip, stride (see spans)"""
    inp = tile_inputs(c)
    L = inp["L"]
    A = (inp["A"] if A is None else A).astype(np.float64)
    taps, Cin, N, K = c["taps"], c["Cin"], c["N"], c["K"]
    dil = c["dil"] + (1 if mut == "dil" else 0)
    first, last = spans(c, L, mut)
    W = inp["W"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        X = snake64(A, inp["sa"], inp["sb"])[0] if c["snake"] else A
    acc = np.zeros((L["M"], N))
    nan_row = L["a_rows"] - 1

    def rows_of(src):
        return np.where(src >= L["a_rows"], nan_row, np.maximum(src, 0))
    for j in range(taps):
        src = last - (taps - 1 - j) * dil
        ok = src >= 0 if mut == "leak" else src > first if mut == "drop_first" else src >= first
        acc += np.where(ok[:, None], X[rows_of(src)], 0.0) @ W[:, :, j].T
    if mut == "ktail":
        for k in range(K, (K + 15) // 16 * 16):
            j, ch = divmod(k, Cin)
            src = last - (taps - 1 - j) * dil
            acc += np.where((src >= first)[:, None], X[rows_of(src)][:, ch:ch + 1], 0.0)
    if mut == "bias" and inp["bias"] is not None:
        b = np.concatenate([inp["bias"].astype(np.float64), np.full(N, 1e30)])[:N]
        acc = acc + b
        inp = {**inp, "bias": None}
    if mut == "swiglu":
        acc = np.concatenate([acc[:, 1:], np.zeros((L["M"], 1))], 1)
    with np.errstate(all="ignore"):
        return epilogue64(c, inp, acc, np.zeros_like(acc))[0]


def tile_mutations(c):
    """the mutations of tile_eval this case can show; the exemptions are listed in the CPU module's docstring"""
    L = layout(c)
    first, last = spans(c, L)
    muts = ["drop_first"]
    if c["taps"] > 1:
        if any(((last - j * c["dil"]) >= first).any() for j in range(1, c["taps"])):
            muts.append("dil")
        if any((((last - j * c["dil"]) < first) & ((last - j * c["dil"]) >= 0)).any() for j in range(1, c["taps"])):
            muts.append("leak")
    if c["K"] % 16:
        muts.append("ktail")
    if c["epi"] == E_SWIGLU:
        muts.append("swiglu")
    if c["bias"] and c["kind"] in (WINDOW, TAIL) and c["bmod"] < c["N"]:
        muts.append("bias")
    if c["kind"] == CLIP and not c["indep"] and len(c["segs"]) > 1:
        muts.append("clip")
    if c["kind"] in (CLIP, VSTRIDE) and not c["indep"] and max(c["segs"]) > 1:
        muts.append("stride")
    return muts


# ---- the f32 twin of the tile ------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def snake32(x, a, b):
    """codec_snake in f32, operation by operation -> (value, the sinf arguments)"""
    arg = (_f32(a) * _f32(x)).astype(np.float32)
    s = torch.sin(_t(arg)).numpy()
    return (_f32(x) + _f32(b) * (s * s).astype(np.float32)).astype(np.float32), arg


def tile_twin(c, args=None):
    """the kernel's arithmetic in f32: the operand through the snake load, ONE fmaf chain over k = 0 .. K - 1 per output (a fused multiply-add
    is the float64 product and sum rounded once to f32: the product is exact in float64), the epilogue operation by operation.  args: a dict
    that collects the arguments of sinf / expf / erff -> out [M][ncols] f32"""
    inp = tile_inputs(c)
    L, taps, dil, Cin, N = inp["L"], c["taps"], c["dil"], c["Cin"], c["N"]
    first, last = spans(c, L)
    A = inp["A"]

    def note(k, a):
        if args is not None:
            args.setdefault(k, []).append(np.asarray(a, np.float32).ravel())
    X = A
    if c["snake"]:
        with np.errstate(invalid="ignore"):
            X, arg = snake32(A, inp["sa"], inp["sb"])
        note("sin", arg[:L["in_rows"]])
    acc = np.zeros((L["M"], N), np.float32)
    Wt = inp["Wt"].astype(np.float64)
    for j in range(taps):
        src = last - (taps - 1 - j) * dil
        op = np.where((src >= first)[:, None], X[np.maximum(src, 0)], np.float32(0)).astype(np.float64)
        for ch in range(Cin):
            acc = (acc.astype(np.float64) + op[:, ch:ch + 1] * Wt[j * Cin + ch][None, :]).astype(np.float32)
    v = acc
    epi = c["epi"]
    if inp["bias"] is not None:
        v = (v + inp["bias"][np.arange(N) % len(inp["bias"])]).astype(np.float32)
    R = inp["R"]
    one, half = np.float32(1), np.float32(0.5)
    if epi == E_GELU:
        arg = (v * np.float32(0.70710678118654752440)).astype(np.float32)
        note("erf", arg)
        v = ((half * v) * (one + torch.erf(_t(arg)).numpy())).astype(np.float32)
    elif epi == E_RES:
        v = v + R
    elif epi == E_LSRES:
        v = (v * inp["ls"]).astype(np.float32) + R
    elif epi == E_SWIGLU:
        g, up = v[:, 0::2], v[:, 1::2]
        note("exp", -g)
        v = ((g / (one + torch.exp(_t(-g)).numpy())).astype(np.float32) * up).astype(np.float32)
    elif epi == E_RESMAP:
        if R is not None:
            v = v + R
        if inp["ls"] is not None:
            v = (v * inp["ls"][:N]).astype(np.float32) + inp["ls"][N:]
        v, arg = snake32(v, inp["sa"], inp["sb"])
        note("sin", arg)
    return np.asarray(v, np.float32)


# ---- RMS ----------------------------------------------------------------------------------------------------------------------------------
def _tree_terms(C):
    """roundings of one row reduction relative to the sum of |terms|: P partial steps, 8 tree levels"""
    return -(-C // 256) + 8


@functools.lru_cache(maxsize=None)
def rms_inputs(C):
    r = np.random.default_rng(1000 + C)
    x = r.standard_normal((3, C)).astype(np.float32)
    x[1] *= np.float32(1e-3)
    x[2] *= np.float32(30.0)
    return dict(C=C, x=x, w=r.standard_normal(C).astype(np.float32))


def rms_ref(C):
    """y = x / sqrt(mean(x^2) + eps) w -> (y, bound).  sum x^2: each term a product (u), the reduction (P + 8) u of the sum; / C and the
    sqrt and the reciprocal DIV each, + eps u: the factor `inv` is within (0.5 (P + 8 + 1 + 5 + 1) + 2 x 5) u relatively; x inv, then w: 2 u"""
    inp = rms_inputs(C)
    x, w = inp["x"].astype(np.float64), inp["w"].astype(np.float64)
    y = x / np.sqrt((x * x).mean(1, keepdims=True) + RMS_EPS) * w
    rel = (0.5 * (_tree_terms(C) + 7) + 12) * U
    return y, rel * np.abs(y) * (1.0 + 2.0 ** -10)


def _block_sum32(p):
    """codec_block_sum on [rows][256] f32 partials: the fixed tree"""
    p = p.astype(np.float32).copy()
    s = 128
    while s > 0:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0]


def _partials32(terms):
    """a thread's sequential partial over c = tid, tid + 256, ..: terms [rows][C] f32 -> [rows][256]"""
    rows, C = terms.shape
    padded = np.zeros((rows, -(-C // 256) * 256), np.float32)
    padded[:, :C] = terms
    p = np.zeros((rows, 256), np.float32)
    for i in range(padded.shape[1] // 256):
        p = p + padded[:, i * 256:(i + 1) * 256]
    return p


def rms_twin(C):
    inp = rms_inputs(C)
    x, w = inp["x"], inp["w"]
    tot = _block_sum32(_partials32((x * x).astype(np.float32)))
    inv = np.float32(1) / np.sqrt(tot / np.float32(C) + np.float32(RMS_EPS), dtype=np.float32)
    return ((x * inv[:, None]).astype(np.float32) * w).astype(np.float32)


# ---- DWLN ---------------------------------------------------------------------------------------------------------------------------------
def dwln_case(C, kind, rate=1):
    return dict(name=f"dwln_{C}_{kind}_{rate}", kind=kind, rate=rate, stride=1, segs=ROW_SEGS, indep=False, kept=None, lead=0, C=C)


DWLN_CASES = [dwln_case(C, WINDOW) for C in ROW_C] + [dwln_case(C, CLIP) for C in ROW_C] + [dwln_case(12, WINDOW, rate=2)]


@functools.lru_cache(maxsize=None)
def _dwln_inputs(C, name):
    r = np.random.default_rng(2000 + _seed(name) % 1000 + C)
    return dict(w=(r.standard_normal((7, C)) * 0.4).astype(np.float32), b=r.standard_normal(C).astype(np.float32),
                lnw=r.standard_normal(C).astype(np.float32), lnb=r.standard_normal(C).astype(np.float32), r=r)


def dwln_inputs(c):
    L = layout(c)
    p = _dwln_inputs(c["C"], c["name"])
    x = np.random.default_rng(3000 + c["C"]).standard_normal((L["a_rows"], c["C"])).astype(np.float32)
    x[L["in_rows"]:] = POISON[np.arange(2 * c["C"]).reshape(2, c["C"]) % 4]
    return dict(case=c, L=L, x=x, **{k: p[k] for k in ("w", "b", "lnw", "lnb")})


def dwln_ref(c, x=None, mut=None):
    """depthwise causal conv k = 7 + bias, LayerNorm eps 1e-5, window by window -> (y, bound).  mut: leak / drop_first (the conv's window
    start), stats (the LayerNorm statistics of the next row).
    val: seven product-and-add steps and the bias, 9 u (sum |x w| + |b|).  mu: (sum d_val) / C + (P + 8 + 5) u mean |val|.  d = val - mu:
    d_val + d_mu + u |d|.  var = mean d^2: 2 mean(|d| d_d) + (P + 8 + 1 + 5) u var.  inv = 1 / sqrt(var + eps): relatively
    0.5 (d_var + u (var + eps)) / (var + eps) + 2 DIV.  y = (d inv) lnw + lnb: |lnw| inv (d_d + |d| (rel_inv + u)) + u |d inv lnw| + u |y|"""
    inp = dwln_inputs(c)
    L, C = inp["L"], c["C"]
    x = (inp["x"] if x is None else x).astype(np.float64)
    w, b, lnw, lnb = (inp[k].astype(np.float64) for k in ("w", "b", "lnw", "lnb"))
    val, sab = np.zeros((L["M"], C)), np.zeros((L["M"], C))
    for o0, o1, i0, i1 in L["segs"]:
        if mut == "leak":
            Xp = np.concatenate([np.zeros((6, C)), x[:i1]])[i0:]
            with np.errstate(invalid="ignore"):
                Xp = np.nan_to_num(Xp, nan=1e30)
        else:
            Xp = np.concatenate([np.zeros((6, C)), x[i0:i1]])
            if mut == "drop_first":
                Xp[6] = 0.0
        for j in range(7):
            val[o0:o1] += Xp[j:j + o1 - o0] * w[j]
            sab[o0:o1] += np.abs(Xp[j:j + o1 - o0] * w[j])
    val, sab = val + b, sab + np.abs(b)
    P = _tree_terms(C)
    dval = 9 * U * sab
    mu = val.mean(1, keepdims=True)
    dmu = dval.mean(1, keepdims=True) + (P + 5) * U * np.abs(val).mean(1, keepdims=True)
    d = val - mu
    dd = dval + dmu + U * np.abs(d)
    var = (d * d).mean(1, keepdims=True)
    dvar = 2 * (np.abs(d) * dd).mean(1, keepdims=True) + (P + 6) * U * var
    if mut == "stats":
        mu, var = np.roll(mu, -1, 0), np.roll(var, -1, 0)
        d = val - mu
    inv = 1.0 / np.sqrt(var + 1e-5)
    rel = 0.5 * (dvar + U * (var + 1e-5)) / (var + 1e-5) + 2 * DIV
    y = d * inv * lnw + lnb
    bound = np.abs(lnw) * inv * (dd + np.abs(d) * (rel + U)) + U * np.abs(d * inv * lnw) + U * np.abs(y)
    return y, bound * (1.0 + 2.0 ** -10)


def dwln_twin(c):
    inp = dwln_inputs(c)
    L, C = inp["L"], c["C"]
    x, w, b, lnw, lnb = (inp[k] for k in ("x", "w", "b", "lnw", "lnb"))
    first, _ = spans(c, L)
    m = np.arange(L["M"])
    acc = np.zeros((L["M"], C), np.float32)
    for j in range(7):
        src = m - (6 - j)
        term = (x[np.maximum(src, 0)] * w[j]).astype(np.float32)
        acc = np.where((src >= first)[:, None], acc + term, acc).astype(np.float32)
    val = (acc + b).astype(np.float32)
    mu = _block_sum32(_partials32(val)) / np.float32(C)
    d = (val - mu[:, None]).astype(np.float32)
    var = _block_sum32(_partials32((d * d).astype(np.float32))) / np.float32(C)
    inv = np.float32(1) / np.sqrt(var + np.float32(1e-5), dtype=np.float32)
    return (((d * inv[:, None]).astype(np.float32) * lnw).astype(np.float32) + lnb).astype(np.float32)


# ---- OUT and CENC_IN: the tile's arithmetic behind other launches --------------------------------------------------------------------------
# codec_out_kernel is the snake load, seven taps of C channels into ONE output column, + b[0], clip: a WindowRows tile case with N = 1 (w [7][C]
# is Wt [7 C][1]); TAIL computes only the rows from kept[frame] * rate on.  cenc_in_kernel is a ClipRows tile case with C_in = 1 and N = C
# (w [7][C] is Wt [7][C]).  Both are one fmaf chain, taps outer and channels inner, then the bias: tile_ref, tile_eval and tile_twin serve
# them unchanged, and the clip (monotone, 1-Lipschitz, exact) leaves the bound as it is.
OUT_TAIL_SEGS = (1, 70, 2, 1, 200)                     # rows 74 .. 273 are the last window: kept 255 / 256 / 257 straddles the 256-thread block edge
OUT_CASES = [
    dict(_c("out_c1", WINDOW, True, E_LIN, W5, 1, 7, 1, rate=2), clip=1),                              # M = 258
    dict(_c("out_c3", WINDOW, True, E_LIN, W5, 3, 7, 1, rate=2), clip=0),
    dict(_c("out_c24", WINDOW, True, E_LIN, W5, 24, 7, 1, rate=2), clip=1),
    dict(_c("out_tail_c1", TAIL, True, E_LIN, OUT_TAIL_SEGS, 1, 7, 1, kept=(0, 40, 72, 73, 255)), clip=1),
    dict(_c("out_tail_c3", TAIL, True, E_LIN, OUT_TAIL_SEGS, 3, 7, 1, kept=(0, 1, 71, 73, 256)), clip=1),
    dict(_c("out_tail_c24", TAIL, True, E_LIN, OUT_TAIL_SEGS, 24, 7, 1, kept=(0, 70, 72, 73, 257)), clip=0),
    dict(_c("out_tail_rate2", TAIL, True, E_LIN, (1, 70, 2, 1, 55), 3, 7, 1, rate=2, kept=(0, 30, 71, 73, 128)), clip=1),     # row 256 of 258
]
CENC_IN_CASES = [_c("cenc_in_c%d" % C, CLIP, False, E_LIN, W5, 1, 7, C) for C in (1, 3, 24)]
for _case in OUT_CASES + CENC_IN_CASES:
    TILE_BY_NAME[_case["name"]] = _case


def out_ref(c):
    """-> (wave [M], bound, computed [M] bool): the rows a TAIL launch computes are those from kept[frame] * rate on"""
    want, bound = tile_ref(c)
    L = layout(c)
    m = np.arange(L["M"])
    done = m >= L["loc_b"][m // c["rate"]].astype(np.int64) * c["rate"] if c["kind"] == TAIL else np.ones(L["M"], bool)
    want = want[:, 0]
    return (np.clip(want, -1.0, 1.0) if c["clip"] else want), bound[:, 0], done


def out_twin(c):
    v = tile_twin(c)[:, 0]
    return np.clip(v, np.float32(-1), np.float32(1)) if c["clip"] else v


# ---- GATHER -----------------------------------------------------------------------------------------------------------------------------
GATHER_S0, GATHER_S1 = 5, 3
GATHER_CASES = [dict(name=f"gather_q{Q}_d{D}", Q=Q, D=D) for Q in (1, 2, 16) for D in (24, 255, 257)]


@functools.lru_cache(maxsize=None)
def _gather_inputs(Q, D):
    r = np.random.default_rng(5000 + 31 * Q + D)
    cb = r.standard_normal((GATHER_S0 + (Q - 1) * GATHER_S1, D)).astype(np.float32)
    codes = np.zeros((4, Q), np.int32)                                        # row 0: every code 0; row 1: every code S - 1; rows 2, 3: random
    codes[1] = [GATHER_S0 - 1] + [GATHER_S1 - 1] * (Q - 1)
    codes[2:, 0] = r.integers(0, GATHER_S0, 2)
    codes[2:, 1:] = r.integers(0, GATHER_S1, (2, Q - 1))
    return dict(cb=cb, codes=codes)


def gather_inputs(c):
    return _gather_inputs(c["Q"], c["D"])


def gather_ref(c, mut=None):
    """out [M][2 D] = codebook 0's row | the rows of codebooks 1 .. Q - 1 summed in codebook order -> (out, bound).  The first half is a
    copy (bound 0: exact); the second is Q - 2 f32 additions, (Q - 2) u sum |e| (0 for Q <= 2: exact; zeros for Q = 1).  mut: "base" (the
    later codebooks start at S1 rather than S0), "code" (codebook q reads code q - 1)"""
    inp = gather_inputs(c)
    Q, D = c["Q"], c["D"]
    cb, codes = inp["cb"].astype(np.float64), inp["codes"]
    M = codes.shape[0]
    out, bound = np.zeros((M, 2 * D)), np.zeros((M, 2 * D))
    out[:, :D] = cb[codes[:, 0]]
    base = GATHER_S1 if mut == "base" else GATHER_S0
    for q in range(1, Q):
        e = cb[base + (q - 1) * GATHER_S1 + codes[:, q - 1 if mut == "code" else q] % GATHER_S1]
        out[:, D:] += e
        bound[:, D:] += np.abs(e)
    return out, bound * max(Q - 2, 0) * U


def gather_twin(c):
    inp = gather_inputs(c)
    Q, D = c["Q"], c["D"]
    cb, codes = inp["cb"], inp["codes"]
    out = np.zeros((codes.shape[0], 2 * D), np.float32)
    out[:, :D] = cb[codes[:, 0]]
    for q in range(1, Q):
        out[:, D:] = out[:, D:] + cb[GATHER_S0 + (q - 1) * GATHER_S1 + codes[:, q]]
    return out


# ---- VQ -------------------------------------------------------------------------------------------------------------------------------------
# cenc_vq_kernel: per chain (chain 0: one stage on columns 0 .. D - 1 with a codebook of S0; chain 1: Q - 1 stages on columns D .. 2 D - 1
# with codebooks of S1), per stage code = argmin_n (|r|^2 - 2 r.c_n) + |c_n|^2, the lowest n among equal values, then r -= c[code].
# What is checked, stage by stage: the residual before a stage is rebuilt EXACTLY from the input and the device's earlier codes (the update
# is one f32 subtraction per element, which numpy's f32 subtraction is too); the device's code satisfies d(code) <= min_n d(n) + bound with
# d(n) = |r - c_n|^2 in float64, which excludes no case; the residual after the last stage is bit-exact.  Bound of a score
# v = (xsq - 2 acc) + csq[n]: xsq is four strided fmaf partials and two adds, (D / 4 + 2) u |r|^2; acc one fmaf chain, D u sum |r c|; the
# subtraction u |xsq - 2 acc|; the last add u |v|; and |csq[n] - |c_n|^2|, the distance of the loader's f32 norm from the exact one, which
# is computed, not estimated.  The device's choice beats the true one under its own scores, so the bound of a code is the sum of the two
# scores' bounds.  Exact ties: duplicated codebook rows give bit-identical scores (the same chain over the same values, the same norm), and
# the lowest index must win: VQ_TIES per stage, in two thread columns of one 64-wide tile, in two tiles, at 0 and S - 1.
VQ_CASES = [dict(name=f"vq_m{M}_d{D}_s{S0}_{S1}_q{Q}", M=M, D=D, S0=S0, S1=S1, Q=Q) for M, D, S0, S1, Q in
            ((1, 8, 3, 3, 1), (64, 24, 64, 65, 2), (65, 40, 130, 64, 5), (65, 8, 65, 130, 2), (1, 40, 130, 3, 5), (64, 24, 3, 130, 2))]


def vq_ties(S):
    """pairs (low, high) of duplicated codebook rows"""
    t = [(0, S - 1)]
    if S > 9:
        t.append((1, 9))                               # thread columns 0 and 2 of tile 0
    if S > 69:
        t.append((5, 69))                              # tiles 0 and 1
    return t


def vq_pack(cb):
    """cb [stages][S][D] f32 -> (the transposes [stages][D][S], |c|^2 [stages][S] as the loader forms them: s = s + v * v in f32, in order)"""
    sq = np.zeros(cb.shape[:2], np.float32)
    for d in range(cb.shape[2]):
        sq = sq + (cb[:, :, d] * cb[:, :, d]).astype(np.float32)
    return np.ascontiguousarray(cb.transpose(0, 2, 1)), sq


@functools.lru_cache(maxsize=None)
def _vq_inputs(name):
    c = next(c for c in VQ_CASES if c["name"] == name)
    M, D, Q = c["M"], c["D"], c["Q"]
    r = np.random.default_rng(_seed(name))
    books = []
    for S, stages in ((c["S0"], 1), (c["S1"], Q - 1)):
        cb = r.standard_normal((stages, S, D)).astype(np.float32)
        for lo, hi in vq_ties(S):
            cb[:, hi] = cb[:, lo]
        books.append(cb)
    x = r.standard_normal((M, 2 * D)).astype(np.float32)
    # rows aimed at a tie: the frame sits beside a duplicated row of EVERY stage's codebook summed, so that each stage's residual is near its pair
    for m in range(M):
        for ch, (cb, S) in enumerate(((books[0], c["S0"]), (books[1], c["S1"]))):
            ties = vq_ties(S)
            if m % 4 != 3 and cb.shape[0]:
                lo = ties[m % len(ties)][0]
                x[m, ch * D:(ch + 1) * D] = cb[:, lo].astype(np.float64).sum(0).astype(np.float32) + np.float32(0.05) * x[m, ch * D:(ch + 1) * D]
    return dict(case=c, x=x, cb0=books[0], cb1=books[1], p0=vq_pack(books[0]), p1=vq_pack(books[1]))


def vq_inputs(c):
    return _vq_inputs(c["name"])


def vq_stages(c):
    """(column of codes, column offset of r, codebook [S][D], its f32 norms) per stage in the order of the codes' columns"""
    inp = vq_inputs(c)
    out = [(0, 0, inp["cb0"][0], inp["p0"][1][0])]
    for st in range(c["Q"] - 1):
        out.append((1 + st, c["D"], inp["cb1"][st], inp["p1"][1][st]))
    return out


def vq_check(c, codes, r_after):
    """the three checks on a launch's codes [M][Q] and final residual [M][2 D] -> the worst (d(code) - min d) / bound"""
    inp = vq_inputs(c)
    D = c["D"]
    r = inp["x"].copy()
    worst = 0.0
    for q, col, cb, csq in vq_stages(c):
        S = cb.shape[0]
        code = codes[:, q]
        assert ((code >= 0) & (code < S)).all(), "a code outside its codebook"
        rr, cc = r[:, col:col + D].astype(np.float64), cb.astype(np.float64)
        d = ((rr[:, None, :] - cc[None]) ** 2).sum(2)
        xsq, dot = (rr * rr).sum(1), np.abs(rr)[:, None, :] * np.abs(cc)[None]
        acc = rr @ cc.T
        v = xsq[:, None] - 2 * acc + (cc * cc).sum(1)[None]
        err = ((D / 4 + 2) * U * xsq[:, None] + 2 * D * U * dot.sum(2) + U * np.abs(xsq[:, None] - 2 * acc) + U * np.abs(v)
               + np.abs(csq.astype(np.float64) - (cc * cc).sum(1))[None])
        best = d.argmin(1)
        rows = np.arange(len(code))
        bound = err[rows, code] + err[rows, best]
        gap = d[rows, code] - d[rows, best]
        assert (gap <= bound).all(), ("a code farther than the nearest by more than the bound", c["name"], q)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.where(bound > 0, gap / bound, 0.0).max()))
        for lo, hi in vq_ties(S):
            assert not (code == hi).any() or lo == hi, ("the higher index of a tie", c["name"], q, lo, hi)
        r[:, col:col + D] = r[:, col:col + D] - cb[code]
    assert np.array_equal(r, r_after), "the residual is not the input minus the chosen rows, one f32 subtraction each"
    return worst


def vq_aimed(c):
    """per stage: how many rows have a duplicated pair as their nearest rows in float64 (walking the TRUE codes)"""
    inp = vq_inputs(c)
    D = c["D"]
    r = inp["x"].copy()
    counts = []
    for q, col, cb, _ in vq_stages(c):
        rr, cc = r[:, col:col + D].astype(np.float64), cb.astype(np.float64)
        best = ((rr[:, None, :] - cc[None]) ** 2).sum(2).argmin(1)
        los = [lo for lo, hi in vq_ties(cb.shape[0]) if lo != hi]
        counts.append(int(np.isin(best, los).sum()))
        r[:, col:col + D] = r[:, col:col + D] - cb[best]
    return counts


def vq_twin(c, tie_high=False):
    """the kernel's arithmetic in f32 -> (codes [M][Q], the final residual).  tie_high: the mutation `<=` for `<` in both tie rules"""
    inp = vq_inputs(c)
    D, M = c["D"], c["M"]
    r = inp["x"].copy()
    codes = np.zeros((M, c["Q"]), np.int32)
    for q, col, cb, csq in vq_stages(c):
        rr = r[:, col:col + D]
        part = np.zeros((M, 4), np.float32)
        for d in range(D):
            part[:, d % 4] = (part[:, d % 4].astype(np.float64) + rr[:, d].astype(np.float64) ** 2).astype(np.float32)
        xsq = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
        acc = np.zeros((M, cb.shape[0]), np.float32)
        for d in range(D):
            acc = (acc.astype(np.float64) + rr[:, d:d + 1].astype(np.float64) * cb[None, :, d].astype(np.float64)).astype(np.float32)
        v = ((xsq[:, None] - np.float32(2) * acc).astype(np.float32) + csq[None]).astype(np.float32)
        code = (v.shape[1] - 1 - v[:, ::-1].argmin(1)) if tie_high else v.argmin(1)
        codes[:, q] = code
        r[:, col:col + D] = rr - cb[code]
    return codes, r


# ---- ATTN_DEC and ATTN_ENC ---------------------------------------------------------------------------------------------------------------------
# codec_attn_kernel (causal, windows of at most CODEC_MAX_T frames) and cenc_attn_kernel (every frame of a clip attends to every frame, keys
# in tiles of 32 under a running maximum), head_dim 64, f32 throughout.  RoPE at the load pairs d with d + 32: q' = (q1 c - q2 s, q1 s + q2 c),
# two products and a sum each, |dq'| <= 2 u (|q1 c| + |q2 s|) (k' alike).  A score is one fmaf chain over 64 terms and the exact scale 2^-3:
#     ds = 2^-3 (sum_d (dq' |k'| + |q'| dk' + dq' dk') + 64 u sum_d |q' k'|)
# A score error changes every normalised weight by at most a factor exp(+-2 ds).  e = expf(s - m): the argument's rounding u R (R = the
# row's score range) and T_exp 2^-23; the sum of n terms n u, the division DIV, the fmaf chain over n keys n u.  With A = sum_k w_k |V_k|:
#     |got - v| <= A rel (1 + 2^-10) + u |v|,   rel = expm1(2 ds) + 2 (R u + T_exp 2^-23) + 2 n u + DIV [+ 2 tiles (R u + T_exp 2^-23 + u)]
# the bracket is the encoder's rescale alpha = expf(m_old - m_new) of the sum and the accumulators, once per 32-key tile.
CODEC_MAX_T = 35
ATTN_DEC_WINDOWS = (1, 2, CODEC_MAX_T, 1)
ATTN_ENC_CLIPS = (1, 31, 32, 33, 65)                   # the 32-key tile edges; 65 frames: three tiles, two rescales
ATTN_HEADS = (1, 3)


def rope_table(n):
    """[n][32][2] f32 (cos, sin), base 10000 over 64 dimensions"""
    ang = np.arange(n, dtype=np.float64)[:, None] * 10000.0 ** (-np.arange(32) / 32.0)[None]
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], 2), np.float32)


@functools.lru_cache(maxsize=None)
def _attn_inputs(enc, heads):
    segs = ATTN_ENC_CLIPS if enc else ATTN_DEC_WINDOWS
    M = sum(segs)
    r = np.random.default_rng(7000 + 10 * heads + enc)
    qkv = r.standard_normal((M, 3, heads, 64)).astype(np.float32)
    starts = np.cumsum((0,) + segs)
    if enc:                                            # later key tiles score higher, so the running maximum moves at every tile
        for s0, n in zip(starts, segs):
            for t in range(n):
                qkv[s0 + t, 1] *= np.float32(1.0 + 0.4 * (t // 32))
    table = rope_table(max(segs) + 2)
    if enc:
        loc = np.array([(s0, n, q0, 0) for s0, n in zip(starts, segs) for q0 in range(0, n, 32)], np.int32)
    else:
        loc = np.array([(n, s0) for s0, n in zip(starts, segs)], np.int32)
    return dict(enc=enc, heads=heads, segs=segs, starts=starts[:-1], M=M, qkv=qkv.reshape(M, 3 * heads * 64), rope=table, loc=loc)


def attn_inputs(enc, heads):
    return _attn_inputs(bool(enc), heads)


def _rope64(x, table):
    """x [T][heads][64] float64, table [T][32][2] -> (x', |dx'|)"""
    c, s = table[:, None, :, 0].astype(np.float64), table[:, None, :, 1].astype(np.float64)
    x1, x2 = x[..., :32], x[..., 32:]
    out = np.concatenate([x1 * c - x2 * s, x1 * s + x2 * c], -1)
    err = 2 * U * np.concatenate([np.abs(x1 * c) + np.abs(x2 * s), np.abs(x1 * s) + np.abs(x2 * c)], -1)
    return out, err


def attn_ref(inp, qkv=None, mut=None):
    """-> (out [M][heads 64], bound).  mut: "mask_more" (key i + 1 admitted), "mask_less" (the own key dropped) for the causal kernel;
    "next_key" (the row after the clip admitted), "no_rescale" (the accumulators keep the old maximum's scale at a tile edge) for the encoder's"""
    enc, heads, M = inp["enc"], inp["heads"], inp["M"]
    x = (inp["qkv"] if qkv is None else qkv).astype(np.float64).reshape(M, 3, heads, 64)
    out, bound = np.zeros((M, heads, 64)), np.zeros((M, heads, 64))
    for s0, n in zip(inp["starts"], inp["segs"]):
        nk = n + 1 if mut in ("next_key", "mask_more") and s0 + n < M else n
        tab = inp["rope"][:nk]
        q, dq = _rope64(x[s0:s0 + n, 0], tab[:n])
        k, dk = _rope64(x[s0:s0 + nk, 1], tab)
        v = x[s0:s0 + nk, 2]
        for h in range(heads):
            s = 0.125 * q[:, h] @ k[:, h].T
            ds = 0.125 * (dq[:, h] @ np.abs(k[:, h]).T + np.abs(q[:, h]) @ dk[:, h].T + dq[:, h] @ dk[:, h].T + 64 * U * np.abs(q[:, h]) @ np.abs(k[:, h]).T)
            i, j = np.arange(n)[:, None], np.arange(nk)[None]
            if enc:
                ok = np.ones((n, nk), bool) if mut == "next_key" else j < n
            else:
                ok = j <= i + 1 if mut == "mask_more" else j < i if mut == "mask_less" else j <= i
            ok = ok & (j < nk)
            sm = np.where(ok, s, -np.inf)
            with np.errstate(invalid="ignore"):
                mx = sm.max(1, keepdims=True)
                e = np.where(ok, np.exp(sm - mx), 0.0)
                if mut == "no_rescale":                # tile by tile: what was accumulated under an older maximum is not brought to the new one
                    e = np.zeros_like(s)
                    run = np.full((n, 1), -np.inf)
                    for k0 in range(0, nk, 32):
                        run = np.maximum(run, s[:, k0:k0 + 32].max(1, keepdims=True))
                        e[:, k0:k0 + 32] = np.exp(s[:, k0:k0 + 32] - run)
                w = e / e.sum(1, keepdims=True)
            with np.errstate(invalid="ignore"):
                R = np.where(ok, mx - sm, 0.0).max(1, keepdims=True)
            cnt = ok.sum(1, keepdims=True)
            tex = T_ULP["exp"] * 2 * U
            rel = np.expm1(2 * np.where(ok, ds, 0.0).max(1, keepdims=True)) + 2 * (R * U + tex) + 2 * cnt * U + DIV
            if enc:
                rel = rel + 2 * (-(-n // 32)) * (R * U + tex + U)
            val = w @ v[:, h]
            out[s0:s0 + n, h] = val
            bound[s0:s0 + n, h] = (np.abs(w) @ np.abs(v[:, h])) * rel * (1.0 + 2.0 ** -10) + U * np.abs(val)
    return out.reshape(M, heads * 64), bound.reshape(M, heads * 64)


def _fma_dot32(a, b):
    """[n][64] x [m][64] f32 -> [n][m]: one fmaf chain over d per pair"""
    acc = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for d in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, d:d + 1].astype(np.float64) * b[None, :, d].astype(np.float64)).astype(np.float32)
    return acc


def _rope32(x, table):
    c, s = table[:, None, :, 0], table[:, None, :, 1]
    x1, x2 = x[..., :32], x[..., 32:]
    return np.concatenate([(x1 * c).astype(np.float32) - (x2 * s).astype(np.float32), (x1 * s).astype(np.float32) + (x2 * c).astype(np.float32)], -1)


def _exp32(a, args=None):
    if args is not None:
        args.setdefault("exp", []).append(np.asarray(a, np.float32).ravel())
    return torch.exp(torch.from_numpy(np.ascontiguousarray(a, np.float32))).numpy()


def attn_twin(inp, args=None):
    """the kernels' arithmetic in f32: RoPE, the fmaf-chain scores, the causal softmax with its sequential sum and division, or the encoder's
    running maximum over 32-key tiles; the fmaf chain over the keys"""
    enc, heads, M = inp["enc"], inp["heads"], inp["M"]
    x = inp["qkv"].reshape(M, 3, heads, 64)
    out = np.zeros((M, heads, 64), np.float32)
    for s0, n in zip(inp["starts"], inp["segs"]):
        tab = inp["rope"][:n]
        q, k, v = _rope32(x[s0:s0 + n, 0], tab), _rope32(x[s0:s0 + n, 1], tab), x[s0:s0 + n, 2]
        for h in range(heads):
            s = (_fma_dot32(q[:, h], k[:, h]) * np.float32(0.125)).astype(np.float32)
            acc = np.zeros((n, 64), np.float32)
            if not enc:
                for i in range(n):
                    e = _exp32(s[i, :i + 1] - s[i, :i + 1].max(), args)
                    tot = np.float32(0)
                    for j in range(i + 1):
                        tot = np.float32(tot + e[j])
                    p = (e / tot).astype(np.float32)
                    a = np.zeros(64, np.float32)
                    for j in range(i + 1):
                        a = (a.astype(np.float64) + np.float64(p[j]) * v[j, h].astype(np.float64)).astype(np.float32)
                    acc[i] = a
                out[s0:s0 + n, h] = acc
                continue
            mx, tot = np.full(n, -np.inf, np.float32), np.zeros(n, np.float32)
            for k0 in range(0, n, 32):
                blk = s[:, k0:k0 + 32]
                nmx = np.maximum(mx, blk.max(1))
                with np.errstate(invalid="ignore"):
                    scale = _exp32(mx - nmx, args)
                tot = (tot * scale).astype(np.float32)
                acc = (acc * scale[:, None]).astype(np.float32)
                for j in range(blk.shape[1]):
                    p = _exp32(blk[:, j] - nmx, args)
                    tot = (tot + p).astype(np.float32)
                    acc = (acc.astype(np.float64) + p[:, None].astype(np.float64) * v[k0 + j, h][None].astype(np.float64)).astype(np.float32)
                mx = nmx
            out[s0:s0 + n, h] = (acc / tot[:, None]).astype(np.float32)
    return out.reshape(M, heads * 64)


# ---- VAE_DW ------------------------------------------------------------------------------------------------------------------------------
# vae_dw_kernel: y = [snake2](b + sum_j w[j][c] [snake1](x[m - (6 - j) dil][c])), j = 0 .. 6 as one fmaf chain (absent taps skipped), the
# bias, then snake2; both snakes (a residual unit) or neither (the decoder's conv_in).  Rows are staged in slabs of 64 with a 6 dil halo.
# Bound: d_val = 8 u (sum |xs w| + |b|) + sum |w| da (da: the snake load's own error, snake64), carried through snake2's derivative
# 1 + |a2 b2| with snake2's own error added.
VAE_DW_SEGS = {1: (1,), 64: (1, 61, 2), 65: (1, 62, 2), 130: (1, 70, 2, 1, 56)}
VAE_DW_CASES = [dict(name=f"vdw_c{C}_d{dil}_m{M}_{'s' if sn else 'p'}", kind=WINDOW, rate=rate, stride=1, segs=VAE_DW_SEGS[M], indep=False,
                     kept=None, lead=0, C=C, dil=dil, snake=sn)
                for C, dil, M, rate, sn in ((5, 1, 1, 1, True), (64, 3, 64, 1, True), (70, 9, 65, 1, True), (70, 9, 130, 1, True), (5, 3, 130, 2, True),
                                            (64, 9, 130, 1, False), (70, 1, 65, 1, False), (5, 9, 64, 1, True))]
for _case in VAE_DW_CASES:
    if _case["rate"] == 2:
        _case["segs"] = (1, 3, 2, 1, 58)               # 65 frames at two rows each: M = 130


@functools.lru_cache(maxsize=None)
def _vdw_inputs(name):
    c = next(c for c in VAE_DW_CASES if c["name"] == name)
    L = layout(c)
    C = c["C"]
    r = np.random.default_rng(_seed(name))
    x = r.standard_normal((L["a_rows"], C)).clip(-4.5, 4.5).astype(np.float32)
    x[L["in_rows"]:] = POISON[np.arange(2 * C).reshape(2, C) % 4]
    a1, a2 = (np.exp(r.uniform(-math.log(SNAKE_A), math.log(SNAKE_A), C)).astype(np.float32) for _ in range(2))
    return dict(case=c, L=L, x=x, w=(0.25 * r.standard_normal((7, C))).astype(np.float32), b=(0.3 * r.standard_normal(C)).astype(np.float32), a1=a1,
                i1=(np.float32(1) / a1).astype(np.float32), a2=a2, i2=(np.float32(1) / a2).astype(np.float32))


def vdw_inputs(c):
    return _vdw_inputs(c["name"])


def vdw_ref(c, x=None, mut=None, inp=None):
    """-> (y [M][C], bound).  mut: leak, drop_first (the window start), dil (dil + 1)"""
    inp = vdw_inputs(c) if inp is None else inp
    L, C = inp["L"], c["C"]
    dil = c["dil"] + (1 if mut == "dil" else 0)
    x = (inp["x"] if x is None else x).astype(np.float64)
    w, b = inp["w"].astype(np.float64), inp["b"].astype(np.float64)
    val, sab, dsn = (np.zeros((L["M"], C)) for _ in range(3))
    pad = 6 * dil
    for o0, o1, i0, i1 in L["segs"]:
        lo = max(i0 - pad, 0) if mut == "leak" else i0
        X = x[lo:i1]
        dX = np.zeros_like(X)
        if c["snake"]:
            X, dX = snake64(X, inp["a1"], inp["i1"])
        front = pad - (i0 - lo)
        Xp, dXp = np.concatenate([np.zeros((front, C)), X]), np.concatenate([np.zeros((front, C)), dX])
        if mut == "drop_first":
            Xp[pad] = 0.0
        t = np.arange(o1 - o0)
        for j in range(7):
            val[o0:o1] += Xp[t + j * dil] * w[j]
            sab[o0:o1] += np.abs(Xp[t + j * dil] * w[j])
            dsn[o0:o1] += dXp[t + j * dil] * np.abs(w[j])
    val = val + b
    dval = 8 * U * (sab + np.abs(b)) + dsn * (1.0 + 2.0 ** -10)
    if not c["snake"]:
        return val, dval
    y, own = snake64(val, inp["a2"], inp["i2"])
    return y, (1.0 + np.abs(inp["a2"].astype(np.float64) * inp["i2"].astype(np.float64))) * dval * (1.0 + 2.0 ** -10) + own


def vdw_twin(c, inp=None, args=None):
    inp = vdw_inputs(c) if inp is None else inp
    L, C, dil = inp["L"], c["C"], c["dil"]
    x = inp["x"]

    def note(a):
        if args is not None:
            args.setdefault("sin", []).append(np.asarray(a, np.float32).ravel())
    if c["snake"]:
        with np.errstate(invalid="ignore"):
            x, arg = snake32(x, inp["a1"], inp["i1"])
        note(arg[:L["in_rows"]])
    first, _ = spans(c, L)
    m = np.arange(L["M"])
    acc = np.zeros((L["M"], C), np.float32)
    for j in range(7):
        src = m - (6 - j) * dil
        nxt = (acc.astype(np.float64) + x[np.maximum(src, 0)].astype(np.float64) * inp["w"][j].astype(np.float64)).astype(np.float32)
        acc = np.where((src >= first)[:, None], nxt, acc)
    val = (acc + inp["b"]).astype(np.float32)
    if not c["snake"]:
        return val
    y, arg = snake32(val, inp["a2"], inp["i2"])
    note(arg)
    return y


# ---- VAE_UNIT ----------------------------------------------------------------------------------------------------------------------------
# vae_unit_kernel: a whole residual unit, y = map(x + b2 + sum_c h[c] Wt[c][n]) with h = snake2(b1 + depthwise(snake1(x))) exactly as
# vae_dw_kernel with both snakes (vdw_ref gives h and its bound dh), the pointwise sum one fmaf chain over c = 0 .. C - 1, then
# (acc + b2) + x, then the reader's map: [v aff[n] + aff[C + n]], snake(v) (none, the snake, or both).  Bound:
#     d_v = (C + 2) u (sum |h Wt| + |b2| + |x|) + sum dh |Wt| (1 + 2^-10)
# through the affine (|aff| d_v + u |v aff| + u |t|) and the snake's derivative 1 + |a b| with the snake's own error, as E_RESMAP.
# A thread owns RPT rows x 4 columns, 256 / (C / 4) threads per column group: unit_rpt is the product's rule.  The issue's C = 4, 12, 100,
# 128 give RPT 1, 1, 8, 8; C = 24 and 40 are added for RPT 2 and 4 (C / 4 = 3, 6, 10, 25 do not divide 256).
def unit_rpt(C):
    per = 256 // (C // 4)
    need = -(-64 // per)
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8


VAE_UNIT_CASES = [dict(name=f"unit_c{C}_d{dil}_m{M}_{mp}", kind=WINDOW, rate=rate, stride=1, segs=VAE_DW_SEGS[M] if rate == 1 else (1, 3, 2, 1, 58),
                       indep=False, kept=None, lead=0, C=C, dil=dil, snake=True, map=mp)
                  for C, dil, M, rate, mp in ((4, 1, 1, 1, "affine"), (12, 3, 64, 1, "none"), (24, 9, 65, 1, "snake"), (40, 3, 130, 2, "affine"),
                                              (100, 9, 130, 1, "affine"), (128, 9, 65, 1, "none"), (128, 1, 130, 1, "affine"), (100, 1, 64, 1, "snake"),
                                              (12, 9, 130, 1, "snake"), (4, 3, 65, 1, "none"))]


@functools.lru_cache(maxsize=None)
def _unit_inputs(name):
    c = next(c for c in VAE_UNIT_CASES if c["name"] == name)
    L = layout(c)
    C = c["C"]
    r = np.random.default_rng(_seed(name))
    x = r.standard_normal((L["a_rows"], C)).clip(-4.5, 4.5).astype(np.float32)
    x[L["in_rows"]:] = POISON[np.arange(2 * C).reshape(2, C) % 4]
    a1, a2 = (np.exp(r.uniform(-math.log(SNAKE_A), math.log(SNAKE_A), C)).astype(np.float32) for _ in range(2))
    ma = np.exp(r.uniform(-math.log(1.25), math.log(1.25), C)).astype(np.float32)      # the map sees x + conv2: |a v| stays below 8
    inp = dict(case=c, L=L, x=x, w=(0.25 * r.standard_normal((7, C))).astype(np.float32), b=(0.3 * r.standard_normal(C)).astype(np.float32), a1=a1,
               i1=(np.float32(1) / a1).astype(np.float32), a2=a2, i2=(np.float32(1) / a2).astype(np.float32),
               W2=(0.5 * r.standard_normal((C, C)) / math.sqrt(C)).astype(np.float32), b2=(0.3 * r.standard_normal(C)).astype(np.float32),
               ma=ma if c["map"] != "none" else None, mi=(np.float32(1) / ma).astype(np.float32) if c["map"] != "none" else None,
               aff=np.concatenate([r.uniform(0.4, 0.9, C), 0.3 * r.standard_normal(C)]).astype(np.float32) if c["map"] == "affine" else None)
    inp["packed"] = np.concatenate([inp[k].ravel() for k in ("w", "b", "a1", "i1", "a2", "i2", "W2", "b2")]).astype(np.float32)
    return inp


def unit_inputs(c):
    return _unit_inputs(c["name"])


def unit_ref(c, x=None, mut=None):
    """-> (y [M][C], bound).  mut: leak, drop_first, dil (of the depthwise conv), groups (the column group of thread t taken as t % (C / 4 + 1):
    conv2's columns shifted by four from the second group on)"""
    inp = unit_inputs(c)
    L, C, M = inp["L"], c["C"], inp["L"]["M"]
    xx = (inp["x"] if x is None else x).astype(np.float64)
    h, dh = vdw_ref(c, x=x, mut=None if mut == "groups" else mut, inp=inp)
    W2, b2 = inp["W2"].astype(np.float64), inp["b2"].astype(np.float64)
    if mut == "groups":
        W2 = np.concatenate([W2[:, :4], np.roll(W2[:, 4:], 4, 1)], 1) if C > 8 else W2[:, ::-1]
    acc = h @ W2
    v = acc + b2 + xx[:M]
    dv = (C + 2) * U * (np.abs(h) @ np.abs(W2) + np.abs(b2) + np.abs(xx[:M])) + (dh @ np.abs(W2)) * (1.0 + 2.0 ** -10)
    if inp["ma"] is None:
        return v, dv
    if inp["aff"] is not None:
        aff = inp["aff"].astype(np.float64)
        t = v * aff[:C] + aff[C:]
        dv = np.abs(aff[:C]) * dv + U * np.abs(v * aff[:C]) + U * np.abs(t)
        v = t
    a, b = inp["ma"].astype(np.float64), inp["mi"].astype(np.float64)
    y, own = snake64(v, a, b)
    return y, (1.0 + np.abs(a * b)) * dv * (1.0 + 2.0 ** -10) + own


def unit_twin(c, args=None):
    inp = unit_inputs(c)
    L, C, M = inp["L"], c["C"], inp["L"]["M"]
    h = vdw_twin(c, inp=inp, args=args)
    acc = np.zeros((M, C), np.float32)
    for k in range(C):
        acc = (acc.astype(np.float64) + h[:, k:k + 1].astype(np.float64) * inp["W2"][k][None].astype(np.float64)).astype(np.float32)
    v = ((acc + inp["b2"]).astype(np.float32) + inp["x"][:M]).astype(np.float32)
    if inp["ma"] is None:
        return v
    if inp["aff"] is not None:
        v = ((v * inp["aff"][:C]).astype(np.float32) + inp["aff"][C:]).astype(np.float32)
    y, arg = snake32(v, inp["ma"], inp["mi"])
    if args is not None:
        args.setdefault("sin", []).append(arg.ravel())
    return y


# ---- what the GPU module hands to the probe -----------------------------------------------------------------------------------------------
def geom(op, **kw):
    g = dict(rows_kind=0, snake=0, epi=0, M=0, a_rows=0, out_extra=0, Cin=0, taps=0, dil=0, K=0, N=0, bmod=0, ldc=0, rate=1, stride=1, lead=0,
             n_clips=0, n_loc=0, in_place=0, C=0, Q=0, S0=0, S1=0, clip=0, heads=0, hd=64, n_table=0, eps=0.0)
    g.update(kw)
    return g


def sub_layout(c, L, i):
    """window / clip i alone: its rows moved to the front -> (a layout for that launch, the slice of A rows, the slice of output rows)"""
    o0, o1, i0, i1 = L["segs"][i]
    c1 = {**c, "segs": (c["segs"][i],), "kept": None if c["kept"] is None else (c["kept"][i] - int(L["loc_a"][o0 // c["rate"]]),)}
    return c1, layout(c1), slice(i0, i1), slice(o0, o1)

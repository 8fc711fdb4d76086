"""The f32 kernels of the waveform codecs by themselves (the tile behind each row locator, RMSNorm, the depthwise conv + LayerNorm, the code
gather, both attentions, the output and input convs, the quantiser, the AudioVAE's depthwise conv and fused unit), through
qasr_codec_case_probe (csrc/codec_cases.hip: one call of the launch entry of csrc/codec_launch.h that the three codec classes call), against
the float64 references and derived bounds of tests/codec_cases.py.  No bar comes from a device run; tests/test_codec_cases_cpu.py proves on
the CPU, on every case's inputs, that honest f32 twins stay inside the bounds and that a defect of any one guard moves an output by >= 10 x
the bound or breaks an exact check.

  tile   every case of codec_cases.TILE_CASES: inside the bound; columns N .. ldc - 1 and the rows past the launch hold the sentinel; a second
         launch gives the same bits; every window / clip launched alone gives the same bits; with every other window (then every other
         but those) overwritten by +-1e30 / NaN patterns the clean windows keep their bits, so no read crosses a window start; the rows of A
         past the last one a locator reaches are NaN patterns throughout.  TailRows cases: every live row has the bits of the WindowRows
         launch of the same arrays, every tile of dead rows holds what was uploaded (the sentinel; in place, the residual).
  rms    C = 4, 255, 256, 257, 4096; rows of three magnitudes.
  dwln   the same C under WindowRows and ClipRows, windows of (1, 8, 2) rows: a row at a window start, one and six rows after it.
  out    codec_out_launch at C = 1, 3, 24, with and without the clip; TAIL with the first kept sample of the last window at 255, 256, 257
         (the 256-thread block edge): kept samples bit-equal to the launch without TAIL, every sample before them untouched.
  cenc_in  cenc_in_launch at C = 1, 3, 24 over clips of (1, 70, 2, 1, 55) samples.
  gather   Q = 1, 2, 16, D = 24, 255, 257, codes 0 and S - 1: the first codebook's row is a copy, the sum within (Q - 2) u sum |e|.
  vq     codec_cases.vq_check: code by code within the derived score bound of the float64 nearest row, the lower index of every
         duplicated pair, the final residual bit for bit; rows past the launch untouched in r and in codes.
  attention  codec_attn_launch over windows of (1, 2, CODEC_MAX_T, 1) frames and cenc_attn_launch over clips of (1, 31, 32, 33, 65), heads 1
         and 3: inside the bound, a window alone, a second launch, the neighbours as NaN patterns.
  vae_dw   vae_dw_launch with both snakes and with neither: C = 5, 64, 70, dilation 1, 3, 9, M = 1, 64, 65, 130, rates 1 and 2.
  vae_unit vae_unit_launch (RPT by the product's rule: 1, 2, 4, 8) at C = 4, 12, 24, 40, 100, 128, dilation 1, 3, 9, M = 1, 64, 65, 130, with no
         map, the snake, and the affine + snake.
  refusals  QASR_ERR_INVALID before any launch.

Every test prints its worst distance as a fraction of its bound (pytest -s).  Worst fractions on the MI355X: see MEASURED below.
"""
import ctypes as C
import numpy as np
import pytest
import codec_cases as K
import gpu_util
from qasr import _lib

pytestmark = pytest.mark.gpu

MEASURED = """worst fractions of the bound on the MI355X (the CPU f32 twins in brackets):
tile WindowRows 0.346 at E_LSRES (0.346), 0.329 at E_GELU (0.185: the device's erff is another implementation), 0.206 plain E_LIN (0.206),
0.156 E_RESMAP (0.156), 0.123 E_RES, 0.114 snake E_RES, 0.098 snake E_LIN, 0.076 E_SWIGLU; TailRows 0.127 (0.127); ClipRows 0.543 at
E_LSRES (0.543), 0.254 at E_GELU (0.204); VaeStrideRows 0.164 (0.164).
rms 0.131 (0.131); dwln 0.804 (0.804); out 0.126 (0.120); cenc_in 0.245 (0.245); gather 0.186 (0.186; bit-exact for Q <= 2);
vq 0.000: the float64 nearest row every time, every tie to the lower index, every residual bit-exact.
The excess of the device over the twin is confined to cases with erff (E_GELU) and sinf (out): the allowance of 4 x the CPU's ulp distance
was not needed by more than 0.33 of a bound.
attention: causal 0.008 / 0.008 (heads 1 / 3; twins 0.008 / 0.009), encoder 0.008 / 0.011 (0.008 / 0.011).
vae_dw 0.294 without the snakes (0.294), 0.218 with them.
vae_unit 0.081 (0.081) at C = 4 without a map; 0.045 and below at every other width (RPT 1, 2, 4, 8 alike).
The module's wall time: 2.9 s (20 tests, none above 0.4 s)."""
PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int32)
ERR_INVALID = 1
EXTRA = K.EXTRA                                        # sentinel rows after the launch's


@pytest.fixture(scope="module")
def eng():
    e = gpu_util.Engine("tiny", max_audio_seconds=2)
    yield e
    e.close()


def _p(a, t=PF):
    return None if a is None else a.ctypes.data_as(t)


def _call(eng, op, g, A, Wt, bias, sa, sb, ls, R, la, lb, out):
    gs = _lib.QasrCodecCase(**g)
    return eng.lib.qasr_codec_case_probe(eng.h, op, C.byref(gs), _p(A), _p(Wt), _p(bias), _p(sa), _p(sb), _p(ls), _p(R), _p(la, PI), _p(lb, PI), _p(out))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _padded(R, rows, ldc):
    """R [M][N] inside a [rows][ldc] image of the sentinel"""
    img = np.full((rows, ldc), K.SENTINEL, np.float32)
    img[:R.shape[0], :R.shape[1]] = R
    return img


# ---- tile -----------------------------------------------------------------------------------------------------------------------------------
def tile_args(c, inp, L=None, A=None, R=None, kind=None):
    """-> (geometry, arrays) of one launch of case c over layout L (default the case's own)"""
    L = inp["L"] if L is None else L
    A = inp["A"] if A is None else A
    R = inp["R"] if R is None else R
    M, ldc = L["M"], inp["ldc"]
    kind = c["kind"] if kind is None else kind
    g = K.geom(K.TILE, rows_kind=kind, snake=int(c["snake"]), epi=c["epi"], M=M, a_rows=A.shape[0], out_extra=EXTRA, Cin=c["Cin"], taps=c["taps"],
               dil=c["dil"], K=c["K"], N=c["N"], bmod=c["bmod"], ldc=ldc, rate=c["rate"], stride=c["stride"], lead=c["lead"] if kind == K.TAIL else 0,
               n_clips=L["n_clips"], n_loc=0 if L["loc_a"] is None else len(L["loc_a"]), in_place=int(c["in_place"]))
    out = np.full((M + EXTRA, ldc), K.SENTINEL, np.float32)
    Rimg = None
    if R is not None:
        Rimg = _padded(R[:M], M + EXTRA, ldc)
        if c["in_place"]:
            out, Rimg = Rimg, None
    arrays = dict(A=_f32(A), Wt=inp["Wt"], bias=inp["bias"], sa=inp["sa"], sb=inp["sb"], ls=inp["ls"], R=Rimg, la=L["loc_a"],
                  lb=L["loc_b"] if kind != K.WINDOW else None, out=out)
    return g, arrays


def run_tile(eng, c, inp, **kw):
    g, a = tile_args(c, inp, **kw)
    before = a["out"].copy()
    eng.check(_call(eng, K.TILE, g, a["A"], a["Wt"], a["bias"], a["sa"], a["sb"], a["ls"], a["R"], a["la"], a["lb"], a["out"]))
    return a["out"], before


def poisoned(inp, which):
    """A with the rows of windows i % 2 == which overwritten by +-1e30 / NaN patterns"""
    A = inp["A"].copy()
    for i, (_, _, i0, i1) in enumerate(inp["L"]["segs"]):
        if i % 2 == which:
            A[i0:i1] = K.POISON[np.arange((i1 - i0) * A.shape[1]).reshape(i1 - i0, -1) % 4]
    return A


def check_tile(eng, c):
    """-> the worst fraction of the bound"""
    inp = K.tile_inputs(c)
    L, M, ncols = inp["L"], inp["L"]["M"], inp["ncols"]
    want, bound = K.tile_ref(c)
    tail = c["kind"] == K.TAIL
    out, before = run_tile(eng, c, inp)
    assert np.array_equal(out[M:], before[M:]), "rows past the launch were written"
    assert np.array_equal(out[:M, ncols:], before[:M, ncols:]), "columns past N were written"
    rows = np.arange(M)
    if tail:
        live = rows >= K.live_rows(c, L)
        full, _ = run_tile(eng, c, inp, kind=K.WINDOW)
        assert np.array_equal(out[:M][live], full[:M][live]), "a live row differs from the WindowRows launch of the same arrays"
        for t in range(0, M, 64):
            if not live[t:t + 64].any():
                assert np.array_equal(out[t:t + 64], before[t:t + 64]), ("a tile of dead rows was written", t)
        f = K.frac(full[:M, :ncols], want, bound)
        f = max(f, K.frac(out[:M, :ncols][live], want[live], bound[live]))
    else:
        live = np.ones(M, bool)
        f = K.frac(out[:M, :ncols], want, bound)
    again, _ = run_tile(eng, c, inp)
    assert again.tobytes() == out.tobytes(), "a second launch gives other bits"
    # every window / clip alone
    if c["indep"]:
        L1 = K.layout({**c, "segs": (1,)})
        one, _ = run_tile(eng, c, inp, L=L1, A=inp["A"][:1])
        assert np.array_equal(one[:1, :ncols], out[:1, :ncols]), "row 0 alone"
    else:
        for i in range(len(L["segs"])):
            c1, L1, ai, oi = K.sub_layout(c, L, i)
            A1 = np.concatenate([inp["A"][ai], inp["A"][L["in_rows"]:]])
            one, _ = run_tile(eng, c1, inp, L=L1, A=A1, R=None if inp["R"] is None else inp["R"][oi])
            n = oi.stop - oi.start
            lv = live[oi]
            assert np.array_equal(one[:n, :ncols][lv], out[oi, :ncols][lv]), ("a window alone gives other bits", i)
    # the other windows poisoned: nothing of them is read
    if len(L["segs"]) > 1 and not c["indep"]:
        for which in (0, 1):
            got, _ = run_tile(eng, c, inp, A=poisoned(inp, which))
            for i, (o0, o1, _, _) in enumerate(L["segs"]):
                if i % 2 != which:
                    lv = live[o0:o1]
                    assert np.array_equal(got[o0:o1, :ncols][lv], out[o0:o1, :ncols][lv]), ("a clean window changed with its neighbours poisoned", i)
    return f


def _kind_cases(kind):
    return [c for c in K.TILE_CASES if c["kind"] == kind]


@pytest.mark.parametrize("kind", [K.WINDOW, K.TAIL, K.CLIP, K.VSTRIDE], ids=["window", "tail", "clip", "vae_stride"])
def test_tile(eng, kind):
    worst = {}
    for c in _kind_cases(kind):
        worst[c["name"]] = check_tile(eng, c)
    print("tile: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- rms, dwln ----------------------------------------------------------------------------------------------------------------------------------
def run_rms(eng, inp, rows=slice(None)):
    x = _f32(inp["x"][rows])
    M, Cw = x.shape
    out = np.full((M + EXTRA, Cw), K.SENTINEL, np.float32)
    g = K.geom(K.RMS, M=M, a_rows=M, out_extra=EXTRA, C=Cw, eps=K.RMS_EPS)
    eng.check(_call(eng, K.RMS, g, x, inp["w"], None, None, None, None, None, None, None, out))
    return out


def test_rms(eng):
    worst = {}
    for Cw in K.ROW_C:
        inp = K.rms_inputs(Cw)
        want, bound = K.rms_ref(Cw)
        out = run_rms(eng, inp)
        assert (out[3:] == K.SENTINEL).all(), "rows past the launch were written"
        worst[Cw] = K.frac(out[:3], want, bound)
        assert run_rms(eng, inp).tobytes() == out.tobytes(), "second launch"
        for i in range(3):
            assert np.array_equal(run_rms(eng, inp, slice(i, i + 1))[0], out[i]), ("row alone", Cw, i)
    print("rms: fractions of the bound " + ", ".join(f"C {k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def run_dwln(eng, c, inp, L=None, x=None):
    L = inp["L"] if L is None else L
    x = _f32(inp["x"] if x is None else x)
    M, Cw = L["M"], c["C"]
    out = np.full((M + EXTRA, Cw), K.SENTINEL, np.float32)
    g = K.geom(K.DWLN, rows_kind=c["kind"], M=M, a_rows=x.shape[0], out_extra=EXTRA, C=Cw, rate=c["rate"], n_clips=L["n_clips"], n_loc=len(L["loc_a"]))
    eng.check(_call(eng, K.DWLN, g, x, inp["w"], inp["b"], inp["lnw"], inp["lnb"], None, None, L["loc_a"], L["loc_b"], out))
    return out


def test_dwln(eng):
    worst = {}
    for c in K.DWLN_CASES:
        inp = K.dwln_inputs(c)
        L, M = inp["L"], inp["L"]["M"]
        want, bound = K.dwln_ref(c)
        out = run_dwln(eng, c, inp)
        assert (out[M:] == K.SENTINEL).all(), "rows past the launch were written"
        worst[c["name"]] = K.frac(out[:M], want, bound)
        assert run_dwln(eng, c, inp).tobytes() == out.tobytes(), "second launch"
        for i in range(len(L["segs"])):
            c1, L1, ai, oi = K.sub_layout(c, L, i)
            one = run_dwln(eng, c1, inp, L=L1, x=inp["x"][ai])
            assert np.array_equal(one[:oi.stop - oi.start], out[oi]), ("a window alone gives other bits", c["name"], i)
        for which in (0, 1):
            x = inp["x"].copy()
            for i, (_, _, i0, i1) in enumerate(L["segs"]):
                if i % 2 == which:
                    x[i0:i1] = K.POISON[np.arange((i1 - i0) * c["C"]).reshape(i1 - i0, -1) % 4]
            got = run_dwln(eng, c, inp, x=x)
            for i, (o0, o1, _, _) in enumerate(L["segs"]):
                if i % 2 != which:
                    assert np.array_equal(got[o0:o1], out[o0:o1]), ("a clean window changed with its neighbours poisoned", c["name"], i)
    print("dwln: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- out, cenc_in, gather ---------------------------------------------------------------------------------------------------------------------
def run_out(eng, c, inp, L=None, A=None, kind=None):
    L = inp["L"] if L is None else L
    A = _f32(inp["A"] if A is None else A)
    kind = c["kind"] if kind is None else kind
    M = L["M"]
    out = np.full(M + EXTRA, K.SENTINEL, np.float32)
    g = K.geom(K.OUT, rows_kind=kind, M=M, a_rows=A.shape[0], out_extra=EXTRA, C=c["Cin"], rate=c["rate"], n_loc=len(L["loc_a"]), clip=c["clip"])
    eng.check(_call(eng, K.OUT, g, A, inp["Wt"], inp["bias"], inp["sa"], inp["sb"], None, None, L["loc_a"], L["loc_b"] if kind == K.TAIL else None, out))
    return out


def test_out(eng):
    worst = {}
    for c in K.OUT_CASES:
        inp = K.tile_inputs(c)
        L, M = inp["L"], inp["L"]["M"]
        want, bound, done = K.out_ref(c)
        out = run_out(eng, c, inp)
        assert (out[M:] == K.SENTINEL).all(), "samples past the launch were written"
        assert (out[:M][~done] == K.SENTINEL).all(), "a sample before the first kept frame was written"
        worst[c["name"]] = K.frac(out[:M][done], want[done], bound[done])
        if c["clip"]:
            assert np.abs(out[:M][done]).max() <= 1.0 and (np.abs(want[done]) == 1.0).any(), "the clip"
        if c["kind"] == K.TAIL:
            full = run_out(eng, c, inp, kind=K.WINDOW)
            assert np.array_equal(full[:M][done], out[:M][done]), "a kept sample differs from the launch without TAIL"
            worst[c["name"]] = max(worst[c["name"]], K.frac(full[:M], want, bound))
        assert run_out(eng, c, inp).tobytes() == out.tobytes(), "second launch"
        for i in range(len(L["segs"])):
            c1, L1, ai, oi = K.sub_layout(c, L, i)
            one = run_out(eng, c1, inp, L=L1, A=np.concatenate([inp["A"][ai], inp["A"][L["in_rows"]:]]))
            assert np.array_equal(one[:oi.stop - oi.start][done[oi]], out[oi][done[oi]]), ("a window alone gives other bits", c["name"], i)
        for which in (0, 1):
            got = run_out(eng, c, inp, A=poisoned(inp, which))
            for i, (o0, o1, _, _) in enumerate(L["segs"]):
                if i % 2 != which:
                    assert np.array_equal(got[o0:o1], out[o0:o1]), ("a clean window changed with its neighbours poisoned", c["name"], i)
    print("out: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def run_cenc_in(eng, c, inp, L=None, A=None):
    L = inp["L"] if L is None else L
    A = _f32(inp["A"] if A is None else A)
    M = L["M"]
    out = np.full((M + EXTRA, c["N"]), K.SENTINEL, np.float32)
    g = K.geom(K.CENC_IN, M=M, a_rows=A.shape[0], out_extra=EXTRA, C=c["N"], n_clips=L["n_clips"], n_loc=len(L["loc_a"]))
    eng.check(_call(eng, K.CENC_IN, g, A, inp["Wt"], inp["bias"], None, None, None, None, L["loc_a"], None, out))
    return out


def test_cenc_in(eng):
    worst = {}
    for c in K.CENC_IN_CASES:
        inp = K.tile_inputs(c)
        L, M = inp["L"], inp["L"]["M"]
        want, bound = K.tile_ref(c)
        out = run_cenc_in(eng, c, inp)
        assert (out[M:] == K.SENTINEL).all(), "rows past the launch were written"
        worst[c["name"]] = K.frac(out[:M], want, bound)
        assert run_cenc_in(eng, c, inp).tobytes() == out.tobytes(), "second launch"
        for i in range(len(L["segs"])):
            c1, L1, ai, oi = K.sub_layout(c, L, i)
            one = run_cenc_in(eng, c1, inp, L=L1, A=np.concatenate([inp["A"][ai], inp["A"][L["in_rows"]:]]))
            assert np.array_equal(one[:oi.stop - oi.start], out[oi]), ("a clip alone gives other bits", c["name"], i)
        for which in (0, 1):
            got = run_cenc_in(eng, c, inp, A=poisoned(inp, which))
            for i, (o0, o1, _, _) in enumerate(L["segs"]):
                if i % 2 != which:
                    assert np.array_equal(got[o0:o1], out[o0:o1]), ("a clean clip changed with its neighbours poisoned", c["name"], i)
    print("cenc_in: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def run_gather(eng, c, inp, rows=slice(None), **over):
    codes = np.ascontiguousarray(inp["codes"][rows])
    M = codes.shape[0]
    out = np.full((M + EXTRA, 2 * c["D"]), K.SENTINEL, np.float32)
    g = K.geom(K.GATHER, M=M, a_rows=1, out_extra=EXTRA, C=c["D"], Q=c["Q"], S0=K.GATHER_S0, S1=K.GATHER_S1, n_loc=codes.size)
    g.update(over)
    rc = _call(eng, K.GATHER, g, None, inp["cb"], None, None, None, None, None, codes, None, out)
    return rc, out


def test_gather(eng):
    worst = {}
    for c in K.GATHER_CASES:
        inp = K.gather_inputs(c)
        want, bound = K.gather_ref(c)
        rc, out = run_gather(eng, c, inp)
        eng.check(rc)
        M, D = want.shape[0], c["D"]
        assert (out[M:] == K.SENTINEL).all(), "rows past the launch were written"
        assert np.array_equal(out[:M, :D], inp["cb"][inp["codes"][:, 0]]), "the first codebook's row is a copy"
        worst[c["name"]] = K.frac(out[:M], want, bound)
        assert run_gather(eng, c, inp)[1].tobytes() == out.tobytes(), "second launch"
        for i in range(M):
            assert np.array_equal(run_gather(eng, c, inp, slice(i, i + 1))[1][0], out[i]), ("row alone", c["name"], i)
    print("gather: fractions of the bound (0 = exact) " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def run_vq(eng, c, inp, rows=slice(None), **over):
    x = np.ascontiguousarray(inp["x"][rows])
    M, D, Q = x.shape[0], c["D"], c["Q"]
    r = np.full((M + EXTRA, 2 * D), K.SENTINEL, np.float32)
    r[:M] = x
    codes = np.full((M + EXTRA, Q), -7, np.int32)
    g = K.geom(K.VQ, M=M, a_rows=1, out_extra=EXTRA, C=D, Q=Q, S0=c["S0"], S1=c["S1"], n_loc=codes.size)
    g.update(over)
    more = (inp["cb1"], inp["p1"][0], inp["p1"][1]) if Q > 1 else (None, None, None)
    rc = _call(eng, K.VQ, g, None, inp["cb0"], inp["p0"][0], inp["p0"][1], more[0], more[1], more[2], None, codes, r)
    return rc, codes, r


def test_vq(eng):
    worst = {}
    for c in K.VQ_CASES:
        inp = K.vq_inputs(c)
        M = c["M"]
        rc, codes, r = run_vq(eng, c, inp)
        eng.check(rc)
        assert (codes[M:] == -7).all() and (r[M:] == K.SENTINEL).all(), "rows past the launch were written"
        worst[c["name"]] = K.vq_check(c, codes[:M], r[:M])
        _, codes2, r2 = run_vq(eng, c, inp)
        assert codes2.tobytes() == codes.tobytes() and r2.tobytes() == r.tobytes(), "second launch"
        for i in sorted({0, M // 2, M - 1}):
            _, c1, r1 = run_vq(eng, c, inp, slice(i, i + 1))
            assert np.array_equal(c1[0], codes[i]) and np.array_equal(r1[0], r[i]), ("a frame alone", c["name"], i)
    print("vq: (d(code) - min d) / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def run_attn(eng, inp, qkv=None, seg=None, **over):
    """seg: that window / clip alone"""
    enc, heads = inp["enc"], inp["heads"]
    qkv = inp["qkv"] if qkv is None else qkv
    loc = inp["loc"]
    if seg is not None:
        s0, n = int(inp["starts"][seg]), inp["segs"][seg]
        qkv = qkv[s0:s0 + n]
        loc = np.array([(0, n, q0, 0) for q0 in range(0, n, 32)] if enc else [(n, 0)], np.int32)
    M = qkv.shape[0]
    out = np.full((M + EXTRA, heads * 64), K.SENTINEL, np.float32)
    g = K.geom(K.ATTN_ENC if enc else K.ATTN_DEC, M=M, a_rows=M, out_extra=EXTRA, heads=heads, hd=64, n_table=inp["rope"].shape[0], n_clips=len(loc),
               n_loc=loc.size)
    g.update(over)
    rc = _call(eng, g.pop("op", K.ATTN_ENC if enc else K.ATTN_DEC), g, _f32(qkv), inp["rope"], None, None, None, None, None, np.ascontiguousarray(loc), None, out)
    return rc, out


@pytest.mark.parametrize("heads", K.ATTN_HEADS)
@pytest.mark.parametrize("enc", [0, 1], ids=["dec", "enc"])
def test_attention(eng, enc, heads):
    inp = K.attn_inputs(enc, heads)
    M = inp["M"]
    want, bound = K.attn_ref(inp)
    rc, out = run_attn(eng, inp)
    eng.check(rc)
    assert (out[M:] == K.SENTINEL).all(), "rows past the launch were written"
    f = K.frac(out[:M], want, bound)
    assert run_attn(eng, inp)[1].tobytes() == out.tobytes(), "second launch"
    for i, (s0, n) in enumerate(zip(inp["starts"], inp["segs"])):
        assert np.array_equal(run_attn(eng, inp, seg=i)[1][:n], out[s0:s0 + n]), ("a window alone gives other bits", i)
    for which in (0, 1):                               # the neighbours are NaN patterns
        qkv = inp["qkv"].copy()
        for i, (s0, n) in enumerate(zip(inp["starts"], inp["segs"])):
            if i % 2 == which:
                qkv[s0:s0 + n] = K.POISON[np.arange(n * qkv.shape[1]).reshape(n, -1) % 4]
        got = run_attn(eng, inp, qkv=qkv)[1]
        for i, (s0, n) in enumerate(zip(inp["starts"], inp["segs"])):
            if i % 2 != which:
                assert np.array_equal(got[s0:s0 + n], out[s0:s0 + n]), ("a clean window changed with its neighbours poisoned", i)
    print(f"attention {'enc' if enc else 'dec'} heads {heads}: fraction of the bound {f:.3f}")
    assert f <= 1.0


def run_vdw(eng, c, inp, L=None, x=None, **over):
    L = inp["L"] if L is None else L
    x = _f32(inp["x"] if x is None else x)
    M, Cw = L["M"], c["C"]
    out = np.full((M + EXTRA, Cw), K.SENTINEL, np.float32)
    g = K.geom(K.VAE_DW, rows_kind=K.WINDOW, snake=int(c["snake"]), M=M, a_rows=x.shape[0], out_extra=EXTRA, C=Cw, dil=c["dil"], rate=c["rate"],
               n_loc=len(L["loc_a"]))
    g.update(over)
    sn = [inp[k] if c["snake"] else None for k in ("a1", "i1", "a2", "i2")]
    rc = _call(eng, K.VAE_DW, g, x, inp["w"], inp["b"], sn[0], sn[1], sn[2], sn[3], L["loc_a"], None, out)
    return rc, out


def test_vae_dw(eng):
    worst = {}
    for c in K.VAE_DW_CASES:
        inp = K.vdw_inputs(c)
        L, M = inp["L"], inp["L"]["M"]
        want, bound = K.vdw_ref(c)
        rc, out = run_vdw(eng, c, inp)
        eng.check(rc)
        assert (out[M:] == K.SENTINEL).all(), "rows past the launch were written"
        worst[c["name"]] = K.frac(out[:M], want, bound)
        assert run_vdw(eng, c, inp)[1].tobytes() == out.tobytes(), "second launch"
        for i in range(len(L["segs"])):
            c1, L1, ai, oi = K.sub_layout(c, L, i)
            one = run_vdw(eng, c1, inp, L=L1, x=np.concatenate([inp["x"][ai], inp["x"][L["in_rows"]:]]))[1]
            assert np.array_equal(one[:oi.stop - oi.start], out[oi]), ("a window alone gives other bits", c["name"], i)
        if len(L["segs"]) > 1:
            for which in (0, 1):
                x = inp["x"].copy()
                for i, (_, _, i0, i1) in enumerate(L["segs"]):
                    if i % 2 == which:
                        x[i0:i1] = K.POISON[np.arange((i1 - i0) * c["C"]).reshape(i1 - i0, -1) % 4]
                got = run_vdw(eng, c, inp, x=x)[1]
                for i, (o0, o1, _, _) in enumerate(L["segs"]):
                    if i % 2 != which:
                        assert np.array_equal(got[o0:o1], out[o0:o1]), ("a clean window changed with its neighbours poisoned", c["name"], i)
    print("vae_dw: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_refusals_of_attention_and_vae_dw(eng):
    for enc in (0, 1):
        inp = K.attn_inputs(enc, 3)
        assert run_attn(eng, inp)[0] == 0
        for over in (dict(hd=128), dict(hd=32), dict(heads=0), dict(heads=65), dict(n_table=0), dict(n_table=34), dict(a_rows=inp["M"] - 1),
                     dict(n_clips=0), dict(n_loc=3), dict(M=inp["M"] + 1), dict(M=inp["M"] - 1)):
            rc, out = run_attn(eng, inp, **over)
            assert rc == ERR_INVALID and (out == K.SENTINEL).all(), (enc, over)
        for k, v in (((1, 0), 36), ((1, 1), 2), ((0, 0), 0)) if not enc else (((1, 0), 2), ((3, 2), 16), ((4, 1), 34), ((0, 1), 0)):
            bad = dict(inp, loc=inp["loc"].copy())
            bad["loc"][k] = v
            assert run_attn(eng, bad)[0] == ERR_INVALID, (enc, k, v)
    c = K.VAE_DW_CASES[3]
    inp = K.vdw_inputs(c)
    assert run_vdw(eng, c, inp)[0] == 0
    for over in (dict(dil=0), dict(dil=28), dict(C=0), dict(rows_kind=K.CLIP), dict(rows_kind=K.TAIL), dict(snake=2), dict(a_rows=100), dict(n_loc=3),
                 dict(rate=0)):
        assert run_vdw(eng, c, inp, **over)[0] == ERR_INVALID, over
    plain = dict(c, snake=False)
    assert run_vdw(eng, plain, inp, snake=1)[0] == ERR_INVALID                                      # the snakes' arrays are missing


def run_unit(eng, c, inp, L=None, x=None, drop=(), **over):
    L = inp["L"] if L is None else L
    x = _f32(inp["x"] if x is None else x)
    M, Cw = L["M"], c["C"]
    out = np.full((M + EXTRA, Cw), K.SENTINEL, np.float32)
    g = K.geom(K.VAE_UNIT, rows_kind=K.WINDOW, M=M, a_rows=x.shape[0], out_extra=EXTRA, C=Cw, dil=c["dil"], rate=c["rate"], n_loc=len(L["loc_a"]))
    g.update(over)
    a = dict(ma=inp["ma"], mi=inp["mi"], aff=inp["aff"], bias=None)
    for k in drop:
        a[k] = None
    a.update({k: v for k, v in over.items() if k in a})
    for k in a:
        g.pop(k, None)
    rc = _call(eng, K.VAE_UNIT, g, x, inp["packed"], a["bias"], a["ma"], a["mi"], a["aff"], None, L["loc_a"], None, out)
    return rc, out


def test_vae_unit(eng):
    worst = {}
    for c in K.VAE_UNIT_CASES:
        inp = K.unit_inputs(c)
        L, M = inp["L"], inp["L"]["M"]
        want, bound = K.unit_ref(c)
        rc, out = run_unit(eng, c, inp)
        eng.check(rc)
        assert (out[M:] == K.SENTINEL).all(), "rows past the launch were written"
        worst[c["name"]] = K.frac(out[:M], want, bound)
        assert run_unit(eng, c, inp)[1].tobytes() == out.tobytes(), "second launch"
        for i in range(len(L["segs"])):
            c1, L1, ai, oi = K.sub_layout(c, L, i)
            one = run_unit(eng, c1, inp, L=L1, x=np.concatenate([inp["x"][ai], inp["x"][L["in_rows"]:]]))[1]
            assert np.array_equal(one[:oi.stop - oi.start], out[oi]), ("a window alone gives other bits", c["name"], i)
        if len(L["segs"]) > 1:
            for which in (0, 1):
                x = inp["x"].copy()
                for i, (_, _, i0, i1) in enumerate(L["segs"]):
                    if i % 2 == which:
                        x[i0:i1] = K.POISON[np.arange((i1 - i0) * c["C"]).reshape(i1 - i0, -1) % 4]
                got = run_unit(eng, c, inp, x=x)[1]
                for i, (o0, o1, _, _) in enumerate(L["segs"]):
                    if i % 2 != which:
                        assert np.array_equal(got[o0:o1], out[o0:o1]), ("a clean window changed with its neighbours poisoned", c["name"], i)
    print("vae_unit: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_refusals_of_vae_unit_and_kept(eng):
    c = next(c for c in K.VAE_UNIT_CASES if c["map"] == "affine" and c["C"] == 100)
    inp = K.unit_inputs(c)
    assert run_unit(eng, c, inp)[0] == 0
    for over in (dict(C=132), dict(C=102), dict(C=0), dict(dil=0), dict(dil=10), dict(rows_kind=K.CLIP), dict(rows_kind=K.TAIL), dict(rows_kind=K.VSTRIDE),
                 dict(a_rows=100), dict(n_loc=3), dict(rate=0), dict(M=0)):
        rc, out = run_unit(eng, c, inp, **over)
        assert rc == ERR_INVALID and (out == K.SENTINEL).all(), over
    assert run_unit(eng, c, inp, drop=("mi",))[0] == ERR_INVALID and run_unit(eng, c, inp, drop=("ma",))[0] == ERR_INVALID       # half a map
    assert run_unit(eng, c, inp, drop=("ma", "mi"))[0] == ERR_INVALID                                                            # an affine without the map
    assert run_unit(eng, c, inp, bias=inp["b2"])[0] == ERR_INVALID
    t = K.TILE_BY_NAME["tail_edge"]                    # kept past its own window's last frame row, though inside the launch
    ti = K.tile_inputs(t)
    g, a = tile_args(t, ti)
    bad = ti["L"]["loc_b"].copy()
    bad[:200] = 200
    assert _call(eng, K.TILE, g, a["A"], a["Wt"], a["bias"], a["sa"], a["sb"], a["ls"], a["R"], a["la"], bad, a["out"]) == ERR_INVALID
    bad[:200] = 199
    assert _call(eng, K.TILE, g, a["A"], a["Wt"], a["bias"], a["sa"], a["sb"], a["ls"], a["R"], a["la"], bad, a["out"]) == 0


def test_refusals_of_the_other_launches(eng):
    c = K.GATHER_CASES[-1]
    inp = K.gather_inputs(c)
    assert run_gather(eng, c, inp)[0] == 0
    for over in (dict(Q=0), dict(Q=65), dict(C=4097), dict(S0=4), dict(S1=2), dict(n_loc=3), dict(M=5)):     # S0 = 4 / S1 = 2: a code outside its codebook
        rc, out = run_gather(eng, c, inp, **over)
        assert rc == ERR_INVALID and (out == K.SENTINEL).all(), over
    bad = dict(inp, codes=inp["codes"].copy())
    bad["codes"][2, 3] = -1
    assert run_gather(eng, c, bad)[0] == ERR_INVALID
    v = K.VQ_CASES[2]
    vi = K.vq_inputs(v)
    assert run_vq(eng, v, vi)[0] == 0
    for over in (dict(Q=0), dict(Q=65), dict(C=0), dict(C=4097), dict(S0=0), dict(S1=0), dict(n_loc=5), dict(M=0)):
        assert run_vq(eng, v, vi, **over)[0] == ERR_INVALID, over
    o = K.OUT_CASES[3]
    oi = K.tile_inputs(o)
    L = oi["L"]

    def orc(drop=(), la=None, lb=None, **over):
        g = K.geom(K.OUT, rows_kind=K.TAIL, M=L["M"], a_rows=oi["A"].shape[0], out_extra=EXTRA, C=o["Cin"], rate=1, n_loc=len(L["loc_a"]), clip=1)
        g.update(over)
        a = dict(A=oi["A"], Wt=oi["Wt"], bias=oi["bias"], sa=oi["sa"], sb=oi["sb"], la=L["loc_a"] if la is None else la, lb=L["loc_b"] if lb is None else lb,
                 out=np.full(L["M"] + EXTRA, K.SENTINEL, np.float32))
        for k in drop:
            a[k] = None
        return _call(eng, K.OUT, g, a["A"], a["Wt"], a["bias"], a["sa"], a["sb"], None, None, a["la"], a["lb"], a["out"])
    assert orc() == 0
    for name in ("A", "Wt", "bias", "sa", "sb", "la", "lb", "out"):
        assert orc(drop=(name,)) == ERR_INVALID, name
    assert orc(rows_kind=K.CLIP) == ERR_INVALID and orc(rows_kind=K.VSTRIDE) == ERR_INVALID and orc(clip=2) == ERR_INVALID and orc(C=0) == ERR_INVALID
    assert orc(a_rows=L["M"] - 1) == ERR_INVALID and orc(n_loc=5) == ERR_INVALID and orc(rate=0) == ERR_INVALID
    bad = L["loc_b"].copy(); bad[100:] = 73
    assert orc(lb=bad) == ERR_INVALID                                                                    # kept before its window
    bad = L["loc_a"].copy(); bad[100] = 99
    assert orc(la=bad) == ERR_INVALID
    e = K.CENC_IN_CASES[1]
    ei = K.tile_inputs(e)
    Le = ei["L"]

    def erc(drop=(), la=None, **over):
        g = K.geom(K.CENC_IN, M=Le["M"], a_rows=ei["A"].shape[0], out_extra=EXTRA, C=e["N"], n_clips=Le["n_clips"], n_loc=len(Le["loc_a"]))
        g.update(over)
        a = dict(A=ei["A"], Wt=ei["Wt"], bias=ei["bias"], la=Le["loc_a"] if la is None else la, out=np.full((Le["M"] + EXTRA, e["N"]), K.SENTINEL, np.float32))
        for k in drop:
            a[k] = None
        return _call(eng, K.CENC_IN, g, a["A"], a["Wt"], a["bias"], None, None, None, None, a["la"], None, a["out"])
    assert erc() == 0
    for name in ("A", "Wt", "bias", "la", "out"):
        assert erc(drop=(name,)) == ERR_INVALID, name
    assert erc(C=0) == ERR_INVALID and erc(a_rows=Le["M"] - 1) == ERR_INVALID and erc(n_clips=4) == ERR_INVALID and erc(n_clips=0) == ERR_INVALID
    bad = Le["loc_a"].copy(); bad[2] = bad[1]
    assert erc(la=bad) == ERR_INVALID
    bad = Le["loc_a"].copy(); bad[-1] -= 1
    assert erc(la=bad) == ERR_INVALID
    bad = Le["loc_a"].copy(); bad[0] = 1
    assert erc(la=bad) == ERR_INVALID


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    c = K.TILE_BY_NAME["w_m129"]
    inp = K.tile_inputs(c)

    def rc(c=c, inp=inp, op=K.TILE, drop=(), la=None, lb=None, **over):
        g, a = tile_args(c, inp)
        g.update(over)
        if la is not None:
            a["la"] = np.array(la, np.int32)
        if lb is not None:
            a["lb"] = np.array(lb, np.int32)
        for k in drop:
            a[k] = None
        return _call(eng, op, g, a["A"], a["Wt"], a["bias"], a["sa"], a["sb"], a["ls"], a["R"], a["la"], a["lb"], a["out"])
    fs = inp["L"]["loc_a"]
    assert rc() == 0
    assert rc(op=3) == ERR_INVALID and rc(op=-1) == ERR_INVALID
    for name in ("A", "Wt", "out", "la"):
        assert rc(drop=(name,)) == ERR_INVALID, name
    for combo in [(k, s, e) for k in range(4) for s in (0, 1) for e in range(6)]:                        # what the product does not instantiate
        if (combo[0], bool(combo[1]), combo[2]) not in K.combos_of_the_dispatch():
            assert rc(rows_kind=combo[0], snake=combo[1], epi=combo[2], lb=fs, n_clips=1) == ERR_INVALID, combo
    assert rc(rows_kind=4) == ERR_INVALID and rc(epi=6) == ERR_INVALID and rc(snake=2) == ERR_INVALID
    bad = fs.copy(); bad[5] = 3
    assert rc(la=bad) == ERR_INVALID                                                                       # fstart not f or fstart[f - 1]
    bad = fs.copy(); bad[0] = -1
    assert rc(la=bad) == ERR_INVALID
    assert rc(n_loc=128) == ERR_INVALID and rc(M=130) == ERR_INVALID                                     # counts that contradict the geometry
    assert rc(a_rows=128) == ERR_INVALID                                                                   # a row would read outside A
    assert rc(K=34) == ERR_INVALID and rc(taps=0) == ERR_INVALID and rc(dil=0) == ERR_INVALID and rc(rate=0) == ERR_INVALID
    assert rc(ldc=65) == ERR_INVALID and rc(bmod=0) == ERR_INVALID and rc(bmod=67) == ERR_INVALID and rc(in_place=1) == ERR_INVALID
    assert rc(M=0) == ERR_INVALID and rc(out_extra=-1) == ERR_INVALID
    assert b"codec case" in eng.lib.qasr_last_error(eng.h)

    t = K.TILE_BY_NAME["tail_edge"]
    ti = K.tile_inputs(t)
    kp = ti["L"]["loc_b"]
    assert rc(t, ti) == 0
    assert rc(t, ti, drop=("lb",)) == ERR_INVALID and rc(t, ti, lead=-1) == ERR_INVALID
    bad = kp.copy(); bad[250:] = 249
    assert rc(t, ti, lb=bad) == ERR_INVALID                                                              # kept before its window
    bad = kp.copy(); bad[10] = 131
    assert rc(t, ti, lb=bad) == ERR_INVALID                                                              # two values in one window
    bad = kp.copy(); bad[250:] = 300
    assert rc(t, ti, lb=bad) == ERR_INVALID                                                              # kept outside

    e = K.TILE_BY_NAME["c_s2"]
    ei = K.tile_inputs(e)
    os_, is_ = ei["L"]["loc_a"], ei["L"]["loc_b"]
    assert rc(e, ei) == 0
    bad = os_.copy(); bad[2] = bad[1]
    assert rc(e, ei, la=bad) == ERR_INVALID                                                              # ostart not increasing
    bad = os_.copy(); bad[-1] += 1
    assert rc(e, ei, la=bad) == ERR_INVALID                                                              # ostart does not end at M
    bad = is_.copy(); bad[2] = bad[1] - 1
    assert rc(e, ei, lb=bad) == ERR_INVALID                                                              # istart decreasing
    bad = is_.copy(); bad[0] = -1
    assert rc(e, ei, lb=bad) == ERR_INVALID
    assert rc(e, ei, stride=3) == ERR_INVALID and rc(e, ei, a_rows=100) == ERR_INVALID                   # a row would read outside A
    assert rc(e, ei, n_clips=4) == ERR_INVALID and rc(e, ei, drop=("lb",)) == ERR_INVALID
    s = K.TILE_BY_NAME["w_swiglu"]
    assert rc(s, K.tile_inputs(s), N=61) == ERR_INVALID and rc(s, K.tile_inputs(s), ldc=30) == ERR_INVALID
    r = K.TILE_BY_NAME["w_res"]
    assert rc(r, K.tile_inputs(r)) == 0 and rc(r, K.tile_inputs(r), drop=("R",)) == ERR_INVALID
    ls = K.TILE_BY_NAME["c_lsres"]
    assert rc(ls, K.tile_inputs(ls), drop=("ls",)) == ERR_INVALID and rc(ls, K.tile_inputs(ls), taps=2, K=48) == ERR_INVALID
    v = K.TILE_BY_NAME["v_s5"]
    assert rc(v, K.tile_inputs(v)) == 0 and rc(v, K.tile_inputs(v), stride=6) == ERR_INVALID

    d = K.DWLN_CASES[0]
    di = K.dwln_inputs(d)

    def drc(drop=(), **over):
        L = di["L"]
        g = K.geom(K.DWLN, rows_kind=d["kind"], M=L["M"], a_rows=di["x"].shape[0], out_extra=EXTRA, C=d["C"], rate=1, n_loc=len(L["loc_a"]))
        g.update(over)
        a = dict(x=di["x"], w=di["w"], b=di["b"], lnw=di["lnw"], lnb=di["lnb"], la=L["loc_a"], out=np.full((L["M"] + EXTRA, d["C"]), K.SENTINEL, np.float32))
        for k in drop:
            a[k] = None
        return _call(eng, K.DWLN, g, a["x"], a["w"], a["b"], a["lnw"], a["lnb"], None, None, a["la"], None, a["out"])
    assert drc() == 0
    assert drc(C=4097) == ERR_INVALID and drc(C=0) == ERR_INVALID and drc(rows_kind=K.TAIL) == ERR_INVALID and drc(rows_kind=K.VSTRIDE) == ERR_INVALID
    for name in ("x", "w", "b", "lnw", "lnb", "la", "out"):
        assert drc(drop=(name,)) == ERR_INVALID, name
    assert drc(a_rows=5) == ERR_INVALID and drc(n_loc=3) == ERR_INVALID
    ri = K.rms_inputs(4)
    out = np.full((5, 4), K.SENTINEL, np.float32)
    for over in (dict(C=0), dict(eps=0.0), dict(a_rows=2), dict(M=0)):
        g = K.geom(K.RMS, **{**dict(M=3, a_rows=3, out_extra=EXTRA, C=4, eps=K.RMS_EPS), **over})
        assert _call(eng, K.RMS, g, ri["x"], ri["w"], None, None, None, None, None, None, None, out) == ERR_INVALID, over
    assert (out == K.SENTINEL).all()

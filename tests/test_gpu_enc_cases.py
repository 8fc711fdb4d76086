"""The encoder-side kernels that are not the GEMM by themselves, through qasr_enc_case_probe (csrc/enc_cases.hip: ONE call of the product's
own launch entry on host data), against the float64 references and derived bounds of tests/enc_cases.py.  No bar comes from a device run;
tests/test_enc_cases_cpu.py proves on the CPU, on the inputs used here, that honest f32 twins of the kernels stay inside the bounds and
that a dropped or admitted edge key, a dropped tile, a ragged query group one key short, a norm over the padded width or with the
neighbour's statistics, a one-pass variance, a shifted tap, a padding column read as data and a width mask off by one each move an output
by >= 10 x the bound (smallest: 97 x for attention, 20 x for the one-pass variance).

  mha      mha_attention_launch: head_dim 64 at mha_form 0 / 1 / 2, head_dim 32 at form 0; every clip length of 1 .. 513 around the 16 / 32 /
           64 / 128 / 256 boundaries in four ragged batches of five clips x 3 heads (15 pairs against the 8-XCD map), plus exactly 8 and
           9 (clip, head) pairs and the encoder's windows of 104 / 104 / 98; readout / Gaussian / edge-spike inputs; NaN rows after the
           last clip, sentinel rows after the output.  Each form within the bound of ITS OWN reference (the forms are not bit-equal); every
           row written and finite; a clip alone gives the bits it gives inside a batch; a second launch gives the same bits.
  window   window_attention_launch at head_dim 32 / 64, lengths 1 .. 128: the same assertions.
  norms    layernorm_f32p_launch (act 0 / 1) and layernorm_gelu_f32_launch at every instantiation's width, both sides of it and the
           generic widths 896 / 1280; row counts around 4 x rows-per-wave; mixed rows and rows of mean 100; the input row after the last
           is NaN (a leaking clamped duplicate would show), the output rows after the last a sentinel.
  conv0    w2v_conv0_launch at 512 (wave kernel), 64, 40, 1024 channels, three ragged clips, given statistics.
  stats    wave_stats_launch, n = 0 .. 40001 at unaligned offsets, one clip with a DC offset of 50 deviations.
  conv1    conv1_launch at 8 / 64 / 480 channels: chunks of 100, 99, 51 and 1 frames; masked columns are +0 bit patterns.
  exact    argmax (both load paths, ties, NaN / infinity), cast, conv rows, frame info: compared without a tolerance.
  refusals QASR_ERR_INVALID before any launch; the encoder refuses a window above 128 tokens where it would pick the window kernel.

Every test prints its worst distance as a fraction of its bound (pytest -s).  Worst fractions on the MI355X: see MEASURED below.
"""
import ctypes as C
import numpy as np
import pytest
import enc_cases as E
import gpu_util
from gemm_cases import bf16_bits, bf16_from_bits
from qasr import _lib

pytestmark = pytest.mark.gpu

MEASURED = """worst fractions of the bound on the MI355X (the CPU f32 twins: mha_attention_kernel 0.740, mha64_attention_kernel 0.908,
window_attention_kernel 0.706, row kernels 0.969 = the half ulp of the output rounding, f32-output norm 0.170, wave stats 0.233); none above
its kernel's twin.  Per batch the largest excess is window hd 32 on (96, 63, 127, 32, 64), readout 0.616 against that batch's twin 0.328: P
values that round the other way than in the twin, which is what the 2^-7 A term allows; no finding:
mha hd 64 form 0: readout 0.740, gauss 0.287, spike 0.321; forms 1 and 2 (equal figures): readout 0.826, gauss 0.293, spike 0.317, on the
encoder's windows 104 / 104 / 98: readout 0.899, gauss 0.246, spike 0.310; hd 32 form 0: readout 0.623, gauss 0.282, spike 0.315.
window hd 32: readout 0.616, gauss 0.268, spike 0.320; hd 64: readout 0.326, gauss 0.297, spike 0.639.
layernorm, every width: bf16 0.969, gelu bf16 0.969, gelu f32 0.170 (mean-100 rows: 0.963 / 0.961 / 0.170).
conv0 0.968 (C 512, 1024), 0.967 (C 64, 40); conv1 0.969; wave stats mean <= 0.015, inv_std <= 0.233 (n = 0), DC clip 0.015.
argmax, cast, conv rows, frame info: exact.  The whole module runs in 5 s."""
ERR_INVALID = 1
SENT = E.SENTINEL
FORMS = ((64, 0), (64, 1), (64, 2), (32, 0))


@pytest.fixture(scope="module")
def eng():
    e = gpu_util.Engine("tiny", max_audio_seconds=2)
    form = e.get_tuning("mha_form")
    yield e
    e.set_tuning("mha_form", form)
    e.close()


def _ptr(a, t):
    return None if a is None else C.cast(a.ctypes.data, t)


def probe(eng, op, out, inp=None, idx=None, off=None, pf=None, pw=None, **geom):
    """-> status; `out` is overwritten in place"""
    g = _lib.QasrEncCase(**geom)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((inp, None), (idx, np.int32), (off, np.int64), (pf, np.float32),
                                                                          (pw, np.uint16))]
    assert out.flags["C_CONTIGUOUS"]
    return eng.lib.qasr_enc_case_probe(eng.h, op, C.byref(g), _ptr(keep[0], C.c_void_p), _ptr(keep[1], C.POINTER(C.c_int32)),
                                       _ptr(keep[2], C.POINTER(C.c_int64)), _ptr(keep[3], C.POINTER(C.c_float)),
                                       _ptr(keep[4], C.POINTER(C.c_uint16)), _ptr(out, C.c_void_p))


def _frac(got, v, bound):
    assert np.isfinite(got).all()
    return float(np.where((bound == 0) & (got == v), 0.0, np.abs(got - v) / np.where(bound == 0, 1e-300, bound)).max())


# ---- attention ----------------------------------------------------------------------------------------------------------------------------------
def run_attn(eng, op, bits, cu, heads, hd, max_len, out_extra=2):
    """-> bf16 bits [rows, heads * hd]; asserts the sentinel rows after them untouched"""
    rows = int(cu[-1])
    out = np.full((rows + out_extra, heads * hd), SENT, np.uint16)
    eng.check(probe(eng, op, out, inp=bits, idx=cu, rows=rows, n_clips=len(cu) - 1, in_extra=bits.shape[0] - rows, out_extra=out_extra,
                    heads=heads, hd=hd, max_len=max_len))
    assert (out[rows:] == SENT).all(), "a row after the last clip was written"
    return out[:rows]


def attn_case(eng, op, clips, heads, hd, kind, tile):
    """every input set of one batch against the reference; alone = batch and launch = launch on the Gaussian set -> worst fraction per set"""
    worst = {}
    for set_kind, spike in E.attn_sets(clips, tile):
        qkv, bits, cu = E.attn_inputs(clips, heads, hd, set_kind, spike, tile)
        v, bound = E.attn_expect_cached(clips, heads, hd, set_kind, spike, tile, kind)
        out = run_attn(eng, op, bits, cu, heads, hd, max(clips))
        f = _frac(bf16_from_bits(out).reshape(v.shape), v, bound)
        worst[set_kind] = max(worst.get(set_kind, 0.0), f)
        if set_kind != "gauss":
            continue
        assert np.array_equal(out, run_attn(eng, op, bits, cu, heads, hd, max(clips))), "a second launch gave other bits"
        for c, L in enumerate(clips):
            alone = np.concatenate([bits[cu[c]:cu[c + 1]], bits[cu[-1]:]])
            got = run_attn(eng, op, alone, np.array([0, L], np.int32), heads, hd, L)
            assert np.array_equal(got, out[cu[c]:cu[c + 1]]), f"clip {c} (length {L}) alone differs from the same clip inside the batch"
    return worst


def _report(name, worst):
    print(f"{name}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("clips", E.MHA_BATCHES)
@pytest.mark.parametrize("hd,form", FORMS)
def test_mha(eng, hd, form, clips):
    eng.set_tuning("mha_form", form)
    _report(f"mha hd {hd} form {form} clips {clips}", attn_case(eng, E.MHA, clips, E.HEADS, hd, E.mha_kind(hd, form), 64))


@pytest.mark.parametrize("heads,clips", [E.PAIRS8, E.PAIRS9])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_mha_eight_and_nine_pairs(eng, form, heads, clips):
    """heads x clips = 8 fills the XCD map exactly, 9 starts a second round with one pair"""
    eng.set_tuning("mha_form", form)
    _report(f"mha hd 64 form {form} {heads * len(clips)} pairs", attn_case(eng, E.MHA, clips, heads, 64, E.mha_kind(64, form), 64))


@pytest.mark.parametrize("form", [1, 2])
def test_mha_on_encoder_windows(eng, form):
    """what the Qwen3 audio encoder launches at head_dim 64: windows of 104 / 104 / 98 tokens as clips"""
    eng.set_tuning("mha_form", form)
    _report(f"mha hd 64 form {form} encoder windows", attn_case(eng, E.MHA, E.ENCODER_WINDOWS, E.HEADS, 64, "mha64", 64))


@pytest.mark.parametrize("clips", E.WINDOW_BATCHES)
@pytest.mark.parametrize("hd", [32, 64])
def test_window(eng, hd, clips):
    _report(f"window hd {hd} clips {clips}", attn_case(eng, E.WINDOW, clips, E.HEADS, hd, "window", 16))


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", E.LN_WIDTHS)
def test_layernorm(eng, D):
    worst = {}
    for rows in E.ln_row_counts(D):
        for kind in ("mixed", "mean100"):
            x, g, b = E.ln_inputs(D, rows, kind)
            for op, form in E.LN_FORMS.items():
                v, bound = E.ln_ref(x[:rows], g, b, form)
                if form == 2:
                    out = np.full((rows + 2, D), E.SENTINEL_F32, np.float32)
                else:
                    out = np.full((rows + 2, D), SENT, np.uint16)
                eng.check(probe(eng, op, out, inp=x, pf=np.concatenate([g, b]), rows=rows, in_extra=1, out_extra=2, D=D, eps=E.LN_EPS))
                assert (out[rows:] == (E.SENTINEL_F32 if form == 2 else SENT)).all(), "a row after the last was written"
                got = out[:rows].astype(np.float64) if form == 2 else bf16_from_bits(out[:rows])
                key = f"{('bf16', 'gelu bf16', 'gelu f32')[form]} {kind}"
                worst[key] = max(worst.get(key, 0.0), _frac(got, v, bound))
    _report(f"layernorm D {D} (rows {E.ln_row_counts(D)})", worst)


# ---- conv0, wave stats, conv1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,frames", E.CONV0_CASES)
def test_conv0(eng, C_, frames):
    inp = E.conv0_inputs(C_, frames)
    v, bound, written = E.conv0_ref(inp)
    rows = inp["rows"]
    out = np.full((rows + 2, C_), SENT, np.uint16)
    pf = np.concatenate([inp["stats"].reshape(-1), inp["w"].reshape(-1), inp["bias"], inp["g"], inp["be"]])
    eng.check(probe(eng, E.CONV0, out, inp=inp["pcm"], off=inp["pcm_off"], idx=np.concatenate([inp["frame_off"], inp["n_out"]]), pf=pf,
                    rows=rows, n_clips=len(frames), out_extra=2, max_len=max(frames), D=C_, n_in=inp["pcm"].size, eps=E.CONV0_EPS))
    assert (out[rows:] == SENT).all() and (out[:rows][~written] == SENT).all(), "a row outside every clip's frames was written"
    _report(f"conv0 C {C_} frames {frames}", {"out": _frac(bf16_from_bits(out[:rows][written]), v[written], bound[written])})


def test_wave_stats(eng):
    pcm, off, ns = E.wave_inputs()
    v, bound = E.wave_ref(pcm, off, ns)
    B = len(ns)
    out = np.full((B + 1, 2), E.SENTINEL_F32, np.float32)
    eng.check(probe(eng, E.WAVE_STATS, out, inp=pcm, off=off, idx=ns, rows=B, out_extra=1, n_in=pcm.size, eps=E.WAVE_EPS))
    assert (out[B:] == E.SENTINEL_F32).all()
    got = out[:B].astype(np.float64)
    frac = np.where((bound == 0) & (got == v), 0.0, np.abs(got - v) / np.where(bound == 0, 1e-300, bound))
    assert np.isfinite(got).all()
    print("wave stats: fractions of the bound (mean, inv_std) per clip " + ", ".join(f"n {n}: {a:.3f} {b:.3f}" for n, (a, b) in zip(ns, frac)))
    assert (frac <= 1.0).all(), frac


@pytest.mark.parametrize("C_,n_mels", E.CONV1_CASES)
def test_conv1(eng, C_, n_mels):
    inp = E.conv1_inputs(C_, n_mels)
    v, bound = E.conv1_ref(inp)
    n, H1, W1 = len(E.CONV1_IMAGES), inp["H1"], E.CONV1_W1
    out = np.full((n + 1, H1, W1, C_), SENT, np.uint16)
    eng.check(probe(eng, E.CONV1, out, inp=inp["mel"], idx=inp["meta"], pf=inp["bias"], pw=bf16_bits(inp["w"]), rows=n, out_extra=1, D=C_,
                    n_in=inp["mel"].size, n_mels=n_mels, mel_stride=E.CONV1_STRIDE, H1=H1, W1=W1))
    assert (out[n:] == SENT).all(), "an image after the last was written"
    for i in range(n):
        assert (out[i, :, inp["meta"][i, 4]:] == 0).all(), f"image {i}: a column from w1 upward is not +0"
    got = bf16_from_bits(out[:n])
    _report(f"conv1 C {C_} n_mels {n_mels}", {"all": _frac(got, v, bound), "oh 0": _frac(got[:, 0], v[:, 0], bound[:, 0]),
                                              f"oh {H1 - 1}": _frac(got[:, -1], v[:, -1], bound[:, -1])})


# ---- exact kernels ------------------------------------------------------------------------------------------------------------------------------------
def _argmax_rows(n, rng):
    """-> (x [rows, n] finite, expected ids): the maximum at 0, at n - 1, at every residue mod 4, duplicated inside one thread's stride
    (i, i + 1024), duplicated across threads, and the -0.0 / +0.0 ties"""
    rows, want = [], []

    def add(places, value=2.0, base=None):
        x = rng.uniform(-1.0, 1.0, n).astype(np.float32) if base is None else np.full(n, base, np.float32)
        for i, val in places:
            x[i] = val
        rows.append(x)
        want.append(min(i for i, val in places if val == max(v_ for _, v_ in places)))

    add([(0, 2.0)])
    add([(n - 1, 2.0)])
    for r in range(4):
        add([(min(n - 1, n // 2 // 4 * 4 + r), 2.0)])
    if n > 1024 + 5:
        add([(5, 2.0), (5 + 1024, 2.0)])
        add([(5 + 1024, 2.0), (2 * 1024 + 6, 2.0)] if n > 2 * 1024 + 6 else [(5 + 1024, 2.0)])
    if n > 9:
        add([(3, 2.0), (4, 2.0)])
        add([(n - 2, 2.0), (2, 2.0), (n - 6, 2.0)])
        add([(2, -0.0), (7, 0.0)], base=-1.0)
        add([(1, 0.0), (6, -0.0)], base=-1.0)
    return np.stack(rows), np.asarray(want, np.int32)


@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 1023, 1024, 1025, 10288])
def test_argmax(eng, n):
    rng = np.random.default_rng(n)
    for ld in (n, n + 1):
        x, want = _argmax_rows(n, rng)
        assert np.array_equal(E.argmax_ref(x)[0], want)
        bad = x[:3].copy()
        bad[0, n // 2], bad[1, n // 3], bad[2, :] = np.nan, np.inf, np.nan
        for rows_x, finite in ((x, True), (bad, False)):
            rows = rows_x.shape[0]
            buf = np.full((rows + 1, ld), np.nan, np.float32)          # the pitch padding and the row after the last are NaN
            buf[:rows, :n] = rows_x
            out = np.full(rows + 3, -7, np.int32)
            out[-1] = 0
            eng.check(probe(eng, E.ARGMAX, out, inp=buf, rows=rows, in_extra=1, out_extra=2, D=n, ld=ld))
            ids, err = E.argmax_ref(rows_x)
            assert np.array_equal(out[:rows], ids), (n, ld, out[:rows], ids)
            assert (out[rows:rows + 2] == -7).all()
            assert out[-1] == (0 if finite else 1), "the error word"
            if not finite:
                assert out[2] == 0                                    # the all-NaN row


def test_cast(eng):
    rng = np.random.default_rng(3)
    for n in (4, 252, 256, 260, 1028):
        x = np.concatenate([(rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)).astype(np.float32), np.full(4, np.nan, np.float32)])
        x[:4] = (1.00390625, 1.01171875, -0.0, 3.4e38)                # two ties to even, -0, a value that rounds to infinity
        out = np.full(n + 4, SENT, np.uint16)
        eng.check(probe(eng, E.CAST, out, inp=x, rows=n, in_extra=4, out_extra=4))
        assert np.array_equal(out[:n], E.cast_ref_bits(x[:n])) and (out[n:] == SENT).all(), n


def _clip_tables(B, total):
    """-> (offsets, lengths) of B clips that fill `total` rows, the last one empty where B > 1"""
    if B == 1:
        return np.array([0], np.int32), np.array([total], np.int32)
    n = np.array([100, 1, 60, total - 161, 0], np.int32)
    return np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32), n


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("total", [255, 256, 257])
def test_conv_rows_and_frame_info(eng, B, total):
    out_off, n_out = _clip_tables(B, total)
    out = np.full((total + 2, 2), -7, np.int32)
    eng.check(probe(eng, E.FRAME_INFO, out, idx=np.concatenate([out_off, n_out]), rows=total, n_clips=B, out_extra=2))
    assert np.array_equal(out[:total], E.frame_info_ref(out_off, n_out, total)) and (out[total:] == -7).all()
    in_off = (np.arange(B) * 1000 + 3).astype(np.int32)
    for short in (0, 1):                                             # 1: every clip has one frame fewer than its slot -> offset 0 there
        n = np.maximum(n_out - short, 0)
        out = np.full(total + 2, -7, np.int64)
        eng.check(probe(eng, E.CONV_ROWS, out, idx=np.concatenate([in_off, out_off, n]), rows=total, n_clips=B, out_extra=2, stride=2, D=8))
        assert np.array_equal(out[:total], E.conv_rows_ref(in_off, out_off, n, total, 2, 8)) and (out[total:] == -7).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    """every refusal is a status: nothing is launched with these arguments"""
    eng.set_tuning("mha_form", 0)
    qkv = np.zeros((40, 3 * 2 * 64), np.uint16)
    out = np.zeros((40, 2 * 64), np.uint16)
    base = dict(rows=40, n_clips=2, heads=2, hd=64, max_len=30)
    cu = np.array([0, 10, 40], np.int32)

    def refused(op, out_, **kw):
        rc = probe(eng, op, out_, **kw)
        assert rc == ERR_INVALID, (op, kw.keys(), rc)
        assert b"enc case" in eng.lib.qasr_last_error(eng.h)

    assert probe(eng, E.MHA, out, inp=qkv, idx=cu, **base) == 0
    for bad_cu in ([1, 10, 40], [0, 10, 10], [0, 20, 10], [0, 10, 39], [0, 10, 41]):
        refused(E.MHA, out, inp=qkv, idx=np.array(bad_cu, np.int32), **base)
    refused(E.MHA, out, inp=qkv, idx=cu, **{**base, "max_len": 29})
    refused(E.MHA, out, inp=qkv, idx=cu, **{**base, "hd": 128, "heads": 1})
    refused(E.MHA, out, inp=qkv, idx=cu, **{**base, "hd": 16, "heads": 8})
    refused(E.WINDOW, out, inp=qkv, idx=cu, **{**base, "hd": 48})
    refused(12, out, inp=qkv, idx=cu, **base)
    for form in (1, 2):                                              # head_dim 32 has form 0 only: the probe runs what was asked for, or nothing
        eng.set_tuning("mha_form", form)
        refused(E.MHA, out, inp=qkv, idx=cu, **{**base, "hd": 32, "heads": 4})
        assert probe(eng, E.WINDOW, out, inp=qkv, idx=cu, **{**base, "hd": 32, "heads": 4}) == 0      # the knob does not concern the window kernel
    eng.set_tuning("mha_form", 0)
    assert probe(eng, E.MHA, out, inp=qkv, idx=cu, **{**base, "hd": 32, "heads": 4}) == 0
    big = np.zeros((129, 3 * 64), np.uint16)
    refused(E.WINDOW, np.zeros((129, 64), np.uint16), inp=big, idx=np.array([0, 129], np.int32), rows=129, n_clips=1, heads=1, hd=64)
    x = np.zeros((2, 2052), np.float32)
    o16 = np.zeros((2, 2052), np.uint16)
    for op in E.LN_FORMS:
        for D in (6, 2052, 0):
            refused(op, o16.view(np.float32) if op == E.LN_GELU_F32 else o16, inp=x, pf=np.ones(2 * 2052, np.float32), rows=1, D=D, eps=1e-5)
    # conv0: channels, a frame range past the pcm array, past the output rows, max_out below a clip
    pcm = np.zeros(100, np.float32)
    c0 = dict(inp=pcm, off=np.array([0], np.int64), idx=np.array([0, 10], np.int32), pf=np.zeros(2 + 13 * 1032, np.float32), rows=10, n_clips=1,
              max_len=10, D=8, n_in=100, eps=1e-5)
    o0 = np.zeros((10, 1032), np.uint16)
    assert probe(eng, E.CONV0, o0, **c0) == 0
    refused(E.CONV0, o0, **{**c0, "D": 1032})
    refused(E.CONV0, o0, **{**c0, "off": np.array([46], np.int64)})
    refused(E.CONV0, o0, **{**c0, "off": np.array([-1], np.int64)})
    refused(E.CONV0, o0, **{**c0, "idx": np.array([1, 10], np.int32)})
    refused(E.CONV0, o0, **{**c0, "max_len": 9})
    ws = dict(inp=pcm, off=np.array([10], np.int64), idx=np.array([90], np.int32), rows=1, n_in=100, eps=1e-5)
    o1 = np.zeros((1, 2), np.float32)
    assert probe(eng, E.WAVE_STATS, o1, **ws) == 0
    refused(E.WAVE_STATS, o1, **{**ws, "idx": np.array([91], np.int32)})
    refused(E.WAVE_STATS, o1, **{**ws, "off": np.array([101], np.int64)})
    # conv1: channels, a ChunkMeta outside mel
    mel = np.zeros((1, 4, 20), np.float32)
    meta = np.array([[0, 0, 20, 20, 10, 5, 3, 0, 3]], np.int32)
    c1 = dict(inp=mel, idx=meta, pf=np.zeros(16, np.float32), pw=np.zeros(9 * 16, np.uint16), rows=1, D=8, n_in=80, n_mels=4, mel_stride=20,
              H1=2, W1=10)
    o2 = np.zeros((1, 2, 10, 16), np.uint16)
    assert probe(eng, E.CONV1, o2, **c1) == 0
    refused(E.CONV1, o2, **{**c1, "D": 12})
    for bad in ([0, 1, 20], [1, 0, 20], [0, 0, 21], [0, -1, 5]):
        m = meta.copy()
        m[0, :3] = bad
        refused(E.CONV1, o2, **{**c1, "idx": m})
    refused(E.CONV1, o2, **{**c1, "n_in": 79})
    refused(E.CAST, np.zeros(8, np.uint16), inp=np.zeros(8, np.float32), rows=6)
    refused(E.ARGMAX, np.zeros(3, np.int32), inp=np.zeros(8, np.float32), rows=2, D=4, ld=3)


def test_encoder_refuses_a_window_above_128_tokens():
    """tiny geometry has head_dim 32, so the encoder takes window_attention_kernel, which holds at most 128 keys: n_window_infer = 2000
    plans windows of 260 tokens, and the encoder must refuse before it launches anything; 117 tokens in one window still run"""
    import torch
    from qasr import config as QC, synth
    sd = synth.synth_state_dict(QC.AUDIO_TINY, QC.TEXT_TINY, seed=3, init="stress")
    e = gpu_util.Engine("tiny", max_audio_seconds=30, n_window_infer=2000)
    try:
        e.load_state_dict(sd)
        g = torch.Generator().manual_seed(2)
        assert np.isfinite(e.encode((torch.randn(128, 900, generator=g) * 0.5).numpy())).all()
        with pytest.raises(RuntimeError, match="exceeds the 128"):
            e.encode((torch.randn(128, 1300, generator=g) * 0.5).numpy())
    finally:
        e.close()

"""What the codecs' network tests can and cannot see (step 0), the float64 references of tests/codec_cases.py against textbook convs and
against a second evaluation over the locator arrays, the f32 twins inside the bounds on every GPU case's inputs, and the mutation
condition: tests/test_gpu_codec_cases.py cannot pass while blind to a defect of one guard of codec_gemm_kernel, codec_rms_kernel,
codec_dwln_kernel, codec_gather_kernel, codec_out_kernel, cenc_in_kernel, cenc_vq_kernel, codec_attn_kernel, cenc_attn_kernel or
vae_dw_kernel or vae_unit_kernel.  No GPU.

Measured here: STEP0 and MEASURED_CPU below.

Exempt from the mutation condition, because no input can show them:
  * leak (a tap admitted before `first`): cases of one tap; cases whose every early tap lies before row 0 of the launch (one window);
  * dil (dilation off by one): cases of one tap, and w_m1, whose one row has no tap but the last inside its window;
  * ktail (the operand's k < K guard): K a multiple of 16 (w_m64, w_m65, w_gelu, w_swiglu, w_resmap_no_r, w_resmap_no_affine, w_snake_tconv,
    tail_rate2, c_gelu, c_swiglu and every K = 48 case).  Where a read element is finite and the WEIGHT's guard holds it adds a * 0 and is
    harmless by itself; the mutation models both guards gone (weight 1);
  * bias (bias[n] for bias[n % bmod]): bmod = N, no bias, and ClipRows / VaeStrideRows, whose bias is bias[n];
  * clip, stride: launches of independent rows or of one clip; stride also where every clip has one output row;
  * N-tail column written, a live tile skipped: exact checks by construction.  A write to column N of row m lands on a sentinel column
    where ldc > N, else on column 0 of row m + 1, which another thread rewrites: only the LAST row shows it for certain, on the first of
    the codec_cases.EXTRA sentinel rows every launch carries (test_n_tail_lands_on_a_sentinel: EXTRA >= 1, every N off the tile has a
    case, some with ldc > N); a skipped live tile leaves
    the sentinel (or, in place, the residual) where the WindowRows launch of the same arrays has a value (asserted on the GPU; here: that
    every TailRows case has skipped tiles and live rows, and that the value there differs from what was uploaded);
  * the neighbour's LayerNorm statistics: none exempt (every DWLN case has more than one row);
  * attention: the own key dropped leaves the first row of a window without a key (NaN, which the GPU test refuses as such); key i + 1
    admitted for the last row of the last window, and the row after the last clip, lie outside every array; a missing rescale shows only
    on rows whose running maximum moves at a 32-key tile edge, so clips of one tile are exempt and a clip of several must show it on at
    least one output;
  * vae_dw, vae_unit: a launch of one window of one row has no earlier tap to drop or move and no neighbour to leak from (drop_first still
    applies).
"""
import numpy as np
import pytest
import codec_cases as K

STEP0 = """max |d| / peak of the float64 oracle against itself with one edge defect in its conv primitives, beside the bound of the network's
GPU test (test_step0_what_the_network_tests_see asserts every line at more than 10 x the bound):
decoder (codec_oracle, reduced geometry, T = 11, pre-clip forward; bound 6.33e-5 of test_gpu_codec.py):
    a tap admitted before the window start 8.1e-1 (12 851 x)   the first tap after it dropped 8.2e-1 (12 940 x)
    dilation 3 -> 4 in one unit 5.6e-1 (8 831 x)                 bias[n] for bias[n % bmod] 2.7e-1 (4 289 x)
encoder convs (codec_enc_oracle, reduced, 3 843 samples; bound 1.23e-5 of test_gpu_codec_enc.py; it has no transposed conv):
    leak 2.2 (182 788 x)   dropped first tap 1.6e-1 (12 662 x)   dilation 5.2e-1 (42 638 x)
AudioVAE (avae_oracle, tiny, decode of 9 frames; bound 5.9e-6 of test_gpu_avae.py):
    leak 8.0e-1 (135 539 x)   dropped first tap 1.6e-1 (26 301 x)   dilation 1.7e-1 (28 942 x)   bias 1.9e-1 (32 395 x)
So NO network test is blind to these four defects on the geometries it runs: the f32-distance bars are tight and the defects are of order
one.  What the network tests cannot reach, and the isolated tests hold, is (a) the geometries no checkpoint has: K = 15 / 35 / 50 with
a tap across a 16-wide K step, N = 2 .. 130 off the 64-wide tile, the odd N guard of E_SWIGLU, bmod 3 and 6, ldc > N, windows shorter
than the reach at dilation 3 and 9, a tile holding three windows, `live` of TailRows on a tile edge and one row either side, clips of
one output row at strides 1 / 2 / 8, C off 256 in the row kernels, exact quantiser ties by position; and (b) the bytes a launch does not
own: rows and columns past the launch, dead tiles, neighbours overwritten by +-1e30 / NaN."""
MEASURED_CPU = """ulp distance of torch's f32 functions from float64 over the arguments the twins of every op form on their cases (the tile, OUT,
CENC_IN, VAE_DW, VAE_UNIT, both attention kernels): sin 0.599 (236 100 arguments, |a x| <= 6.97), exp 0.548 (41 296), erf 0.547 (8 580):
codec_cases.ULP_CPU = 0.60 / 0.55 / 0.55, the device is granted 4 x that.
f32 twins as fractions of the bound: tile WindowRows plain E_LIN 0.206, E_GELU 0.185, E_RES 0.123, E_LSRES 0.346, E_SWIGLU 0.086, E_RESMAP
0.156, snake E_LIN 0.099, snake E_RES 0.115; TailRows 0.094 / 0.067 / 0.127; ClipRows 0.140, E_GELU 0.204, E_LSRES 0.543, E_SWIGLU 0.100,
snake 0.102 / 0.115; VaeStrideRows 0.164; rms 0.131; dwln 0.804; out 0.120; cenc_in 0.245; gather 0.186; vq 0.000 (the nearest row every
time).  The bounds grant every rounding its worst case; roundings that do not conspire stay below, the row kernels least so.
Weakest mutation as a multiple of the bound: tile drop_first 9.2e4, dil 1.5e5, leak 1.4e5, clip 1.7e5, swiglu 2.3e5, ktail / bias / stride
NaN or 1e30 (counted as seen); dwln stats 5.9e4, drop_first 1.6e5, leak 4.0e5; out / cenc_in drop_first 3.1e4, leak 6.0e4, clip 1.2e6;
gather 1.2e6; vq: the higher index on a tie, a one-ulp residual and a shifted code each break an exact check.
Attention twins 0.008 / 0.009 (causal, heads 1 / 3) and 0.008 / 0.011 (encoder) of the bound, which grants each of the 64 fmaf steps of a
score its worst case through exp(2 ds); weakest mutated row: own key dropped 142 x, key i + 1 admitted 388 x, the next clip's first key
349 x, a missing rescale 235 x.  vae_dw twin 0.294; drop_first 2.5e5, dil 2.1e6, leak 2.8e6.  vae_unit twin 0.081; drop_first 1.8e4,
a wrong column group 5.3e4, dil 4.6e4, leak 4.4e4."""


def _worst(d, name, v):
    d[name] = max(d.get(name, 0.0), v)


# ---- the references against each other -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.TILE_CASES, ids=lambda c: c["name"])
def test_window_reference_equals_the_walk_over_the_locator_arrays(c):
    want, bound = K.tile_ref(c)
    got = K.tile_eval(c)
    assert want.shape == got.shape == (K.layout(c)["M"], K.tile_inputs(c)["ncols"])
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (bound > 0).all() and np.isfinite(bound).all()


@pytest.mark.parametrize("c", [c for c in K.TILE_CASES if not c["snake"]], ids=lambda c: c["name"])
def test_window_reference_equals_the_textbook_conv(c):
    """torch's conv1d (stride, dilation, left pad) clip by clip, and the transposed conv from the unpacked [C_in][C_out][2 s] weight"""
    inp = K.tile_inputs(c)
    first, last = K.spans(c, inp["L"])
    X, W = inp["A"].astype(np.float64), inp["W"].astype(np.float64)
    walk = np.zeros((inp["L"]["M"], c["N"]))
    for j in range(c["taps"]):
        src = last - (c["taps"] - 1 - j) * c["dil"]
        walk += np.where((src >= first)[:, None], X[np.maximum(src, 0)], 0.0) @ W[:, :, j].T
    assert np.abs(K.conv_ref(c) - walk).max() <= 1e-12
    if c["tconv"]:
        assert np.abs(K.tconv_ref(c) - walk).max() <= 1e-12


def test_every_instantiation_is_launched():
    """CODEC_TILE_COMBOS of csrc/codec_launch.h is what codec_tile_launch instantiates; every entry has a case, off the tile in M and N"""
    combos = K.combos_of_the_dispatch()
    assert len(combos) == len(set(combos)) == 18
    for combo in combos:
        cs = [c for c in K.TILE_CASES if (c["kind"], c["snake"], c["epi"]) == combo]
        assert any(K.layout(c)["M"] % 64 and c["N"] % 64 for c in cs), combo
    assert {(c["kind"], c["snake"], c["epi"]) for c in K.TILE_CASES} == set(combos)


def test_the_product_launches_the_tile_only_through_the_dispatch():
    import glob
    import os
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "qwen3-asr-swift_amd", "csrc")
    users = [os.path.basename(p) for p in glob.glob(os.path.join(root, "*")) if "hipLaunchKernelGGL((codec_gemm_kernel<" in open(p).read()]
    assert sorted(users) == ["codec_launch.hip"], users


def test_the_issue_s_shapes_are_present():
    Ms = {K.layout(c)["M"] for c in K.TILE_CASES}
    assert {1, 63, 64, 65, 129} <= Ms
    assert {5, 16, 24} <= {c["Cin"] for c in K.TILE_CASES} and {1, 2, 3, 7} <= {c["taps"] for c in K.TILE_CASES}
    assert {35, 15} <= {c["K"] for c in K.TILE_CASES} and {1, 3, 9} <= {c["dil"] for c in K.TILE_CASES}
    assert {2, 6, 62, 64, 66, 130} <= {c["N"] for c in K.TILE_CASES}
    assert {3, 6} <= {c["bmod"] for c in K.TILE_CASES if c["bmod"] < c["N"]}
    assert {1, 2, 8} <= {c["rate"] for c in K.TILE_CASES if c["kind"] == K.WINDOW}
    assert {1, 2, 8} <= {c["stride"] for c in K.TILE_CASES if c["kind"] == K.CLIP}
    assert {2, 5} <= {c["stride"] for c in K.TILE_CASES if c["kind"] == K.VSTRIDE}
    assert any(c["segs"] == K.W5 for c in K.TILE_CASES) and any(c["ldc_extra"] for c in K.TILE_CASES)


def test_tail_cases_have_the_edges():
    """live of window 0 at 64, 63 and 65; nothing dead; a clamped lead; live rows in every case, skipped tiles in all but tail_edge_m1"""
    lives = {}
    for c in K.TILE_CASES:
        if c["kind"] != K.TAIL:
            continue
        L = K.layout(c)
        live = K.live_rows(c, L)
        m = np.arange(L["M"])
        dead = m < live
        tiles = [dead[t:t + 64].all() for t in range(0, L["M"], 64)]
        assert not all(tiles) and any(tiles) == (c["name"] != "tail_edge_m1"), c["name"]     # live = 63: tile 0 holds one live row
        assert not tiles[-1], "a window's last row is live"
        lives[c["name"]] = int(live[0])
        if c["segs"] == K.TAIL_SEGS:
            assert live[200] == 200 and live[230] == 230, "window 1: nothing dead; window 2: the lead clamps to the window start"
    assert (lives["tail_edge"], lives["tail_edge_m1"], lives["tail_edge_p1"], lives["tail_rate2"]) == (64, 63, 65, 64)
    c = K.TILE_BY_NAME["tail_lead1"]
    live = K.live_rows(c, K.layout(c))
    assert live[299] == 297 and live[255] == 297 and live[199] == 129      # tile 192..255 straddles; of 256..299 only 297..299 are live


# ---- the transcendental functions of the CPU --------------------------------------------------------------------------------------------
def _ulps(f32_fn, f64_fn, args):
    import torch
    a = np.unique(np.concatenate(args))
    a = a[np.isfinite(a)]
    got = f32_fn(torch.from_numpy(a)).numpy().astype(np.float64)
    want = f64_fn(a.astype(np.float64))
    ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-300))) - 23), 2.0 ** -149)
    return float((np.abs(got - want) / ulp).max())


def test_transcendental_ulps_of_the_cpu():
    """the largest ulp distance of torch's f32 sin / exp / erf from float64 over the arguments the twins of every op that calls them form on
    their cases: the tile, OUT, VAE_DW, VAE_UNIT (sinf), E_SWIGLU and both attention kernels (expf), E_GELU (erff)"""
    import torch
    args = {}
    for c in K.TILE_CASES + K.OUT_CASES + K.CENC_IN_CASES:
        K.tile_twin(c, args)
    for c in K.VAE_DW_CASES:
        K.vdw_twin(c, args=args)
    for c in K.VAE_UNIT_CASES:
        K.unit_twin(c, args)
    for enc in (0, 1):
        for heads in K.ATTN_HEADS:
            K.attn_twin(K.attn_inputs(enc, heads), args)
    assert set(args) == {"sin", "exp", "erf"}
    got = dict(sin=_ulps(torch.sin, np.sin, args["sin"]), exp=_ulps(torch.exp, np.exp, args["exp"]),
               erf=_ulps(torch.erf, lambda a: torch.erf(torch.from_numpy(a)).numpy(), args["erf"]))
    print("ulp distance of torch f32 from float64: " + ", ".join(f"{k} {v:.3f} over {sum(len(a) for a in args[k])} arguments" for k, v in got.items()))
    print("largest |a x| of a snake: %.2f" % max(np.abs(a[np.isfinite(a)]).max() for a in args["sin"]))
    for k, v in got.items():
        assert v <= K.ULP_CPU[k], (k, v)
    assert max(np.abs(a[np.isfinite(a)]).max() for a in args["sin"]) < 8.0


# ---- the twins inside the bounds ------------------------------------------------------------------------------------------------------------
def test_tile_twins_stay_inside_the_bounds():
    worst = {}
    for c in K.TILE_CASES:
        want, bound = K.tile_ref(c)
        f = K.frac(K.tile_twin(c), want, bound)
        _worst(worst, "%s %s %s" % (("window", "tail", "clip", "vstride")[c["kind"]], "snake" if c["snake"] else "plain",
                                    ("lin", "gelu", "res", "lsres", "swiglu", "resmap")[c["epi"]]), f)
        assert f <= 1.0, (c["name"], f)
    print("tile twins, worst fraction of the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_row_twins_stay_inside_the_bounds():
    worst = {}
    for C in K.ROW_C:
        want, bound = K.rms_ref(C)
        _worst(worst, "rms", K.frac(K.rms_twin(C), want, bound))
    for c in K.DWLN_CASES:
        want, bound = K.dwln_ref(c)
        _worst(worst, "dwln", K.frac(K.dwln_twin(c), want, bound))
    print("row twins, worst fraction of the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- the mutation condition ---------------------------------------------------------------------------------------------------------------------
def _seen(mv, v, bound):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(mv - v) / bound
    d[~np.isfinite(d)] = np.inf
    return float(d.max())


def test_tile_mutations_move_an_output_by_ten_bounds():
    weakest = {}
    for c in K.TILE_CASES:
        want, bound = K.tile_ref(c)
        for mut in K.tile_mutations(c):
            s = _seen(K.tile_eval(c, mut), want, bound)
            weakest[mut] = min(weakest.get(mut, np.inf), s)
            assert s >= 10.0, (c["name"], mut, s)
    print("tile mutations, weakest as a multiple of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))
    assert set(weakest) == {"leak", "drop_first", "dil", "ktail", "swiglu", "bias", "clip", "stride"}


def test_tail_rows_a_skipped_live_tile_is_an_exact_failure():
    """where TailRows must compute, the WindowRows value differs from what was uploaded (the sentinel; in place, the residual)"""
    for c in K.TILE_CASES:
        if c["kind"] != K.TAIL:
            continue
        inp, L = K.tile_inputs(c), K.layout(c)
        want, _ = K.tile_ref(c)
        live = np.arange(L["M"]) >= K.live_rows(c, L)
        before = inp["R"].astype(np.float64) if c["in_place"] else np.full_like(want, float(K.SENTINEL))
        assert (np.abs(want - before)[live] > 0).all(axis=1).all(), c["name"]


def test_dwln_mutations_move_an_output_by_ten_bounds():
    weakest = {}
    for c in K.DWLN_CASES:
        want, bound = K.dwln_ref(c)
        for mut in ("leak", "drop_first", "stats"):
            s = _seen(K.dwln_ref(c, mut=mut)[0], want, bound)
            weakest[mut] = min(weakest.get(mut, np.inf), s)
            assert s >= 10.0, (c["name"], mut, s)
    print("dwln mutations, weakest as a multiple of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))


def test_row_cases_hold_the_window_start():
    """a row at a window start (six taps absent), one and six rows after it, under both locators"""
    for c in K.DWLN_CASES:
        L = K.layout(c)
        first, _ = K.spans(c, L)
        off = np.arange(L["M"]) - first
        assert {0, 1, 6} <= set(off.tolist()), c["name"]
    assert {c["C"] for c in K.DWLN_CASES} >= set(K.ROW_C) == {4, 255, 256, 257, 4096}


# ---- the output conv, the encoder's input conv, the code gather -----------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.OUT_CASES + K.CENC_IN_CASES, ids=lambda c: c["name"])
def test_out_and_cenc_in_references_and_twins(c):
    want, bound = K.tile_ref(c)
    assert np.abs(K.tile_eval(c) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    if not c["snake"]:
        first, last = K.spans(c, K.layout(c))
        assert np.abs(K.conv_ref(c) + K.tile_inputs(c)["bias"].astype(np.float64) - want).max() <= 1e-12
    f = K.frac(K.tile_twin(c), want, bound)
    print(f"{c['name']}: twin at {f:.3f} of the bound")
    assert f <= 1.0
    if "clip" in c:
        w, b, done = K.out_ref(c)
        assert K.frac(K.out_twin(c)[done], w[done], b[done]) <= 1.0
        assert done.any() and (c["kind"] == K.TAIL) == (not done.all())
        raw = np.abs(want[:, 0][done])
        assert (raw < 0.9).any() and (not c["clip"] or (raw > 1.1).any()), "clipped and unclipped samples"


def test_out_and_cenc_in_cases_and_mutations():
    assert {c["Cin"] for c in K.OUT_CASES} == {1, 3, 24} == {c["N"] for c in K.CENC_IN_CASES}
    firsts = set()
    for c in K.OUT_CASES:                              # the first computed sample of the last window: before, on and after a 256-thread block edge
        if c["kind"] == K.TAIL:
            firsts.add(int(np.flatnonzero(K.out_ref(c)[2])[-1] + 1 - K.out_ref(c)[2][::-1].argmin()))
    assert {255, 256, 257} <= firsts, firsts
    weakest = {}
    for c in K.OUT_CASES + K.CENC_IN_CASES:
        want, bound = K.tile_ref(c)
        muts = ["leak", "drop_first"] + (["clip"] if c["kind"] == K.CLIP else [])
        for mut in muts:
            got = K.tile_eval(c, mut)
            if "clip" in c and c["clip"]:              # through the clip, on the rows a TAIL launch computes
                done = K.out_ref(c)[2]
                s = _seen(np.clip(got[done], -1, 1), np.clip(want[done], -1, 1), bound[done])
            else:
                s = _seen(got, want, bound)
            weakest[mut] = min(weakest.get(mut, np.inf), s)
            assert s >= 10.0, (c["name"], mut, s)
    print("out / cenc_in mutations, weakest as a multiple of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))


def test_gather_twins_and_mutations():
    worst, weakest = 0.0, {}
    assert {(c["Q"], c["D"]) for c in K.GATHER_CASES} == {(q, d) for q in (1, 2, 16) for d in (24, 255, 257)}
    for c in K.GATHER_CASES:
        want, bound = K.gather_ref(c)
        codes = K.gather_inputs(c)["codes"]
        assert (codes[0] == 0).all() and codes[1, 0] == K.GATHER_S0 - 1 and (codes[1, 1:] == K.GATHER_S1 - 1).all()
        worst = max(worst, K.frac(K.gather_twin(c), want, bound))
        for mut in ("base", "code"):
            if c["Q"] == 1:
                continue                               # one codebook: nothing but the copy
            d = np.abs(K.gather_ref(c, mut)[0] - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = float(np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0)).max())
            weakest[mut] = min(weakest.get(mut, np.inf), s)
            assert s >= 10.0, (c["name"], mut, s)
    print(f"gather twin: {worst:.3f} of the bound; mutations, weakest: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))
    assert worst <= 1.0


def test_vq_twin_passes_and_the_higher_index_on_a_tie_fails():
    """the f32 twin passes the three checks of vq_check on every case; with `<=` for `<` it returns the higher index of a duplicated pair,
    which vq_check refuses; every stage of every case has rows whose nearest codebook row is duplicated"""
    assert {c["M"] for c in K.VQ_CASES} == {1, 64, 65} and {c["D"] for c in K.VQ_CASES} == {8, 24, 40} and {c["Q"] for c in K.VQ_CASES} == {1, 2, 5}
    assert {c["S0"] for c in K.VQ_CASES} | {c["S1"] for c in K.VQ_CASES} == {3, 64, 65, 130}
    assert K.vq_ties(130) == [(0, 129), (1, 9), (5, 69)] and K.vq_ties(3) == [(0, 2)]
    worst = 0.0
    for c in K.VQ_CASES:
        codes, r = K.vq_twin(c)
        worst = max(worst, K.vq_check(c, codes, r))
        aimed = K.vq_aimed(c)
        assert all(n >= 1 for n in aimed), (c["name"], aimed)
        hi_codes, hi_r = K.vq_twin(c, tie_high=True)
        assert (hi_codes != codes).any()
        with pytest.raises(AssertionError, match="the higher index of a tie"):
            K.vq_check(c, hi_codes, hi_r)
        bad = r.copy()
        bad[0, 0] = np.nextafter(bad[0, 0], np.float32(np.inf))
        with pytest.raises(AssertionError, match="residual"):
            K.vq_check(c, codes, bad)
        far = codes.copy()                             # a code that is not the nearest: outside the bound
        far[:, 0] = (far[:, 0] + 1) % c["S0"]
        if c["S0"] > 3:
            with pytest.raises(AssertionError):
                K.vq_check(c, far, r)
    print(f"vq twin: worst (d(code) - min d) / bound {worst:.3f}")


# ---- the two attention kernels, the AudioVAE's depthwise conv ------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", K.ATTN_HEADS)
@pytest.mark.parametrize("enc", [0, 1], ids=["dec", "enc"])
def test_attention_twins_and_mutations(enc, heads):
    inp = K.attn_inputs(enc, heads)
    want, bound = K.attn_ref(inp)
    assert (bound > 0).all()
    f = K.frac(K.attn_twin(inp), want, bound)
    seen = {}
    for mut in (("next_key", "no_rescale") if enc else ("mask_more", "mask_less")):
        got = K.attn_ref(inp, mut=mut)[0]
        rows = np.ones(inp["M"], bool)
        for s0, n in zip(inp["starts"], inp["segs"]):
            if mut == "mask_less":
                rows[s0] = False                        # exempt: the first row of a window has no key left (NaN on the device: refused as such)
            if mut == "mask_more":
                rows[s0 + n - 1] = s0 + n < inp["M"]    # exempt: the last row of the last window (the key lies outside every array)
            if mut == "next_key":
                rows[s0:s0 + n] = s0 + n < inp["M"]     # exempt: the last clip
            if mut == "no_rescale":
                rows[s0:s0 + n] = n > 32                # exempt: clips of one key tile
        with np.errstate(invalid="ignore"):
            d = np.abs(got - want) / bound
        d[np.isnan(d)] = np.inf
        per_row = d.max(1)
        if mut == "no_rescale":                        # shows on the rows whose maximum moves at a tile edge: an output of every such clip
            for s0, n in zip(inp["starts"], inp["segs"]):
                if n > 32:
                    assert (per_row[s0:s0 + n] >= 10.0).any(), n
            rows &= per_row >= 10.0
        seen[mut] = float(per_row[rows].min())
        assert seen[mut] >= 10.0, (mut, seen[mut])
    print(f"attention {'enc' if enc else 'dec'} heads {heads}: twin at {f:.3f} of the bound; weakest row per mutation "
          + ", ".join(f"{k} {v:.3g}" for k, v in seen.items()))
    assert f <= 1.0


def test_attention_cases():
    assert K.ATTN_DEC_WINDOWS[:3] == (1, 2, K.CODEC_MAX_T) and K.ATTN_ENC_CLIPS == (1, 31, 32, 33, 65) and K.ATTN_HEADS == (1, 3)
    inp = K.attn_inputs(1, 1)
    assert [tuple(t) for t in inp["loc"][-3:]] == [(97, 65, 0, 0), (97, 65, 32, 0), (97, 65, 64, 0)]


def test_vae_dw_twins_and_mutations():
    assert {c["C"] for c in K.VAE_DW_CASES} == {5, 64, 70} and {c["dil"] for c in K.VAE_DW_CASES} == {1, 3, 9}
    assert {K.layout(c)["M"] for c in K.VAE_DW_CASES} == {1, 64, 65, 130} and {c["snake"] for c in K.VAE_DW_CASES} == {True, False}
    worst, weakest = 0.0, {}
    for c in K.VAE_DW_CASES:
        want, bound = K.vdw_ref(c)
        worst = max(worst, K.frac(K.vdw_twin(c), want, bound))
        L = K.layout(c)
        muts = ["drop_first"] + (["dil", "leak"] if len(L["segs"]) > 1 else [])     # exempt: one window of one row has no earlier tap and no neighbour
        for mut in muts:
            s = _seen(K.vdw_ref(c, mut=mut)[0], want, bound)
            weakest[mut] = min(weakest.get(mut, np.inf), s)
            assert s >= 10.0, (c["name"], mut, s)
    print(f"vae_dw twin: {worst:.3f} of the bound; mutations, weakest: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))
    assert worst <= 1.0


def test_n_tail_lands_on_a_sentinel():
    assert K.EXTRA >= 1
    off = [c for c in K.TILE_CASES if c["N"] % 64]
    assert {c["N"] for c in off} >= {2, 6, 62, 66, 130} and any(c["ldc_extra"] for c in off)
    for c in off:                                      # the output image is [M + EXTRA][ldc]: (M - 1, N) is a sentinel column or row M's column 0
        inp = K.tile_inputs(c)
        assert inp["ldc"] >= inp["ncols"] and (inp["ldc"] > inp["ncols"]) == (c["ldc_extra"] > 0)


def test_vae_unit_twins_and_mutations():
    assert {c["C"] for c in K.VAE_UNIT_CASES} == {4, 12, 24, 40, 100, 128} and {c["dil"] for c in K.VAE_UNIT_CASES} == {1, 3, 9}
    assert {K.layout(c)["M"] for c in K.VAE_UNIT_CASES} == {1, 64, 65, 130} and {c["map"] for c in K.VAE_UNIT_CASES} == {"none", "snake", "affine"}
    assert {K.unit_rpt(c["C"]) for c in K.VAE_UNIT_CASES} == {1, 2, 4, 8}
    assert all(256 % (C // 4) for C in (12, 24, 40, 100))                      # C / 4 does not divide 256
    assert any(s == K.W5[:2] + K.W5[2:4] + (56,) or len(c["segs"]) == 5 for c in K.VAE_UNIT_CASES for s in [c["segs"]])
    worst, weakest = 0.0, {}
    for c in K.VAE_UNIT_CASES:
        want, bound = K.unit_ref(c)
        worst = max(worst, K.frac(K.unit_twin(c), want, bound))
        L = K.layout(c)
        for mut in ["drop_first", "groups"] + (["dil", "leak"] if len(L["segs"]) > 1 else []):
            s = _seen(K.unit_ref(c, mut=mut)[0], want, bound)
            weakest[mut] = min(weakest.get(mut, np.inf), s)
            assert s >= 10.0, (c["name"], mut, s)
    print(f"vae_unit twin: {worst:.3f} of the bound; mutations, weakest: " + ", ".join(f"{k} {v:.3g}" for k, v in weakest.items()))
    assert worst <= 1.0


# ---- step 0: what the network tests see -----------------------------------------------------------------------------------------------------
import contextlib  # noqa: E402


@contextlib.contextmanager
def _patched(obj, name, fn):
    old = getattr(obj, name)
    setattr(obj, name, fn)
    try:
        yield
    finally:
        setattr(obj, name, old)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def _codec_defects(O):
    """defective primitives of tests/codec_oracle.py: name -> (attribute, replacement)"""
    conv, tconv, unit = O.causal_conv, O.causal_transpose_conv, O.residual_unit

    def leak(x, w, b=None, dilation=1):
        """the first (k - 1) dilation rows read what lies before the window: here real rows (the window's own, wrapped) instead of zeros"""
        pad = (w.shape[2] - 1) * dilation
        if pad == 0:
            return conv(x, w, b, dilation)
        ghost = x[np.arange(-pad, 0) % x.shape[0]]
        return conv(np.concatenate([ghost, x]), w, b, dilation)[pad:]

    def drop_first(x, w, b=None, dilation=1):
        """the tap that lands on the window's first row is dropped"""
        x0 = x.copy()
        x0[0] = 0
        return conv(x0, w, b, dilation)

    def dil(x, W, p, dilation):
        return unit(x, W, p, dilation + 1 if p.endswith(".2.block.3") or p.endswith(".2.block.1") else dilation)

    def bias(x, w, b, stride):
        """bias[n] for bias[n % bmod]: only the first of a row's `stride` phases gets its bias"""
        y = tconv(x, w, b, stride) - b
        y[0::stride] += b
        return y
    return {"a tap admitted before the window start": ("causal_conv", leak), "the first tap after it dropped": ("causal_conv", drop_first),
            "dilation 3 -> 4 in one unit": ("residual_unit", dil), "bias[n] for bias[n % bmod]": ("causal_transpose_conv", bias)}


def test_step0_what_the_network_tests_see():
    """the float64 oracles against themselves with one edge defect each, as max |d| / peak beside the bound of the network's GPU test"""
    import codec_oracle as O
    import codec_enc_oracle as E
    import avae_oracle as V
    import avae_cases as VK
    from qasr import synth
    seen = {}
    # decoder, reduced geometry, T = 11, pre-clip forward (bound: test_gpu_codec.py TOL["forward"])
    W = O.Weights(synth.synth_speech_tokenizer_state_dict(0, O.REDUCED))
    codes = O.make_codes(11, 11, O.REDUCED)
    ref = O.forward(codes, W, O.REDUCED, clip=False)
    for name, (attr, fn) in _codec_defects(O).items():
        with _patched(O, attr, fn):
            seen["decoder", name] = (_rel(O.forward(codes, W, O.REDUCED, clip=False), ref), 6.33e-05)
    # encoder convs, reduced geometry, two frames and three samples (bound: test_gpu_codec_enc.py TOL["conv"]); no transposed conv there
    We = O.Weights(synth.synth_speech_tokenizer_encoder_state_dict(0, O.REDUCED))
    pcm = E.make_pcm(7, 1920 * 2 + 3)
    ref = E.conv(pcm, We, O.REDUCED)
    for name, (attr, fn) in _codec_defects(O).items():
        if attr == "causal_transpose_conv":
            continue
        unit = E.residual_unit
        repl = fn if attr == "causal_conv" else (lambda x, W_, p, d: unit(x, W_, p, d + 1 if p.endswith(".2.block.1") else d))
        with _patched(E, attr, repl):
            seen["encoder", name] = (_rel(E.conv(pcm, We, O.REDUCED), ref), 1.23e-05)
    # AudioVAE, tiny geometry, decode of 9 frames (bound: test_gpu_avae.py TOL["tiny/dec/pcm"])
    Wv = V.Weights(VK.stored("tiny"), VK.GEOMS["tiny"])
    z = VK.clip_z(9, VK.GEOMS["tiny"]["latent_dim"])
    ref = V.decode(z, Wv)[1]
    conv, conv_t, vunit = V.NP.conv, V.NP.conv_t, V.unit

    def v_leak(self, x, key, left, stride=1, dil=1):
        if left == 0:
            return conv(self, x, key, left, stride, dil)
        ghost = x[np.arange(-left, 0) % x.shape[0]]
        return conv(self, np.concatenate([ghost, x]), key, 0, stride, dil)

    def v_drop(self, x, key, left, stride=1, dil=1):
        x0 = np.array(x, copy=True)
        x0[0] = 0
        return conv(self, x0, key, left, stride, dil)

    def v_bias(self, x, key, s):
        b = self.w[key + ".bias"]
        y = conv_t(self, x, key, s) - b
        y[0::s] += b
        return y

    def v_dil(be, x, p, d):
        if not p.endswith("layers.1.res2"):
            return vunit(be, x, p, d)
        h = be.conv(be.snake(x, p + ".snake1"), p + ".conv1", 6 * (d + 1), dil=d + 1)
        return x + be.conv(be.snake(h, p + ".snake2"), p + ".conv2", 0)
    for name, (obj, attr, fn) in {"a tap admitted before the window start": (V.NP, "conv", v_leak),
                                  "the first tap after it dropped": (V.NP, "conv", v_drop),
                                  "dilation 3 -> 4 in one unit": (V, "unit", v_dil),
                                  "bias[n] for bias[n % bmod]": (V.NP, "conv_t", v_bias)}.items():
        with _patched(obj, attr, fn):
            seen["audiovae", name] = (_rel(V.decode(z, Wv)[1], ref), 5.9e-06)
    for (net, name), (d, bound) in seen.items():
        print(f"step 0 {net}: {name}: {d:.1e} of the peak | bound {bound:.1e} | {d / bound:.0f} x")
    assert all(d > 10 * bound for d, bound in seen.values()), seen      # every network test SEES every one of these defects

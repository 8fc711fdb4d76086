"""The references and bounds of tests/enc_cases.py, without a GPU, on the inputs tests/test_gpu_enc_cases.py runs: an honest f32 twin of
every kernel stays inside its bound, and every wrong kernel of the list below moves at least one output by >= 10 x the bound, so the GPU
tests cannot pass while blind to it.

  attention  the clip's last key dropped; the row after the clip admitted (the next packed clip's first key, NaN rows after the last clip);
             a whole last partial tile dropped (64 keys; window: 16); the first key of the second tile dropped; the ragged last query
             group (32 rows for the 32x32x16 form, else 16) computed with one key fewer
  norms      division by the padded width (the next multiple of 256 above D); statistics taken from the neighbouring row (the clamped
             duplicate of layernorm_f32p_rows_kernel); a one-pass variance on the mean-100 rows of the f32-output form
  conv0      tap 0 shifted by one sample; the LayerNorm sums divided by the padded thread count (C = 40 -> 64); the last frame of a clip
             not written.  (conv0 has no padding column: its padded lanes hold zero weights and a zero bias by construction.)
  conv1      tap kw = 2 shifted by one sample; the columns from clen upward read as data; the width mask off by one either way

Measured here: MEASURED_CPU below (pytest -s prints every figure).
"""
import math
import numpy as np
import pytest
import torch
import enc_cases as E
from gemm_cases import bf16_round, bf16_bits, bf16_from_bits

MEASURED_CPU = """f32 twins as fractions of the bound: mha_attention_kernel <= 0.740 (head_dim 64), 0.623 (head_dim 32); mha64_attention_kernel
<= 0.908; window_attention_kernel <= 0.706; layernorm bf16 forms 0.969 (= the half ulp of the output rounding), f32 form <= 0.170; conv0 0.968;
conv1 0.969; wave stats <= 0.233.  Weakest mutation: attention 97 x the bound over all cases (tile2_first, head_dim 32, 513 keys); norms: padded
width 328 x, neighbour statistics 771 x, one-pass variance on the mean-100 rows 20.5 x (D = 4) .. 62 x; conv0: tap 31327 x, padded width 10256 x;
conv1: tap 659893 x, width mask one short 495 x, padding column and width mask one long: NaN / non-zero in a +0 column."""

ATTN_CASES = ([("mha", 64, 0, E.HEADS, b) for b in E.MHA_BATCHES] + [("mha", 64, 1, E.HEADS, b) for b in E.MHA_BATCHES] +
              [("mha", 32, 0, E.HEADS, b) for b in E.MHA_BATCHES] +
              [("mha", 64, f, *p) for f in (0, 1) for p in (E.PAIRS8, E.PAIRS9)] + [("mha", 64, 1, E.HEADS, E.ENCODER_WINDOWS)] +
              [("window", hd, 0, E.HEADS, b) for hd in (32, 64) for b in E.WINDOW_BATCHES])


def _frac(got, v, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - v) / bound
    r = np.where((bound == 0) & (got == v), 0.0, r)
    return float(np.where(np.isnan(r), np.inf, r).max())


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("hd,L", [(32, 1), (64, 65), (64, 130)])
def test_attn_ref_against_sdpa(kind, hd, L):
    """the three references are softmax attention up to the rounding of P (2^-8 of every weight, numerator and denominator)"""
    rng = np.random.default_rng(L)
    q, k, v = (E.randn_bf16(rng, (L, hd)) for _ in range(3))
    got, bound = E.attn_ref(q, k, v, kind)
    tq, tk, tv = (torch.tensor(a, dtype=torch.float64)[None] for a in (q, k, v))
    want = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv)[0].numpy()
    w = torch.softmax(torch.tensor(q @ k.T / math.sqrt(hd)), -1).numpy()
    assert (np.abs(got - want) <= 2.0 ** -7 * (w @ np.abs(v)) + 1e-12).all()
    assert (bound > 0).all()


@pytest.mark.parametrize("family,hd,form,heads,clips", ATTN_CASES)
def test_attention_twin_and_mutations(family, hd, form, heads, clips):
    kind = "window" if family == "window" else E.mha_kind(hd, form)
    tile = 16 if family == "window" else 64
    group = E.query_group(kind)
    worst, moved = 0.0, {m: 0.0 for m in E.MUTATIONS}
    for set_kind, spike in E.attn_sets(clips, tile):
        qkv, _, cu = E.attn_inputs(clips, heads, hd, set_kind, spike, tile)
        v, bound = E.attn_expect_cached(clips, heads, hd, set_kind, spike, tile, kind)
        twin = np.empty_like(v)
        for c in range(len(clips)):
            r = slice(cu[c], cu[c + 1])
            for h in range(heads):
                twin[r, h] = E.TWINS[kind](qkv[r, 0, h], qkv[r, 1, h], qkv[r, 2, h])
        worst = max(worst, _frac(twin, v, bound))
        if set_kind == "readout":
            continue
        for m in E.MUTATIONS:                            # head 0 is enough to show the defect
            bad, _ = E.attn_expect(qkv[:, :, :1], cu, kind, mutation=m, tile=tile, group=group)
            moved[m] = max(moved[m], _frac(bad, v[:, :1], bound[:, :1]))
    applies = {"last_key": max(clips) > 1, "admit_next": True, "last_tile": any(L > tile and L % tile for L in clips),
               "tile2_first": max(clips) > tile, "ragged_group": any(L % group and L > 1 for L in clips)}
    low = min(moved[m] for m in E.MUTATIONS if applies[m])
    print(f"{family} hd {hd} form {form} heads {heads} clips {clips}: twin {worst:.3f} of the bound, smallest mutation {low:.1f} x "
          + ", ".join(f"{m} {moved[m]:.0f}" for m in E.MUTATIONS if applies[m]))
    assert worst <= 1.0, worst
    for m in E.MUTATIONS:
        if applies[m]:
            assert moved[m] >= 10.0, (m, moved[m])


@pytest.mark.parametrize("D", E.LN_WIDTHS)
def test_layernorm_twin_and_mutations(D):
    worst = {f: 0.0 for f in E.LN_FORMS.values()}
    moved = {"padded_width": math.inf, "neighbour_stats": math.inf}
    one_pass = 0.0
    Dp = (D // 256 + 1) * 256
    for rows in E.ln_row_counts(D):
        for kind in ("mixed", "mean100"):
            x, g, b = E.ln_inputs(D, rows, kind)
            x = x[:rows]
            for form in E.LN_FORMS.values():
                v, bound = E.ln_ref(x, g, b, form)
                worst[form] = max(worst[form], _frac(E.ln_twin(x, g, b, form), v, bound))
                if kind == "mixed":
                    moved["padded_width"] = min(moved["padded_width"], _frac(E.ln_ref(x, g, b, form, div=Dp)[0], v, bound))
                    if rows > 1:
                        moved["neighbour_stats"] = min(moved["neighbour_stats"], _frac(E.ln_ref(x, g, b, form, shift_stats=True)[0], v, bound))
                elif form == 2:
                    one_pass = max(one_pass, _frac(E.ln_twin(x, g, b, form, one_pass=True), v, bound))
    print(f"layernorm D {D}: twin " + ", ".join(f"form {f} {w:.3f}" for f, w in worst.items()) +
          f"; padded width {moved['padded_width']:.0f} x, neighbour statistics {moved['neighbour_stats']:.0f} x, one-pass variance {one_pass:.1f} x")
    assert max(worst.values()) <= 1.0, worst
    assert moved["padded_width"] >= 10.0 and moved["neighbour_stats"] >= 10.0, moved


def test_layernorm_one_pass_variance_misses_the_bound():
    """mean 100, unit deviation, f32 output: E[x^2] - mean^2 in f32 loses 1e4 x 2^-24 of a variance of 1 per rounding"""
    worst = {}
    for D in E.LN_WIDTHS:
        for rows in E.ln_row_counts(D):
            x, g, b = E.ln_inputs(D, rows, "mean100")
            v, bound = E.ln_ref(x[:rows], g, b, 2)
            worst[D] = max(worst.get(D, 0.0), _frac(E.ln_twin(x[:rows], g, b, 2, one_pass=True), v, bound))
            assert _frac(E.ln_twin(x[:rows], g, b, 2), v, bound) <= 1.0
    print("one-pass variance, multiples of the bound per width: " + ", ".join(f"{D}: {w:.1f}" for D, w in worst.items()))
    assert all(w >= 10.0 for D, w in worst.items() if D >= 64), worst


@pytest.mark.parametrize("C,frames", E.CONV0_CASES)
def test_conv0_twin_and_mutations(C, frames):
    inp = E.conv0_inputs(C, frames)
    v, bound, written = E.conv0_ref(inp)
    twin = E.conv0_twin(inp)
    worst = _frac(twin[written], v[written], bound[written])
    moved = {"tap": _frac(E.conv0_ref(inp, tap_shift=True)[0][written], v[written], bound[written])}
    if C % 64:
        moved["padded_width"] = _frac(E.conv0_ref(inp, div=-(-C // 64) * 64)[0][written], v[written], bound[written])
    last = inp["frame_off"][1] + frames[1] - 1
    unwritten = v.copy()
    unwritten[last] = float(bf16_from_bits(np.array([E.SENTINEL], np.uint16))[0])
    moved["last_frame"] = _frac(unwritten[written], v[written], bound[written])
    print(f"conv0 C {C} frames {frames}: twin {worst:.3f} of the bound; " + ", ".join(f"{k} {m:.0f} x" for k, m in moved.items()))
    assert worst <= 1.0, worst
    assert min(moved.values()) >= 10.0, moved


@pytest.mark.parametrize("C,n_mels", E.CONV1_CASES)
def test_conv1_twin_and_mutations(C, n_mels):
    inp = E.conv1_inputs(C, n_mels)
    v, bound = E.conv1_ref(inp)
    assert np.isfinite(v).all()
    worst = _frac(E.conv1_twin(inp), v, bound)
    moved = {"tap": _frac(E.conv1_ref(inp, tap_shift=True)[0], v, bound), "padding": _frac(E.conv1_ref(inp, pad_as_data=True)[0], v, bound),
             "mask+1": _frac(E.conv1_ref(inp, mask_shift=1)[0], v, bound), "mask-1": _frac(E.conv1_ref(inp, mask_shift=-1)[0], v, bound)}
    print(f"conv1 C {C} n_mels {n_mels}: twin {worst:.3f} of the bound; " + ", ".join(f"{k} {m:.0f} x" for k, m in moved.items()))
    assert worst <= 1.0, worst
    assert min(moved.values()) >= 10.0, moved


def test_wave_stats_twin_and_conditioning():
    pcm, off, ns = E.wave_inputs()
    v, bound = E.wave_ref(pcm, off, ns)
    twin = E.wave_twin(pcm, off, ns)
    with np.errstate(invalid="ignore"):
        frac = np.where((bound == 0) & (twin == v), 0.0, np.abs(twin - v) / bound)        # n = 0: the mean is exactly 0
    print("wave stats: twin fractions of the bound (mean, inv_std) per clip " + ", ".join(f"n {n}: {a:.3f} {b:.3f}" for n, (a, b) in zip(ns, frac)))
    assert (frac <= 1.0).all(), frac
    rel = bound[:, 1] / v[:, 1]
    print(f"wave stats: relative inv_std bound {rel[-2]:.2e} at n 40001 without offset, {rel[-1]:.2e} with the DC offset")
    assert rel[-1] > 100 * rel[5]                          # the DC clip (n 4000) against n 1024 without offset: the conditioning shows


def test_exact_references():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1000).astype(np.float32)
    assert np.array_equal(E.cast_ref_bits(x), bf16_bits(bf16_round(x.astype(np.float64))))
    assert np.array_equal(E.cast_ref_bits(np.array([1.00390625, 1.01171875, np.inf, -0.0, 3.4e38], np.float32)),
                          np.array([0x3F80, 0x3F82, 0x7F80, 0x8000, 0x7F80], np.uint16))    # two ties to even, inf, -0, overflow
    y = rng.standard_normal((7, 50)).astype(np.float32)
    ids, err = E.argmax_ref(y)
    assert np.array_equal(ids, y.argmax(1)) and err == 0
    y[3] = np.nan
    y[4, 9] = np.inf
    ids, err = E.argmax_ref(y)
    assert ids[3] == 0 and ids[4] == 9 and err == 1
    assert np.array_equal(E.conv_rows_ref([0, 10], [0, 4], [3, 2], 6, 2, 8), [0, 16, 32, 0, 80, 96])
    assert np.array_equal(E.frame_info_ref([0, 3, 5], [3, 2, 0], 5), [[0, 3], [1, 3], [2, 3], [0, 2], [1, 2]])

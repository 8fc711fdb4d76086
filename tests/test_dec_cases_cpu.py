"""The references and bounds of tests/dec_cases.py, checked without a GPU on every case tests/test_gpu_dec_cases.py runs:
  * honest f32 twins (numpy f32 with the K axis reversed, the factored quantised sum in f32) stay inside the bounds;
  * no activation row behind a norm holds an element whose first rounding depends on the device's inv (the issue's condition: 90 % of the rows);
  * every wrong kernel of the list below moves some output by >= 10 x its bound, or breaks an exact check (a NaN, an unwritten row, a partial
    that is not the first maximum).

Worst fractions of the bound of the twins (pytest -s prints them): bf16 linear BF16 / LOGITS 0.968, RESID 0.969, SWIGLU coherent 2 bf16 ulps
(quantised: 2 at 4 bit, 3 at 8 bit; bar 3), Gaussian SWIGLU share of outputs not bit-equal to float64 0.024 % (quantised: 0.034 %); quantised linear 0.967 (4 bit behind a norm at K = 2048: 0.86, the f32
error of the factored sum is a visible part of the bound there); LM heads, every case of HEAD_CASES / HEADQ_CASES: bf16 0.966 /
0.962 (K 1024 / 2048), 0.964 / 0.967 generic; quantised K 1024 0.929 / 0.930 (4 bit, bf16 / f32 scales), 0.955 (8 bit), K 2048 0.913 / 0.950, generic
0.942 / 0.943.  With the magnitude of the dequantised
weights in place of the factored one the f32 error would be understated 12 x at 4 bit (test_plain_magnitude_understates).
Smallest ratio (defect's displacement / bound) per wrong kernel, bf16 linear: dropped k-step 67, doubled 48, dropped second phase 9035, rows of a
later group read from group 0 13, residual of row 0 5212, up tile of the next block 165, the neighbour's inv 81, inv over half of K 56, the norm
weight of the neighbouring chunk 18; row B admitted, row B - 1 dropped, a later group written at group 0: an exact check breaks.  The
residual's missing inner rounding is a defect of at most one bf16 ulp of the accumulator, below any accumulation bound: it is held against the
EXACT readout, where it breaks bit-equality.  Quantised linear, per kernel family: the neighbour's scale 4295, the neighbour's bias 3943, no bias
140687, swapped nibbles / bytes 2407, the 4-bit offset omitted 93825, a dropped / doubled last k-block 305 / 304, the dropped second phase of
K = 6144 1432, rows of a later group read from group 0 2401; row B admitted, row B - 1 dropped, a later group written at group 0: an exact check.  LM heads and the greedy tail: every defect breaks an exact check.
"""
import numpy as np
import pytest
import dec_cases as D
import gemm_cases as G
from gemm_cases import bf16_round, bf16_from_bits

SENT = D.SENTINEL_VALUE


def _gemv_all():
    for c in D.gemv_cases():
        for kind in D.gemv_kinds(c[0], c[3]):
            yield c, kind


def _gemvq_all():
    for c in D.gemvq_cases():
        for kind in D.gemvq_kinds(c[0]):
            yield c, kind


def test_no_row_behind_a_norm_is_ambiguous():
    seen = set()
    for (epi, K, N, norm, generic), kind in _gemv_all():
        if norm:
            seen.add((K, kind))
    for c, kind in _gemvq_all():
        if c[3]:
            seen.add((c[1], kind))
    seen |= {(1024, "gauss"), (2048, "gauss")}             # the LM heads
    for K, kind in sorted(seen):
        amb = D.rms_stage(D.x_rows(K, kind, 1), D.norm_weight(K))[1]
        clean = float((~amb.any(1)).mean())
        assert clean >= 0.9, (K, kind, clean)
        assert clean == 1.0, (K, kind, clean)               # norm_rows draws until every row is clean
    plain = D.rms_stage(D.x_rows(1024, "gauss", 0), D.norm_weight(1024))[1]
    print(f"rows behind a norm: none ambiguous; plain Gaussian rows of 1024: {(~plain.any(1)).mean() * 100:.0f} % clean, "
          f"{plain.mean() * 100:.3f} % of the elements ambiguous")
    assert plain.any(), "the ambiguity test never fires on plain rows: INV_REL is not applied"


def test_rmsnorm_candidates_bracket_an_f32_norm():
    """rmsnorm_rows in numpy f32 lands on one of the two candidates at every element of plain Gaussian rows"""
    for K in (96, 1024, 1056, 2048):
        x, w = D.x_rows(K, "gauss", 0), D.norm_weight(K)
        x32 = x.astype(np.float32)
        inv = (np.float32(1.0) / np.sqrt((x32 * x32).sum(1, keepdims=True, dtype=np.float32) / np.float32(K) + np.float32(D.EPS))).astype(np.float32)
        got = bf16_round(w * bf16_round((x32 * inv).astype(np.float64)))
        lo, hi = D.rms_stage(x, w)[2]
        assert ((got == lo) | (got == hi)).all(), K


def test_bf16_linear_twins_stay_inside_the_bounds():
    worst, diff, total = {}, 0, 0
    for c, kind in _gemv_all():
        epi, K, N, norm, generic = c
        d, e = D.gemv_inputs(epi, K, N, norm, kind), D.gemv_expect(epi, K, N, norm, kind)
        tw = D.gemv_twin(epi, d)
        if epi == D.SWIGLU and kind == "gauss":
            diff, total = diff + int((tw != e["ref"]).sum()), total + tw.size
            continue
        f = D.gemv_frac(epi, e, tw, D.ROWS)
        key = D.EPI_NAMES[epi] + (" coherent (ulps)" if epi == D.SWIGLU else "")
        worst[key] = max(worst.get(key, 0.0), f)
        assert f <= (3 if epi == D.SWIGLU else 1.0), (c, kind, f)
    print("bf16 linear f32 twins, worst fraction of the bound:", {k: round(v, 3) for k, v in worst.items()},
          f"; Gaussian SWIGLU: {diff} of {total} outputs not bit-equal to float64 ({diff / total * 100:.3f} %)")
    assert 0 < diff < 0.01 * total


def test_quantised_linear_twins_stay_inside_the_bounds():
    worst, diff, total = {}, 0, 0
    for c, kind in _gemvq_all():
        epi, K, N, norm, generic, bits, sbf = c
        tuned = bool(D.gemvq_route(epi, K, N, norm, generic))
        d, e = D.gemvq_inputs(epi, K, N, norm, bits, sbf, kind), D.gemvq_expect(epi, K, N, norm, bits, sbf, kind, tuned)
        tw = D.gemvq_twin(epi, d, bits, tuned)
        if epi == D.SWIGLU and kind == "gauss":
            diff, total = diff + int((tw != e["ref"]).sum()), total + tw.size
            continue
        f = D.gemv_frac(epi, e, tw, D.ROWS)
        key = f"{bits} bit {D.EPI_NAMES[epi]}" + (" coherent (ulps)" if epi == D.SWIGLU else "")
        worst[key] = max(worst.get(key, 0.0), f)
        assert f <= (3 if epi == D.SWIGLU else 1.0), (c, kind, f)
    print("quantised linear f32 twins, worst fraction of the bound:", {k: round(v, 3) for k, v in worst.items()},
          f"; Gaussian SWIGLU: {diff} of {total} outputs not bit-equal to float64 ({diff / total * 100:.3f} %)")
    assert 0 < diff < 0.01 * total


def test_plain_magnitude_understates():
    """with sum |w x| of the dequantised weights as the magnitude, the f32 error of the factored sum is understated by the ratio of the two
    (near 12 at 4 bit: (16 + q) against |q - 8|)"""
    K, N, bits = 2048, 144, 4
    m = D.quant_matrix(K, N, bits, 0)
    w = np.repeat(m["s"], 64, 1) * m["q"] + np.repeat(m["b"], 64, 1)
    ratio = {}
    for kind in ("gauss", "positive"):
        x = D.x_rows(K, kind, 0)
        _, mag = D.quant_dot(x, m, bits, True)
        ratio[kind] = float(np.median(mag / (np.abs(x) @ np.abs(w).T)))
    print("factored magnitude / magnitude of the dequantised weights (median):", {k: round(v, 2) for k, v in ratio.items()})
    assert ratio["positive"] > 4.0 and ratio["gauss"] > 4.0


# ---- wrong kernels -------------------------------------------------------------------------------------------------------------------------------
def _displacement(epi, exp, out, B):
    """-> ratio to the bound (SWIGLU: to the three ulps); inf where an exact check breaks (NaN, sentinel left in a row)"""
    if not np.isfinite(out).all() or (out == SENT).all(1).any():
        return np.inf
    f = D.gemv_frac(epi, exp, out, B)
    return f / 3.0 if epi == D.SWIGLU else f


def test_gemv_wrong_kernels():
    smallest = {}
    for mut in D.GEMV_MUTATIONS:
        hit = 0
        for c, kind in _gemv_all():
            epi, K, N, norm, generic = c
            if epi == D.SWIGLU and kind == "gauss":
                continue
            d, e = D.gemv_inputs(epi, K, N, norm, kind), D.gemv_expect(epi, K, N, norm, kind)
            for B in (17, 64) if mut.startswith("group") else (16,):
                out = D.gemv_model(epi, d, B, mut, waves=4 if K == 96 else 8)
                if out is None:
                    continue
                if mut == "resid_no_inner_round":
                    continue                                # held against the exact readout below
                assert _displacement(epi, e, D.gemv_model(epi, d, B), B) <= 1.0, (c, kind, "the model without a defect")
                r = _displacement(epi, e, out, B)
                hit += 1
                smallest[mut] = min(smallest.get(mut, np.inf), r)
                assert r >= 10.0, (mut, c, kind, B, r)
        assert hit or mut == "resid_no_inner_round", mut
    # the residual's inner rounding: the defect is at most one bf16 ulp of the accumulator, below any accumulation bound; the readout
    # (accumulator = a weight, residual on a finer grid) is exact and sees it
    rng = np.random.default_rng(5)
    W, r = G.randn_bf16(rng, (144, 1024), 1 / 32), bf16_round(rng.standard_normal((64, 144)) * 2.0 ** -4)
    k = np.array([D.readout_k(1024, i, 0) for i in range(64)])
    want = D.readout_expect(D.RESID, W, k, r)
    wrong = bf16_round(r + W[:, k].T * (1 + 2.0 ** -10))    # an accumulator that kept bits below bf16 (here: 2^-10 of itself)
    assert (want == bf16_round(r + W[:, k].T)).all() and (wrong != want).any()
    print("bf16 linear, smallest displacement / bound per wrong kernel:", {k: (round(v, 1) if np.isfinite(v) else "exact check") for k, v in smallest.items()})


def test_quant_wrong_kernels():
    """per defect and kernel family (K, norm, generic, bits, scale dtype: one template body whatever the epilogue), the largest displacement
    over the family's cases and input kinds"""
    smallest = {}
    for mut in D.QUANT_MUTATIONS:
        best = {}
        for c, kind in _gemvq_all():
            epi, K, N, norm, generic, bits, sbf = c
            tuned = bool(D.gemvq_route(epi, K, N, norm, generic))
            if (epi == D.SWIGLU and kind == "gauss") or N > 288 or (mut == "no_offset" and not (bits == 4 and tuned)):
                continue
            if mut == "drop_phase2" and not (K == 6144 and tuned):      # the two column phases of the tuned K = 6144 form
                continue
            d, e = D.gemvq_inputs(epi, K, N, norm, bits, sbf, kind), D.gemvq_expect(epi, K, N, norm, bits, sbf, kind, tuned)
            fam = (K, norm if tuned else -1, generic, bits, sbf)      # the generic kernel's norm is a launch of its own
            best[fam] = max(best.get(fam, 0.0), _displacement(epi, e, D.gemvq_twin(epi, d, bits, tuned, mut), D.ROWS))
        for fam, r in best.items():
            smallest[mut] = min(smallest.get(mut, np.inf), r)
            assert r >= 10.0, (mut, fam, r)
    print("quantised linear, smallest displacement / bound per wrong kernel:", {k: round(v, 1) for k, v in smallest.items()})
    assert set(smallest) == set(D.QUANT_MUTATIONS)


def test_readouts_see_a_wrong_pack():
    """the readout columns reach every (k-step, half fragment); an image with the halves of a fragment or the nibbles / bytes of a word
    exchanged changes what a one-hot row reads"""
    for K in (1024, 2048, 3072, 6144, 96, 1056, 192):
        seen = {(k // 32, k % 32 // 16) for sh in D.readout_shifts(K, D.ROWS) for k in (D.readout_k(K, r, sh) for r in range(D.ROWS))}
        assert len(seen) == K // 32 * 2, (K, len(seen))
    rng = np.random.default_rng(9)
    W = G.randn_bf16(rng, (144, 1024), 1 / 32)
    k = np.array([D.readout_k(1024, r, 0) for r in range(64)])
    assert (D.readout_expect(D.BF16, W, k) != D.readout_expect(D.BF16, W, k ^ 16)).any()
    for bits in (4, 8):
        m = D.quant_matrix(1024, 144, bits, 0)
        want = D.quant_readout_expect(D.BF16, m, bits, True, k)
        assert (want != D.quant_readout_expect(D.BF16, m, bits, True, k ^ 1)).any()
        if bits == 4:       # the offset form: 16 + q against b - 16 s gives the bits of s q + b only up to the f32 rounding of b'
            plain = D.quant_readout_expect(D.BF16, m, bits, False, k)
            print(f"4-bit readout: {(want != plain).mean() * 100:.2f} % of the outputs differ between the offset form and s q + b")


# ---- LM heads ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,generic", [(c[0], c[1], c[2]) for c in D.HEAD_CASES])
def test_head_twin_and_wrong_partials(K, N, generic):
    d = D.head_inputs(K, N, not generic)
    v, mag = D.head_expect(K, N, not generic)
    tw = D.head_twin(d)
    f = D.frac_bf16(tw.astype(np.float64), v, mag)
    assert f <= 1.0, f
    pairs = D.tie_pairs(N, not generic)
    assert [int(a) for a in tw.argmax(1)[:len(pairs)]] == [p[0] for p in pairs], "a planted pair is not its row's maximum"
    assert all((tw[:, lo] == tw[:, hi]).all() for lo, hi in pairs)
    tiles = D.head_tiles(N, not generic)
    assert sorted(t for p in tiles for t in p) == list(range(N // 16))
    assert D.partials_defects(tw, *D.head_partials_model(tw, tiles)) == []
    for mut in ("tie_high",) + (("skip_tail",) if not generic else ()):
        assert D.partials_defects(tw, *D.head_partials_model(tw, tiles, mut)), mut
    print(f"head K {K} N {N}: f32 twin {f:.3f} of the bound")


@pytest.mark.parametrize("K,N,generic,bits,sbf", [c[:5] for c in D.HEADQ_CASES])
def test_headq_twin_and_wrong_partials(K, N, generic, bits, sbf):
    d = D.headq_inputs(K, N, bits, sbf, not generic)
    v, mag = D.headq_expect(K, N, bits, sbf, not generic)
    tw = D.headq_twin(d, bits, not generic)
    f = D.frac_bf16(tw.astype(np.float64), v, mag)
    assert f <= 1.0, f
    pairs = D.tie_pairs(N, not generic)
    assert [int(a) for a in tw.argmax(1)[:len(pairs)]] == [p[0] for p in pairs], "a planted pair is not its row's maximum"
    assert all((tw[:, lo] == tw[:, hi]).all() for lo, hi in pairs)
    tiles = D.head_tiles(N, True) if not generic else [list(range(N // 16))]      # the generic quantised head: one partial per row
    assert D.partials_defects(tw, *D.head_partials_model(tw, tiles)) == []
    for mut in ("tie_high",) + (("skip_tail",) if not generic else ()):
        assert D.partials_defects(tw, *D.head_partials_model(tw, tiles, mut)), mut
    print(f"quantised head K {K} N {N} {bits} bit {'f32' if sbf else 'bf16'} scales: f32 twin {f:.3f} of the bound")


def test_compare_before_rounding_is_seen():
    """a head that compares unrounded sums reports a later index whose ROUNDED logit only ties the first maximum"""
    acc = np.zeros((1, 32), np.float32)
    acc[0, 5], acc[0, 9] = 1.001, 1.002
    logits = bf16_round(acc).astype(np.float32)
    pi = acc.argmax(1)[:, None].astype(np.int32)
    assert D.partials_defects(logits, logits[[0], pi[0]][:, None], pi)
    assert D.partials_defects(logits, *D.head_partials_model(logits, [[0, 1]])) == []


# ---- greedy tail ------------------------------------------------------------------------------------------------------------------------------------------
def test_finalize_wrong_kernels_break_the_exact_check():
    """on the inputs the device runs, each defect changes something the test compares"""
    vocab, max_new, half = 97, 12, 16
    rng = np.random.default_rng(1)
    table = G.randn_bf16(rng, (vocab, 64))
    cos, sin = rng.standard_normal((64, half)).astype(np.float32), rng.standard_normal((64, half)).astype(np.float32)
    keys = ("tokens", "lens", "finished", "ctx_len", "n_active", "err", "x", "cos_rows", "sin_rows")
    for n_parts in (1, 256, 257, 600):
        plain = D.finalize_inputs(17, n_parts, vocab, max_new, "plain")
        want = D.finalize_ref(plain, table, cos, sin, 1, 0)
        assert want["err"] == 0 and want["finished"][0] == 1 and want["finished"][2] == 1, "eos and the length cap are not exercised"
        assert want["n_active"] == plain["n_active"] - 2 and (want["tokens"][1] == plain["tokens"][1]).all()
        if n_parts > 1:         # the winner is the LOWER index, which stands in the later part
            b = 3
            top = plain["pi"][b][plain["pv"][b] == 32.0]
            assert want["tok"][b] == top.min() and top.min() != top[0]
        assert D.finalize_ref(plain, table, cos, sin, 1, 1)["finished"][0] == 0, "ignore_eos"
        for scenario, err in (("insane", 1), ("insane_finished", 0)):
            assert D.finalize_ref(D.finalize_inputs(17, n_parts, vocab, max_new, scenario), table, cos, sin, 1, 0)["err"] == err, scenario
        for mut in D.FINALIZE_MUTATIONS:
            d = D.finalize_inputs(17, n_parts, vocab, max_new, "insane") if mut == "no_clamp" else plain
            ref, bad = D.finalize_ref(d, table, cos, sin, 1, 0), D.finalize_ref(d, table, cos, sin, 1, 0, mut)
            assert any(not np.array_equal(ref[k], bad[k]) for k in keys), (mut, n_parts)

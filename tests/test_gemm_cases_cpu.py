"""The float64 references of tests/gemm_cases.py against independent formulations (torch.nn.functional in float64, a plain two-matrix
product), and the CPU floors that tests/test_gpu_gemm_cases.py builds its bars on.  No GPU.

Measured here (numpy + OpenBLAS f32 against float64, the inputs of gemm_cases.*_inputs):
  * conv / groupconv references vs torch conv2d / conv1d in float64: within 1e-12 of the largest output;
  * SwiGLU: the f32 twin (np.float32 accumulation over the reversed K axis, f32 sigmoid, same rounding points) differs from the float64
    reference in 0.0166 % of the 458 208 pooled Gaussian outputs (76; worst 35 bf16 ulps, at an up value that cancels to 3e-7 under
    sum |a w| = 5) -> the device's bar is 3 x that share; on the cancellation-free inputs it stays within 2 bf16 ulps (bar 3);
  * the F32 bound: an f32 product with the K axis reversed sits at <= 1.2e-7 of sum |a w| (bound 2e-6), its bf16 rounding at 0.97 of
    the BF16 bound.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
import gemm_cases as G

CONV_GEOM = [(8, 1, 1, 1), (8, 2, 3, 3), (72, 5, 4, 1), (64, 16, 25, 3), (24, 32, 13, 3)]


@pytest.mark.parametrize("C,H,W,n", CONV_GEOM)
@pytest.mark.parametrize("hw_major", [True, False])
def test_conv_reference_vs_torch(C, H, W, n, hw_major):
    rng = np.random.default_rng(C + H)
    N = C
    x, w, bias = G.randn_bf16(rng, (n, H, W, C)), G.randn_bf16(rng, (N, 9 * C), (9 * C) ** -0.5), rng.standard_normal(N)
    OH, OW = G.conv_out_hw(H, W)
    valid = [(0, 1, OW - 1, OW)[i % 4] for i in range(n)]
    pre, v, mag, masked = G.conv_ref(x, w, bias, valid, hw_major)
    # torch: NCHW input, weight [out][in][kh][kw] from the [out][kh][kw][in] K order
    tw = torch.from_numpy(w.reshape(N, 3, 3, C).transpose(0, 3, 1, 2).copy())
    y = F.conv2d(torch.from_numpy(x.transpose(0, 3, 1, 2).copy()), tw, torch.from_numpy(bias), stride=2, padding=1)
    assert y.shape == (n, N, OH, OW)
    act = F.gelu(y)
    for i in range(n):
        act[i, :, :, valid[i]:] = 0.0
    order = (0, 2, 3, 1) if hw_major else (0, 3, 2, 1)          # rows (img, oh, ow) | (img, ow, oh)
    want_pre = y.permute(*order).reshape(-1, N).numpy()
    want = act.permute(*order).reshape(-1, N).numpy()
    scale = max(1.0, float(np.abs(want_pre).max()))
    assert np.abs(pre - want_pre).max() <= 1e-12 * scale and np.abs(v - want).max() <= 1e-12 * scale
    assert (v[masked] == 0).all() and masked.sum() == sum((OW - valid[i]) * OH for i in range(n))
    assert (mag >= np.abs(pre) - 1e-12).all()


@pytest.mark.parametrize("KP,cpg,groups", [(4, 8, 2), (8, 16, 4), (128, 64, 2), (128, 80, 4)])
def test_groupconv_reference_vs_torch(KP, cpg, groups):
    rng = np.random.default_rng(KP + cpg)
    lens = [KP // 2 + 1, 1, KP + 3, 2, KP // 2]
    D = groups * cpg
    x = G.randn_bf16(rng, (sum(lens), D))
    w = G.randn_bf16(rng, (groups, cpg, KP * cpg), (KP * cpg) ** -0.5)
    bias = rng.standard_normal(D)
    pre, mag = G.groupconv_ref(x, w, bias, lens, KP, cpg, groups)
    tw = torch.from_numpy(w.reshape(D, KP, cpg).transpose(0, 2, 1).copy())       # [out][in per group][tap]
    off = 0
    for L in lens:
        y = F.conv1d(torch.from_numpy(x[off:off + L].T.copy())[None], tw, torch.from_numpy(bias), padding=KP // 2, groups=groups)
        assert y.shape == (1, D, L + 1)                                          # even kernel: one frame too many, the last is dropped
        want = y[0, :, :L].T.numpy()
        assert np.abs(pre[off:off + L] - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))
        off += L
    assert (mag >= np.abs(pre) - 1e-12).all()
    assert (G.frame_info(lens)[:, 1] == np.repeat(lens, lens)).all()


def test_swiglu_deinterleave_vs_two_matrices():
    rng = np.random.default_rng(5)
    M, N, K = 7, 96, 40
    A, W = G.randn_bf16(rng, (M, K)), G.randn_bf16(rng, (N, K))
    rows = np.arange(N).reshape(N // 32, 2, 16)
    Wg, Wu = W[rows[:, 0].reshape(-1)], W[rows[:, 1].reshape(-1)]               # the two matrices the blocks were interleaved from
    g, u = G.bf16_round(A @ Wg.T), G.bf16_round(A @ Wu.T)
    want = G.bf16_round(G.bf16_round(g / (1.0 + np.exp(-g))) * u)
    assert np.array_equal(G.swiglu_ref(A, W), want)


def test_bf16_helpers_vs_torch():
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-6, 6, 4096), [1.00390625, 1.01171875, 255.5, -0.0]])
    x = x.astype(np.float32).astype(np.float64)
    t = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16)
    assert np.array_equal(G.bf16_round(x), t.to(torch.float64).numpy())
    assert np.array_equal(G.bf16_bits(G.bf16_round(x)), t.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(G.bf16_from_bits(G.bf16_bits(G.bf16_round(x))), G.bf16_round(x))
    assert G.ulp_bf16(1.0) == 2.0 ** -7 and G.ulp_bf16(1.99) == 2.0 ** -7 and G.ulp_bf16(2.0) == 2.0 ** -6 and G.ulp_bf16(0.0) == 2.0 ** -133
    xs = np.linspace(-8, 8, 4001)
    assert np.abs(G.gelu(xs) - F.gelu(torch.from_numpy(xs)).numpy()).max() <= 1e-15
    assert np.abs(np.diff(G.gelu(xs)) / np.diff(xs)).max() <= G.GELU_SLOPE


def test_cpu_floors():
    """the share the SwiGLU bar is built on, and the distance of an honest f32 realisation from the F32 / BF16 bounds"""
    share = G.swiglu_twin_share()
    worst_g = worst_c = 0.0
    for s in G.SWIGLU_SHAPES:
        A, W = G.swiglu_inputs(*s)
        worst_g = max(worst_g, float(G.ulps_bf16(G.swiglu_twin_f32(A, W), G.swiglu_ref(A, W)).max()))
        A, W = G.swiglu_inputs(*s, coherent=True)
        ref = G.swiglu_ref(A, W)
        worst_c = max(worst_c, float(G.ulps_bf16(G.swiglu_twin_f32(A, W), ref).max()))
        assert 0.05 < np.abs(ref).max() and (ref > 0).any() and (ref < 0).any()
    print(f"swiglu f32 twin: {share * 100:.4f} % of the Gaussian outputs differ (worst {worst_g:.0f} bf16 ulps); cancellation-free inputs: "
          f"worst {worst_c:.0f} ulps")
    assert 1e-4 < share < 5e-3 and worst_c <= 3
    worst = worst_b = 0.0
    for M, N, K in G.DENSE_SHAPES:
        d = G.dense_inputs(M, N, K)
        f32 = (np.ascontiguousarray(d["A"][:, ::-1], np.float32) @ np.ascontiguousarray(d["W"][:, ::-1], np.float32).T).astype(np.float64)
        worst = max(worst, float((np.abs(f32 - d["acc"]) / (d["mag"] + 1e-30)).max()))
        worst_b = max(worst_b, float((np.abs(G.bf16_round(f32) - d["acc"]) / G.bound_bf16(d["acc"], d["mag"])).max()))
    print(f"f32 product, K reversed: worst |d| / sum |a w| = {worst:.2e} (bound {G.F32_REL:.0e}); bf16 of it: {worst_b:.3f} of the BF16 bound")
    assert worst <= G.F32_REL and worst_b <= 1.0

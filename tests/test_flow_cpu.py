"""The CosyVoice3 flow decoder without a device: the float64 oracle (tests/flow_oracle.py) against hand-computed pieces, the twin's
distance from it on every case the GPU file runs (tests/flow_cases.py holds the table), the synthetic weights' conditions, and the
C ABI's host-only entries and loader refusals on a build of the library."""
import ctypes as C
import math

import numpy as np
import pytest

import flow_cases as FC
import flow_oracle as O
from qasr import synth, _lib


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def sd2():
    return synth.synth_cosyvoice_flow_state_dict(FC.SEED, depth=FC.DEPTH_SWEEP)


@pytest.fixture(scope="module")
def sd22():
    return synth.synth_cosyvoice_flow_state_dict(FC.SEED, depth=FC.DEPTH_FULL)


@pytest.fixture(scope="module")
def pair2(sd2):
    return O.FlowOracle(sd2), O.FlowOracle(sd2, twin=True)


# ---- the oracle against hand-computed pieces ------------------------------------------------------------------------------------------
def test_sinusoid():
    s0, s1 = O.sinusoid(0.0), O.sinusoid(1.0)
    assert s0.shape == (256,) and np.all(s0[:128] == 0.0) and np.all(s0[128:] == 1.0)          # sin 0 | cos 0
    assert s1[0] == pytest.approx(math.sin(1000.0)) and s1[128] == pytest.approx(math.cos(1000.0))
    assert s1[127] == pytest.approx(math.sin(1000.0 / 10000.0)) and s1[255] == pytest.approx(math.cos(0.1))
    assert s1[1] == pytest.approx(math.sin(1000.0 * math.exp(-math.log(10000.0) / 127)))


def test_schedule_end_points():
    for n in (1, 2, 10, 64):
        t = O.schedule(n)
        assert t.shape == (n + 1,) and t[0] == 0.0 and t[-1] == pytest.approx(1.0, abs=1e-15) and np.all(np.diff(t) > 0)
    assert O.schedule(2)[1] == pytest.approx(1.0 - math.sqrt(0.5))
    lib = _lib.load(strict=True)
    t = (C.c_float * 11)()
    assert lib.qasr_flow_schedule(10, t) == 0 and t[0] == 0.0 and t[10] == 1.0
    assert np.abs(np.array(t[:]) - O.schedule(10)).max() < 2e-7
    assert lib.qasr_flow_schedule(0, t) == 1 and lib.qasr_flow_schedule(65, t) == 1 and lib.qasr_flow_schedule(10, None) == 1


def test_rope_head_zero_only():
    g = np.random.default_rng(0)
    x = g.standard_normal((3, 1024))
    y = O.rope(x)
    assert np.array_equal(y[:, 64:], x[:, 64:]) and np.array_equal(y[0], x[0])                 # features 64 .. 1023 and position 0 untouched
    c, s = math.cos(1.0), math.sin(1.0)                                                          # pair (0, 1) at position 1: 1 radian
    assert y[1, 0] == pytest.approx(x[1, 0] * c - x[1, 1] * s) and y[1, 1] == pytest.approx(x[1, 0] * s + x[1, 1] * c)
    th = 10000.0 ** (-31 / 32)                                                                   # the last pair turns slowest
    assert y[2, 62] == pytest.approx(x[2, 62] * math.cos(2 * th) - x[2, 63] * math.sin(2 * th))
    z = O.rope(x, all_heads=True)
    assert np.array_equal(z[:, :64], y[:, :64]) and not np.array_equal(z[1:, 64:], x[1:, 64:])


def test_causal_conv_row_zero():
    g = np.random.default_rng(1)
    w, b, h = g.standard_normal((1024, 31, 64)), g.standard_normal(1024), g.standard_normal((40, 1024))
    y = O.causal_group_conv(h, w, b)
    for ch in (0, 63, 64, 1023):                                                                 # row 0 sees only its own tap, the last one
        grp = ch // 64
        assert y[0, ch] == pytest.approx(b[ch] + w[ch, 30] @ h[0, grp * 64:(grp + 1) * 64])
    h2 = h.copy()
    h2[5:] += 1.0                                                                                # causal: rows before 5 do not move
    assert np.array_equal(O.causal_group_conv(h2, w, b)[:5], y[:5])
    ch, t = 70, 35                                                                               # a full window, by hand
    want = b[ch] + sum(w[ch, j] @ h[t - 30 + j, 64:128] for j in range(31))
    assert y[t, ch] == pytest.approx(want)


def test_lookahead_conv_last_row():
    g = np.random.default_rng(2)
    w, b, x = g.standard_normal((16, 4, 80)), g.standard_normal(16), g.standard_normal((6, 80))
    y = O.lookahead_conv(x, w, b)
    assert np.allclose(y[5], b + w[:, 0] @ x[5])                                                 # the last row sees only tap 0
    assert np.allclose(y[0], b + sum(w[:, j] @ x[j] for j in range(4)))
    yl = O.left_conv(x, w[:, :3], b)
    assert np.allclose(yl[0], b + w[:, 2] @ x[0]) and np.allclose(yl[5], b + sum(w[:, j] @ x[3 + j] for j in range(3)))


def test_repeat_order():
    a = np.array([[1.0, 10.0], [2.0, 20.0]])
    assert O.repeat2(a).tolist() == [[1.0, 10.0], [1.0, 10.0], [2.0, 20.0], [2.0, 20.0]]       # a a b b


def test_adaln_chunk_orders():
    p = np.repeat(np.arange(6.0), 1024)
    m = O.adaln_chunks(p)
    assert [float(m[k][0]) for k in ("shift_msa", "scale_msa", "gate_msa", "shift_mlp", "scale_mlp", "gate_mlp")] == [0, 1, 2, 3, 4, 5]
    f = O.final_chunks(np.repeat(np.arange(2.0), 1024))
    assert float(f["scale"][0]) == 0.0 and float(f["shift"][0]) == 1.0                          # the final one: scale, then shift


def test_activations():
    x = np.array([-1.0, 0.0, 2.0])
    assert np.allclose(O.silu(x), [-1.0 / (1.0 + math.e), 0.0, 2.0 / (1.0 + math.exp(-2.0))])
    assert np.allclose(O.mish(x), [-math.tanh(math.log1p(math.exp(-1.0))), 0.0, 2.0 * math.tanh(math.log1p(math.exp(2.0)))])
    assert np.allclose(O.mish(x), [-0.30340146, 0.0, 1.94395896])
    k = math.sqrt(2.0 / math.pi)
    assert np.allclose(O.gelu_tanh(x), [-0.5 * (1.0 + math.tanh(k * (-1.044715))), 0.0, 1.0 + math.tanh(k * (2.0 + 0.044715 * 8.0))])
    assert np.allclose(O.gelu_tanh(x), [-0.15880801, 0.0, 1.95459769])


def test_rounding_helpers_and_dequantise():
    assert O.bf16(1.0 + 2.0 ** -8) == 1.0 and O.bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6 and O.bf16(-3.140625) == -3.140625
    import torch
    w = torch.randn((8, 128), generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    for bits, tol in ((4, 0.5), (8, 0.03)):
        q, s, z = synth.quantize_linear(w, bits)
        d = O.dequantise({"a.weight": q, "a.scales": s, "a.biases": z}, "a")
        assert d.shape == (8, 128) and np.abs(d - w.float().numpy()).max() < tol


def test_mu_and_spks_by_hand(pair2):
    o, _ = pair2
    m = o.mu([3, 1, 4])
    assert m.shape == (6, 80) and np.array_equal(m[0], m[1]) and np.array_equal(m[4], m[5]) and not np.array_equal(m[1], m[2])
    e = o.emb[[3, 1, 4]]
    w1, b1 = o.look1
    h = [np.maximum(b1 + sum(w1[:, j] @ e[r + j] for j in range(4) if r + j < 3), 0.0) for r in range(3)]
    w2, b2 = o.look2
    assert np.allclose(m[0], b2 + w2[:, 2] @ h[0]) and np.allclose(m[4], b2 + w2[:, 0] @ h[0] + w2[:, 1] @ h[1] + w2[:, 2] @ h[2])
    assert np.array_equal(o.spks(None), np.zeros(80))
    v = np.random.default_rng(3).standard_normal(192)
    assert np.allclose(o.spks(v), o.spks(5.0 * v), atol=1e-7) and np.allclose(o.spks(v), o.spk_w @ (v / np.linalg.norm(v)) + o.spk_b)


def test_unconditioned_branch_is_zeros(pair2):
    o, _ = pair2
    x, mu, spks, cond = FC.inputs(8, True, 2)
    a = o.velocity(x, np.zeros_like(mu), None, None, 0.3)
    b = o.velocity(x, np.zeros_like(mu), np.zeros(80), np.zeros((8, 80)), 0.3)
    assert np.array_equal(a, b) and not np.allclose(a, o.velocity(x, mu, spks, cond, 0.3))


# ---- the synthetic weights: a DiT with dead gates tests nothing -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle22(sd22):
    return O.FlowOracle(sd22)


def test_synthetic_weight_conditions(oracle22):
    o = oracle22
    assert o.depth == 22
    x, mu, spks, cond = FC.inputs(FC.FULL_T, True, 2)
    tr = []
    v = o.velocity(x, mu, spks, cond, FC.FULL_TIME, trace=tr)
    rms = [a for a in tr if isinstance(a, float)]
    gates = [a for a in tr if isinstance(a, tuple)]
    assert len(rms) == 23 and all(rms[0] / 10 < r < rms[0] * 10 for r in rms), rms            # within a decade of its start
    assert rms[-1] > 2 * rms[0]                                                                  # and the blocks do move it
    assert all(0.1 <= g <= 1.0 for pair in gates for g in pair), gates
    assert 0.1 < np.sqrt((v ** 2).mean()) < 10


# ---- the twin's distance from the oracle, case by case: the table of tests/flow_cases.py ------------------------------------------------
def _same(name, got, want):
    assert want is not None and 0.8 * want <= got <= 1.25 * want, f"{name}: measured {got:.3e}, the table holds {want}"


def test_twin_distance(pair2, sd22, oracle22):
    o, tw = pair2
    vel = {}
    for T, t, spk, Tp in FC.velocity_cases():
        x, mu, spks, cond = FC.inputs(T, spk, Tp)
        vel[FC.case_key(T, t, spk, Tp)] = rel(tw.velocity(x, mu, spks, cond, t), o.velocity(x, mu, spks, cond, t))
    print("TWIN_VELOCITY = {" + ", ".join('"%s": %.2e' % kv for kv in vel.items()) + "}")
    x, mu, spks, cond = FC.inputs(FC.SOLVE_T, True, 2)
    z = np.random.default_rng(11).standard_normal((FC.SOLVE_T, 80)).astype(np.float32)
    sol, ref = {}, {}
    for n in FC.SOLVE_STEPS:
        ref[n] = o.solve(mu, spks, cond, z, n)[0]
        sol[n] = rel(tw.solve(mu, spks, cond, z, n)[0], ref[n])
    print("TWIN_SOLVE = {" + ", ".join("%d: %.2e" % kv for kv in sol.items()) + "}")
    # what the solve bound must tell apart: mu fed to the unconditioned branch, and RoPE on every head
    wrong_cfg = rel(o.solve(mu, spks, cond, z, 10, wrong_cfg=True)[0], ref[10])
    wrong_rope = rel(o.solve(mu, spks, cond, z, 10, rope_all_heads=True)[0], ref[10])
    print(f"wrong CFG {wrong_cfg:.2e}, RoPE on every head {wrong_rope:.2e}, bound {FC.MARGIN * sol[10]:.2e}")
    assert wrong_cfg > FC.MARGIN * sol[10] and wrong_rope > FC.MARGIN * sol[10]
    o22, tw22 = oracle22, O.FlowOracle(sd22, twin=True)
    x, mu, spks, cond = FC.inputs(FC.FULL_T, True, 2)
    full = rel(tw22.velocity(x, mu, spks, cond, FC.FULL_TIME), o22.velocity(x, mu, spks, cond, FC.FULL_TIME))
    tok, ptok, feat, emb, z = FC.generate_inputs()
    T = 2 * (len(tok) + len(ptok))
    cond = np.zeros((T, 80))
    cond[:feat.shape[1]] = feat.T
    mu = o22.mu(list(ptok) + list(tok))
    gen = rel(tw22.solve(mu, tw22.spks(emb), cond, z, 10)[0], o22.solve(mu, o22.spks(emb), cond, z, 10)[0])
    sd8 = synth.synth_cosyvoice_flow_state_dict(FC.SEED, depth=FC.DEPTH_SWEEP, bits=8)             # the 8-bit file of the GPU loader test
    x, mu, spks, cond = FC.inputs(FC.FULL_T, True, 2)
    w8 = rel(O.FlowOracle(sd8, twin=True).velocity(x, mu, spks, cond, FC.FULL_TIME), O.FlowOracle(sd8).velocity(x, mu, spks, cond, FC.FULL_TIME))
    print(f"TWIN_VELOCITY_FULL = {full:.2e}\nTWIN_GENERATE_FULL = {gen:.2e}\nTWIN_VELOCITY_8BIT = {w8:.2e}")
    for k, v in vel.items():
        _same(k, v, FC.TWIN_VELOCITY.get(k))
    for n, v in sol.items():
        _same(f"solve {n}", v, FC.TWIN_SOLVE.get(n))
    _same("velocity depth 22", full, FC.TWIN_VELOCITY_FULL)
    _same("generate depth 22", gen, FC.TWIN_GENERATE_FULL)
    _same("velocity 8 bit", w8, FC.TWIN_VELOCITY_8BIT)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------------------
def test_host_abi():
    lib = _lib.load(strict=True)
    assert [lib.qasr_flow_mel_frames(n) for n in (0, 1, 5, 250)] == [0, 2, 10, 500]
    fp, ip = (C.c_float * 320)(), (C.c_int32 * 4)(1, 2, 3, 4)
    assert lib.qasr_flow_mu(None, ip, 4, fp) == 1 and lib.qasr_flow_spks(None, fp, fp) == 1
    assert lib.qasr_flow_velocity(None, fp, fp, None, None, 1, 0.5, fp) == 1
    assert lib.qasr_flow_solve(None, fp, None, None, 1, fp, 10, None, fp) == 1
    assert lib.qasr_flow_generate(None, ip, 4, None, 0, None, 0, None, 10, 1.0, 0, None, fp) == 1
    assert lib.qasr_flow_generate_batch(None, None, None, None, None, None, None, None, 10, 1.0, None, 1, None, None) == 1
    assert lib.qasr_flow_unload(None) == 1 and lib.qasr_flow_timing(None, fp) == 1
    assert lib.qasr_flow_is_loaded(None) == 0 and lib.qasr_flow_memory_footprint(None) == 0 and lib.qasr_flow_depth(None) == 0
    lib.qasr_flow_destroy(None)
    # what generate checks of a clip, on the host
    err = lambda: lib.qasr_flow_last_error(None).decode()
    ok = lambda *a: lib.qasr_flow_check_clip(*a)
    assert ok(ip, 4, None, 0, 0, 6561, 0) == 0 and ok(ip, 4, ip, 2, 4, 6561, 0) == 0
    assert ok(None, 4, None, 0, 0, 6561, 0) == 1 and "null" in err()
    assert ok(ip, 0, None, 0, 0, 6561, 0) == 1 and "no tokens" in err()                        # n = 0
    assert ok(ip, 4, None, 0, 0, 4, 0) == 1 and "token 3 is 4" in err()                        # an id outside the table: refused, not clamped
    neg = (C.c_int32 * 2)(0, -1)
    assert ok(ip, 4, neg, 2, 4, 6561, 0) == 1 and "token 1 is -1" in err()
    assert ok(ip, 4, ip, 2, 2, 6561, 0) == 1 and "prompt mel" in err()                         # Tp != 2 x prompt tokens
    assert ok(ip, 4, None, 0, 2, 6561, 0) == 1 and "prompt mel" in err()
    assert ok(ip, 4, None, 0, 0, 6561, 6) == 1 and "max_frames" in err() and ok(ip, 4, None, 0, 0, 6561, 8) == 0


def test_loader_refusals(tmp_path, sd2):
    lib = _lib.load(strict=True)
    h = C.c_void_p()
    err = lambda: lib.qasr_flow_last_error(None).decode()
    assert lib.qasr_flow_create(0, None, 0, None, C.byref(h)) == 1 and "model_dir" in err()
    assert lib.qasr_flow_create(0, b".", 0, None, None) == 1
    assert lib.qasr_flow_create(0, str(tmp_path / "none").encode(), 0, None, C.byref(h)) == 4
    assert lib.qasr_flow_create(0, b".", (1 << 15) + 1, None, C.byref(h)) == 1 and "max_frames" in err()
    b1 = "decoder.transformer_blocks.1."
    cases = ((dict(drop=("decoder.proj_out.bias",)), 4, "decoder.proj_out.bias"),
             (dict(drop=(b1 + "ff.ff.2.scales",)), 4, b1 + "ff.ff.2.scales"),
             (dict(drop=(b1 + "attn.to_k.weight",)), 4, b1 + "attn.to_k.weight"),
             (dict(reshape={b1 + "attn.to_v.weight": (1024, 64)}), 1, b1 + "attn.to_v.weight"),
             (dict(reshape={"decoder.input_embed.conv_pos_embed.conv2.0.weight": (1024, 31, 32)}), 1, "conv_pos_embed.conv2.0.weight"),
             (dict(reshape={"spk_embed_affine_layer.weight": (80, 128)}), 1, "spk_embed_affine_layer.weight"),
             (dict(reshape={"input_embedding.weight": (6561, 64)}), 1, "input_embedding.weight"),
             (dict(reshape={b1 + "attn_norm.linear.bias": (1024,)}), 1, b1 + "attn_norm.linear.bias"),
             (dict(extra={"decoder.transformer_blocks.1.attn.to_q.lora": np.zeros(4)}), 1, "attn.to_q.lora"),
             (dict(extra={"encoder_proj.weight": np.zeros((4, 4))}), 1, "encoder_proj.weight"))
    for i, (kw, code, word) in enumerate(cases):
        d = synth.write_cosyvoice_flow_safetensors(sd2, str(tmp_path / f"bad{i}"), **kw)
        assert lib.qasr_flow_create(0, d.encode(), 0, None, C.byref(h)) == code, (kw, err())
        assert word in err() and err().startswith("flow decoder: "), (kw, err())
    float_sd = dict(sd2)                                                                        # a float checkpoint is not served
    float_sd["decoder.norm_out.linear.weight"] = sd2["decoder.proj_out.weight"].new_zeros((2048, 128))
    d = synth.write_cosyvoice_flow_safetensors(float_sd, str(tmp_path / "float"))
    assert lib.qasr_flow_create(0, d.encode(), 0, None, C.byref(h)) == 1 and "U32" in err()

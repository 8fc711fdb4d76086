"""The CosyVoice3 flow-matching mel decoder on the MI355X (csrc/flow_cosyvoice.hip, csrc/api_flow.cpp) over the C ABI, against the float64
oracle tests/flow_oracle.py, with synthetic weights (qasr.synth) on the real widths: the shape sweep at depth 2, one velocity case and
one generate case at depth 22.

Tolerances.  The device runs its GEMMs on bf16 operands; tests/test_flow_cpu.py::test_twin_distance measures, on these very inputs,
how far that precision plan alone (the oracle's twin) lies from float64, as max |d| / peak, and tests/flow_cases.py holds the figures.
A device result must lie within MARGIN = 4 x its case's figure (DESIGN.md sections 18 and 22).  mu is f32 throughout: its bound is the
worst case of an f32 sum of K = 3072 terms, K 2^-24 of the peak.  Everything the solver adds on top of the velocity is pinned bit for bit:
solve to a float32 Euler loop over velocity, generate to solve on its own noise, a clip in a batch to the clip alone.
Every test prints the device's figure (FLOW_PARITY lines); DESIGN.md section 22 holds the table they fill."""
import ctypes as C

import numpy as np
import pytest

import flow_cases as FC
import flow_oracle as O
from qasr import synth, vocoder, _lib
from qasr.flow import CosyVoiceFlow, schedule, synthesize_tokens
from qasr.model import QasrError

pytestmark = pytest.mark.gpu

MU_TOKENS = (1, 2, 3, 4, 5, 33)                        # the first five: no longer than the look-ahead (4 taps) and the causal reach (3)
MU_TOL = 3072 * 2.0 ** -24
BATCH_T = (2, 130, 4, 66, 30)
BATCH_SEEDS = (3, 1 << 63, 0, 0xFFFFFFFFFFFFFFFF, 77)
THREE_PASSES = 130                                     # holds (2) | (130) | (4, 66, 30)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def report(case, twin, got):
    print(f"FLOW_PARITY {case}: twin {twin:.2e} bound {FC.MARGIN * twin:.2e} device {got:.2e}")
    assert got <= FC.MARGIN * twin, (case, got, FC.MARGIN * twin)


def stored_bytes(sd):
    return sum(v.numel() * (2 if k.endswith((".scales", ".biases")) else 4) for k, v in sd.items())


@pytest.fixture(scope="module")
def sd2():
    return synth.synth_cosyvoice_flow_state_dict(FC.SEED, depth=FC.DEPTH_SWEEP)


@pytest.fixture(scope="module")
def dir2(sd2, tmp_path_factory):
    return synth.write_cosyvoice_flow_safetensors(sd2, str(tmp_path_factory.mktemp("flow2")))


@pytest.fixture(scope="module")
def flow(dir2):
    m = CosyVoiceFlow.from_pretrained(dir2, max_frames=512)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle(sd2):
    return O.FlowOracle(sd2)


@pytest.fixture(scope="module")
def sd22():
    return synth.synth_cosyvoice_flow_state_dict(FC.SEED, depth=FC.DEPTH_FULL)


@pytest.fixture(scope="module")
def flow22(sd22, tmp_path_factory):
    m = CosyVoiceFlow.from_pretrained(synth.write_cosyvoice_flow_safetensors(sd22, str(tmp_path_factory.mktemp("flow22"))), max_frames=256)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle22(sd22):
    return O.FlowOracle(sd22)


def euler_loop(flow, mu, spks, cond, z, n):
    """the solver restated over velocity(): float32, each product and sum rounded once, in the order of fl_euler_kernel"""
    t, x = schedule(n), z.copy()
    one_plus, cfg = np.float32(1.0) + np.float32(0.7), np.float32(0.7)
    for i in range(n):
        vc = flow.velocity(x, mu, t[i], spks, cond)
        vu = flow.velocity(x, np.zeros_like(mu), t[i])
        v = one_plus * vc - cfg * vu
        x = x + (t[i + 1] - t[i]) * v
        assert x.dtype == np.float32
    return x, vc, vu


# ---- stages -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", MU_TOKENS)
def test_mu(flow, oracle, n):
    tok = np.random.default_rng(n).integers(0, 6561, n).astype(np.int32)
    tok[0], tok[-1] = (6560, 0) if n > 1 else (6560, 6560)
    got, want = flow.mu(tok), oracle.mu(tok)
    d = rel(got, want)
    print(f"FLOW_PARITY mu n={n}: bound {MU_TOL:.2e} device {d:.2e}")
    assert got.shape == (2 * n, 80) and d <= MU_TOL
    assert np.array_equal(got[0::2], got[1::2])                                                 # a a b b


def test_spks(flow, oracle):
    e = np.random.default_rng(4).standard_normal(192).astype(np.float32)
    assert rel(flow.spks(e), oracle.spks(e)) <= 192 * 2.0 ** -24
    assert np.array_equal(flow.spks(None), np.zeros(80, dtype=np.float32))


@pytest.mark.parametrize("T,t,spk,Tp", FC.velocity_cases(), ids=[FC.case_key(*c) for c in FC.velocity_cases()])
def test_velocity(flow, oracle, T, t, spk, Tp):
    x, mu, spks, cond = FC.inputs(T, spk, Tp)
    got = flow.velocity(x, mu, t, spks, cond)
    key = FC.case_key(T, t, spk, Tp)
    report(key, FC.TWIN_VELOCITY[key], rel(got, oracle.velocity(x, mu, spks, cond, t)))
    assert np.array_equal(got, flow.velocity(x, mu, t, spks, cond))                             # the same bits run to run
    if not spk and not Tp:                                                                       # NULL is zeros
        assert np.array_equal(got, flow.velocity(x, mu, t, np.zeros(80, dtype=np.float32), np.zeros((T, 80), dtype=np.float32)))


def test_velocity_depth22(flow22, oracle22):
    assert flow22.depth == 22
    x, mu, spks, cond = FC.inputs(FC.FULL_T, True, 2)
    got = flow22.velocity(x, mu, FC.FULL_TIME, spks, cond)
    report("velocity depth 22", FC.TWIN_VELOCITY_FULL, rel(got, oracle22.velocity(x, mu, spks, cond, FC.FULL_TIME)))


def test_velocity_8bit(tmp_path):
    sd = synth.synth_cosyvoice_flow_state_dict(FC.SEED, depth=FC.DEPTH_SWEEP, bits=8)
    m = CosyVoiceFlow.from_pretrained(synth.write_cosyvoice_flow_safetensors(sd, str(tmp_path / "w8")), max_frames=128)
    try:
        assert m.depth == 2 and m.memory_footprint == stored_bytes(sd)
        x, mu, spks, cond = FC.inputs(FC.FULL_T, True, 2)
        report("velocity 8 bit", FC.TWIN_VELOCITY_8BIT, rel(m.velocity(x, mu, FC.FULL_TIME, spks, cond), O.FlowOracle(sd).velocity(x, mu, spks, cond, FC.FULL_TIME)))
    finally:
        m.close()


# ---- the solver -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FC.SOLVE_STEPS)
def test_solve(flow, oracle, n):
    x, mu, spks, cond = FC.inputs(FC.SOLVE_T, True, 2)
    z = np.random.default_rng(11).standard_normal((FC.SOLVE_T, 80)).astype(np.float32)
    mel, v = flow.solve(mu, z, spks, cond, n, return_velocity=True)
    want, vc, vu = euler_loop(flow, mu, spks, cond, z, n)
    assert np.array_equal(mel, want)                                                            # bit for bit
    assert np.array_equal(v[0], vc) and np.array_equal(v[1], vu)                                # the last step's two velocities
    assert np.array_equal(mel, flow.solve(mu, z, spks, cond, n))                                # and with the cached modulation table
    report(f"solve n={n}", FC.TWIN_SOLVE[n], rel(mel, oracle.solve(mu, spks, cond, z, n)[0]))


def test_solve_refusals(flow):
    x, mu, _, _ = FC.inputs(4, False, 0)
    for n in (-1, 65):
        with pytest.raises(QasrError, match="n_steps"):
            flow.solve(mu, x, n_steps=n)
    big = np.zeros((514, 80), dtype=np.float32)
    with pytest.raises(QasrError, match="max_frames"):
        flow.velocity(big, big, 0.5)


# ---- the whole model --------------------------------------------------------------------------------------------------------------------
def test_generate_depth22(flow22, oracle22):
    tok, ptok, feat, emb, z_host = FC.generate_inputs()
    T = 2 * (len(tok) + len(ptok))
    mel, z = flow22.generate(tok, ptok, feat, emb, 10, 1.0, FC.GEN_SEED, strip_prompt=False, return_noise=True)
    assert mel.shape == (80, T) and z.shape == (80, T)
    assert np.abs(z.T - z_host).max() <= 4e-6                                                   # qasr_hift_noise at counters 80 t + m
    cond = np.zeros((T, 80), dtype=np.float32)
    cond[:feat.shape[1]] = feat.T
    mu, spks = flow22.mu(np.concatenate([ptok, tok])), flow22.spks(emb)
    assert np.array_equal(mel.T, flow22.solve(mu, np.ascontiguousarray(z.T), spks, cond, 10))   # the stage entries chained: the same bits
    again = flow22.generate(tok, ptok, feat, emb, 10, 1.0, FC.GEN_SEED, strip_prompt=False)
    assert np.array_equal(mel, again)                                                            # run to run
    stripped = flow22.generate(tok, ptok, feat, emb, 10, 1.0, FC.GEN_SEED)
    assert np.array_equal(stripped, mel[:, 2 * len(ptok):])
    want = oracle22.solve(oracle22.mu(list(ptok) + list(tok)), oracle22.spks(emb), cond, z_host, 10)[0]
    report("generate depth 22", FC.TWIN_GENERATE_FULL, rel(mel.T, want))


def test_generate_temperature(flow):
    tok = np.arange(3, dtype=np.int32)
    _, z0 = flow.generate(tok, temperature=0.0, seed=9, n_steps=1, return_noise=True)
    assert np.all(z0 == 0.0)
    _, z1 = flow.generate(tok, temperature=1.0, seed=9, n_steps=1, return_noise=True)
    _, z2 = flow.generate(tok, temperature=0.5, seed=9, n_steps=1, return_noise=True)
    want = vocoder.noise(9, np.arange(80 * 6, dtype=np.uint64))[1].reshape(6, 80)
    assert np.abs(z1.T - want).max() <= 4e-6 and np.abs(z2.T - 0.5 * want).max() <= 4e-6
    _, z3 = flow.generate(tok, temperature=1.0, seed=10, n_steps=1, return_noise=True)
    assert not np.array_equal(z1, z3)


def test_generate_refusals(flow):
    tok = np.arange(3, dtype=np.int32)
    with pytest.raises(QasrError, match="no tokens"):
        flow.generate(np.zeros(0, dtype=np.int32))
    with pytest.raises(QasrError, match="outside"):
        flow.generate(np.array([1, 6561], dtype=np.int32))
    with pytest.raises(QasrError, match="prompt mel"):
        flow.generate(tok, tok[:2], np.zeros((80, 2), dtype=np.float32))
    with pytest.raises(QasrError, match="prompt mel"):
        flow.generate(tok, None, np.zeros((80, 2), dtype=np.float32))
    with pytest.raises(QasrError, match="max_frames"):
        flow.generate(np.zeros(257, dtype=np.int32))


def test_ragged_batch(flow, dir2):
    g = np.random.default_rng(21)
    toks = [g.integers(0, 6561, T // 2).astype(np.int32) for T in BATCH_T]
    embs = [g.standard_normal(192).astype(np.float32) if i % 2 else None for i in range(len(toks))]
    alone = [flow.generate(t, spk_emb=e, n_steps=2, seed=s) for t, e, s in zip(toks, embs, BATCH_SEEDS)]
    assert [a.shape for a in alone] == [(80, T) for T in BATCH_T]
    batched = flow.generate_batch(toks, spk_emb=embs, n_steps=2, seeds=BATCH_SEEDS)
    rev = flow.generate_batch(toks[::-1], spk_emb=embs[::-1], n_steps=2, seeds=BATCH_SEEDS[::-1])[::-1]
    small = CosyVoiceFlow.from_pretrained(dir2, max_frames=THREE_PASSES)
    try:
        passes = small.generate_batch(toks, spk_emb=embs, n_steps=2, seeds=BATCH_SEEDS)
        with pytest.raises(QasrError, match="max_frames"):
            small.generate(np.zeros(66, dtype=np.int32))
    finally:
        small.close()
    for i in range(len(toks)):                                                                  # bit-identical per clip in every case
        assert np.array_equal(alone[i], batched[i]) and np.array_equal(alone[i], rev[i]) and np.array_equal(alone[i], passes[i]), i
    assert flow.generate_batch([]) == []


def test_synthesize_tokens(flow, tmp_path):
    voc = vocoder.HiFTVocoder.from_pretrained(synth.write_cosyvoice_hifigan_safetensors(synth.synth_cosyvoice_hifigan_state_dict(0), str(tmp_path / "hift")),
                                              max_frames=64)
    try:
        g = np.random.default_rng(31)
        tok, ptok = g.integers(0, 6561, 5).astype(np.int32), g.integers(0, 6561, 2).astype(np.int32)
        feat = (g.standard_normal((80, 4)) - 2.0).astype(np.float32)
        pcm, rows = synthesize_tokens(flow, voc, tok, ptok, feat, None, n_steps=2, seed=5, vocoder_seed=6, return_mel=True)
        assert pcm.shape == (480 * 2 * 5 + 16,) and rows.shape == (10, 80) and np.isfinite(pcm).all()
        full = flow.generate(tok, ptok, feat, None, 2, 1.0, 5, strip_prompt=False)
        assert np.array_equal(rows, full[:, 4:].T)                                               # the prompt frames are sliced off
        assert np.array_equal(pcm, voc.decode(rows, 6))
    finally:
        voc.close()


# ---- loader, unload ---------------------------------------------------------------------------------------------------------------------
def test_loader_and_footprint(flow, flow22, sd2, sd22):
    assert flow.depth == 2 and flow22.depth == 22 and flow.is_loaded and flow22.is_loaded
    assert flow.memory_footprint == stored_bytes(sd2) and flow22.memory_footprint == stored_bytes(sd22)
    assert set(flow.timing()) == {"modulation", "input_embed", "blocks", "output", "euler"}


def test_unload(dir2):
    m = CosyVoiceFlow.from_pretrained(dir2, max_frames=64)
    try:
        x, mu, _, _ = FC.inputs(4, False, 0)
        m.velocity(x, mu, 0.5)
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        lib, fp, ip = m.lib, (C.c_float * 640)(), (C.c_int32 * 2)(1, 2)
        pp, ipp = (C.POINTER(C.c_float) * 1)(fp), (C.POINTER(C.c_int32) * 1)(ip)
        n1, sd_ = (C.c_size_t * 1)(2), (C.c_uint64 * 1)(0)
        assert lib.qasr_flow_mu(m.h, ip, 2, fp) == 3 and lib.qasr_flow_spks(m.h, None, fp) == 3
        assert lib.qasr_flow_velocity(m.h, fp, fp, None, None, 4, 0.5, fp) == 3
        assert lib.qasr_flow_solve(m.h, fp, None, None, 4, fp, 2, None, fp) == 3
        assert lib.qasr_flow_generate(m.h, ip, 2, None, 0, None, 0, None, 2, 1.0, 0, None, fp) == 3
        assert lib.qasr_flow_generate_batch(m.h, ipp, n1, None, None, None, None, None, 2, 1.0, sd_, 1, None, pp) == 3
        assert lib.qasr_flow_mu(m.h, None, 0, None) == 3                                         # NOT_LOADED comes before every other refusal
        assert "unloaded" in lib.qasr_flow_last_error(m.h).decode()
        m.unload()
    finally:
        m.close()

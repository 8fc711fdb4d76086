"""The CosyVoice3 speech tokenizer and voice profiles without a device: the host entries of the C ABI (resampler, length functions, the FSQ
twin, the profile's cut rule, the loader's refusals) against tests/s3tok_oracle.py, and the table of tests/s3tok_cases.py: how far the
precision plan alone (the oracle's twin) lies from float64 on the inputs of tests/test_gpu_s3tok.py.  DESIGN.md section 24."""
import ctypes as C
import math

import numpy as np
import pytest

import s3tok_cases as SC
import s3tok_oracle as O
from qasr import _lib, s3tok, synth


# ---- host arithmetic ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(16000, 24000), (24000, 16000), (44100, 16000), (44100, 24000), (16000, 16000), (24000, 24000)])
def test_resampler_bit_for_bit(src, dst):
    for n in (1, 2, 3, 160, 441, 4801, 16000):
        x = SC.pcm(n, n, src)
        got, want = s3tok.resample(x, src, dst), O.resample(x, src, dst)
        assert got.size == want.size == s3tok.resampled_length(n, src, dst) == O.resampled_length(n, src, dst)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (src, dst, n)
    if src == dst:
        assert np.array_equal(s3tok.resample(x, src, dst), x)
    else:                                                                  # the last sample repeats: the final outputs interpolate towards x[-1] itself
        assert s3tok.resample(np.ones(100, np.float32), src, dst).tolist() == [1.0] * s3tok.resampled_length(100, src, dst)


def test_length_functions():
    for n in list(range(0, 2000, 7)) + [160 * T + r for _, T in SC.token_cases() for r in (0, 1, 159)] + SC.whisper_samples():
        assert s3tok.whisper_frames(n) == O.whisper_frames(n) == n // 160, n
    for T in range(0, 600):
        assert s3tok.tokens_of(T) == O.tokens_of(T), T
    for n, T in SC.token_cases():
        assert s3tok.tokens_of(T) == n
    assert {T % 2 for _, T in SC.token_cases()} == {0, 1} and {O.conv_len(T) % 2 for _, T in SC.token_cases()} == {0, 1}
    for n in list(range(0, 3000, 13)) + [479] + list(SC.FLOW_SAMPLES):
        assert s3tok.flow_frames(n) == O.flow_frames(n) == (n // 480 if n >= 480 else 0), n
    for n in SC.FLOW_SAMPLES:
        assert O.flow_mel(SC.pcm(n, n, 24000)).shape == (80, s3tok.flow_frames(n))
    for n in SC.whisper_samples()[:4]:
        assert O.whisper_mel(SC.pcm(n, n)).shape == (128, s3tok.whisper_frames(n))
    assert [s3tok.tokens_of(s3tok.whisper_frames(160 * SC.mel_frames(n, i) + 11 * i)) for i, n in enumerate(SC.BATCH_TOKENS)] == list(SC.BATCH_TOKENS)


def test_fsq_host_on_crafted_projections():
    e = O.FSQ_EDGE
    vals = np.array([0.0, -0.0, 1e-6, e - 1e-3, e + 1e-3, -e + 1e-3, -e - 1e-3, 0.5, -0.5, 3.0, -3.0, 40.0, -40.0, 1e30, -1e30, e * 0.999], dtype=np.float32)
    p = np.stack([np.roll(vals, k)[:8] for k in range(16)])
    got = s3tok.fsq_host(p)
    assert np.array_equal(got, O.fsq_codes(p)) and got.min() >= 0 and got.max() < 6561
    assert s3tok.fsq_host(np.zeros((1, 8)))[0] == sum(3 ** k for k in range(8))             # every digit 1
    assert s3tok.fsq_host(np.full((1, 8), 9.0))[0] == 6560 and s3tok.fsq_host(np.full((1, 8), -9.0))[0] == 0
    one = np.zeros((1, 8), dtype=np.float32)
    one[0, 3] = e + 1e-3                                                                    # digit k weighs 3^k
    assert s3tok.fsq_host(one)[0] == sum(3 ** k for k in range(8)) + 27
    assert np.array_equal(O.digits_of(got), O.fsq_digits(p))


def test_profile_cut_rule():
    for nt, nf, L in ((26, 50, 25), (25, 50, 25), (25, 53, 25), (10, 0, 0), (0, 8, 0), (3, 7, 3), (4, 7, 3)):
        assert s3tok.profile_cut(nt, nf) == O.profile_cut(nt, nf) == L
    n16 = 16160                                                                              # 1.01 s at 16 kHz: 26 tokens and 50 frames disagree
    assert s3tok.tokens_of(s3tok.whisper_frames(n16)) == 26 and s3tok.flow_frames(s3tok.resampled_length(n16, 16000, 24000)) == 50


def test_synthetic_weight_conditions():
    """What the code-level comparisons of the GPU test rest on: unit-variance projections, every FSQ level in at least a fifth of the
    digits, and at most 15 % of a case's digits within MARGIN x the twin's distance of a level boundary."""
    for n, T in SC.token_cases():
        if n < 15:
            continue
        _, p = SC.reference(2, n, T)
        d = O.fsq_digits(p)
        share = [float((d == k).mean()) for k in range(3)]
        und = float(SC.undecided(p, SC.MARGIN * SC.TWIN_PROJ_ABS[n]).mean())
        print(f"tokens {n}: projection std {p.std():.3f}, level shares {share}, undecided {und:.3f}")
        assert 0.8 < p.std() < 1.25 and min(share) >= 0.2 and und <= SC.UNDECIDED_MAX


# ---- the twin's distance from the oracle, case by case: the table of tests/s3tok_cases.py ---------------------------------------------------
def _same(name, got, want):
    assert want is not None and 0.8 * want <= got <= 1.25 * want, f"{name}: measured {got:.3e}, the table holds {want}"


def test_twin_distance():
    tw = SC.oracle(2, twin=True)
    hid, prj, pabs, flips = {}, {}, {}, {}
    for n, T in SC.token_cases():
        h64, p64 = SC.reference(2, n, T)
        h, p = tw.both(SC.mel_input(n, T))
        hid[n], prj[n], pabs[n] = SC.rel(h, h64), SC.rel(p, p64), float(np.abs(p - p64).max())
        flips[n] = float((O.fsq_digits(p) != O.fsq_digits(p64)).mean())
    fmt = lambda d: "{" + ", ".join("%d: %.2e" % kv for kv in d.items()) + "}"
    print(f"TWIN_HIDDEN = {fmt(hid)}\nTWIN_PROJ = {fmt(prj)}\nTWIN_PROJ_ABS = {fmt(pabs)}\ndigits the twin flips: {fmt(flips)}")
    T = SC.mel_frames(SC.FULL_TOKENS, 0)
    h64, p64 = SC.reference(12, SC.FULL_TOKENS, T)
    h, p = SC.oracle(12, twin=True).both(SC.mel_input(SC.FULL_TOKENS, T))
    full_h, full_p = SC.rel(h, h64), SC.rel(p, p64)
    print(f"TWIN_HIDDEN_FULL = {full_h:.2e}\nTWIN_PROJ_FULL = {full_p:.2e}")
    for n in hid:
        _same(f"hidden {n}", hid[n], SC.TWIN_HIDDEN.get(n))
        _same(f"projections {n}", prj[n], SC.TWIN_PROJ.get(n))
        _same(f"projections (absolute) {n}", pabs[n], SC.TWIN_PROJ_ABS.get(n))
    _same("hidden depth 12", full_h, SC.TWIN_HIDDEN_FULL)
    _same("projections depth 12", full_p, SC.TWIN_PROJ_FULL)


def test_mel_twin_distance():
    wh = {n: SC.rel(O.whisper_mel(SC.pcm(n, n), twin=True), O.whisper_mel(SC.pcm(n, n))) for n in SC.whisper_samples()}
    fl = {n: SC.rel(O.flow_mel(SC.pcm(n, n, 24000), twin=True), O.flow_mel(SC.pcm(n, n, 24000))) for n in SC.FLOW_SAMPLES}
    fmt = lambda d: "{" + ", ".join("%d: %.2e" % kv for kv in d.items()) + "}"
    print(f"TWIN_WHISPER = {fmt(wh)}\nTWIN_FLOW = {fmt(fl)}")
    for n, v in wh.items():
        _same(f"whisper mel {n}", v, SC.TWIN_WHISPER.get(n))
    for n, v in fl.items():
        _same(f"flow mel {n}", v, SC.TWIN_FLOW.get(n))


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------------
def test_host_abi():
    lib = _lib.load(strict=True)
    fp, ip, sz = (C.c_float * 2048)(), (C.c_int32 * 64)(), (C.c_size_t * 1)()
    assert lib.qasr_s3tok_whisper_mel(None, fp, 320, fp) == 1 and lib.qasr_s3tok_flow_mel(None, fp, 480, fp) == 1
    assert lib.qasr_s3tok_hidden(None, fp, 4, fp) == 1 and lib.qasr_s3tok_project(None, fp, 4, fp) == 1
    assert lib.qasr_s3tok_encode(None, fp, 320, ip) == 1 and lib.qasr_s3tok_encode_batch(None, None, None, 1, None) == 1
    assert lib.qasr_s3tok_profile(None, fp, 2048, 16000, ip, sz, fp, sz, None, None) == 1
    assert lib.qasr_s3tok_profile_batch(None, None, None, None, 1, None, None, None, None, None, None) == 1
    assert lib.qasr_s3tok_unload(None) == 1 and lib.qasr_s3tok_timing(None, fp) == 1
    assert lib.qasr_s3tok_is_loaded(None) == 0 and lib.qasr_s3tok_memory_footprint(None) == 0 and lib.qasr_s3tok_depth(None) == 0
    assert lib.qasr_s3tok_resample(None, 4, 16000, 24000, fp) == 1 and lib.qasr_s3tok_resample(fp, 4, 0, 24000, fp) == 1
    assert lib.qasr_s3tok_fsq_host(None, 2, ip) == 1 and lib.qasr_s3tok_resampled_length(100, 0, 5) == 0
    lib.qasr_s3tok_destroy(None)


@pytest.fixture(scope="module")
def sd1():
    return synth.synth_cosyvoice_s3tok_state_dict(SC.SEED, dict(depth=1))


def test_loader_refusals(tmp_path, sd1):
    lib = _lib.load(strict=True)
    h = C.c_void_p()
    err = lambda: lib.qasr_s3tok_last_error(None).decode()
    assert lib.qasr_s3tok_create(0, None, 0, None, C.byref(h)) == 1 and "model_dir" in err()
    assert lib.qasr_s3tok_create(0, b".", 0, None, None) == 1
    assert lib.qasr_s3tok_create(0, str(tmp_path / "none").encode(), 0, None, C.byref(h)) == 4
    assert lib.qasr_s3tok_create(0, b".", (1 << 14) + 1, None, C.byref(h)) == 1 and "max_tokens" in err()
    b0 = "encoder.blocks.0."
    cases = ((dict(drop=("encoder.conv2.bias",)), 4, "encoder.conv2.bias"),
             (dict(drop=(b0 + "attn.fsmn_block.weight",)), 4, b0 + "attn.fsmn_block.weight"),
             (dict(drop=(b0 + "attn.query.weight",)), 4, b0 + "attn.query.weight"),
             (dict(drop=("quantizer._codebook.project_down.weight",)), 4, "project_down.weight"),
             (dict(reshape={"encoder.conv1.weight": (1280, 128, 3)}), 1, "encoder.conv1.weight"),
             (dict(reshape={b0 + "attn.fsmn_block.weight": (1280, 31)}), 1, b0 + "attn.fsmn_block.weight"),
             (dict(reshape={b0 + "mlp.0.weight": (1280, 5120)}), 1, b0 + "mlp.0.weight"),
             (dict(reshape={"quantizer._codebook.project_down.bias": (9,)}), 1, "project_down.bias"),
             (dict(extra={b0 + "attn.key.bias": np.zeros(1280)}), 1, b0 + "attn.key.bias"),
             (dict(extra={"encoder.positional_embedding": np.zeros((4, 4))}), 1, "encoder.positional_embedding"),
             (dict(dtype="F64"), 1, "F64"))
    for i, (kw, code, word) in enumerate(cases):
        d = synth.write_cosyvoice_s3tok_safetensors(sd1, str(tmp_path / f"bad{i}"), **kw)
        assert lib.qasr_s3tok_create(0, d.encode(), 0, None, C.byref(h)) == code, (kw, err())
        assert word in err() and err().startswith("speech tokenizer: "), (kw, err())
        assert not h.value

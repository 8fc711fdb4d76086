"""The Qwen3-TTS speech tokenizer decoder on the MI355X (csrc/codec_qwen3tts.hip, csrc/api_codec.cpp) over the C ABI, against the float64
oracle tests/codec_oracle.py, with synthetic weights (qasr.synth) on a reduced geometry (edges, chunking, batching) and the real one.

Tolerances: the reference's own precision is f32.  tests/test_codec_cpu.py::test_f32_distance measures, per stage, the max |d| between
the oracle and its f32 twin on these inputs, normalised by the stage output's peak:
    reduced geometry: rvq 2.33e-07, pre_transformer 4.15e-07, forward (pre-clip) 6.33e-06, decode 1.22e-05
    real geometry (tests/test_codec_cpu.py::test_real_geometry_preclip_and_f32_distance): forward (pre-clip, T = 1, 3, 35) 8.42e-06,
                      pre_transformer (T = 35) 6.00e-07, decode (T = 36, clipped) 1.36e-05
Each bound is 10 x that figure (another f32 summation order through a deep chain, as in DESIGN.md sections 13 and 14); clipped outputs
take the pre-clip bound.  The device's measured distances are printed by every test and recorded in DESIGN.md section 15."""
import ctypes as C

import numpy as np
import pytest

import codec_oracle as O
from qasr import synth, _lib
from qasr.codec import SpeechTokenizerDecoder, window_positions
from qasr.model import QasrError

pytestmark = pytest.mark.gpu

F32 = {"rvq": 2.33e-07, "pre_transformer": 4.15e-07, "forward": 6.33e-06, "decode": 1.22e-05, "real_forward": 8.42e-06,
       "real_pre_transformer": 6.00e-07, "real_decode": 1.36e-05}
TOL = {k: 10 * v for k, v in F32.items()}
G, R = O.REDUCED, O.REAL
BATCH_T = (1, 36, 7, 61, 35)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def sd():
    return synth.synth_speech_tokenizer_state_dict(0, G)


@pytest.fixture(scope="module")
def W(sd):
    return O.Weights(sd)


@pytest.fixture(scope="module")
def model_dir(sd, tmp_path_factory):
    return synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("codec")), G)


@pytest.fixture(scope="module")
def dec(model_dir):
    m = SpeechTokenizerDecoder.from_pretrained(model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def batch(W):
    """The ragged batch and its float64 decodes, computed once and shared."""
    codes = [O.make_codes(T, T, G) for T in BATCH_T]
    return codes, [O.decode(c, W, G) for c in codes]


@pytest.fixture(scope="module")
def real():
    """The real geometry: weights, handle, float64 oracle weights."""
    import tempfile
    sd = synth.synth_speech_tokenizer_state_dict(1, R)
    with tempfile.TemporaryDirectory() as d:
        m = SpeechTokenizerDecoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, d))
    yield m, O.Weights(sd)
    m.close()


@pytest.mark.parametrize("T", [1, 2, 11, 35])
def test_stages_reduced(dec, W, T):
    codes = O.make_codes(T, T, G)
    q = O.quantizer_decode(codes, W, G)
    got_q = dec.quantizer_decode(codes)
    x = O.pre_conv(q, W).astype(np.float32)
    got_p = dec.pre_transformer(x)
    raw, clipped = dec.forward(codes, clip=False), dec.forward(codes)
    want = O.forward(codes, W, G, clip=False)
    d = dict(rvq=rel(got_q, q), pre_transformer=rel(got_p, O.pre_transformer(x.astype(np.float64), W, G)), forward=rel(raw, want),
             clipped=float(np.abs(clipped - np.clip(want, -1, 1)).max() / np.abs(want).max()))
    print("reduced T = %d: device vs float64 oracle, of peak: %s (bounds rvq %.2e, pre_transformer %.2e, forward %.2e)"
          % (T, ", ".join("%s %.2e" % kv for kv in d.items()), TOL["rvq"], TOL["pre_transformer"], TOL["forward"]))
    assert got_q.shape == (T, G["hidden_size"]) and got_p.shape == (T, G["latent_dim"]) and raw.shape == clipped.shape == (1920 * T,)
    assert np.abs(clipped).max() <= 1.0 and np.array_equal(clipped, np.clip(raw, -1, 1))
    assert d["rvq"] <= TOL["rvq"] and d["pre_transformer"] <= TOL["pre_transformer"]
    assert d["forward"] <= TOL["forward"] and d["clipped"] <= TOL["forward"]


@pytest.mark.parametrize("T", [1, 3, 35])
def test_forward_real(real, T):
    m, W = real
    codes = O.make_codes(100 + T, T, R)
    got = m.forward(codes, clip=False)
    d = rel(got, O.forward(codes, W, R, clip=False))
    print("real T = %d forward: device vs float64 oracle %.2e of peak (bound %.2e)" % (T, d, TOL["real_forward"]))
    assert got.shape == (1920 * T,) and d <= TOL["real_forward"]


def test_pre_transformer_real(real):
    m, W = real
    codes = O.make_codes(135, 35, R)
    x = O.pre_conv(O.quantizer_decode(codes, W, R), W).astype(np.float32)
    d = rel(m.pre_transformer(x), O.pre_transformer(x.astype(np.float64), W, R))
    print("real T = 35 pre_transformer: device vs float64 oracle %.2e of peak (bound %.2e)" % (d, TOL["real_pre_transformer"]))
    assert d <= TOL["real_pre_transformer"]


def test_decode_real(real):
    m, W = real
    codes = O.make_codes(136, 36, R)
    got = m.decode(codes)
    d = rel(got, O.decode(codes, W, R))
    print("real T = 36 decode: device vs float64 oracle %.2e of peak (bound %.2e)" % (d, TOL["real_decode"]))
    assert got.shape == (1920 * 36,) and d <= TOL["real_decode"]


@pytest.mark.parametrize("T", [35, 36, 61])
def test_decode_reduced(dec, W, T):
    assert [e - s for s, c, e in window_positions(T)] == {35: [35], 36: [25, 21], 61: [25, 35, 21]}[T]
    codes = O.make_codes(T, T, G)
    got = dec.decode(codes)
    d = rel(got, O.decode(codes, W, G))
    print("reduced T = %d decode: device vs float64 oracle %.2e of peak (bound %.2e)" % (T, d, TOL["decode"]))
    assert got.shape == (1920 * T,) and got.dtype == np.float32 and d <= TOL["decode"]
    if T == 35:
        assert np.array_equal(got, dec.forward(codes))


@pytest.mark.parametrize("max_windows", [0, 2])
def test_ragged_batch(dec, model_dir, batch, max_windows):
    """Nine windows of five utterances; with max_windows = 2 a pass boundary falls inside an utterance."""
    codes, want = batch
    m = dec if max_windows == 0 else SpeechTokenizerDecoder.from_pretrained(model_dir, max_windows=max_windows)
    try:
        got = m.decode_batch(codes)
    finally:
        if m is not dec:
            m.close()
    worst = 0.0
    for g, w, T in zip(got, want, BATCH_T):
        assert g.shape == (1920 * T,)
        worst = max(worst, rel(g, w))
    print("ragged batch, max_windows %d: device vs float64 oracle %.2e of peak (bound %.2e)" % (max_windows, worst, TOL["decode"]))
    assert worst <= TOL["decode"]


def test_bit_identity(dec, model_dir, batch):
    codes, _ = batch
    alone = [dec.decode(c) for c in codes]
    runs = [dec.decode_batch(codes), dec.decode_batch(codes[::-1])[::-1]]
    for mw in (2, 64):
        m = SpeechTokenizerDecoder.from_pretrained(model_dir, max_windows=mw)
        try:
            runs.append(m.decode_batch(codes))
        finally:
            m.close()
    runs.append(dec.decode_batch(codes))
    for other in runs:
        for a, b in zip(alone, other):
            assert np.array_equal(a, b)
    # a window alone equals the same window inside a longer utterance's batch: T = 36's second window is frames 15..36
    c36 = codes[1]
    assert np.array_equal(dec.forward(c36[:, 15:36])[10 * 1920:], alone[1][25 * 1920:])


def test_loader(sd, W, tmp_path_factory):
    codes = O.make_codes(11, 11, G)
    assert any(k.endswith("_codebook.embed") for k in sd) and any(k.endswith("cluster_usage") for k in sd)
    assert min(float(v.min()) for k, v in sd.items() if k.endswith("cluster_usage")) < 1e-7         # the clamp is exercised
    key = "decoder.decoder.2.block.3.conv1.conv.weight"
    for kw, code in ((dict(drop=(key,)), 4), (dict(reshape={key: (12, 12, 5)}), 1),
                     (dict(drop=("decoder.quantizer.rvq_rest.vq.layers.2._codebook.cluster_usage",)), 4)):
        d = synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("bad")), G, **kw)
        with pytest.raises(QasrError) as e:
            SpeechTokenizerDecoder.from_pretrained(d)
        name = key if "cluster_usage" not in str(kw) else "rvq_rest.vq.layers.2._codebook.cluster_usage"
        assert ("qasr error %d:" % code) in str(e.value) and name in str(e.value)
    bad_geom = dict(G, head_dim=32)
    with pytest.raises(QasrError) as e:
        SpeechTokenizerDecoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("geom")), bad_geom))
    assert "qasr error 1:" in str(e.value) and "head_dim" in str(e.value)
    # bf16-stored weights: the oracle on the bf16-rounded values
    def bf16(a):
        u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    m = SpeechTokenizerDecoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("bf16")), G, dtype="BF16"))
    try:
        Wb = O.Weights({k: bf16(v) for k, v in sd.items()})
        dq = rel(m.quantizer_decode(codes), O.quantizer_decode(codes, Wb, G))
        df = rel(m.forward(codes, clip=False), O.forward(codes, Wb, G, clip=False))
        assert m.memory_footprint == 2 * sum(v.size for v in sd.values())
    finally:
        m.close()
    print("bf16-stored weights: rvq %.2e, forward %.2e of peak (bounds %.2e, %.2e)" % (dq, df, TOL["rvq"], TOL["forward"]))
    assert dq <= TOL["rvq"] and df <= TOL["forward"]
    assert rel(O.quantizer_decode(codes, Wb, G), O.quantizer_decode(codes, W, G)) > 1e-4           # the rounding is visible


def test_lifecycle_and_errors(dec, model_dir, W):
    codes = O.make_codes(7, 7, G)
    want = O.forward(codes, W, G)
    assert dec.is_loaded and dec.memory_footprint > 0 and dec.num_quantizers == 16
    for bad in (G["acoustic_codebook_size"], -1):
        c = codes.copy()
        c[5, 3] = bad
        for call in (lambda: dec.forward(c), lambda: dec.decode(c), lambda: dec.quantizer_decode(c), lambda: dec.decode_batch([codes, c])):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 1:" in str(e.value) and "quantizer 5" in str(e.value)
        assert rel(dec.forward(codes), want) <= TOL["forward"]                                    # the next valid call is right
    for call in (lambda: dec.forward(np.zeros((16, 0), np.int32)), lambda: dec.decode(np.zeros((16, 0), np.int32)),
                 lambda: dec.forward(O.make_codes(36, 36, G))):
        with pytest.raises(QasrError) as e:
            call()
        assert "qasr error 1:" in str(e.value)
    lib = _lib.load(strict=True)
    ip = codes.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.qasr_codec_forward(dec.h, ip, 1, 7, 1, None) == 1 and lib.qasr_codec_decode(dec.h, None, 7, None) == 1
    assert set(dec.timing()) == {"quantizer", "pre_transformer", "upsample", "block1", "block2", "block3", "block4", "output"}
    m = SpeechTokenizerDecoder.from_pretrained(model_dir)
    try:
        assert rel(m.decode(codes), want) <= TOL["forward"]
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        for call in (lambda: m.decode(codes), lambda: m.forward(codes), lambda: m.quantizer_decode(codes)):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 3:" in str(e.value)
    finally:
        m.close()

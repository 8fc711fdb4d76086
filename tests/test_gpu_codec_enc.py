"""The Qwen3-TTS speech tokenizer encoder on the MI355X (csrc/codec_enc_qwen3tts.hip, csrc/api_codec_enc.cpp) over the C ABI, against the
float64 oracle tests/codec_enc_oracle.py, with synthetic weights (qasr.synth) on the reduced geometry (edges, ragged lengths, batching)
and the real one.

Tolerances: the reference's own precision is f32.  tests/test_codec_enc_cpu.py::test_f32_distance measures, on these inputs, the max |d|
between the oracle and its torch f32 twin, normalised by the stage output's peak (the F32 table below).  Each bound is 10 x its figure
(another f32 summation order through a deep chain, as in DESIGN.md sections 13 to 15).  Codes are compared chain by chain: see
test_quantize and test_encode_vs_oracle.  The device's distances are printed by every test; DESIGN.md section 16 holds the parity table they fill."""
import ctypes as C

import numpy as np
import pytest

import codec_enc_oracle as O
from qasr import synth, _lib
from qasr.codec import SpeechTokenizerDecoder, SpeechTokenizerEncoder, num_frames
from qasr.model import QasrError

pytestmark = pytest.mark.gpu

F32 = {"conv": 1.23e-06, "latent": 1.03e-06, "real_conv": 1.44e-06, "real_latent": 1.33e-06}
TOL = {k: 10 * v for k, v in F32.items()}
G, R = O.REDUCED, O.REAL
LENGTHS = (1, 1920, 1921, 1920 * 37 + 517, 1920 * 97)
REAL_LENGTHS = (1920 * 3, 1920 * 33 + 7)
BATCH_N = (1, 1921, 1920 * 37 + 517, 700, 1920 * 5)
NEAR_TIE, CHAIN_CAP, FIRST_MATCH, E2E_CAP = 1e-5, 0.02, 0.98, 0.10


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def sd():
    return synth.synth_speech_tokenizer_encoder_state_dict(0, G)


@pytest.fixture(scope="module")
def W(sd):
    return O.Weights(sd)


@pytest.fixture(scope="module")
def model_dir(sd, tmp_path_factory):
    return synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("codec_enc")), G)


@pytest.fixture(scope="module")
def enc(model_dir):
    m = SpeechTokenizerEncoder.from_pretrained(model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ref(W):
    """The float64 conv output and latent of every reduced length, computed once and shared."""
    out = {}
    for n in LENGTHS:
        c = O.conv(O.make_pcm(n, n), W, G)
        out[n] = (c, O.transformer(c, W, G))
    return out


@pytest.fixture(scope="module")
def real():
    """The real geometry: handle, float64 oracle weights and the oracle's conv outputs and latents (seconds of CPU: once per module)."""
    import tempfile
    sd = synth.synth_speech_tokenizer_encoder_state_dict(1, R)
    with tempfile.TemporaryDirectory() as d:
        m = SpeechTokenizerEncoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, d), max_samples=1920 * 40)
    W = O.Weights(sd)
    want = {}
    for n in REAL_LENGTHS + (1920 * 40,):
        c = O.conv(O.make_pcm(n, n), W, R)
        want[n] = (c, O.transformer(c, W, R))
    yield m, W, want
    m.close()


def chain_report(got, h, W, g, accept):
    """Device codes `got` [Q, T] against the float64 RVQ encode of h [T, hidden], per frame and quantizer chain, stage by stage.  At a
    chain's first differing stage accept(t, name, stage, r, cb, code_dev, code_oracle) must hold (r: the float64 residual entering the
    stage); the chain's later stages are left out.  Returns (chains left out / chains, frames whose semantic code matches / frames)."""
    T = h.shape[0]
    left_out, first_ok = 0, 0
    for name, row, count in O.chains(g):
        r = O.project(np.asarray(h, dtype=np.float64), W, name)
        alive = np.ones(T, dtype=bool)
        for i in range(count):
            cb = O.codebook(W, "encoder.quantizer.%s.vq.layers.%d._codebook" % (name, i))
            want = O.distances(r, cb).argmin(axis=-1)
            dev = got[row + i]
            for t in np.nonzero(alive & (dev != want))[0]:
                assert accept(int(t), name, i, r[t], cb, int(dev[t]), int(want[t])), (name, i, int(t), int(dev[t]), int(want[t]))
                alive[t] = False
            r = r - cb[want]
            if row == 0:
                first_ok = int((dev == want).sum())
        left_out += int((~alive).sum())
    return left_out / (2.0 * T), first_ok / float(T)


def near_tie(t, name, stage, r, cb, dev, want):
    d = ((r[None, :] - cb[[dev, want]]) ** 2).sum(axis=-1)
    return d[0] - d[1] <= NEAR_TIE * d[1]


def check_frame_shapes(m, n, c, h):
    F = num_frames(n)
    assert F == -(-n // 1920) and c.shape == (F, m.latent_dim) and h.shape == (F, m.hidden_size)
    assert c.dtype == h.dtype == np.float32 and np.isfinite(c).all() and np.isfinite(h).all()


@pytest.mark.parametrize("n", LENGTHS)
def test_stages_reduced(enc, ref, n):
    pcm = O.make_pcm(n, n)
    c, h = enc.conv(pcm), enc.latent(pcm)
    check_frame_shapes(enc, n, c, h)
    d = dict(conv=rel(c, ref[n][0]), latent=rel(h, ref[n][1]))
    print("reduced n = %d (%d frames): device vs float64 oracle, of peak: conv %.2e (bound %.2e), latent %.2e (bound %.2e)"
          % (n, c.shape[0], d["conv"], TOL["conv"], d["latent"], TOL["latent"]))
    assert d["conv"] <= TOL["conv"] and d["latent"] <= TOL["latent"]


@pytest.mark.parametrize("n", REAL_LENGTHS)
def test_stages_real(real, n):
    m, W, want = real
    pcm = O.make_pcm(n, n)
    c, h = m.conv(pcm), m.latent(pcm)
    check_frame_shapes(m, n, c, h)
    d = dict(conv=rel(c, want[n][0]), latent=rel(h, want[n][1]))
    print("real n = %d (%d frames): device vs float64 oracle, of peak: conv %.2e (bound %.2e), latent %.2e (bound %.2e)"
          % (n, c.shape[0], d["conv"], TOL["real_conv"], d["latent"], TOL["real_latent"]))
    assert d["conv"] <= TOL["real_conv"] and d["latent"] <= TOL["real_latent"]


@pytest.mark.parametrize("geometry", ["reduced", "real"])
def test_quantize(enc, ref, W, real, geometry):
    """quantize on the oracle's latent cast to f32, against the float64 RVQ on that same f32 input: at a chain's first differing stage
    the device's code is a verified near-tie (its float64 distance exceeds the best by at most 1e-5 of it)."""
    if geometry == "reduced":
        m, Wq, g, h = enc, W, G, ref[1920 * 97][1].astype(np.float32)
    else:
        m, Wq, g, h = real[0], real[1], R, real[2][1920 * 40][1].astype(np.float32)
    assert h.shape[0] == (97 if geometry == "reduced" else 40)
    got = m.quantize(h)
    assert got.shape == (16, h.shape[0]) and got.dtype == np.int32
    assert got.min() >= 0 and got[0].max() < g["semantic_codebook_size"] and got[1:].max() < g["acoustic_codebook_size"]
    left, first = chain_report(got, h, Wq, g, near_tie)
    exact = float((got == O.rvq_encode(h.astype(np.float64), Wq, g)).mean())
    print("%s quantize, %d frames: chains with a near-tie stage left out %.4f (cap %.2f), semantic code equal %.4f (floor %.2f), "
          "codes equal to the float64 encode %.4f" % (geometry, h.shape[0], left, CHAIN_CAP, first, FIRST_MATCH, exact))
    assert left <= CHAIN_CAP and first >= FIRST_MATCH


@pytest.mark.parametrize("n", LENGTHS)
def test_encode_consistent(enc, n):
    pcm = O.make_pcm(n, n)
    codes = enc.encode(pcm)
    assert codes.shape == (16, num_frames(n)) and codes.dtype == np.int32
    assert np.array_equal(codes, enc.quantize(enc.latent(pcm)))
    print("n = %d: encode equals quantize(latent) on all %d codes" % (n, codes.size))


@pytest.mark.parametrize("n", [1920 * 37 + 517, 1920 * 97])
def test_encode_vs_oracle(enc, ref, W, n):
    """End to end against the float64 encode: a chain's first differing stage is accepted only if the measured latent difference of
    that frame explains the flip: d(code_dev) - d(code_oracle) <= 4 |c_dev - c_oracle| |(h_dev - h_oracle)[t] @ w| in float64."""
    pcm = O.make_pcm(n, n)
    codes, h_dev, h = enc.encode(pcm), enc.latent(pcm).astype(np.float64), ref[n][1]
    dh = {name: O.project(h_dev - h, W, name) for name, _, _ in O.chains(G)}

    def explained(t, name, stage, r, cb, dev, want):
        d = ((r[None, :] - cb[[dev, want]]) ** 2).sum(axis=-1)
        return d[0] - d[1] <= 4.0 * np.linalg.norm(cb[dev] - cb[want]) * np.linalg.norm(dh[name][t])

    left, first = chain_report(codes, h, W, G, explained)
    print("reduced n = %d (%d frames) encode vs float64 oracle: chains left out after an explained flip %.4f (cap %.2f), semantic code "
          "equal %.4f, codes equal %.4f" % (n, h.shape[0], left, E2E_CAP, first, float((codes == O.rvq_encode(h, W, G)).mean())))
    assert left <= E2E_CAP


@pytest.fixture(scope="module")
def batch(enc):
    clips = [O.make_pcm(40 + i, n) for i, n in enumerate(BATCH_N)]
    return clips, [enc.conv(p) for p in clips], [enc.latent(p) for p in clips], [enc.encode(p) for p in clips]


@pytest.mark.parametrize("max_samples", [0, 1920 * 37 + 517 + 700])
def test_ragged_batch(enc, model_dir, W, batch, max_samples):
    """Five clips of ragged lengths; the small max_samples holds (1, 1921) | (1920 * 37 + 517, 700) | (1920 * 5): three passes."""
    clips = batch[0]
    m = enc if max_samples == 0 else SpeechTokenizerEncoder.from_pretrained(model_dir, max_samples=max_samples)
    try:
        lat, codes = m.latent_batch(clips), m.encode_batch(clips)
    finally:
        if m is not enc:
            m.close()
    worst = 0.0
    for p, h, c, n in zip(clips, lat, codes, BATCH_N):
        assert h.shape == (num_frames(n), G["hidden_size"]) and c.shape == (16, num_frames(n))
        worst = max(worst, rel(h, O.latent(p, W, G)))
    print("ragged batch, max_samples %d: latent device vs float64 oracle %.2e of peak (bound %.2e)" % (max_samples, worst, TOL["latent"]))
    assert worst <= TOL["latent"]
    for a, b in zip(batch[2], lat):
        assert np.array_equal(a, b)
    for a, b in zip(batch[3], codes):
        assert np.array_equal(a, b)


def test_bit_identity(enc, model_dir, batch):
    clips, conv1, lat1, codes1 = batch
    small = SpeechTokenizerEncoder.from_pretrained(model_dir, max_samples=1920 * 37 + 517 + 700)
    try:
        runs = [(enc.conv_batch(clips), enc.latent_batch(clips), enc.encode_batch(clips)),
                (enc.conv_batch(clips[::-1])[::-1], enc.latent_batch(clips[::-1])[::-1], enc.encode_batch(clips[::-1])[::-1]),
                (small.conv_batch(clips), small.latent_batch(clips), small.encode_batch(clips)),
                (small.conv_batch(clips[::-1])[::-1], small.latent_batch(clips[::-1])[::-1], small.encode_batch(clips[::-1])[::-1])]
    finally:
        small.close()
    for cv, lt, cd in runs:
        for a, b in zip(conv1 + lat1 + codes1, cv + lt + cd):
            assert a.shape == b.shape and np.array_equal(a, b)
    # neighbours filled with 1e30 on both sides change no bit: the conv and the attention stay inside the clip
    for k in (1, 2, 3):
        loud = [np.full(1920 * 3 + 11, 1e30, np.float32), clips[k], np.full(977, 1e30, np.float32)]
        with np.errstate(all="ignore"):
            cv, lt, cd = enc.conv_batch(loud)[1], enc.latent_batch(loud)[1], enc.encode_batch(loud)[1]
        assert np.array_equal(cv, conv1[k]) and np.array_equal(lt, lat1[k]) and np.array_equal(cd, codes1[k])
    print("bit identity: %d clips alone = batched = reversed = three passes = between 1e30 neighbours" % len(clips))


def test_loader(sd, W, ref, tmp_path_factory):
    n = 1921
    pcm = O.make_pcm(n, n)
    assert any(k.endswith("_codebook.embed") for k in sd) and any(k.endswith("cluster_usage") for k in sd)    # both codebook forms
    assert min(float(v.min()) for k, v in sd.items() if k.endswith("cluster_usage")) < 1e-7                  # the clamp is exercised
    # one checkpoint with both halves loads for both handles
    dsd = synth.synth_speech_tokenizer_state_dict(0, G)
    both = synth.write_speech_tokenizer_safetensors(synth.merge_speech_tokenizer_state_dicts(dsd, sd), str(tmp_path_factory.mktemp("both")), G)
    e, d = SpeechTokenizerEncoder.from_pretrained(both), SpeechTokenizerDecoder.from_pretrained(both)
    try:
        codes = e.encode(pcm)
        dl = rel(e.latent(pcm), ref[n][1])
        wave = d.decode(codes)
        assert wave.shape == (1920 * codes.shape[1],) and np.isfinite(wave).all() and dl <= TOL["latent"]
    finally:
        e.close()
        d.close()
    key = "encoder.encoder.2.block.1.conv1.conv.weight"
    for kw, code in ((dict(drop=(key,)), 4), (dict(reshape={key: (5, 5, 7)}), 1),
                     (dict(drop=("encoder.pre_transformer.output_proj.weight",)), 4),
                     (dict(drop=("encoder.quantizer.rvq_rest.vq.layers.2._codebook.cluster_usage",)), 4)):
        bad = synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("bad")), G, **kw)
        with pytest.raises(QasrError) as ei:
            SpeechTokenizerEncoder.from_pretrained(bad)
        name = list(kw.get("drop", ()) or kw["reshape"])[0]
        assert ("qasr error %d:" % code) in str(ei.value) and name in str(ei.value)
    with pytest.raises(QasrError) as ei:
        SpeechTokenizerEncoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("geom")), dict(G, head_dim=32)))
    assert "qasr error 1:" in str(ei.value) and "head_dim" in str(ei.value)
    # bf16-stored weights: the oracle on the bf16-rounded values
    def bf16(a):
        u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    m = SpeechTokenizerEncoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, str(tmp_path_factory.mktemp("bf16")), G, dtype="BF16"))
    try:
        Wb = O.Weights({k: bf16(v) for k, v in sd.items()})
        cb = O.conv(pcm, Wb, G)
        dc, dl = rel(m.conv(pcm), cb), rel(m.latent(pcm), O.transformer(cb, Wb, G))
        assert m.memory_footprint == 2 * sum(v.size for v in sd.values())
    finally:
        m.close()
    print("bf16-stored weights, n = %d: conv %.2e, latent %.2e of peak (bounds %.2e, %.2e)" % (n, dc, dl, TOL["conv"], TOL["latent"]))
    assert dc <= TOL["conv"] and dl <= TOL["latent"]
    assert rel(cb, ref[n][0]) > 1e-4                                                                         # the rounding is visible


def test_lifecycle_and_errors(enc, model_dir):
    pcm = O.make_pcm(7, 1920 * 2 + 3)
    want = enc.encode(pcm)
    assert enc.is_loaded and enc.memory_footprint > 0 and enc.num_quantizers == 16 and want.shape == (16, 3)
    assert [num_frames(n) for n in (0, 1, 1919, 1920, 1921)] == [0, 1, 1, 1, 2]
    lib = _lib.load(strict=True)
    fp, ip = pcm.ctypes.data_as(C.POINTER(C.c_float)), want.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.qasr_codec_enc_encode(enc.h, fp, pcm.size, None) == 1 and lib.qasr_codec_enc_encode(enc.h, None, pcm.size, ip) == 1
    assert lib.qasr_codec_enc_encode(enc.h, fp, 0, ip) == 1 and lib.qasr_codec_enc_quantize(enc.h, None, 3, ip) == 1
    assert lib.qasr_codec_enc_conv(enc.h, fp, pcm.size, None) == 1 and lib.qasr_codec_enc_latent(enc.h, None, pcm.size, None) == 1
    assert lib.qasr_codec_enc_encode(None, fp, pcm.size, ip) == 1
    with pytest.raises(QasrError) as e:
        enc.quantize(np.zeros((0, G["hidden_size"]), np.float32))
    assert "qasr error 1:" in str(e.value)
    assert enc.encode_batch([]) == []
    assert np.array_equal(enc.encode(pcm), want)                                                  # the next valid call is right
    assert set(enc.timing()) == {"input", "block1", "block2", "block3", "block4", "downsample", "pre_transformer", "quantizer"}
    assert all(v > 0 for v in enc.timing().values())
    m = SpeechTokenizerEncoder.from_pretrained(model_dir, max_samples=4000)
    try:
        assert np.array_equal(m.encode(pcm), want)
        for call in (lambda: m.encode(np.zeros(4001, np.float32)), lambda: m.encode_batch([pcm, np.zeros(4001, np.float32)]),
                     lambda: m.latent(np.zeros(4001, np.float32))):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 1:" in str(e.value) and "max_samples" in str(e.value)
        assert np.array_equal(m.encode(pcm), want)
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        for call in (lambda: m.encode(pcm), lambda: m.conv(pcm), lambda: m.latent(pcm), lambda: m.quantize(np.zeros((2, G["hidden_size"]), np.float32))):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 3:" in str(e.value)
    finally:
        m.close()
    # order_with an ASR engine: the encoder's work goes on the engine's stream
    from qasr import config as QC
    from qasr.model import Qwen3ASRModel
    asr = Qwen3ASRModel.from_state_dict(synth.synth_state_dict(QC.AUDIO_TINY, QC.TEXT_TINY, seed=3, init="stress"), preset="tiny", device=0,
                                        max_audio_seconds=4, max_new_tokens=8)
    try:
        m = SpeechTokenizerEncoder.from_pretrained(model_dir, order_with=asr, max_samples=8000)
        try:
            assert np.array_equal(m.encode(pcm), want)
        finally:
            m.close()
    finally:
        asr.close()

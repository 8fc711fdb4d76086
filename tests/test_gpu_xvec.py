"""The Qwen3-TTS ECAPA-TDNN speaker encoder on the MI355X (csrc/xvec_qwen3tts.hip, csrc/api_xvec.cpp) over the C ABI, against the float64
oracle tests/xvec_oracle.py, with synthetic weights (qasr.synth) on the real geometry (8.8 M parameters).

Tolerances: the reference's own precision is f32.  tests/test_xvec_cpu.py::test_f32_distance measures, on these inputs, the max |d|
between the oracle and its torch f32 twin, normalised by the output's peak (the F32 table below).  Each bound is 10 x its figure (another
f32 summation order through a deep chain, as in DESIGN.md sections 13 to 16).  The mel and embed figures are worst cases over the
shortest clips, whose bins sit just above the 1e-5 clamp; "network" is the twin's distance for the network alone on a given float32
log-mel of 63, 64, 65 and 129 frames, about 50 times smaller, so that an error confined to a few rows at a tile edge cannot hide in
test_network_at_tile_edges.  Every test prints the device's distances; DESIGN.md section 17 holds the parity table they fill."""
import ctypes as C

import numpy as np
import pytest

import xvec_oracle as O
from qasr import synth, _lib
from qasr.model import QasrError
from qasr.tts_speaker import SpeakerEncoder, num_frames

pytestmark = pytest.mark.gpu

F32 = {"mel": 1.35e-04, "embed": 2.24e-05, "network": 4.13e-07}
TOL = {k: 10 * v for k, v in F32.items()}
RES_TILE, RED_TILE = 64, 64                            # rows of a Res2Net tile and of a GEMM / reduction tile (csrc/xvec_qwen3tts.h)
MEL_LENGTHS = (1, 2, 255, 256, 512, 513, 1023, 1024, 256 * 63 + 17)
# frames 1 | 2 .. 5 (shorter than every dilation's reach) | T - 1, T, T + 1, 2 T + 1 of both tiles | about 300
TILE_LENGTHS = tuple(256 * (f - 1) for T in sorted({RES_TILE, RED_TILE}) for f in (T - 1, T, T + 1, 2 * T + 1))
EMBED_LENGTHS = MEL_LENGTHS + (256 * 3,) + TILE_LENGTHS + (256 * 299 + 100,)
BATCH_N = (1, 513, 256 * 63 + 17, 700, 256 * 20)
NETWORK_FRAMES = tuple(sorted({f for T in (RES_TILE, RED_TILE) for f in (T - 1, T, T + 1, 2 * T + 1)}))
THREE_PASSES = 256 * 63 + 17 + 513                     # holds (1, 513) | (256 * 63 + 17) | (700, 256 * 20)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def sd():
    return synth.synth_tts_speaker_encoder_state_dict(0)


@pytest.fixture(scope="module")
def W(sd):
    return O.Weights(sd)


@pytest.fixture(scope="module")
def model_dir(sd, tmp_path_factory):
    return synth.write_tts_speaker_encoder_safetensors(sd, str(tmp_path_factory.mktemp("xvec")))


@pytest.fixture(scope="module")
def enc(model_dir):
    m = SpeakerEncoder.from_pretrained(model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def ref(W):
    """The float64 log-mel and embedding of every length, computed once and shared."""
    out = {}
    for n in EMBED_LENGTHS:
        m = O.mel(O.make_pcm(n, n))
        out[n] = (m, O.network(m, W))
    return out


@pytest.fixture(scope="module")
def batch(enc):
    clips = [O.make_pcm(40 + i, n) for i, n in enumerate(BATCH_N)]
    return clips, [enc.mel(p) for p in clips], [enc.embed(p) for p in clips]


def test_tile_lengths():
    assert [n // 256 + 1 for n in TILE_LENGTHS] == [63, 64, 65, 129] and (256 * 299 + 100) // 256 + 1 == 300
    assert [n // 256 + 1 for n in (256, 512, 256 * 3, 1024)] == [2, 3, 4, 5]


@pytest.mark.parametrize("n", MEL_LENGTHS)
def test_mel_vs_oracle(enc, ref, n):
    got = enc.mel(O.make_pcm(n, n))
    assert got.shape == (n // 256 + 1, 128) == (num_frames(n), 128) and got.dtype == np.float32 and np.isfinite(got).all()
    d = rel(got, ref[n][0])
    print("n = %d (%d frames): log-mel device vs float64 oracle %.2e of peak (bound %.2e)" % (n, got.shape[0], d, TOL["mel"]))
    assert d <= TOL["mel"]


@pytest.mark.parametrize("n", EMBED_LENGTHS)
def test_embed_vs_oracle(enc, ref, n):
    x = O.make_pcm(n, n)
    got = enc.embed(x)
    assert got.shape == (1024,) and got.dtype == np.float32 and np.isfinite(got).all()
    d = rel(got, ref[n][1])
    print("n = %d (%d frames): embedding device vs float64 oracle %.2e of peak (bound %.2e)" % (n, n // 256 + 1, d, TOL["embed"]))
    assert d <= TOL["embed"]
    assert np.array_equal(enc.embed_mel(enc.mel(x)), got)                                # the stages chain to the same bits


@pytest.mark.parametrize("frames", NETWORK_FRAMES)
def test_network_at_tile_edges(enc, W, frames):
    """The network alone (qasr_xvec_embed_mel) on the float32 log-mel of a well-conditioned clip, one frame below, at and above a tile
    and two tiles plus one: the bound is 10 x the twin's distance on these very rows, not the short clips' worst case."""
    n = 256 * (frames - 1)
    m32 = np.ascontiguousarray(O.mel(O.make_pcm(n, n)), dtype=np.float32)
    got = enc.embed_mel(m32)
    d = rel(got, O.network(m32.astype(np.float64), W))
    print("%d frames: network device vs float64 oracle %.2e of peak (bound %.2e)" % (frames, d, TOL["network"]))
    assert m32.shape == (frames, 128) and got.shape == (1024,) and d <= TOL["network"]


def test_ragged_batch_and_bit_identity(enc, model_dir, W, batch):
    """Five ragged clips through the default handle and through one whose max_samples forces three passes, against the oracle; then a
    clip's rows bit for bit alone, batched, reversed, split, and between neighbours filled with 1e30."""
    clips, mel1, emb1 = batch
    small = SpeakerEncoder.from_pretrained(model_dir, max_samples=THREE_PASSES)
    try:
        runs = [(enc.mel(clips), enc.embed_batch(clips)), (enc.mel(clips[::-1])[::-1], enc.embed_batch(clips[::-1])[::-1]),
                (small.mel(clips), small.embed_batch(clips)), (small.mel(clips[::-1])[::-1], small.embed_batch(clips[::-1])[::-1])]
    finally:
        small.close()
    for name, (ml, em) in zip(("default", "default reversed", "three passes", "three passes reversed"), runs):
        assert em.shape == (len(clips), 1024)
        worst = max(rel(e, O.network(O.mel(p), W)) for p, e in zip(clips, em)) if name in ("default", "three passes") else 0.0
        if worst:
            print("ragged batch, %s: embedding device vs float64 oracle %.2e of peak (bound %.2e)" % (name, worst, TOL["embed"]))
        assert worst <= TOL["embed"]
        for k in range(len(clips)):
            assert ml[k].shape == (BATCH_N[k] // 256 + 1, 128)
            assert np.array_equal(ml[k], mel1[k]) and np.array_equal(em[k], emb1[k]), (name, k)
    for k in range(len(clips)):                            # no tap, halo or reduction reaches across a clip boundary
        loud = [np.full(256 * 70 + 11, 1e30, np.float32), clips[k], np.full(977, 1e30, np.float32)]
        with np.errstate(all="ignore"):
            ml, em = enc.mel(loud)[1], enc.embed_batch(loud)[1]
        assert np.array_equal(ml, mel1[k]) and np.array_equal(em, emb1[k]), k
    assert np.array_equal(enc.embed(clips[2]), emb1[2])                                   # and run to run
    print("bit identity: %d clips alone = batched = reversed = three passes = between 1e30 neighbours" % len(clips))


def test_loader(sd, W, ref, tmp_path_factory):
    n = 256 * 63 + 17
    pcm = O.make_pcm(n, n)
    talker = [("talker.model.layers.0.mlp.weight", np.ones((8, 8), np.float32)), ("talker.codec_head.weight", np.zeros(5, np.float32))]
    m = SpeakerEncoder.from_pretrained(synth.write_tts_speaker_encoder_safetensors(sd, str(tmp_path_factory.mktemp("extra")), extra=talker))
    try:
        assert m.memory_footprint == 4 * sum(v.size for v in sd.values()) and rel(m.embed(pcm), ref[n][1]) <= TOL["embed"]
    finally:
        m.close()
    key = "speaker_encoder.blocks.2.res2net_block.blocks.6.conv.weight"
    for kw, code in ((dict(drop=(key,)), 4), (dict(reshape={key: (64, 64, 3)}), 1)):
        with pytest.raises(QasrError) as ei:
            SpeakerEncoder.from_pretrained(synth.write_tts_speaker_encoder_safetensors(sd, str(tmp_path_factory.mktemp("bad")), **kw))
        assert ("qasr error %d:" % code) in str(ei.value) and key in str(ei.value)
    with pytest.raises(QasrError) as ei:
        SpeakerEncoder.from_pretrained(synth.write_tts_speaker_encoder_safetensors({}, str(tmp_path_factory.mktemp("none")), extra=talker))
    assert "qasr error 4:" in str(ei.value) and "speaker_encoder." in str(ei.value)

    def bf16(a):
        u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
        return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    m = SpeakerEncoder.from_pretrained(synth.write_tts_speaker_encoder_safetensors(sd, str(tmp_path_factory.mktemp("bf16")), dtype="BF16"))
    try:
        want = O.network(ref[n][0], O.Weights({k: bf16(v) for k, v in sd.items()}))
        d = rel(m.embed(pcm), want)
        assert m.memory_footprint == 2 * sum(v.size for v in sd.values())
    finally:
        m.close()
    print("bf16-stored weights, n = %d: embedding %.2e of peak (bound %.2e); rounding moves the float64 result by %.2e"
          % (n, d, TOL["embed"], rel(want, ref[n][1])))
    assert d <= TOL["embed"] and rel(want, ref[n][1]) > 1e-4                              # the rounding is visible
    # the embedding width is fc.weight's
    sd192 = synth.synth_tts_speaker_encoder_state_dict(2, embedding_dim=192)
    m = SpeakerEncoder.from_pretrained(synth.write_tts_speaker_encoder_safetensors(sd192, str(tmp_path_factory.mktemp("e192"))), max_samples=48000)
    try:
        got = m.embed(pcm)
        d = rel(got, O.network(ref[n][0], O.Weights(sd192)))
        assert m.embedding_dim == 192 and got.shape == (192,)
    finally:
        m.close()
    print("E = 192, n = %d: embedding %.2e of peak (bound %.2e)" % (n, d, TOL["embed"]))
    assert d <= TOL["embed"]


def test_lifecycle_and_errors(enc, model_dir):
    pcm = O.make_pcm(7, 256 * 9 + 3)
    want = enc.embed(pcm)
    assert enc.is_loaded and enc.memory_footprint > 0 and enc.embedding_dim == 1024 and enc.sample_rate == 24000
    assert [num_frames(n) for n in (0, 1, 255, 256, 257)] == [0, 1, 1, 2, 2]
    t = enc.timing()
    assert set(t) == {"mel", "conv", "block1", "block2", "block3", "pool"} and all(v > 0 for v in t.values()), t
    lib = _lib.load(strict=True)
    FP = C.POINTER(C.c_float)
    out = np.zeros(1024, np.float32)
    fp, op = pcm.ctypes.data_as(FP), out.ctypes.data_as(FP)
    pp, nn = (FP * 2)(fp, fp), (C.c_size_t * 2)(pcm.size, 0)
    refusals = (lambda: lib.qasr_xvec_embed(enc.h, fp, pcm.size, 16000, op), 7), (lambda: lib.qasr_xvec_embed(enc.h, fp, 0, 24000, op), 6), \
        (lambda: lib.qasr_xvec_embed_batch(enc.h, pp, nn, 2, op), 6), (lambda: lib.qasr_xvec_embed(enc.h, None, pcm.size, 24000, op), 1), \
        (lambda: lib.qasr_xvec_embed(enc.h, fp, pcm.size, 24000, None), 1), (lambda: lib.qasr_xvec_mel(enc.h, pp, nn, 1, None), 1), \
        (lambda: lib.qasr_xvec_embed_mel(enc.h, None, 3, op), 1), (lambda: lib.qasr_xvec_embed_mel(enc.h, fp, 0, op), 6), \
        (lambda: lib.qasr_xvec_embed(None, fp, pcm.size, 24000, op), 1)
    for call, code in refusals:
        assert call() == code
        assert np.array_equal(enc.embed(pcm), want)                                       # the next valid call is right
    assert enc.embed_batch([]).shape == (0, 1024) and enc.mel([]) == []
    m = SpeakerEncoder.from_pretrained(model_dir, max_samples=4000)
    try:
        assert np.array_equal(m.embed(pcm), want)
        for call in (lambda: m.embed(np.zeros(4001, np.float32)), lambda: m.embed_batch([pcm, np.zeros(4001, np.float32)]),
                     lambda: m.mel([np.zeros(4001, np.float32)]), lambda: m.embed_mel(np.zeros((17, 128), np.float32))):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 5:" in str(e.value)
            assert np.array_equal(m.embed(pcm), want)
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        for call in (lambda: m.embed(pcm), lambda: m.embed_batch([pcm]), lambda: m.mel([pcm]), lambda: m.embed_mel(np.zeros((3, 128), np.float32))):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 3:" in str(e.value)
        assert lib.qasr_xvec_embed(m.h, fp, pcm.size, 16000, op) == 3                     # unloaded comes before every other refusal
    finally:
        m.close()
    # order_with an ASR engine: the encoder's work goes on the engine's stream
    from qasr import config as QC
    from qasr.model import Qwen3ASRModel
    asr = Qwen3ASRModel.from_state_dict(synth.synth_state_dict(QC.AUDIO_TINY, QC.TEXT_TINY, seed=3, init="stress"), preset="tiny", device=0,
                                        max_audio_seconds=4, max_new_tokens=8)
    try:
        m = SpeakerEncoder.from_pretrained(model_dir, order_with=asr, max_samples=8000)
        try:
            assert np.array_equal(m.embed(pcm), want)
        finally:
            m.close()
    finally:
        asr.close()

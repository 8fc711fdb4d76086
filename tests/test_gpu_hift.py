"""The CosyVoice3 HiFT vocoder on the MI355X (csrc/voc_cosyvoice.hip, csrc/api_voc.cpp) over the C ABI, against the float64 oracle
tests/hift_oracle.py, with synthetic weights (qasr.synth) on the real geometry (20.8 M parameters).

Tolerances: the reference's own precision is f32.  tests/test_hift_cpu.py::test_f32_distance measures, on these inputs, the max |d|
between the oracle and its torch f32 twin per stage, normalised by the output's peak (the F32 table below).  Each bound is 10 x its
figure (another f32 summation order through a deep chain, as in DESIGN.md sections 13 to 17).  The source has one figure per kind
of F0 track, from a twin whose phase does not drift (cycles, reduced every frame), so that neither a wrong noise counter (0.025 of a
voiced track's peak) nor radians summed in f32 (3e-3) fits under a bound.  The f0 -> phase -> waveform chain is
ill-conditioned over a long clip, so the end-to-end entry is pinned bit for bit to the three stages and each stage to float64 on a
given float32 input: f0 on a mel, source on an F0 track, network (decode_source) on a mel and a source.  Every test prints the
device's distances; DESIGN.md section 21 holds the parity table they fill."""
import ctypes as C

import numpy as np
import pytest

import hift_oracle as O
from qasr import synth, _lib
from qasr.model import QasrError
from qasr.vocoder import HiFTVocoder, num_samples

pytestmark = pytest.mark.gpu

F32 = {"f0": 1.5e-06, "source/voiced": 1.6e-04, "source/unvoiced": 1.5e-07, "source/alternating": 1.0e-04, "source/threshold": 1.3e-04,
       "network": 1.2e-05}
TOL = {k: 10 * v for k, v in F32.items()}
TILE = 64                                              # rows of a GEMM tile (csrc/voc_cosyvoice.h)
# frames 1 .. 5 (shorter than the look-ahead and every causal reach) | T - 1, T, T + 1, 2 T + 1 of the tile
F0_FRAMES = (1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
SOURCE_FRAMES = (1, 2, 65, 130)
SOURCE_SEEDS = (5, 0xC0FFEE1234567)
# 8 frames are 64 rows of the first stage: one tile exactly
DECODE_FRAMES = (1, 2, 3, 5, 8, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 130)
SRC_SEED = 11
BATCH_T = (1, 65, 2, 130, 7)
BATCH_SEEDS = (3, 1 << 63, 0, 0xFFFFFFFFFFFFFFFF, 77)
THREE_PASSES = 130                                     # holds (1, 65, 2) | (130) | (7)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def sd():
    return synth.synth_cosyvoice_hifigan_state_dict(0)


@pytest.fixture(scope="module")
def W(sd):
    return O.Weights(sd)


@pytest.fixture(scope="module")
def model_dir(sd, tmp_path_factory):
    return synth.write_cosyvoice_hifigan_safetensors(sd, str(tmp_path_factory.mktemp("hift")))


@pytest.fixture(scope="module")
def voc(model_dir):
    m = HiFTVocoder.from_pretrained(model_dir, max_frames=512)
    yield m
    m.close()


@pytest.fixture(scope="module")
def network_ref(W):
    """Per T: the mel, the float32 source, the float64 waveform; filled on demand, computed once."""
    cache = {}

    def get(T):
        if T not in cache:
            mel = O.clip_mel(T)
            src = O.source(O.f0(mel, W).astype(np.float32), SRC_SEED, W).astype(np.float32)
            cache[T] = (mel, src, O.decode_source(mel, src, W))
        return cache[T]
    return get


@pytest.fixture(scope="module")
def network_got(voc, network_ref):
    cache = {}

    def get(T):
        if T not in cache:
            mel, src, _ = network_ref(T)
            cache[T] = voc.decode_source(mel, src)
        return cache[T]
    return get


@pytest.fixture(scope="module")
def batch(voc):
    mels = [O.make_mel(40 + i, T) for i, T in enumerate(BATCH_T)]
    return mels, [voc.decode(m, s) for m, s in zip(mels, BATCH_SEEDS)]


@pytest.mark.parametrize("T", F0_FRAMES)
def test_f0_vs_oracle(voc, W, T):
    mel = O.clip_mel(T)
    got = voc.f0(mel)
    want = O.f0(mel, W)
    d = rel(got, want)
    print("T = %d: F0 device vs float64 oracle %.2e of peak (bound %.2e)" % (T, d, TOL["f0"]))
    assert got.shape == (T,) and got.dtype == np.float32 and np.isfinite(got).all() and (got >= 0).all()
    assert d <= TOL["f0"]


@pytest.mark.parametrize("T", SOURCE_FRAMES)
@pytest.mark.parametrize("kind", O.TRACKS)
def test_source_vs_oracle(voc, W, kind, T):
    track = O.f0_track(kind, T)
    outs = []
    for seed in SOURCE_SEEDS:
        got = voc.source(track, seed)
        want = O.source(track, seed, W)
        d = rel(got, want)
        print("%s, T = %d, seed %#x: source device vs float64 oracle %.2e of peak (bound %.2e)" % (kind, T, seed, d, TOL["source/" + kind]))
        assert got.shape == (480 * T,) and got.dtype == np.float32 and np.isfinite(got).all()
        assert d <= TOL["source/" + kind]
        assert np.array_equal(voc.source(track, seed), got)                            # the same seed: the same bits
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1])                                        # another seed: another stream
    if kind == "threshold" and T >= 3:                                                 # 10.0 and 0.0 are unvoiced, the float after 10.0 is not
        assert np.abs(outs[0][:960]).max() < 0.2 and track[0] == 10.0 and track[1] == 0.0 and track[2] > 10.0


@pytest.mark.parametrize("T", DECODE_FRAMES)
def test_decode_source_vs_oracle(network_ref, network_got, T):
    want, got = network_ref(T)[2], network_got(T)
    d = rel(got, want)
    print("T = %d: waveform device vs float64 oracle %.2e of peak (bound %.2e)" % (T, d, TOL["network"]))
    assert got.shape == (480 * T + 16,) == (num_samples(T),) and got.dtype == np.float32 and np.isfinite(got).all()
    assert np.abs(got).max() <= np.float32(0.99) and d <= TOL["network"]


@pytest.mark.parametrize("T", DECODE_FRAMES)
def test_decode_source_edges(network_ref, network_got, T):
    """The first 16 samples (frames 0 .. 3 alone under the window sum, which starts at hann[0]^2 = 0), the first 64 (what the reflected
    row in front of the last stage reaches first) and the last 32 (the untrimmed centre padding and the last frames' window sum), each
    against the oracle on its own."""
    want, got = network_ref(T)[2], network_got(T)
    peak = np.abs(want).max()
    for name, sl in (("first 16", slice(0, 16)), ("first 64 (reflected row)", slice(0, 64)), ("last 32", slice(-32, None))):
        d = float(np.abs(got[sl].astype(np.float64) - want[sl]).max() / peak)
        print("T = %d, %s samples: %.2e of peak (bound %.2e)" % (T, name, d, TOL["network"]))
        assert d <= TOL["network"]
    assert got[0] == 0.0 and want[0] == 0.0                                            # hann[0] = 0 over the clamped window sum


def test_decode_is_the_stages_chained(voc, batch):
    mels, alone = batch
    for mel, seed, pcm in zip(mels, BATCH_SEEDS, alone):
        staged = voc.decode_source(mel, voc.source(voc.f0(mel), seed))
        assert np.array_equal(staged, pcm), mel.shape
        assert not np.array_equal(voc.decode(mel, seed + 1 & 0xFFFFFFFFFFFFFFFF), pcm)
    print("bit identity: decode = decode_source(source(f0)) for T = %s" % (BATCH_T,))


def test_ragged_batch_and_bit_identity(voc, model_dir, W, batch):
    """Five ragged clips with their own seeds through the default handle and through one whose max_frames forces three passes; then a
    clip bit for bit alone, batched, reversed, split, and between loud neighbours."""
    mels, alone = batch
    small = HiFTVocoder.from_pretrained(model_dir, max_frames=THREE_PASSES)
    try:
        runs = [voc.decode_batch(mels, BATCH_SEEDS), voc.decode_batch(mels[::-1], BATCH_SEEDS[::-1])[::-1],
                small.decode_batch(mels, BATCH_SEEDS), small.decode_batch(mels[::-1], BATCH_SEEDS[::-1])[::-1]]
        assert np.array_equal(small.decode(mels[3], BATCH_SEEDS[3]), alone[3])
        with pytest.raises(QasrError) as e:
            small.decode(O.make_mel(1, THREE_PASSES + 1))
        assert "qasr error 1:" in str(e.value) and "max_frames" in str(e.value)
    finally:
        small.close()
    for name, out in zip(("default", "default reversed", "three passes", "three passes reversed"), runs):
        for k in range(len(mels)):
            assert out[k].shape == (480 * BATCH_T[k] + 16,)
            assert np.array_equal(out[k], alone[k]), (name, k)
    for k in range(len(mels)):                             # no look-ahead tap, reflect pad or upsample gather reaches across a clip boundary
        loud = [np.full((9, 80), 30.0, np.float32), mels[k], np.full((3, 80), -30.0, np.float32)]
        seeds = [1, BATCH_SEEDS[k], 2]
        assert np.array_equal(voc.decode_batch(loud, seeds)[1], alone[k]), k
        quiet = [np.zeros((2, 80), np.float32), mels[k], O.make_mel(5, 11)]
        assert np.array_equal(voc.decode_batch(quiet, seeds)[1], alone[k]), k
    assert np.array_equal(voc.decode(mels[1], BATCH_SEEDS[1]), alone[1])                 # and run to run
    print("bit identity: %d clips alone = batched = reversed = three passes = between changed neighbours" % len(mels))


def test_loader(sd, model_dir, tmp_path_factory):
    key = "resblocks.7.convs2.1.weight"
    for kw, code in ((dict(drop=(key,)), 4), (dict(reshape={key: (64, 64, 7)}), 1)):
        with pytest.raises(QasrError) as ei:
            HiFTVocoder.from_pretrained(synth.write_cosyvoice_hifigan_safetensors(sd, str(tmp_path_factory.mktemp("bad")), **kw))
        assert ("qasr error %d:" % code) in str(ei.value) and key in str(ei.value)
    # the keys the reference ignores are not read: without them the same bits, and the footprint counts the tensors read
    read = {k: v for k, v in sd.items() if k in synth.cosyvoice_hifigan_tensor_shapes(ignored=False)}
    assert len(read) < len(sd)
    mel = O.clip_mel(5)
    a = HiFTVocoder.from_pretrained(model_dir, max_frames=8)
    b = HiFTVocoder.from_pretrained(synth.write_cosyvoice_hifigan_safetensors(read, str(tmp_path_factory.mktemp("lean"))), max_frames=8)
    try:
        assert a.memory_footprint == b.memory_footprint == 4 * sum(v.size for v in read.values())
        assert np.array_equal(a.decode(mel, 9), b.decode(mel, 9))
    finally:
        a.close()
        b.close()


def test_lifecycle_and_errors(voc, model_dir):
    mel = O.clip_mel(5)
    want = voc.decode(mel, 4)
    assert voc.is_loaded and voc.memory_footprint > 0 and voc.sample_rate == 24000
    assert [num_samples(T) for T in (0, 1, 2, 500)] == [0, 496, 976, 240016]
    t = voc.timing()
    assert set(t) == {"f0", "source", "stft", "conv_pre", "stage0", "stage1", "stage2_tail"} and all(v > 0 for v in t.values()), t
    voc.f0(mel)
    t = voc.timing()
    assert t["f0"] > 0 and t["stage0"] == 0, t
    lib = _lib.load(strict=True)
    FP = C.POINTER(C.c_float)
    out = np.zeros(480 * 5 + 16, np.float32)
    src = np.zeros(480 * 5, np.float32)
    mp, op, sp = mel.ctypes.data_as(FP), out.ctypes.data_as(FP), src.ctypes.data_as(FP)
    pp, oo = (FP * 2)(mp, mp), (FP * 2)(op, op)
    tt, ss = (C.c_size_t * 2)(5, 0), (C.c_uint64 * 2)(1, 2)
    refusals = (lambda: lib.qasr_hift_decode(voc.h, mp, 0, 4, op), lambda: lib.qasr_hift_decode(voc.h, None, 5, 4, op),
                lambda: lib.qasr_hift_decode(voc.h, mp, 5, 4, None), lambda: lib.qasr_hift_f0(voc.h, mp, 0, op),
                lambda: lib.qasr_hift_f0(voc.h, None, 5, op), lambda: lib.qasr_hift_source(voc.h, sp, 0, 1, op),
                lambda: lib.qasr_hift_source(voc.h, sp, 5, 1, None), lambda: lib.qasr_hift_decode_source(voc.h, mp, 5, None, op),
                lambda: lib.qasr_hift_decode_source(voc.h, mp, 0, sp, op), lambda: lib.qasr_hift_decode_batch(voc.h, pp, tt, ss, 2, oo),
                lambda: lib.qasr_hift_decode_batch(voc.h, pp, tt, None, 1, oo), lambda: lib.qasr_hift_decode(voc.h, mp, 513, 4, op),
                lambda: lib.qasr_hift_decode(None, mp, 5, 4, op))
    for call in refusals:
        assert call() == 1
        assert np.array_equal(voc.decode(mel, 4), want)                                   # the next valid call is right
    assert voc.decode_batch([], []) == []
    m = HiFTVocoder.from_pretrained(model_dir, max_frames=8)
    try:
        assert np.array_equal(m.decode(mel, 4), want)
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        for call in (lambda: m.decode(mel, 4), lambda: m.f0(mel), lambda: m.source(np.ones(5, np.float32), 1),
                     lambda: m.decode_source(mel, src), lambda: m.decode_batch([mel], [1])):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 3:" in str(e.value)
        assert lib.qasr_hift_decode(m.h, mp, 0, 4, op) == 3                               # unloaded comes before every other refusal
    finally:
        m.close()
    # order_with an ASR engine: the vocoder's work goes on the engine's stream
    from qasr import config as QC
    from qasr.model import Qwen3ASRModel
    asr = Qwen3ASRModel.from_state_dict(synth.synth_state_dict(QC.AUDIO_TINY, QC.TEXT_TINY, seed=3, init="stress"), preset="tiny", device=0,
                                        max_audio_seconds=4, max_new_tokens=8)
    try:
        m = HiFTVocoder.from_pretrained(model_dir, order_with=asr, max_frames=8)
        try:
            assert np.array_equal(m.decode(mel, 4), want)
        finally:
            m.close()
    finally:
        asr.close()

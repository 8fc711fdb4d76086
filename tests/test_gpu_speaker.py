"""WeSpeaker ResNet34 speaker embeddings on the MI355X (csrc/spk_wespeaker.hip, csrc/spk_conv.h) over the C ABI, against the float64
restatement in tests/wespeaker_oracle.py.

Tolerances: the front end is f32 (accurate logf, sums of <= 257 terms): a log-mel value moves by ~1e-6 except where the power is tiny
next to the frame's energy, where f32 cancellation in the FFT shows up in the log.  The network rounds its MFMA operands to bf16
(DEVICE policy in the oracle); the unrounded REFERENCE sits a little further away.  The synthetic weights keep 8 different clips at
pairwise cosine <= 0.9 (test_speaker_cpu.py), so these bounds are not met by chance.
Measured on an MI355X: fbank |d| <= 2.2e-4; embeddings cosine >= 0.99997 against DEVICE and >= 0.99996 against REFERENCE (max |d|
2.0e-3), every clip of 0.5 .. 12 s.  The device follows the DEVICE policy no more closely than DEVICE follows REFERENCE
(1 - cos 1.2e-5 .. 3.4e-5 on the oracle side), presumably because bf16 rounding flips from the f32 accumulation order grow through the 33
layers.  Bounds: fbank 1e-3 (the issue's), DEVICE 0.9999 (the issue's; ~3x margin), REFERENCE 0.9995 (~10x margin on 1 - cos).
Bit-identity between a batch and single calls is a self-consistency check of the packing, not parity."""
import ctypes as C
import numpy as np
import pytest
import torch

import wespeaker_oracle as O
from qasr import _lib, synth, config as QC
from qasr.model import Qwen3ASRModel, QasrError
from qasr.speaker import WeSpeakerModel, cosine_similarity

pytestmark = pytest.mark.gpu

TOL_FBANK, COS_DEVICE, COS_REF = 1e-3, 0.9999, 0.9995


@pytest.fixture(scope="module")
def sd():
    return synth.synth_wespeaker_state_dict(0)


@pytest.fixture(scope="module")
def W_dev(sd):
    return O.Weights(sd, O.DEVICE)


@pytest.fixture(scope="module")
def W_ref(sd):
    return O.Weights(sd, O.REFERENCE)


@pytest.fixture(scope="module")
def model_dir(sd, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wespeaker"))
    synth.write_wespeaker_safetensors(sd, d)
    return d


@pytest.fixture(scope="module")
def spk(model_dir):
    m = WeSpeakerModel.from_pretrained(model_dir)
    yield m
    m.close()


def _clip(seed, seconds):
    """speech-like: the synthetic waveform with a level that changes every 0.25 s and a short pause"""
    n = int(round(seconds * 16000))
    x = synth.synth_waveform(seed, seconds).astype(np.float64)
    rng = np.random.default_rng(seed)
    x *= np.repeat(rng.uniform(0.2, 1.0, n // 4000 + 1), 4000)[:n]
    return x.astype(np.float32)


def _cos(a, b):
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def _noisy(seed, n):
    """noise with a tone on top: every mel band well above the f32 FFT's rounding floor"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000
    return (0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * (180 + 50 * seed) * t)).astype(np.float32)


def test_fbank_matches_oracle(spk):
    """Lengths 1, 199, 8 000, 160 000 and a clip with digital silence in the middle, in one call.  The clips are noisy on purpose: in a
    deep spectral null of a purely tonal frame (a mel band 1e-8 below the frame's peak) the f32 FFT, the reference's own precision,
    parts from float64 by a few 1e-3 in the log."""
    mid = _noisy(4, 32000)
    mid[8000:20000] = 0.0                                              # digital silence in the middle
    clips = [np.array([0.3], np.float32), _noisy(2, 199), _noisy(1, 8000), _noisy(3, 160000), mid]
    got = spk.fbank(clips)
    worst = 0.0
    for x, g in zip(clips, got):
        want = O.fbank(x)
        assert g.shape == want.shape
        worst = max(worst, float(np.abs(g - want).max()))
    print("fbank max |d| %.2e" % worst)
    assert worst <= TOL_FBANK
    assert np.array_equal(spk.fbank(clips[3]), got[3])                 # alone == in a batch


def test_embeddings_match_oracle(spk, W_dev, W_ref):
    clips = [_clip(10, 0.5), _clip(11, 1.3), _clip(12, 4.0), _clip(13, 12.0),
             np.random.default_rng(7).uniform(-0.5, 0.5, 16000).astype(np.float32)]
    worst_dev, worst_ref, dmax = 1.0, 1.0, 0.0
    for x in clips:
        g = spk.embed(x)
        assert abs(float(np.linalg.norm(g)) - 1.0) < 1e-5
        d, r = O.embed(x, W_dev), O.embed(x, W_ref)
        worst_dev, worst_ref = min(worst_dev, _cos(g, d)), min(worst_ref, _cos(g, r))
        dmax = max(dmax, float(np.abs(g - r).max()))
    print("cos vs DEVICE %.7f, vs REFERENCE %.7f, max |d| vs REFERENCE %.2e" % (worst_dev, worst_ref, dmax))
    assert worst_dev >= COS_DEVICE and worst_ref >= COS_REF


def test_ragged_batch_bit_identical(spk, W_dev):
    rng = np.random.default_rng(11)
    secs = rng.uniform(0.5, 10.0, 64)
    secs[:3] = (0.5, 0.73, 1.1)
    clips = [_clip(100 + k, float(s)) for k, s in enumerate(secs)]
    order = rng.permutation(64)
    got = spk.embed_batch([clips[k] for k in order])
    batch = np.empty_like(got)
    batch[order] = got
    ms = spk.timing()
    single = np.stack([spk.embed(c) for c in clips])
    assert np.array_equal(batch, single)
    again = spk.embed_batch([clips[k] for k in order])
    assert np.array_equal(again, got)
    for k in range(3):
        assert _cos(batch[k], O.embed(clips[k], W_dev)) >= COS_DEVICE
    print("64 ragged clips (%.0f s): %.2f ms device" % (secs.sum(), ms))


def test_split_capacity_and_errors(model_dir, spk):
    clips = [_clip(200 + k, 1.0 + 0.1 * k) for k in range(7)]
    small = WeSpeakerModel.from_pretrained(model_dir, max_batch_samples=40000)
    try:
        got = small.embed_batch(clips)                                 # 7 clips, ~ 2.5 passes of 40 000 samples
        assert np.array_equal(got, spk.embed_batch(clips))
        with pytest.raises(QasrError, match="qasr error 5"):
            small.embed(np.zeros(40001, np.float32))
        assert small.embed(np.full(40000, 0.01, np.float32)).shape == (256,)
        with pytest.raises(QasrError, match="qasr error 7"):
            small.embed(clips[0], sample_rate=8000)
        with pytest.raises(QasrError, match="qasr error 6"):
            small.embed(np.zeros(0, np.float32))
        with pytest.raises(QasrError, match="qasr error 6"):
            small.embed_batch([clips[0], np.zeros(0, np.float32)])
        assert small.is_loaded and small.memory_footprint == sum(v.size for v in synth.synth_wespeaker_state_dict(0).values()) * 4
        small.unload()
        assert not small.is_loaded and small.memory_footprint == 0
        with pytest.raises(QasrError, match="qasr error 3"):
            small.embed(clips[0])
    finally:
        small.close()
    segs = spk.embed_segments(np.concatenate(clips[:3]), [(0.0, 1.0), (1.0, 2.1)])
    assert np.array_equal(segs, spk.embed_batch([clips[0], clips[1]]))
    assert abs(cosine_similarity(segs[0], segs[0]) - 1.0) < 1e-6


def test_checkpoint_dtypes(sd, tmp_path):
    """The same values (rounded to bf16, and kept only where f16 holds them exactly) written as F32, F16 and BF16 give bit-identical
    embeddings."""
    def exact(v):
        b = torch.as_tensor(v).to(torch.bfloat16).to(torch.float32)
        h = b.to(torch.float16).to(torch.float32)
        return torch.where(h == b, b, torch.zeros_like(b)).numpy()
    sdr = {k: exact(v) for k, v in sd.items()}
    clips = [_clip(300, 1.7), _clip(301, 0.6)]
    out = {}
    for dtype in ("F32", "F16", "BF16"):
        d = str(tmp_path / dtype)
        synth.write_wespeaker_safetensors(sdr, d, dtype=dtype)
        m = WeSpeakerModel.from_pretrained(d, max_batch_samples=16000 * 4)
        try:
            out[dtype] = m.embed_batch(clips)
            assert m.memory_footprint == sum(v.size for v in sdr.values()) * (4 if dtype == "F32" else 2)
        finally:
            m.close()
    assert np.array_equal(out["F32"], out["F16"]) and np.array_equal(out["F32"], out["BF16"])


@pytest.fixture(scope="module")
def asr():
    sd = synth.synth_state_dict(QC.AUDIO_TINY, QC.TEXT_TINY, seed=3, init="stress")
    m = Qwen3ASRModel.from_state_dict(sd, preset="tiny", max_audio_seconds=10, max_new_tokens=32)
    yield m
    m.close()


def test_sharing_an_engine(asr, model_dir):
    """A speaker model ordered on an (unmarked) engine's stream: transcribe_batch tokens are identical with and without embed_batch calls
    between the batches, and no call fails."""
    clips = [synth.synth_waveform(k, 1.0 + 0.3 * k) for k in range(4)]
    base = [asr.transcribe_batch(clips, max_tokens=8, ignore_eos=True) for _ in range(2)]
    m = WeSpeakerModel.from_pretrained(model_dir, order_with=asr, max_batch_samples=16000 * 40)
    try:
        got, embs = [], []
        for r in range(2):
            embs.append(m.embed_batch([_clip(400 + k, 0.5 + k) for k in range(6)]))
            got.append(asr.transcribe_batch(clips, max_tokens=8, ignore_eos=True))
            embs.append(m.embed_batch([_clip(400 + k, 0.5 + k) for k in range(6)]))
    finally:
        m.close()
    assert got == base
    assert all(np.array_equal(e, embs[0]) for e in embs)

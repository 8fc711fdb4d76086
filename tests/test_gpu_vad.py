"""Silero VAD v5 on the MI355X (csrc/vad_silero.hip) over the C ABI, against the float64 restatement in tests/silero_oracle.py.

Tolerances: the device runs the reference's f32 arithmetic (accurate expf / tanhf / sqrtf, fmaf chains in a fixed order); the oracle is
float64.  A probability passes through ~1.2 k-term f32 sums (relative rounding ~1e-7 each, growing as sqrt of the chain length over the
layers) and a sigmoid whose slope is <= 1/4, so |dp| stays a few 1e-7; h and c carry the same error and accumulate it over the
recurrence (|f| < 1 damps it), a few 1e-6 after hundreds of chunks.  Measured on an MI355X: |dp| <= 1.1e-7 and |dh|, |dc| <= 3.1e-6
(ticks of 1 / 7 / 64 streams, and whole buffers up to 47.3 s); the bounds below keep a ~10x margin over that (down from a first
2e-5 / 5e-5).
Bit-identity between ticks and whole buffers is a self-consistency check, not parity."""
import ctypes as C
import numpy as np
import pytest

import silero_oracle as O
from qasr import _lib, synth, config as QC
from qasr.model import Qwen3ASRModel, QasrError
from qasr.vad import SileroVADModel, binarize
from qasr import streaming as S

pytestmark = pytest.mark.gpu

TOL_P, TOL_S = 1e-6, 3e-5


@pytest.fixture(scope="module")
def sd():
    return synth.synth_silero_state_dict(0)


@pytest.fixture(scope="module")
def W(sd):
    return O.Weights(sd)


@pytest.fixture(scope="module")
def model_dir(sd, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("silero"))
    synth.write_silero_safetensors(sd, d)
    return d


@pytest.fixture(scope="module")
def vad(model_dir):
    v = SileroVADModel.from_pretrained(model_dir, max_streams=64)
    yield v
    v.close()


def _audio(seed, n):
    """noise whose level changes every few chunks (graded probabilities) with tones on top in places"""
    rng = np.random.default_rng(seed)
    amp = np.repeat(rng.choice([0.0, 0.001, 0.003, 0.01, 0.05], size=n // 1536 + 1), 1536)[:n]
    x = amp * rng.standard_normal(n)
    t = np.arange(n) / 16000
    x += np.where(rng.random(n // 4000 + 1).repeat(4000)[:n] > 0.6, 0.3 * np.sin(2 * np.pi * (200 + 40 * seed) * t), 0.0)
    return x.astype(np.float32)


def _speechy(seed, seconds):
    rng = np.random.default_rng(seed)
    parts, total = [], 0
    while total < seconds * 16000:
        parts += [np.zeros(int(rng.uniform(0.3, 0.9) * 16000), np.float32), synth.synth_waveform(seed * 10 + len(parts), rng.uniform(0.4, 1.5))]
        total += parts[-1].shape[0] + parts[-2].shape[0]
    return np.concatenate(parts)[:int(seconds * 16000)]


def test_ticks_match_oracle(vad, W):
    """processChunk of 1, 7 and 64 streams per call, fed interleaved in shuffled order, streams reset at different chunks: probability
    and h, c, context after every chunk vs the oracle; each stream bit-identical to the same stream fed alone."""
    rng = np.random.default_rng(1)
    worst = [0.0, 0.0]
    for S_ in (1, 7, 64):
        T = 5
        audio = {s: _audio(100 + s, T * 512) for s in range(S_)}
        ref = {s: O.Stream(W) for s in range(S_)}
        vad.reset_state(-1)
        got = {s: [] for s in range(S_)}
        for t in range(T):
            for s in range(S_):
                if t > 0 and (s + t) % 4 == 0:                        # resets at different chunks
                    vad.reset_state(s)
                    ref[s].reset()
                    got[s].append(None)
            order = rng.permutation(S_)
            chunks = np.stack([audio[s][t * 512:(t + 1) * 512] for s in order])
            p = vad.process_chunks(chunks, order)
            for k, s in enumerate(order):
                want = ref[s].process_chunk(chunks[k])
                got[s].append(float(p[k]))
                worst[0] = max(worst[0], abs(float(p[k]) - want))
                h, c, ctx = vad.state(int(s))
                worst[1] = max(worst[1], float(np.abs(h - ref[s].h).max()), float(np.abs(c - ref[s].c).max()))
                assert np.array_equal(ctx, chunks[k][-64:])
        assert worst[0] <= TOL_P and worst[1] <= TOL_S, (S_, worst)
        # the same streams alone (B = 1, another slot): bit-identical
        for s in range(min(S_, 3)):
            vad.reset_state(63)
            alone = []
            for t in range(T):
                if t > 0 and (s + t) % 4 == 0:
                    vad.reset_state(63)
                    alone.append(None)
                alone.append(float(vad.process_chunks(audio[s][t * 512:(t + 1) * 512][None], [63])[0]))
            assert alone == got[s], s
    print("ticks: max |dp| %.2e, max |dh|,|dc| %.2e" % tuple(worst))


def test_whole_buffers_match_oracle(vad, W):
    """qasr_vad_probs on ragged rows (0, 1, 511, 512, 513, 16 000 samples, 30 s, 47.3 s) vs the oracle, final state included."""
    ns = [0, 1, 511, 512, 513, 16000, 480000, 756800]
    rows = [_audio(200 + i, n) for i, n in enumerate(ns)]
    got = vad.probs(rows)
    want, st = O.probs_rows(W, rows)
    dp = ds = 0.0
    for b, n in enumerate(ns):
        assert got[b].shape == (-(-n // 512),)
        if n:
            dp = max(dp, float(np.abs(got[b] - want[b]).max()))
        h, c, ctx = vad.state(b)
        ds = max(ds, float(np.abs(h - st[b][0]).max()), float(np.abs(c - st[b][1]).max()))
        assert np.array_equal(ctx, st[b][2]), b
    print("whole buffers: max |dp| %.2e, max |dh|,|dc| %.2e" % (dp, ds))
    assert dp <= TOL_P and ds <= TOL_S


def test_ticks_and_buffer_bit_identical(vad):
    """Self-consistency: one buffer through qasr_vad_probs and the same chunks (last one zero-padded) through qasr_vad_process."""
    x = _audio(7, 16000 * 3 + 300)
    whole = vad.probs([x], stream_ids=[3])[0]
    hw, cw, xw = vad.state(3)
    vad.reset_state(5)
    padded = np.zeros(len(whole) * 512, np.float32)
    padded[:x.shape[0]] = x
    ticks = np.array([vad.process_chunks(padded[i * 512:(i + 1) * 512][None], [5])[0] for i in range(len(whole))], np.float32)
    ht, ct, xt = vad.state(5)
    assert np.array_equal(ticks, whole)
    assert np.array_equal(hw, ht) and np.array_equal(cw, ct) and np.array_equal(xw, xt)


def _clear_of_thresholds(p, cfg=S.VADConfig()):
    return float(np.min(np.abs(np.concatenate([p - cfg.onset, p - cfg.offset])))) > 1e-3


def test_detect_speech(vad, W):
    """qasr_vad_detect_speech == binarize(oracle probabilities) on bursts of synthetic speech with silence between (a seed whose oracle
    probabilities keep 1e-3 away from both thresholds, so that f32 noise cannot move a boundary)."""
    for seed in range(1, 40):
        x = _speechy(seed, 9.0)
        p = O.probs_rows(W, [x])[0][0]
        if _clear_of_thresholds(p):
            break
    else:
        pytest.fail("no seed keeps the oracle probabilities 1e-3 from the thresholds")
    want = O.binarize(p)
    got = vad.detect_speech(x, 16000)
    assert len(want) >= 3
    assert [(s.start_time, s.end_time) for s in got] == want
    assert binarize(p.astype(np.float32)) == got
    assert vad.detect_speech(np.zeros(0, np.float32), 16000) == []
    with pytest.raises(QasrError):
        vad.detect_speech(x, 8000)


@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_load_from_disk(sd, tmp_path, dtype):
    """model.safetensors with the reference's key names in f32 and in f16 (widened to f32 on load)."""
    synth.write_silero_safetensors(sd, str(tmp_path), dtype=dtype)
    sd2 = {k: (v.astype(np.float16).astype(np.float32) if dtype == "F16" else v) for k, v in sd.items()}
    x = _audio(9, 16000)
    v = SileroVADModel.from_pretrained(str(tmp_path), max_streams=2)
    try:
        got = v.probs([x])[0]
    finally:
        v.close()
    want = O.probs_rows(O.Weights(sd2), [x])[0][0]
    assert np.abs(got - want).max() <= TOL_P


def test_vtable(vad):
    """sc_vad_vtable_t: process_chunk / reset through the function pointers == qasr_vad_process on another stream."""
    vt = vad.vtable(9)
    assert vt.input_sample_rate(vt.context) == 16000 and vt.chunk_size(vt.context) == 512
    vt.reset(vt.context)
    vad.reset_state(10)
    x = _audio(11, 512 * 4)
    for i in range(4):
        ch = np.ascontiguousarray(x[i * 512:(i + 1) * 512])
        a = vt.process_chunk(vt.context, ch.ctypes.data_as(C.POINTER(C.c_float)), 512)
        b = float(vad.process_chunks(ch[None], [10])[0])
        assert a == b
    assert vt.process_chunk(vt.context, x.ctypes.data_as(C.POINTER(C.c_float)), 100) == 0.0     # wrong length: 0, message set


@pytest.fixture(scope="module")
def asr():
    from oracle import tokenizer as otok
    sd = synth.synth_state_dict(QC.AUDIO_TINY, QC.TEXT_TINY, seed=3, init="stress")
    m = Qwen3ASRModel.from_state_dict(sd, preset="tiny", max_audio_seconds=10, max_new_tokens=32)
    b2u = otok.byte_to_unicode()
    m.set_vocab({b: b2u[b] for b in range(256)})
    yield m
    m.close()


def test_streaming_asr_end_to_end(asr, vad, W):
    """StreamingASR with the device VAD: transcribe_stream (chunk by chunk), transcribe_stream_batched (one qasr_vad_probs),
    transcribe_streams_batched (many buffers) give the same segments and texts, and those of the flow driven by the oracle VAD."""
    cfg = S.StreamingASRConfig(max_tokens=5, max_segment_duration=2.5)
    audios = []
    for seed in range(1, 60):
        x = _speechy(seed, 6.0)
        if _clear_of_thresholds(O.probs_rows(W, [x])[0][0]):
            audios.append(x)
        if len(audios) == 2:
            break
    assert len(audios) == 2
    st = S.StreamingASR.with_vad(asr, vad)
    seqs = [list(st.transcribe_stream(a, config=cfg)) for a in audios]
    bats = [st.transcribe_stream_batched(a, config=cfg) for a in audios]
    many = st.transcribe_streams_batched(audios, config=cfg)
    assert bats == seqs and many == seqs
    assert all(len(s) >= 2 for s in seqs)
    for a, seq in zip(audios, seqs):
        ref = O.Stream(W)
        oracle_flow = list(S.StreamingASR(asr, ref.process_chunk, ref.reset).transcribe_stream(a, config=cfg))
        assert oracle_flow == seq


def test_sharing_an_engine(asr, model_dir):
    """A VAD ordered on the engine's stream: transcribe_batch tokens are identical with and without VAD ticks and whole-buffer passes
    issued between the batches."""
    clips = [synth.synth_waveform(k, 1.0 + 0.3 * k) for k in range(4)]
    base = [asr.transcribe_batch(clips, max_tokens=8, ignore_eos=True) for _ in range(2)]
    v = SileroVADModel.from_pretrained(model_dir, max_streams=8, order_with=asr)
    try:
        got = []
        for r in range(2):
            v.process_chunks(np.stack([_audio(k, 512) for k in range(8)]))
            v.probs([_audio(20 + r, 16000 * 5)] * 1)
            got.append(asr.transcribe_batch(clips, max_tokens=8, ignore_eos=True))
            v.process_chunks(np.stack([_audio(k + 8, 512) for k in range(8)]))
    finally:
        v.close()
    assert got == base


def test_scale_32_streams_30s(vad, W):
    """32 x 30 s in one qasr_vad_probs call; rows 0, 13 and 31 vs the oracle."""
    rows = [_audio(300 + k, 480000) for k in range(32)]
    got = vad.probs(rows)
    ms, graph = vad.timing()
    want = O.probs_rows(W, [rows[0], rows[13], rows[31]])[0]
    for w, b in zip(want, (0, 13, 31)):
        assert np.abs(got[b] - w).max() <= TOL_P, b
    print("32 x 30 s: %.3f ms device" % ms)

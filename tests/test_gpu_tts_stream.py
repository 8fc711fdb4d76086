"""Qwen3-TTS streaming synthesis on the MI355X: the stream pool qasr_tts_pool_* (csrc/api_tts.cpp, csrc/tts_talker.hip; DESIGN.md
section 20) over the small4 Talker of tests/talker_cases.py and the reduced codec with 2048-entry codebooks.

Everything here is bit equality, so there is no tolerance: a stream's chunk list is qasr_tts_stream_chunks of its length, its codes are
qasr_tts_generate of the same request alone, and a chunk's samples are the tail of qasr_codec_forward on [zero pad | context | chunk].
References come from the one-shot calls while no pool is open (a pool owns the handle's rows)."""
import ctypes as C

import numpy as np
import pytest

import talker_cases as K
import tts_stream_cases as S
from qasr import _lib, synth, tts
from qasr.codec import SpeechTokenizerDecoder
from qasr.model import QasrError

pytestmark = pytest.mark.gpu
T = K.TOKENS
POLL = 8
MAX_FRAMES = 32
SPF = 1920


class Net:
    def __init__(self, tmp, max_batch, model_dir=None):
        self.g = K.GEOMETRIES["small4"]
        self.dir = model_dir or synth.write_tts_talker_safetensors(synth.synth_tts_talker_state_dict(self.g, 0), str(tmp.mktemp("small4")))
        cfg = tts.default_config("0.6B", 4, **{k: v for k, v in self.g.items() if k != "bits"})
        cfg.bits = self.g["bits"]
        self.m = tts.Qwen3TTSModel.from_pretrained(self.dir, cfg, max_batch=max_batch, max_frames=MAX_FRAMES, max_text=64,
                                                   max_instruct=K.MAX_INSTRUCT)
        self.rows = K.make_rows(17, self.g["hidden"])

    def args(self, i):
        r = self.rows[i]
        return dict(text=r["text"], language=r["language"], speaker=r.get("speaker"), xvector=r.get("xvector"), instruct=r.get("instruct"))

    def alone(self, i, sampling, seed, row_index):
        """qasr_tts_generate of row i alone: the codes a stream of the same request must give."""
        a = self.args(i)
        return self.m.generate_codes([a["text"]], [a["language"]], sampling, seed, [a["speaker"]], [a["xvector"]], [a["instruct"]], [row_index])[0]


@pytest.fixture(scope="module")
def net(tmp_path_factory):
    n = Net(tmp_path_factory, 4)
    yield n
    n.m.close()


@pytest.fixture(scope="module")
def codec_dir(tmp_path_factory):
    geo = dict(synth.CODEC_REDUCED, semantic_codebook_size=2048, acoustic_codebook_size=2048)
    return synth.write_speech_tokenizer_safetensors(synth.synth_speech_tokenizer_state_dict(0, geo), str(tmp_path_factory.mktemp("codec")), geo)


@pytest.fixture(scope="module")
def codec(codec_dir):
    c = SpeechTokenizerDecoder.from_pretrained(codec_dir)
    yield c
    c.close()


@pytest.fixture(params=(1, 0), ids=("tail_rows", "whole_windows"))
def tail_rows(request):
    """Both values of the knob codec_tail_rows: the vocoder skips the rows only a chunk's dropped context needs | whole windows."""
    lib, old = _lib.load(), C.c_int()
    assert lib.qasr_get_tuning(b"codec_tail_rows", C.byref(old)) == 0 and old.value in (0, 1)
    assert lib.qasr_set_tuning(b"codec_tail_rows", request.param) == 0
    yield request.param
    assert lib.qasr_set_tuning(b"codec_tail_rows", old.value) == 0


def drain(pool, got=None):
    got = {} if got is None else got
    while pool.live:
        chunks = pool.step()
        assert chunks                                                       # a step returns nothing only when no stream is live
        for c in chunks:
            got.setdefault(c.stream, []).append(c)
    assert pool.step() == []
    return got


def check_stream(codec, chunks, ref, cfg, cap):
    """chunks of one stream against generate (ref [16, n]) + the chunk rule + the codec on each chunk's window."""
    n = ref.shape[1]
    spans = [(c.frame_index, c.codes.shape[1], c.is_final) for c in chunks]
    assert spans == tts.stream_chunks(n, n < cap, tts.StreamingConfig(*cfg)), (spans, n, cfg)
    assert np.array_equal(np.concatenate([c.codes for c in chunks], axis=1), ref)
    for c in chunks:
        f = c.codes.shape[1]
        assert c.samples.dtype == np.float32 and c.samples.shape == (SPF * f,)
        if f:
            want = codec.forward(S.window_codes(ref, c.frame_index, f, cfg[2]))[-SPF * f:]
            assert np.array_equal(c.samples, want), (c.frame_index, f)


def same_chunks(a, b):
    return len(a) == len(b) and all(x.frame_index == y.frame_index and x.is_final == y.is_final and np.array_equal(x.codes, y.codes) and
                                    np.array_equal(x.samples, y.samples) for x, y in zip(a, b))


def stream_alone(net, codec, i, cfg, sampling, seed, row_index):
    with tts.TtsStreamPool(net.m, codec, sampling, seed) as pool:
        s = pool.open(config=tts.StreamingConfig(*cfg), row_index=row_index, **net.args(i))
        return drain(pool)[s]


@pytest.mark.parametrize("cfg", ((2, 5, 3), (3, 25, 10)))
def test_one_stream_equals_generate_plus_codec(net, codec, cfg, tail_rows):
    s = tts.SamplingConfig(max_tokens=24)
    ref = net.alone(2, s, 7, 55)
    assert ref.shape[1] > cfg[0]                                            # more than the first chunk
    chunks = stream_alone(net, codec, 2, cfg, s, 7, 55)
    check_stream(codec, chunks, ref, cfg, 24)
    if cfg[0] == 2:
        assert S.window_codes(ref, 0, 2, 3).shape == (16, 4) and not S.window_codes(ref, 0, 2, 3)[:, :2].any()      # the zero pad ran
    # the generator over a pool of one
    a = net.args(2)
    gen = list(net.m.synthesize_stream(codec, a["text"], a["language"], s, tts.StreamingConfig(*cfg), 7, a["speaker"], a["xvector"],
                                       a["instruct"], 55))
    assert same_chunks(gen, chunks) and gen[-1].is_final
    assert np.array_equal(net.alone(2, s, 7, 55), ref)                      # the pool is gone: the one-shot call is back, same bits


def eos_bias(net, idx):
    """an EOS bias under which streams end at different frames, as test_rows_finish_at_different_frames of test_gpu_talker.py finds it"""
    a = [net.args(i) for i in idx]
    codes = K.forced_codes(len(idx), 1)
    logits = net.m.forced([x["text"] for x in a], [x["language"] for x in a], codes, [x["speaker"] for x in a], [x["xvector"] for x in a],
                          [x["instruct"] for x in a], want=("talker",))["talker"][:, 0]
    return float(np.median([(l[:2048].max() - l[T["codec_eos"]]) / 0.9 for l in logits]))


def test_admission_at_different_frames(net, codec_dir, tail_rows):
    codec2 = SpeechTokenizerDecoder.from_pretrained(codec_dir, max_windows=2)      # three due windows split into two passes
    try:
        idx, cfgs, ridx = (0, 5, 11), ((2, 5, 3), (1, 4, 2), (3, 25, 10)), (200, 205, 211)
        # the scenario needs streams that end at different frames, one of them by EOS, and an A that outlives its first two steps: half the
        # EOS bias that lets EOS win every other frame, seed 4 (23, 20 and 16 frames with the synthetic weights of seed 0)
        seed = 4
        s = tts.SamplingConfig(eos_logit_bias=0.5 * eos_bias(net, idx), max_tokens=24)
        refs = [net.alone(i, s, seed, r) for i, r in zip(idx, ridx)]
        lens = [r.shape[1] for r in refs]
        print("frames per stream", lens)
        assert len(set(lens)) >= 2 and min(lens) < 24 and lens[0] > 7      # the precondition of the scenario, not the check
        alone = [stream_alone(net, codec2, i, c, s, seed, r) for i, c, r in zip(idx, cfgs, ridx)]
        with tts.TtsStreamPool(net.m, codec2, s, seed) as pool:
            a = pool.open(config=tts.StreamingConfig(*cfgs[0]), row_index=ridx[0], **net.args(idx[0]))
            got = {a: pool.step() + pool.step()}
            assert [c.frame_index for c in got[a]] == [0, 2] and pool.live == 1
            b = pool.open(config=tts.StreamingConfig(*cfgs[1]), row_index=ridx[1], **net.args(idx[1]))
            c = pool.open(config=tts.StreamingConfig(*cfgs[2]), row_index=ridx[2], **net.args(idx[2]))
            assert len({a, b, c}) == 3 and pool.live == 3
            drain(pool, got)
        for j, sid in enumerate((a, b, c)):
            check_stream(codec2, got[sid], refs[j], cfgs[j], 24)
            assert same_chunks(got[sid], alone[j]), j
    finally:
        codec2.close()


def test_slots(net, codec, tmp_path_factory, tail_rows):
    two = Net(tmp_path_factory, 2, net.dir)
    try:
        s, cfg = tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=10), (2, 5, 3)
        refs = {i: two.alone(i, s, 0, i) for i in (1, 2, 3)}
        assert all(r.shape[1] == 10 for r in refs.values())                 # greedy rows that run into max_tokens
        sc = tts.StreamingConfig(*cfg)
        with tts.TtsStreamPool(two.m, codec, s, 0) as pool:
            assert pool.step() == [] and pool.live == 0                     # an empty pool
            s1 = pool.open(config=sc, row_index=1, **two.args(1))
            got = {1: pool.step() + pool.step()}                            # stream 1 at 7 frames when stream 2 joins
            s2 = pool.open(config=sc, row_index=2, **two.args(2))
            with pytest.raises(QasrError) as e:
                pool.open(config=sc, row_index=3, **two.args(3))
            assert "qasr error 5" in str(e.value) and "no free slot" in str(e.value)
            got[2] = []
            while not (got[1] and got[1][-1].is_final):
                for c in pool.step():
                    got[1 if c.stream == s1 else 2].append(c)
            assert pool.live == 1 and not (got[2] and got[2][-1].is_final)
            s3 = pool.open(config=sc, row_index=3, **two.args(3))           # the slot of the finished stream
            assert s3 == s1
            got[3] = []
            while pool.live:
                for c in pool.step():
                    got[2 if c.stream == s2 else 3].append(c)
        for i in (1, 2, 3):
            check_stream(codec, got[i], refs[i], cfg, 10)
        # close in mid-run frees the slot and leaves the other stream's bits alone
        with tts.TtsStreamPool(two.m, codec, s, 0) as pool:
            s1 = pool.open(config=sc, row_index=1, **two.args(1))
            s2 = pool.open(config=sc, row_index=2, **two.args(2))
            first = pool.step()
            assert sorted(c.stream for c in first) == sorted((s1, s2))
            pool.close(s1)
            assert pool.live == 1
            s3 = pool.open(config=sc, row_index=3, **two.args(3))           # a stream that joins in the closed one's slot
            assert s3 == s1
            got = drain(pool, {s2: [c for c in first if c.stream == s2]})
            check_stream(codec, got[s2], refs[2], cfg, 10)
            check_stream(codec, got[s3], refs[3], cfg, 10)
            with pytest.raises(QasrError, match="outside the pool"):
                pool.close(2)
    finally:
        two.m.close()


def test_edges(net, codec, tail_rows):
    # EOS as the first token: one empty final chunk at frame 0
    chunks = stream_alone(net, codec, 3, (3, 25, 10), tts.SamplingConfig(eos_logit_bias=1e4, max_tokens=5), 0, 0)
    assert [(c.frame_index, c.codes.shape, c.samples.shape, c.is_final) for c in chunks] == [(0, (16, 0), (0,), True)]
    greedy = lambda n: tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=n)
    long = net.alone(3, greedy(POLL + 1), 0, 0)
    assert long.shape == (16, POLL + 1)
    # max_tokens on a boundary: that chunk is final, nothing behind it; max_tokens = 1
    for n, cfg, want in ((7, (2, 5, 3), [(0, 2, False), (2, 5, True)]), (1, (1, 15, 10), [(0, 1, True)]), (1, (3, 25, 10), [(0, 1, True)]),
                         # one run of frames that crosses the poll interval; the same with the boundary behind max_tokens
                         (POLL + 1, (POLL + 1, 5, 0), [(0, POLL + 1, True)]), (POLL + 1, (10, 10, 0), [(0, POLL + 1, True)]),
                         (POLL + 1, (1, POLL, 4), [(0, 1, False), (1, POLL, True)])):
        chunks = stream_alone(net, codec, 3, cfg, greedy(n), 0, 0)
        assert [(c.frame_index, c.codes.shape[1], c.is_final) for c in chunks] == want, (n, cfg)
        check_stream(codec, chunks, long[:, :n], cfg, n)


def test_refusals(net, codec):
    a = net.args(0)
    s = tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=6)
    base = net.alone(0, s, 0, 0)
    with pytest.raises(QasrError) as e:
        tts.TtsStreamPool(net.m, codec, tts.SamplingConfig(top_p=0.9))
    assert "qasr error 7" in str(e.value) and "top_p" in str(e.value)
    assert np.array_equal(net.alone(0, s, 0, 0), base)                      # no pool was made
    two_rows = net.m._request([a["text"]] * 2, [a["language"]] * 2, None, None, None, None)
    ok = dict(text=a["text"], language=a["language"])
    cases = [
        (dict(ok, config=tts.StreamingConfig(0, 25, 10)), "qasr error 1", "first_chunk_frames"),
        (dict(ok, config=tts.StreamingConfig(3, 0, 10)), "qasr error 1", "chunk_frames"),
        (dict(ok, config=tts.StreamingConfig(3, 25, -1)), "qasr error 1", "decoder_left_context"),
        (dict(ok, config=tts.StreamingConfig(36, 25, 10)), "qasr error 7", "first_chunk_frames"),
        (dict(ok, config=tts.StreamingConfig(3, 26, 10)), "qasr error 7", "decoder_left_context + chunk_frames"),
        (dict(ok, config=tts.StreamingConfig(1, 35, 1)), "qasr error 7", "noChunking"),
        (dict(ok, _request=two_rows), "qasr error 1", "B must be 1"),
        (dict(text=[1, 2, 3, 4, 5, 6, 7, 8], language=2050), "qasr error 1", "shorter than the 9 template tokens"),
        (dict(text=[1, 2, 3, 4, 5, 6, 7, 8, 512], language=2050), "qasr error 1", "outside the text vocabulary"),
        (dict(text=a["text"], language=3072), "qasr error 1", "outside the codec vocabulary"),
        (dict(text=a["text"], language=2050, instruct=[600]), "qasr error 1", "outside the text vocabulary"),
        (dict(text=list(range(1, 70)), language=2050), "qasr error 5", "max_text"),
    ]
    with tts.TtsStreamPool(net.m, codec, s) as pool:
        for kw, code, word in cases:
            with pytest.raises(QasrError) as e:
                pool.open(**kw)
            assert code in str(e.value) and word in str(e.value), (str(e.value), word)
            assert pool.live == 0
        for call in (lambda: net.alone(0, s, 0, 0), lambda: net.m.forced([a["text"]], [a["language"]], np.zeros((1, 16, 2), dtype=np.int32)),
                     lambda: net.m.synthesize(codec, a["text"], a["language"], s), lambda: tts.TtsStreamPool(net.m, codec, s)):
            with pytest.raises(QasrError) as e:
                call()
            assert "qasr error 1" in str(e.value) and "stream pool" in str(e.value), str(e.value)
        sid = pool.open(config=tts.StreamingConfig(2, 5, 3), **net.args(0))  # the pool stayed usable through all of it
        check_stream(codec, drain(pool)[sid], base, (2, 5, 3), 6)
    assert np.array_equal(net.alone(0, s, 0, 0), base)                      # after destroy: the same bits as before


@pytest.mark.parametrize("T,context", ((35, 10), (25, 10), (13, 3), (11, 10), (35, 34), (4, 0), (1, 0)))
def test_forward_tail_equals_the_tail_of_forward(codec, tail_rows, T, context):
    rng = np.random.default_rng(100 * T + context)
    codes = rng.integers(0, 2048, (3, 16, T)).astype(np.int32)
    want = codec.forward(codes)[:, SPF * context:]
    codec.forward(rng.integers(0, 2048, (3, 16, T)).astype(np.int32))        # the dead rows hold another call's data
    got = codec.forward_tail(codes, context)
    assert got.shape == (3, SPF * (T - context)) and np.array_equal(got, want)
    if T == 35:                                                              # windows of different lengths in one pass: a shorter call first
        codec.forward(codes[:, :, :20])
        assert np.array_equal(codec.forward_tail(codes, context, clip=False), codec.forward(codes, clip=False)[:, SPF * context:])


def test_forward_tail_refusals(codec):
    lib = _lib.load()
    codes = np.zeros((1, 16, 36), dtype=np.int32)
    out = np.zeros(SPF * 36, dtype=np.float32)
    ip, fp = codes.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_float))
    for B, T, ctx, word in ((1, 36, 0, b"1..35 frames"), (1, 0, 0, b"1..35 frames"), (1, 10, 10, b"context shorter than the window"),
                            (1, 10, 11, b"context shorter than the window"), (0, 10, 0, b"windows")):
        assert lib.qasr_codec_forward_tail(codec.h, ip, B, T, ctx, 1, fp) == 1, (B, T, ctx)
        assert word in lib.qasr_codec_last_error(codec.h), (B, T, ctx)
    assert lib.qasr_codec_forward_tail(codec.h, None, 1, 10, 3, 1, fp) == 1 and lib.qasr_codec_forward_tail(codec.h, ip, 1, 10, 3, 1, None) == 1
    codes[0, 3, 2] = 2048
    assert lib.qasr_codec_forward_tail(codec.h, ip, 1, 10, 3, 1, fp) == 1 and b"outside" in lib.qasr_codec_last_error(codec.h)
    with pytest.raises(QasrError, match="shorter than the window"):
        codec.forward_tail(np.zeros((16, 5), dtype=np.int32), 5)
    ok = np.zeros((16, 5), dtype=np.int32)
    assert np.array_equal(codec.forward_tail(ok, 2), codec.forward(ok)[SPF * 2:])      # the handle stays usable

"""The pure-CPU side of Qwen3-TTS streaming (include/qasr.h): qasr_tts_stream_chunks, the chunks a stream is cut
into, against the reference's loop restated in tests/tts_stream_cases.py and against cases written out by hand; qasr_codec_tail_leads,
the rows of a window each vocoder stage needs before the first kept one, against leads measured on tests/codec_oracle.py."""
import ctypes as C

import numpy as np
import pytest

import codec_oracle as O
import tts_stream_cases as S
from qasr import _lib, codec, synth, tts
from qasr.model import QasrError


@pytest.mark.parametrize("cfg", S.CONFIGS)
def test_chunks_equal_the_reference_loop(cfg):
    sc = tts.StreamingConfig(*cfg)
    for n in range(0, 61):
        for eos in (True, False):
            if n == 0 and not eos:
                continue                                                    # a stream that stops at max_tokens holds at least one frame
            got = tts.stream_chunks(n, eos, sc)
            if (n, eos, cfg[0]) == (1, False, 1):
                # the one departure (include/qasr.h): at safeMaxTokens = 1 the reference yields the frame non-final and an empty final chunk
                # behind it; a stream that stops at max_tokens ends with its last chunk here
                assert S.reference_chunks(n, eos, cfg[0], cfg[1]) == [(0, 1, False), (1, 0, True)] and got == [(0, 1, True)]
            else:
                assert got == S.reference_chunks(n, eos, cfg[0], cfg[1]), (cfg, n, eos)
            # the chunks tile the frames, only the last is final, only an EOS sentinel is empty
            assert [c[0] for c in got] == [sum(x[1] for x in got[:i]) for i in range(len(got))]
            assert sum(c[1] for c in got) == n and [c[2] for c in got] == [False] * (len(got) - 1) + [True]
            assert all(c[1] > 0 for c in got[:-1]) and (got[-1][1] > 0 or eos)


def test_cases_that_have_bitten():
    d, ll = tts.StreamingConfig.default(), tts.StreamingConfig.low_latency()
    assert (d.first_chunk_frames, d.chunk_frames, d.decoder_left_context) == (3, 25, 10)
    assert (ll.first_chunk_frames, ll.chunk_frames, ll.decoder_left_context) == (1, 15, 10)
    # EOS as the first token: one empty final chunk at frame 0
    assert tts.stream_chunks(0, True, d) == [(0, 0, True)]
    assert tts.stream_chunks(0, True, ll) == [(0, 0, True)]
    # EOS on the frame after a boundary: the boundary's chunk went out non-final, an empty final chunk follows
    assert tts.stream_chunks(3, True, d) == [(0, 3, False), (3, 0, True)]
    assert tts.stream_chunks(28, True, d) == [(0, 3, False), (3, 25, False), (28, 0, True)]
    assert tts.stream_chunks(16, True, ll) == [(0, 1, False), (1, 15, False), (16, 0, True)]
    # EOS inside a chunk: the rest is the final chunk
    assert tts.stream_chunks(30, True, d) == [(0, 3, False), (3, 25, False), (28, 2, True)]
    assert tts.stream_chunks(2, True, d) == [(0, 2, True)]
    # the cap exactly on a boundary: that chunk is final, no sentinel
    assert tts.stream_chunks(3, False, d) == [(0, 3, True)]
    assert tts.stream_chunks(28, False, d) == [(0, 3, False), (3, 25, True)]
    assert tts.stream_chunks(29, False, d) == [(0, 3, False), (3, 25, False), (28, 1, True)]
    # max_tokens = 1
    assert tts.stream_chunks(1, False, d) == [(0, 1, True)]
    assert tts.stream_chunks(1, False, ll) == [(0, 1, True)]
    assert tts.stream_chunks(1, True, ll) == [(0, 1, False), (1, 0, True)]


def test_presets_and_refusals():
    lib = _lib.load()
    sc = _lib.QasrTtsStreamConfig()
    lib.qasr_tts_default_stream_config(0, C.byref(sc))
    assert (sc.first_chunk_frames, sc.chunk_frames, sc.decoder_left_context) == (3, 25, 10)
    lib.qasr_tts_default_stream_config(1, C.byref(sc))
    assert (sc.first_chunk_frames, sc.chunk_frames, sc.decoder_left_context) == (1, 15, 10)
    for bad in (tts.StreamingConfig(0, 25, 10), tts.StreamingConfig(3, 0, 10)):
        with pytest.raises(QasrError, match="qasr error 1"):
            tts.stream_chunks(5, True, bad)
    with pytest.raises(QasrError, match="qasr error 1"):
        tts.stream_chunks(-1, True)
    with pytest.raises(QasrError, match="qasr error 1"):
        tts.stream_chunks(0, False)
    a = (C.c_int32 * 1)()
    sc = tts.StreamingConfig.default().c_struct()
    assert lib.qasr_tts_stream_chunks(30, 1, C.byref(sc), a, a, a, 1) == -5                 # QASR_ERR_CAPACITY
    assert lib.qasr_tts_stream_chunks(30, 1, C.byref(sc), None, None, None, 8) == 3
    assert lib.qasr_tts_stream_chunks(30, 1, None, None, None, None, 8) == -1


def test_tail_leads_of_the_real_rates():
    assert codec.tail_leads((8, 5, 4, 3)) == [20, 14, 23, 28, 29, 6]
    assert codec.tail_leads() == [20, 14, 23, 28, 29, 6]
    for bad in ((0, 5, 4, 3), (8, 5, 4, 65)):
        with pytest.raises(QasrError, match="qasr error 1"):
            codec.tail_leads(bad)
    assert _lib.load().qasr_codec_tail_leads(None, None) == 1


@pytest.mark.parametrize("rates,T,context", (((8, 5, 4, 3), 8, 6), ((2, 3, 7, 4), 18, 16)))
def test_tail_leads_equal_the_oracle_dependency(rates, T, context):
    """Per stage: the lead is the minimum found by bisection, so poisoning one row more (one row fewer than the lead left real) reaches
    a kept sample, and poisoning everything before the lead does not.  The contexts are long enough that no lead is clamped."""
    g = dict(O.REDUCED, upsample_rates=rates)
    geo = dict(synth.CODEC_REDUCED, upsample_rates=rates)
    W = O.Weights(synth.synth_speech_tokenizer_state_dict(0, geo), np.float64)
    leads = codec.tail_leads(rates)
    for stage in range(6):
        rate, _ = S.stage_rate_and_channels(stage, g)
        assert leads[stage] <= context * rate, (stage, "the case clamps this lead")
        assert S.measured_lead(stage, T, context, W, g) == leads[stage], stage
        assert not S.poisoned_reaches_kept(stage, context * rate - leads[stage], T, context, W, g, seed=1)
        assert S.poisoned_reaches_kept(stage, context * rate - leads[stage] + 1, T, context, W, g, seed=1)

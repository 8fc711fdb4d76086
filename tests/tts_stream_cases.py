"""What the Qwen3-TTS streaming tests share (tests/test_tts_stream_cpu.py, tests/test_gpu_tts_stream.py): the reference's chunking loop
restated in Python, and the codes of the window a chunk is decoded in."""
import numpy as np

import codec_oracle as O

CONFIGS = ((3, 25, 10), (1, 15, 10), (1, 1, 0), (35, 35, 0), (4, 7, 3))     # (first_chunk_frames, chunk_frames, decoder_left_context)
MIN_DECODE_FRAMES = 4                                                       # decodeAndEmitChunk: zero frames in front of shorter windows


def reference_chunks(n_frames, ended_by_eos, first, chunk):
    """runStreamingGeneration (Qwen3TTS.swift:329-552) with the networks taken out: the stream yields n_frames frames and then EOS
    (ended_by_eos) or runs into safeMaxTokens = n_frames.  Returns [(frame_index, n_frames, is_final)] in the order of the yields.

    Nothing here is taken from the library: where the two differ (safeMaxTokens = 1 with firstChunkFrames = 1, see
    tests/test_tts_stream_cpu.py) the test says so."""
    out = []
    if ended_by_eos and n_frames == 0:                                      # the first token is EOS
        return [(0, 0, True)]
    safe_max = n_frames + 1 if ended_by_eos else n_frames                   # EOS is sampled in iteration n_frames
    assert n_frames >= 1
    total, emitted, emitted_final, threshold = 1, 0, False, first           # the prompt pass gave frame 0
    if total >= threshold:
        out.append((0, total, False))
        emitted, threshold = total, total + chunk
    for it in range(1, safe_max):
        is_eos = ended_by_eos and it == n_frames
        if not is_eos:
            total += 1
        last = it == safe_max - 1
        if (is_eos or total >= threshold or last) and total > emitted:
            final = is_eos or last
            out.append((emitted, total - emitted, final))
            emitted_final = emitted_final or final
            emitted, threshold = total, total + chunk
        if is_eos:
            break
    if emitted < total:
        out.append((emitted, total - emitted, True))
        emitted_final = True
    if not emitted_final:
        out.append((emitted, 0, True))                                      # EOS arrived with no new frame: the sentinel
    return out


def window_codes(codes, frame_index, n_frames, left_context):
    """decodeAndEmitChunk's input: [zero pad | context | chunk] of codes [16, T], and the chunk's samples are the window's last
    1920 * n_frames."""
    start = max(frame_index - left_context, 0)
    w = np.ascontiguousarray(codes[:, start:frame_index + n_frames], dtype=np.int32)
    pad = max(MIN_DECODE_FRAMES - w.shape[1], 0)
    return np.concatenate([np.zeros((codes.shape[0], pad), dtype=np.int32), w], axis=1)


# ---- the vocoder's leads, measured on the oracle (tests/codec_oracle.py) by NaN poisoning ------------------------------------------
def stage_rate_and_channels(stage, g):
    """Stage 0: the input of decoder.decoder.0; 1 .. 4: the inputs of blocks 1 .. 4; 5: the input of the output conv."""
    rate = int(np.prod(g["upsampling_ratios"]))
    if stage == 0:
        return rate, g["latent_dim"]
    for s in g["upsample_rates"][:stage - 1]:
        rate *= s
    return rate, g["decoder_dim"] >> (stage - 1)


def vocoder_from(stage, h, W, g):
    """The oracle's vocoder from the input of `stage` on: [T x rate, C] -> the waveform before the clip."""
    if stage == 0:
        h = O.causal_conv(h, W["decoder.decoder.0.conv.weight"], W["decoder.decoder.0.conv.bias"])
    for i, s in enumerate(g["upsample_rates"]):
        if i + 1 >= max(stage, 1):
            h = O.decoder_block(h, W, "decoder.decoder.%d" % (i + 1), s)
    h = O.snake_beta(h, W["decoder.decoder.5.alpha"], W["decoder.decoder.5.beta"])
    return O.causal_conv(h, W["decoder.decoder.6.conv.weight"], W["decoder.decoder.6.conv.bias"])[:, 0]


def poisoned_reaches_kept(stage, dead_rows, T, context, W, g, seed=0):
    """NaN in the first dead_rows rows of the stage's input of a T-frame window: does any sample from frame `context` on see it?"""
    rate, C = stage_rate_and_channels(stage, g)
    x = np.random.default_rng(seed).standard_normal((T * rate, C))
    x[:dead_rows] = np.nan
    spf = int(np.prod(g["upsampling_ratios"])) * int(np.prod(g["upsample_rates"]))
    with np.errstate(invalid="ignore"):
        wave = vocoder_from(stage, x, W, g)
    assert wave.shape == (T * spf,)
    return bool(np.isnan(wave[context * spf:]).any())


def measured_lead(stage, T, context, W, g):
    """The fewest input rows before the first kept one that must be real: by bisection over the number of poisoned rows."""
    rate, _ = stage_rate_and_channels(stage, g)
    lo, hi = 0, context * rate + 1                     # lo rows poisoned: clean; hi rows poisoned: the first kept row itself is NaN
    assert not poisoned_reaches_kept(stage, lo, T, context, W, g) and poisoned_reaches_kept(stage, hi, T, context, W, g)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if poisoned_reaches_kept(stage, mid, T, context, W, g):
            hi = mid
        else:
            lo = mid
    return context * rate - lo

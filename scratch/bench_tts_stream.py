#!/usr/bin/env python3
"""Qwen3-TTS streaming on one MI355X: synthetic weights on the real codec geometry and the real 0.6B Talker geometry (MLX 4 bit).

Part 1, the default of the tuning knob codec_tail_rows.  Per window shape (T 35 / context 10, T 25 / context 10) and window count
(1, 8, 32): device milliseconds (qasr_codec_timing, HIP events on the work stream, summed over the stages) of
  forward   qasr_codec_forward on the same windows -- the parent's path for a streamed chunk
  tail_1    qasr_codec_forward_tail with codec_tail_rows = 1 (the vocoder skips the rows only the dropped context needs)
  tail_0    qasr_codec_forward_tail with codec_tail_rows = 0 (whole windows; differs from `forward` in the bytes copied back)
The three alternate in blocks, every block starts with untimed calls; the figure is the median over the timed calls, the spread their
min .. max.  tail_1 decides the default only if its median at T 35 / context 10 is below forward's by more than both spreads.

Part 2, the pool, for the record: open -> first chunk of one stream (split by qasr_tts_pool_timing into admission, frames, codec), the
steady-state step (25 frames + a 35-frame window per stream) and audio seconds per wall second at 1, 8, 32 and 64 live streams, and the
stall one admission puts on the running streams.  Host clock around calls that end in a stream synchronise.

Writes profiles/tts_stream.json and prints it as one JSON line.

usage: python scratch/bench_tts_stream.py [--windows 1,8,32] [--streams 1,8,32,64] [--calls 10] [--small] [--part 1|2|12]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
import numpy as np  # noqa: E402
from qasr import synth, tts, _lib  # noqa: E402
from qasr.codec import SpeechTokenizerDecoder  # noqa: E402

BLOCKS, WARM = 2, 2
SHAPES = ((35, 10), (25, 10))
TEXT = 30


def stats(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls": len(t)}


def bench_codec(codec, lib, windows, calls, out):
    rng = np.random.default_rng(0)
    per = max(calls // BLOCKS, 1)
    for T, ctx in SHAPES:
        for W in windows:
            codes = rng.integers(0, 2048, (W, 16, T)).astype(np.int32)
            times = {"forward": [], "tail_1": [], "tail_0": []}
            for _ in range(BLOCKS):
                for name in times:
                    if name != "forward":
                        assert lib.qasr_set_tuning(b"codec_tail_rows", int(name[-1])) == 0
                    for r in range(WARM + per):
                        codec.forward(codes) if name == "forward" else codec.forward_tail(codes, ctx)
                        if r >= WARM:
                            times[name].append(sum(codec.timing().values()))
            same = bool(np.array_equal(codec.forward_tail(codes, ctx), codec.forward(codes)[:, 1920 * ctx:]))
            row = {"T": T, "context": ctx, "windows": W, "bit_equal": same}
            row.update({k: stats(v) for k, v in times.items()})
            row["speedup"] = row["forward"]["median_ms"] / row["tail_1"]["median_ms"]
            row["beyond_spread"] = row["tail_1"]["max_ms"] < row["forward"]["min_ms"]
            out["codec"].append(row)
            print(json.dumps(row), flush=True)
    lead = [r for r in out["codec"] if (r["T"], r["context"]) == SHAPES[0]]
    out["codec_tail_rows_default"] = 1 if lead and all(r["beyond_spread"] for r in lead) else 0


def bench_pool(m, codec, streams, repeats, out):
    rng = np.random.default_rng(1)
    text = lambda: [1, 2, 3] + [int(v) for v in rng.integers(4, 400, TEXT)] + [5, 6, 7, 8, 9]
    s = tts.SamplingConfig(eos_logit_bias=-1e4, max_tokens=3 + 25 + 25)
    for N in streams:
        first, steady, stall, split = [], [], [], []
        for rep in range(repeats + 1):                                     # the first repeat is untimed (graph capture, allocations)
            with tts.TtsStreamPool(m, codec, s, seed=rep) as pool:         # one stream joins N - 1 running ones
                for i in range(N - 1):
                    pool.open(text(), 2050, row_index=i)
                if N > 1:
                    pool.step()                                             # N - 1 streams at 3 frames
                pool.open(text(), 2050, row_index=N - 1)
                t0 = time.perf_counter()
                pool.step()                                                 # admission of one stream among N - 1 running + its 3 frames
                dt = time.perf_counter() - t0
                tm = pool.timing()
                if rep:
                    stall.append(tm["admission"])
                    if N == 1:
                        first.append(1e3 * dt)
                        split.append(tm)
            with tts.TtsStreamPool(m, codec, s, seed=rep) as pool:         # N streams in step: 3 frames, 25 frames, then the steady step
                for i in range(N):
                    pool.open(text(), 2050, row_index=i)
                pool.step()
                pool.step()
                t0 = time.perf_counter()
                chunks = pool.step()                                        # 25 frames of N streams + N windows of 10 + 25 frames
                d2 = time.perf_counter() - t0
                assert len(chunks) == N and all(c.codes.shape[1] == 25 and c.frame_index == 28 for c in chunks)
                if rep:
                    steady.append(1e3 * d2)
        row = {"streams": N, "admission_stall": stats(stall)}
        if steady:
            row["steady_step"] = stats(steady)
            row["audio_s_per_wall_s"] = N * 25 * 0.08 / (1e-3 * row["steady_step"]["median_ms"])
        if first:
            row["open_to_first_chunk"] = stats(first)
            row["first_chunk_split_ms"] = {k: statistics.median(t[k] for t in split) for k in split[0]}
        out["pool"].append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="1,8,32")
    ap.add_argument("--streams", default="1,8,32,64")
    ap.add_argument("--calls", type=int, default=10, help="timed calls per variant and shape")
    ap.add_argument("--repeats", type=int, default=3, help="timed pool runs per stream count")
    ap.add_argument("--small", action="store_true", help="the reduced test geometries (a quick check of the script)")
    ap.add_argument("--part", default="12")
    a = ap.parse_args()
    windows, streams = [int(v) for v in a.windows.split(",")], [int(v) for v in a.streams.split(",")]
    lib = _lib.load(strict=True)
    cgeo = dict(synth.CODEC_REDUCED, semantic_codebook_size=2048, acoustic_codebook_size=2048) if a.small else None
    out = {"geometry": "small" if a.small else "0.6B, real codec", "bits": 4, "codec": [], "pool": []}
    path = os.path.join(ROOT, "profiles", "tts_stream.json")
    if os.path.exists(path) and a.part != "12":                             # the two parts may run as two calls
        old = json.load(open(path))
        out.update({k: old[k] for k in ("codec", "pool", "codec_tail_rows_default") if k in old})
    with tempfile.TemporaryDirectory() as d:
        synth.write_speech_tokenizer_safetensors(synth.synth_speech_tokenizer_state_dict(0, cgeo), d, cgeo)
        codec = SpeechTokenizerDecoder.from_pretrained(d, max_windows=max(windows + streams))
    try:
        if "1" in a.part:
            out["codec"] = []
            bench_codec(codec, lib, windows, a.calls, out)
        if "2" in a.part:
            out["pool"] = []
            geo = dict(synth.TTS_TALKER_SMALL if a.small else synth.TTS_TALKER_REAL, bits=4)
            if not a.small:
                geo.update(text_vocab=4096, tts_pad=4093, tts_bos=4094, tts_eos=4095)
            with tempfile.TemporaryDirectory() as d:
                synth.write_tts_talker_safetensors(synth.synth_tts_talker_state_dict(geo, 0), d)
                cfg = tts.default_config("0.6B", 4, **{k: v for k, v in geo.items() if k != "bits"})
                cfg.bits = 4
                m = tts.Qwen3TTSModel.from_pretrained(d, cfg, max_batch=max(streams), max_frames=64, max_text=64)
            try:
                bench_pool(m, codec, streams, a.repeats, out)
            finally:
                m.close()
    finally:
        codec.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

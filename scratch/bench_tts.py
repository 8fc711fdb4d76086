#!/usr/bin/env python3
"""Qwen3-TTS Talker + code predictor frame rate on one MI355X: synthetic weights on the real 0.6B geometry (MLX 4 bit unless --bits 8),
EOS suppressed through a large negative eos_logit_bias, 125 frames (10 s of audio) per row at B = 1, 8 and 32.  The timed region is
qasr_tts_generate: prompt pass, frames, codes in host memory.  Writes profiles/tts_bench.json and prints it as one JSON line.

usage: python scratch/bench_tts.py [--bits 4] [--frames 125] [--batches 1,8,32] [--reps 3] [--small]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
import numpy as np  # noqa: E402
from qasr import synth, tts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="the reduced test geometry (a quick check of the script)")
    a = ap.parse_args()
    # the text vocabulary is cut to 4096 rows: the table is only gathered from, its size does not enter a frame
    geo = dict(synth.TTS_TALKER_SMALL if a.small else synth.TTS_TALKER_REAL, bits=a.bits)
    if not a.small:
        geo.update(text_vocab=4096, tts_pad=4093, tts_bos=4094, tts_eos=4095)
    batches = [int(b) for b in a.batches.split(",")]
    with tempfile.TemporaryDirectory() as d:
        synth.write_tts_talker_safetensors(synth.synth_tts_talker_state_dict(geo, 0), d)
        cfg = tts.default_config("0.6B", 4, **{k: v for k, v in geo.items() if k != "bits"})
        cfg.bits = a.bits
        m = tts.Qwen3TTSModel.from_pretrained(d, cfg, max_batch=max(batches), max_frames=a.frames, max_text=64)
    rng = np.random.default_rng(0)
    s = tts.SamplingConfig(eos_logit_bias=-1e4, max_tokens=a.frames)
    out = {"geometry": "small" if a.small else "0.6B", "bits": a.bits, "frames": a.frames, "device_bytes": m.device_bytes, "rows": []}
    try:
        for B in batches:
            texts = [[1, 2, 3] + [int(v) for v in rng.integers(4, 400, 30)] + [5, 6, 7, 8, 9] for _ in range(B)]
            m.generate_codes(texts, 2050, s, seed=1)                      # captures the frame's graph for this batch size
            times = []
            for r in range(a.reps):
                t0 = time.perf_counter()
                codes = m.generate_codes(texts, 2050, s, seed=2 + r)
                times.append(time.perf_counter() - t0)
                assert all(c.shape == (16, a.frames) for c in codes)
            best = min(times)
            out["rows"].append({"B": B, "seconds": best, "ms_per_frame": 1e3 * best / a.frames,
                                "audio_seconds_per_second": B * a.frames / 12.5 / best, "all_seconds": times})
    finally:
        m.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tts_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Times the Qwen3-TTS speech tokenizer encoder (qasr.codec.SpeechTokenizerEncoder) on the device with synthetic weights at the real
geometry and writes profiles/codec_enc_bench.json: 1 x 10 s, 1 x 30 s, 32 x 10 s, with the per-stage HIP-event times of
qasr_codec_enc_timing and the wall time.  Nothing gates on these figures.

    python scratch/bench_codec_enc.py [--max-samples 0] [--repeats 3] [--out profiles/codec_enc_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
from qasr import synth                                                   # noqa: E402
from qasr.codec import SpeechTokenizerEncoder                            # noqa: E402


def pcm(seed, seconds):
    rng = np.random.default_rng(seed)
    t = np.arange(int(24000 * seconds)) / 24000.0
    return (0.4 * np.sin(2 * np.pi * rng.uniform(100, 2000) * t) + 0.1 * rng.standard_normal(t.size)).astype(np.float32)


def timed(fn, repeats):
    fn()                                                                 # warm-up: code object load
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        if best is None or wall < best:
            best = wall
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-samples", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_enc_bench.json"))
    a = ap.parse_args()
    sd = synth.synth_speech_tokenizer_encoder_state_dict(1, synth.CODEC_REAL)
    with tempfile.TemporaryDirectory() as d:
        m = SpeechTokenizerEncoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, d), max_samples=a.max_samples)
    out = {"geometry": "real", "max_samples": a.max_samples or 720000, "weights": "synthetic (qasr.synth seed 1)", "cases": {}}
    try:
        for name, items in (("1x10s", [pcm(0, 10)]), ("1x30s", [pcm(1, 30)]), ("32x10s", [pcm(10 + i, 10) for i in range(32)])):
            wall = timed(lambda: m.encode_batch(items), a.repeats if len(items) < 32 else 1)
            st = m.timing()
            out["cases"][name] = {"wall_ms": round(wall, 3), "device_ms": round(sum(st.values()), 3),
                                  "stage_ms": {k: round(v, 3) for k, v in st.items()},
                                  "audio_seconds": sum(c.size for c in items) / 24000.0}
            print(name, json.dumps(out["cases"][name]), flush=True)
    finally:
        m.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

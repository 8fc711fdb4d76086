"""Times the Qwen3-TTS speech tokenizer decoder (qasr.codec) on the device with synthetic weights at the real geometry and writes
profiles/codec_bench.json: one 35-frame window, 1 x 30 s, 32 x 30 s (375 frames each, 480 windows), with the per-stage HIP-event times
of qasr_codec_timing.  Nothing gates on these figures.

    python scratch/bench_codec.py [--max-windows 64] [--repeats 3] [--out profiles/codec_bench.json]
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
from qasr.codec import SpeechTokenizerDecoder                            # noqa: E402


def codes(seed, T, g):
    rng = np.random.default_rng(seed)
    return rng.integers(0, g["acoustic_codebook_size"], size=(g["num_quantizers"], T)).astype(np.int32)


def timed(fn, repeats):
    fn()                                                                 # warm-up: workspace allocation, code object load
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
    ap.add_argument("--max-windows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_bench.json"))
    a = ap.parse_args()
    g = synth.CODEC_REAL
    sd = synth.synth_speech_tokenizer_state_dict(1, g)
    with tempfile.TemporaryDirectory() as d:
        m = SpeechTokenizerDecoder.from_pretrained(synth.write_speech_tokenizer_safetensors(sd, d), max_windows=a.max_windows)
    out = {"geometry": "real", "max_windows": a.max_windows, "weights": "synthetic (qasr.synth seed 1)", "cases": {}}
    try:
        for name, items in (("one_window_35_frames", [codes(0, 35, g)]), ("1x30s", [codes(1, 375, g)]),
                            ("32x30s", [codes(10 + i, 375, g) for i in range(32)])):
            wall = timed(lambda: m.decode_batch(items), a.repeats if len(items) < 32 else 1)
            st = m.timing()
            out["cases"][name] = {"wall_ms": round(wall, 3), "device_ms": round(sum(st.values()), 3),
                                  "stage_ms": {k: round(v, 3) for k, v in st.items()},
                                  "audio_seconds": sum(c.shape[1] for c in items) / 12.5}
            print(name, json.dumps(out["cases"][name]), flush=True)
    finally:
        m.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Times the Qwen3-TTS speaker encoder (qasr.tts_speaker.SpeakerEncoder) on the device with synthetic weights and writes
profiles/xvec_bench.json: 1 x 10 s and 64 x 10 s, device time from the HIP events of qasr_xvec_timing (per stage and summed), warm,
the median of --runs runs, with the estimates of DESIGN.md section 17 (written before the first timed run) beside them.  Nothing gates
on these figures.

    python scratch/bench_xvec.py [--runs 20] [--out profiles/xvec_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
from qasr import synth                                                   # noqa: E402
from qasr.tts_speaker import SpeakerEncoder, STAGES                      # noqa: E402

ESTIMATE_MS = {"1x10s": 0.45, "64x10s": 17.0}                            # DESIGN.md section 17, before measurement


def pcm(seed, seconds):
    rng = np.random.default_rng(seed)
    t = np.arange(int(24000 * seconds)) / 24000.0
    return (0.1 * np.sin(2 * np.pi * rng.uniform(100, 2000) * t) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xvec_bench.json"))
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("at least 20 runs")
    sd = synth.synth_tts_speaker_encoder_state_dict(1)
    with tempfile.TemporaryDirectory() as d:
        m = SpeakerEncoder.from_pretrained(synth.write_tts_speaker_encoder_safetensors(sd, d))
    out = {"weights": "synthetic (qasr.synth seed 1)", "runs": a.runs, "timer": "HIP events on the work stream (qasr_xvec_timing)", "cases": {}}
    try:
        for name, items in (("1x10s", [pcm(0, 10)]), ("64x10s", [pcm(10 + i, 10) for i in range(64)])):
            for _ in range(3):                                           # warm: code objects loaded, buffers touched
                m.embed_batch(items)
            runs = []
            for _ in range(a.runs):
                m.embed_batch(items)
                runs.append(m.timing())
            total = [sum(r.values()) for r in runs]
            out["cases"][name] = {"device_ms_median": round(statistics.median(total), 4), "device_ms_min": round(min(total), 4),
                                  "device_ms_max": round(max(total), 4), "estimate_ms": ESTIMATE_MS[name],
                                  "stage_ms_median": {k: round(statistics.median(r[k] for r in runs), 4) for k in STAGES},
                                  "audio_seconds": sum(c.size for c in items) / 24000.0}
            print(name, json.dumps(out["cases"][name]), flush=True)
    finally:
        m.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

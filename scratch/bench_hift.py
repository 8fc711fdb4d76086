"""Times the CosyVoice3 HiFT vocoder (qasr.vocoder.HiFTVocoder) on the device with synthetic weights and writes profiles/hift_bench.json:
--clips clips of --frames mel frames each in one decode_batch call (default 32 x 500, 10 s of audio each), device time from the HIP
events of qasr_hift_timing (per stage and summed), warm, the median of --runs runs; audio seconds per second and the achieved f32
FLOP/s against the algorithmic count below (2 x multiply-adds of every conv and Linear, from the shapes; activations, transforms and
the source are left out: under 1 %).  Nothing gates on these figures.

    python scratch/bench_hift.py [--clips 32] [--frames 500] [--runs 5] [--out profiles/hift_bench.json]
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
from qasr.vocoder import HiFTVocoder, STAGES                             # noqa: E402


def flops_per_frame():
    """Algorithmic FLOPs of one mel frame (a clip of T frames: T times this, plus one row of the last stage), per part."""
    ch, up_k, rates, down_k, src_k, res_k = synth.HIFT_CH, synth.HIFT_UP_K, (8, 5, 3), synth.HIFT_DOWN_K, synth.HIFT_SRC_K, synth.HIFT_RES_K
    part = {"f0": 2 * (4 * 80 * 512 + 4 * 3 * 512 * 512 + 512), "conv_pre": 2 * 5 * 80 * 512}
    rows = 1
    for i in range(3):
        rows *= rates[i]
        C = ch[i + 1]
        macs = up_k[i] * ch[i] * C + down_k[i] * 18 * C + 6 * src_k[i] * C * C + 6 * sum(res_k) * C * C
        part["stage%d" % i] = 2 * rows * macs
    part["conv_post"] = 2 * rows * 7 * 64 * 18
    return part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hift_bench.json"))
    a = ap.parse_args()
    sd = synth.synth_cosyvoice_hifigan_state_dict(1)
    with tempfile.TemporaryDirectory() as d:
        m = HiFTVocoder.from_pretrained(synth.write_cosyvoice_hifigan_safetensors(sd, d), max_frames=a.clips * a.frames)
    rng = np.random.default_rng(0)
    mels = [(1.5 * rng.standard_normal((a.frames, 80)) - 1.0).astype(np.float32) for _ in range(a.clips)]
    seeds = list(range(a.clips))
    part = flops_per_frame()
    flops = sum(part.values()) * a.clips * a.frames
    try:
        for _ in range(a.warm):                                          # warm: code objects loaded, buffers touched
            m.decode_batch(mels, seeds)
        runs = []
        for _ in range(a.runs):
            m.decode_batch(mels, seeds)
            runs.append(m.timing())
    finally:
        m.close()
    total = [sum(r.values()) for r in runs]
    med = statistics.median(total)
    audio = a.clips * (480 * a.frames + 16) / 24000.0
    out = {"weights": "synthetic (qasr.synth seed 1)", "clips": a.clips, "frames": a.frames, "warm_passes": a.warm, "runs": a.runs,
           "timer": "HIP events on the work stream (qasr_hift_timing)", "device_ms_median": round(med, 3),
           "device_ms_min": round(min(total), 3), "device_ms_max": round(max(total), 3),
           "stage_ms_median": {k: round(statistics.median(r[k] for r in runs), 3) for k in STAGES}, "audio_seconds": round(audio, 3),
           "audio_seconds_per_second": round(audio / (med * 1e-3), 1), "gflop_per_frame": round(sum(part.values()) / 1e9, 4),
           "gflop_per_frame_by_part": {k: round(v / 1e9, 4) for k, v in part.items()}, "algorithmic_tflop": round(flops / 1e12, 3),
           "achieved_f32_tflops": round(flops / 1e12 / (med * 1e-3), 2)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

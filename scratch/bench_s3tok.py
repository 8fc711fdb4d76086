"""Times the CosyVoice3 speech tokenizer and voice-profile front end (qasr.s3tok.SpeechTokenizer) on the device with synthetic weights and
writes profiles/s3tok_bench.json: --clips clips of --seconds seconds at 16 kHz (default 32 x 10 s: 250 tokens each) through profile_batch
and encode_batch, depth 12.  Host wall time around each call (every call ends in a stream synchronise), warm, the median of --runs runs,
beside the device's own stage times (HIP events, qasr_s3tok_timing); audio seconds per second, and the achieved bf16 FLOP/s against the
algorithmic count 2 x 12 D^2 multiply-adds per token and block (the four attention linears and the MLP; stems, attention products, FSMN
and FSQ are left out: under 5 %).  Nothing gates on these figures.

    python scratch/bench_s3tok.py [--clips 32] [--seconds 10] [--runs 5] [--out profiles/s3tok_bench.json]

Kernel statistics: one run of its own under the profiler, then the export of the measured encode_batch (the dispatches between the first
and the second FSQ launch: the call after the warm one) from the profiler's database:

    rocprofv3 --kernel-trace --stats -d DIR -o s3tok -- python scratch/bench_s3tok.py --only encode --runs 1 --warm 1 --out /dev/null
    python scratch/bench_s3tok.py --stats-from DIR/s3tok_results.db --stats-out profiles/s3tok_kernel_stats.csv
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
from qasr import s3tok, synth                                            # noqa: E402
from qasr.s3tok import STAGES, SpeechTokenizer                           # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0                                          # MI355X dense bf16 MFMA, as profiles/README.md counts it
D = 1280


def clip(seed, n):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * (150.0 + 10 * seed) * t)).astype(np.float32)


def measure(m, fn, clips, warm, runs):
    for _ in range(warm):
        fn(clips)
    wall, dev = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn(clips)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(m.timing())
    tokens = sum(s3tok.tokens_of(s3tok.whisper_frames(c.size)) for c in clips)
    audio = sum(c.size for c in clips) / 16000.0
    flops = tokens * m.depth * 12 * D * D * 2
    med, dmed = statistics.median(wall), statistics.median(sum(d.values()) for d in dev)
    return {"clips": len(clips), "tokens": tokens, "audio_seconds": round(audio, 2), "wall_ms_median": round(med, 3), "wall_ms_min": round(min(wall), 3),
            "wall_ms_max": round(max(wall), 3), "tokenizer_device_ms_median": round(dmed, 3),
            "stage_ms_median": {k: round(statistics.median(d[k] for d in dev), 3) for k in STAGES},
            "audio_seconds_per_second": round(audio / (med * 1e-3), 1), "algorithmic_tflop": round(flops / 1e12, 3),
            "achieved_bf16_tflops_wall": round(flops / 1e12 / (med * 1e-3), 1), "achieved_bf16_tflops_device": round(flops / 1e12 / (dmed * 1e-3), 1),
            "fraction_of_dense_bf16_peak_wall": round(flops / 1e12 / (med * 1e-3) / BF16_DENSE_PEAK_TFLOPS, 3),
            "fraction_of_dense_bf16_peak_device": round(flops / 1e12 / (dmed * 1e-3) / BF16_DENSE_PEAK_TFLOPS, 3)}


def export_stats(db, path):
    """Per-kernel calls, total / average / min / max ns and share of the kernel time of one measured encode_batch."""
    import csv
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, duration from kernels order by start").fetchall()
    fsq = [i for i, r in enumerate(rows) if "s3_fsq_kernel" in r[0]]
    per = {}
    for name, _, dur in rows[fsq[0] + 1:fsq[1] + 1]:
        per.setdefault(name, []).append(dur)
    total = sum(sum(v) for v in per.values())
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage"])
        for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([k, len(v), sum(v), round(sum(v) / len(v), 1), min(v), max(v), round(100.0 * sum(v) / total, 2)])
    print("wrote", path, "kernel time", round(total / 1e6, 3), "ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stats-from", default=None, help="a rocprofv3 database of a --only encode --runs 1 --warm 1 run: export its kernel statistics and exit")
    ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "s3tok_kernel_stats.csv"))
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", choices=("encode", "profile"), default=None, help="one entry only (a kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s3tok_bench.json"))
    a = ap.parse_args()
    if a.stats_from:
        return export_stats(a.stats_from, a.stats_out)
    sd = synth.synth_cosyvoice_s3tok_state_dict(1, dict(depth=a.depth), bf16_values=True)
    n = int(a.seconds * 16000)
    per_clip = s3tok.tokens_of(s3tok.whisper_frames(n))
    with tempfile.TemporaryDirectory() as d:
        m = SpeechTokenizer.from_pretrained(synth.write_cosyvoice_s3tok_safetensors(sd, d, dtype="BF16"), max_tokens=min(a.clips * per_clip, 1 << 14))
    clips = [clip(i, n) for i in range(a.clips)]
    try:
        out = {"weights": f"synthetic (qasr.synth seed 1), depth {a.depth}, stored as BF16", "warm_passes": a.warm, "runs": a.runs,
               "timer": "time.perf_counter around the call (host packing, resampling, copies and the synchronise included); device: HIP events of qasr_s3tok_timing",
               "bf16_dense_peak_tflops": BF16_DENSE_PEAK_TFLOPS, "gflop_per_token": round(a.depth * 12 * D * D * 2 / 1e9, 4)}
        if a.only != "profile":
            out["encode_batch"] = measure(m, m.encode_batch, clips, a.warm, a.runs)
            out["encode_one_clip"] = measure(m, m.encode_batch, clips[:1], a.warm, a.runs)
        if a.only != "encode":
            out["profile_batch"] = measure(m, lambda c: m.profile_batch(c, [16000] * len(c)), clips, a.warm, a.runs)
    finally:
        m.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

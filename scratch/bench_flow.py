"""Times the CosyVoice3 flow-matching mel decoder (qasr.flow.CosyVoiceFlow) on the device with synthetic weights and writes
profiles/flow_bench.json: --clips clips of --tokens speech tokens each (default 32 x 250: 500 mel frames, 10 s of audio each) in one
generate_batch call, depth 22, 4 bit, 10 steps; device time from the HIP events of qasr_flow_timing (per stage and summed), warm, the
median of --runs runs; mel frames and audio seconds per second, and the achieved bf16 FLOP/s against the algorithmic count below
(2 x multiply-adds of every Linear, conv and attention product of the DiT, from the shapes; the mu path, norms and activations are left
out: under 1 %).  The same figures at one clip.  Nothing gates on these figures.

    python scratch/bench_flow.py [--clips 32] [--tokens 250] [--runs 5] [--out profiles/flow_bench.json]
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
from qasr.flow import CosyVoiceFlow, STAGES                              # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0                                          # MI355X dense bf16 MFMA, as profiles/README.md counts it


def flops_per_row(depth, T):
    """Algorithmic FLOPs of one mel row in one DiT forward, per part; attention depends on the clip's length T."""
    d, ff = 1024, 2048
    return {"input_embed": 2 * (320 * d + 2 * 31 * 64 * d), "block_linears": 2 * depth * (4 * d * d + 2 * d * ff), "attention": 4 * depth * T * d,
            "output": 2 * d * 80}


def measure(m, clips, tokens, steps, warm, runs):
    rng = np.random.default_rng(0)
    toks = [rng.integers(0, 6561, tokens).astype(np.int32) for _ in range(clips)]
    embs = [rng.standard_normal(192).astype(np.float32) for _ in range(clips)]
    seeds = list(range(clips))
    first = None
    for _ in range(warm):                                                # warm: code objects loaded, buffers touched, modulation table cached
        m.generate_batch(toks, spk_emb=embs, n_steps=steps, seeds=seeds)
        first = first or m.timing()
    rec = []
    for _ in range(runs):
        m.generate_batch(toks, spk_emb=embs, n_steps=steps, seeds=seeds)
        rec.append(m.timing())
    total = [sum(r.values()) for r in rec]
    med = statistics.median(total)
    T = 2 * tokens
    part = flops_per_row(m.depth, T)
    rows = clips * T * 2 * steps                                         # frames x CFG branches x steps
    flops = sum(part.values()) * rows
    audio = clips * T * 0.02
    return {"clips": clips, "tokens": tokens, "mel_frames": clips * T, "device_ms_median": round(med, 3), "device_ms_min": round(min(total), 3),
            "device_ms_max": round(max(total), 3), "stage_ms_median": {k: round(statistics.median(r[k] for r in rec), 3) for k in STAGES},
            "per_step_ms": {k: round(statistics.median(r[k] for r in rec) / steps, 3) for k in STAGES if k != "modulation"},
            "modulation_table_ms_first_call": round(first["modulation"], 3), "mel_frames_per_second": round(clips * T / (med * 1e-3), 1),
            "audio_seconds": round(audio, 2), "audio_seconds_per_second": round(audio / (med * 1e-3), 1),
            "gflop_per_row_forward": round(sum(part.values()) / 1e9, 4), "gflop_per_row_forward_by_part": {k: round(v / 1e9, 4) for k, v in part.items()},
            "algorithmic_tflop": round(flops / 1e12, 3), "achieved_bf16_tflops": round(flops / 1e12 / (med * 1e-3), 1),
            "fraction_of_dense_bf16_peak": round(flops / 1e12 / (med * 1e-3) / BF16_DENSE_PEAK_TFLOPS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=250)
    ap.add_argument("--depth", type=int, default=22)
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_bench.json"))
    a = ap.parse_args()
    sd = synth.synth_cosyvoice_flow_state_dict(1, depth=a.depth, bits=a.bits)
    with tempfile.TemporaryDirectory() as d:
        m = CosyVoiceFlow.from_pretrained(synth.write_cosyvoice_flow_safetensors(sd, d), max_frames=a.clips * 2 * a.tokens)
    try:
        batch = measure(m, a.clips, a.tokens, a.steps, a.warm, a.runs)
        one = measure(m, 1, a.tokens, a.steps, a.warm, a.runs)
    finally:
        m.close()
    # what the cached modulation table replaces: the AdaLN linears as GEMMs over every row of every forward (a calculation, not a measurement)
    ada_params = a.depth * 6 * 1024 * 1024 + 2 * 1024 * 1024
    rows = a.clips * 2 * a.tokens * 2
    out = {"weights": f"synthetic (qasr.synth seed 1), depth {a.depth}, {a.bits} bit", "steps": a.steps, "warm_passes": a.warm, "runs": a.runs,
           "timer": "HIP events on the work stream (qasr_flow_timing): the solver passes; the mu path and host copies are outside it",
           "bf16_dense_peak_tflops": BF16_DENSE_PEAK_TFLOPS, "batch": batch, "one_clip": one,
           "yardsticks": {"wav2vec2_7b_encoder_fraction_of_bf16_peak": 0.42, "hift_ms_same_32x10s": 361.1},
           "flow_plus_hift_ms_per_audio_second": round((batch["device_ms_median"] + 361.1 * a.clips / 32.0) / batch["audio_seconds"], 3)
           if (a.clips, a.tokens) == (32, 250) else None,
           "adaln_per_forward_calculated": {"note": "a calculation: the 23 AdaLN linears as per-row GEMMs in every forward, which the table removes",
                                            "gflop_per_forward": round(2 * ada_params * rows / 1e9, 1), "gflop_per_solve": round(2 * ada_params * rows * a.steps / 1e9, 1),
                                            "weight_bytes_bf16_per_forward": 2 * ada_params, "output_bytes_f32_per_forward": 4 * rows * (a.depth * 6 + 2) * 1024}}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Times the VoxCPM2 AudioVAE (qasr.audiovae.AudioVAE) on the device with synthetic weights on the real geometry and writes
profiles/avae_bench.json: --clips clips of --seconds seconds each, one decode_batch and one encode_batch call, under each value of the knob
vae_fuse_c given (default 0, 64 and 128): device time from the HIP events of qasr_avae_timing per stage, warm, the median of --runs reads;
audio seconds per second and the achieved f32 FLOP/s against the algorithmic count below (2 x multiply-adds of every conv, from the
shapes; Snake, the affine and tanh are left out).  Nothing gates on these figures.

    python scratch/bench_avae.py [--clips 32] [--seconds 10] [--runs 5] [--fuse 0 64 128] [--out profiles/avae_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
from qasr import synth, _lib                                              # noqa: E402
from qasr.audiovae import AudioVAE                                        # noqa: E402


def flops_per_frame(g):
    """Algorithmic FLOPs of one latent frame per timing stage, both directions."""
    rows, c = 1, g["encoder_dim"]
    for r in g["encoder_rates"]:
        rows *= r
    part = {"enc_conv_in": 2 * rows * 7 * c}
    for i, s in enumerate(g["encoder_rates"]):
        part["enc_block%d" % i] = 2 * (rows * 3 * (7 * c + c * c) + (rows // s) * 2 * s * c * 2 * c)
        rows, c = rows // s, 2 * c
    part["enc_fc_mu"] = 2 * 3 * c * g["latent_dim"]
    c = g["decoder_dim"]
    part["dec_conv_in"] = 2 * (7 * g["latent_dim"] + g["latent_dim"] * c)
    rows = 1
    for i, s in enumerate(g["decoder_rates"]):
        part["dec_block%d" % i] = 2 * (rows * 2 * c * s * (c // 2) + rows * s * 3 * (7 * (c // 2) + (c // 2) ** 2))
        rows, c = rows * s, c // 2
    part["dec_conv_out"] = 2 * rows * 7 * c
    return part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--fuse", type=int, nargs="+", default=[0, 64, 128])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "avae_bench.json"))
    a = ap.parse_args()
    g = synth.VOXCPM2_AUDIOVAE_REAL
    frames = int(round(a.seconds * 25))
    sd = synth.synth_voxcpm2_audiovae_state_dict(g, 1, weight_norm=False)
    with tempfile.TemporaryDirectory() as d:
        m = AudioVAE.from_pretrained(synth.write_voxcpm2_audiovae_safetensors(sd, d, g), max_frames=a.clips * frames)
    lib = _lib.load(strict=True)
    old = C.c_int()
    lib.qasr_get_tuning(b"vae_fuse_c", C.byref(old))
    rng = np.random.default_rng(0)
    zs = [rng.standard_normal((frames, g["latent_dim"])).astype(np.float32) for _ in range(a.clips)]
    pcms = [(0.3 * rng.standard_normal(frames * m.hop)).astype(np.float32) for _ in range(a.clips)]
    part = flops_per_frame(g)
    total_frames = a.clips * frames
    out = {"weights": "synthetic (qasr.synth seed 1), real geometry", "clips": a.clips, "frames_per_clip": frames, "warm_passes": a.warm,
           "runs": a.runs, "timer": "HIP events on the work stream (qasr_avae_timing)", "default_vae_fuse_c": old.value,
           "gflop_per_frame_by_stage": {k: round(v / 1e9, 5) for k, v in part.items()}, "by_vae_fuse_c": {}}
    try:
        for fuse in a.fuse:
            assert lib.qasr_set_tuning(b"vae_fuse_c", fuse) == 0
            res = {}
            for direction, call, audio in (("decode", lambda: m.decode_batch(zs), total_frames * m.samples_per_frame / m.out_sample_rate),
                                           ("encode", lambda: m.encode_batch(pcms), total_frames * m.hop / m.sample_rate)):
                for _ in range(a.warm):                                    # warm: code objects loaded, buffers touched
                    call()
                runs = []
                for _ in range(a.runs):
                    call()
                    runs.append({k: v for k, v in m.timing().items() if k.startswith(direction[:3])})
                total = [sum(r.values()) for r in runs]
                med = statistics.median(total)
                stage = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
                flops = sum(part[k] for k in stage) * total_frames
                res[direction] = {"device_ms_median": round(med, 3), "device_ms_min": round(min(total), 3), "device_ms_max": round(max(total), 3),
                                  "stage_ms_median": {k: round(v, 3) for k, v in stage.items()},
                                  "stage_f32_tflops": {k: round(part[k] * total_frames / 1e12 / (v * 1e-3), 2) for k, v in stage.items() if v > 0},
                                  "audio_seconds": round(audio, 3), "audio_seconds_per_second": round(audio / (med * 1e-3), 1),
                                  "algorithmic_tflop": round(flops / 1e12, 3), "achieved_f32_tflops": round(flops / 1e12 / (med * 1e-3), 2)}
            out["by_vae_fuse_c"][str(fuse)] = res
    finally:
        lib.qasr_set_tuning(b"vae_fuse_c", old.value)
        m.close()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

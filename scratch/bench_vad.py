"""Silero VAD on the device (csrc/vad_silero.hip): tick device time for B in {1, 8, 64} streams, host wall time of one vtable
process_chunk call, and whole-buffer device time for 32 x 30 s.  Prints one JSON line (device times: HIP events around H2D + kernels +
D2H, qasr_vad_timing; medians).  Synthetic weights (qasr.synth.synth_silero_state_dict): the arithmetic does not depend on the values."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "qwen3-asr-swift_amd")]
from qasr import synth                      # noqa: E402
from qasr.vad import SileroVADModel          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    synth.write_silero_safetensors(synth.synth_silero_state_dict(0), d)
    v = SileroVADModel.from_pretrained(d, max_streams=64)
    rng = np.random.default_rng(0)
    res = {"metric": "silero_vad", "unit": "ms"}
    for B in (1, 8, 64):
        x = (0.05 * rng.standard_normal((B, 512))).astype(np.float32)
        ids = np.arange(B, dtype=np.int32)
        for _ in range(20):
            v.process_chunks(x, ids)
        ms, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            v.process_chunks(x, ids)
            walls.append((time.perf_counter() - t0) * 1e3)
            m, g = v.timing()
            assert g
            ms.append(m)
        res[f"tick_B{B}_device_ms"] = float(np.median(ms))
        res[f"tick_B{B}_wall_ms"] = float(np.median(walls))
    vt = v.vtable(0)
    ch = (0.05 * rng.standard_normal(512)).astype(np.float32)
    p = ch.ctypes.data_as(C.POINTER(C.c_float))
    fn = vt.process_chunk
    for _ in range(20):
        fn(vt.context, p, 512)
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn(vt.context, p, 512)
        walls.append((time.perf_counter() - t0) * 1e3)
    res["vtable_process_chunk_wall_ms"] = float(np.median(walls))
    rows = [(0.05 * rng.standard_normal(480000)).astype(np.float32) for _ in range(32)]
    v.probs(rows)
    ms, walls = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        v.probs(rows)
        walls.append((time.perf_counter() - t0) * 1e3)
        ms.append(v.timing()[0])
    res["probs_32x30s_device_ms"] = float(np.median(ms))
    res["probs_32x30s_wall_ms"] = float(np.median(walls))
    res["probs_32x30s_audio_s_per_s"] = 32 * 30.0 / (res["probs_32x30s_device_ms"] / 1e3)
    v.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

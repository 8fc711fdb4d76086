"""WeSpeaker speaker embeddings on the device (csrc/spk_wespeaker.hip): device time of 64 x 10 s windows in one embed_batch call and of one
10 s clip, with the fraction of the dense bf16 MFMA peak that the 3x3 convolutions' FLOPs represent.  Prints one JSON line (device
times: HIP events around H2D + kernels + D2H of the call, qasr_spk_timing; medians).  Synthetic weights
(qasr.synth.synth_wespeaker_state_dict): the arithmetic does not depend on the values.  Per-kernel times: run this script under
`rocprofv3 --kernel-trace --stats` in a run of its own (profiles/spk_kernel_stats.csv)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "qwen3-asr-swift_amd")]
from qasr import synth                       # noqa: E402
from qasr.speaker import WeSpeakerModel      # noqa: E402

BF16_DENSE_PEAK_TFLOPS = 2500.0              # MI355X dense bf16 MFMA peak


def conv_flops(n_samples):
    """2 * MACs of every convolution of one clip (stem, 3x3 convs, shortcuts)"""
    T = n_samples // 160 + 1
    F, tot = 80, 2 * 80 * T * 32 * 9
    for st, nb in enumerate((3, 4, 6, 3)):
        C, Cp = 32 << st, (16 << st if st else 32)
        for i in range(nb):
            if st > 0 and i == 0:
                F, T = (F + 1) // 2, (T + 1) // 2
                tot += 2 * F * T * C * (9 * Cp + 9 * C + Cp)
            else:
                tot += 2 * F * T * C * 18 * C
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp()
    synth.write_wespeaker_safetensors(synth.synth_wespeaker_state_dict(0), d)
    m = WeSpeakerModel.from_pretrained(d)
    rng = np.random.default_rng(0)
    res = {"metric": "wespeaker", "unit": "ms"}
    for B in (64, 1):
        clips = [(0.1 * rng.standard_normal(160000)).astype(np.float32) for _ in range(B)]
        m.embed_batch(clips)
        ms = []
        for _ in range(a.reps):
            m.embed_batch(clips)
            ms.append(m.timing())
        t = float(np.median(ms))
        fl = B * conv_flops(160000)
        res[f"embed_{B}x10s_device_ms"] = t
        res[f"embed_{B}x10s_tflop"] = fl / 1e12
        res[f"embed_{B}x10s_peak_fraction"] = fl / (t * 1e-3) / (BF16_DENSE_PEAK_TFLOPS * 1e12)
    m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Qwen3-TTS ICL prompt on one MI355X, both values of the tuning knob tts_packed_prompt: synthetic weights on the real 0.6B geometry (MLX
4 bit), reference and target text of 30 ids each, F reference frames (25 | 125 | 375 = 2 | 10 | 30 s of reference audio) at B = 1 and 8.
The timed region is qasr_tts_generate_icl with max_tokens = 1: the prompt, one frame, the codes in host memory (a host clock around a call
that ends in a stream synchronise).  Per (F, B) the two knob values alternate in blocks (a knob change drops the captured frame graph, so
every block starts with untimed calls); the figure is the median over all timed calls of a value.  Also records the distance between the
two values' forced Talker logits at the timed geometry.  Writes profiles/tts_icl_prompt.json and prints it as one JSON line.

usage: python scratch/bench_tts_icl.py [--frames 25,125,375] [--batches 1,8] [--calls 24] [--small]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
import numpy as np  # noqa: E402
from qasr import synth, tts, _lib  # noqa: E402

TR = TT = 30
BLOCKS, WARM = 4, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="25,125,375")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--calls", type=int, default=24, help="timed calls per knob value and shape (at least 20)")
    ap.add_argument("--small", action="store_true", help="the reduced test geometry (a quick check of the script)")
    a = ap.parse_args()
    geo = dict(synth.TTS_TALKER_SMALL if a.small else synth.TTS_TALKER_REAL, bits=4)
    if not a.small:
        geo.update(text_vocab=4096, tts_pad=4093, tts_bos=4094, tts_eos=4095)
    frames, batches = [int(v) for v in a.frames.split(",")], [int(v) for v in a.batches.split(",")]
    lib = _lib.load(strict=True)
    with tempfile.TemporaryDirectory() as d:
        synth.write_tts_talker_safetensors(synth.synth_tts_talker_state_dict(geo, 0), d)
        cfg = tts.default_config("0.6B", 4, **{k: v for k, v in geo.items() if k != "bits"})
        cfg.bits = 4
        m = tts.Qwen3TTSModel.from_pretrained(d, cfg, max_batch=max(batches), max_frames=8, max_text=64, max_ref_frames=max(frames),
                                              max_ref_text=TR)
    rng = np.random.default_rng(0)
    H = geo["hidden"]
    s = tts.SamplingConfig(eos_logit_bias=-1e4, max_tokens=1)
    out = {"geometry": "small" if a.small else "0.6B", "bits": 4, "ref_text": TR, "target_text": TT, "device_bytes": m.device_bytes,
           "launches_per_position_step_path": 5 * geo["layers"] + 1, "rows": []}
    per = max(a.calls // (BLOCKS // 2), 1)
    try:
        for F in frames:
            for B in batches:
                kw = dict(texts=[[1, 2, 3] + [int(v) for v in rng.integers(4, 400, TT)] + [5, 6, 7, 8, 9] for _ in range(B)], languages=2050,
                          xvectors=[(0.5 * rng.standard_normal(H)).astype(np.float32) for _ in range(B)],
                          ref_texts=[[int(v) for v in rng.integers(4, 400, TR)] for _ in range(B)],
                          ref_codes=[rng.integers(0, 2048, (16, F)).astype(np.int32) for _ in range(B)])
                times = {0: [], 1: []}
                for blk in range(BLOCKS):
                    knob = blk % 2
                    assert lib.qasr_set_tuning(b"tts_packed_prompt", knob) == 0
                    for r in range(WARM + per):
                        t0 = time.perf_counter()
                        codes = m.generate_codes_icl(sampling=s, seed=1 + r, **kw)
                        dt = time.perf_counter() - t0
                        assert all(c.shape == (16, 1) for c in codes)
                        if r >= WARM:
                            times[knob].append(dt)
                forced = rng.integers(0, 2048, (B, 16, 1)).astype(np.int32)
                logits = {}
                for knob in (0, 1):
                    assert lib.qasr_set_tuning(b"tts_packed_prompt", knob) == 0
                    logits[knob] = m.forced_icl(codes=forced, want=("talker",), **kw)["talker"].astype(np.float64)
                dist = float(np.abs(logits[1] - logits[0]).max() / np.abs(logits[0]).max())
                P = 11 + TR + TT + F
                row = {"F": F, "B": B, "P": P, "packed_positions": B * (P - 1), "packed_vs_step_talker_logits": dist}
                for knob in (0, 1):
                    t = times[knob]
                    row["packed_%d" % knob] = {"median_ms": 1e3 * statistics.median(t), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t), "calls": len(t)}
                row["speedup"] = row["packed_0"]["median_ms"] / row["packed_1"]["median_ms"]
                out["rows"].append(row)
                print(json.dumps(row), flush=True)
    finally:
        m.close()
    out["faster_everywhere"] = 1 if all(r["speedup"] > 1 for r in out["rows"]) else 0 if all(r["speedup"] < 1 for r in out["rows"]) else None
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tts_icl_prompt.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

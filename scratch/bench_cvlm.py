"""Times the CosyVoice3 speech-token LLM (qasr.cosyvoice.CosyVoiceLLM) on the device with synthetic weights and writes
profiles/cvlm_bench.json: the real 0.5B geometry (24 layers, hidden 896, 14 / 2 heads, inter 4864, vocabularies 151936 and 6761), 4 bit,
default sampling with the stops masked by a large min_ratio, --tokens tokens (default 250: 10 s of audio) at 1, 8 and 32 rows, and one
prompt of 1000 positions.  Host wall time around the calls, warm (the step's graph is captured by then), the median of --runs runs; the
step time is the difference between a run of --tokens tokens and one of 10 tokens, divided by the steps between them, so that the
prompt pass and the call's fixed cost drop out.  These figures fill the "measured" column of DESIGN.md section 23.  Nothing gates on them.

    python scratch/bench_cvlm.py [--tokens 250] [--runs 5] [--out profiles/cvlm_bench.json]
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
from qasr import cosyvoice as cv, synth                                  # noqa: E402

PROMPT_POSITIONS = 1000
LAUNCHES_PER_STEP = 24 * 6 + 3


def timed(m, texts, tokens, sampling, runs):
    rec = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = m.generate(texts, max_tokens=[tokens] * len(texts), sampling=sampling, seed=1)
        rec.append((time.perf_counter() - t0) * 1e3)
        assert all(len(t) == tokens for t in out), [len(t) for t in out]
    return statistics.median(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=250)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cvlm_bench.json"))
    a = ap.parse_args()
    sd = synth.synth_cosyvoice_llm_state_dict(None, 0)
    rng = np.random.default_rng(0)
    sampling = cv.CosySamplingConfig(min_ratio=1e6)
    with tempfile.TemporaryDirectory() as tmp:
        synth.write_cosyvoice_llm_safetensors(sd, tmp)
        del sd
        m = cv.CosyVoiceLLM.from_pretrained(tmp, bits=4, max_batch=32, max_text=PROMPT_POSITIONS, max_prompt_tokens=0, max_tokens=a.tokens)
    try:
        rec = {"geometry": "Qwen2.5-0.5B shape, 24 layers, 4 bit, synthetic weights", "tokens": a.tokens, "runs": a.runs,
               "parameter_bytes": m.memory_footprint, "device_bytes": m.device_bytes, "launches_per_step": LAUNCHES_PER_STEP, "rows": []}
        for B in (1, 8, 32):
            texts = [rng.integers(0, 151936, 30).astype(np.int32) for _ in range(B)]
            timed(m, texts, 12, sampling, 1)                             # warm: the first step eager, the second captured
            short, full = timed(m, texts, 10, sampling, a.runs), timed(m, texts, a.tokens, sampling, a.runs)
            step = (full - short) / (a.tokens - 10)
            rec["rows"].append({"B": B, "call_ms_10_tokens": round(short, 3), f"call_ms_{a.tokens}_tokens": round(full, 3),
                                "step_ms": round(step, 4), "us_per_launch": round(step * 1e3 / LAUNCHES_PER_STEP, 3),
                                "tokens_per_second_per_row": round(1e3 / step, 1), "tokens_per_second": round(B * 1e3 / step, 1),
                                "audio_seconds_per_second": round(B * 1e3 / step / 25.0, 1)})
            print(rec["rows"][-1], flush=True)
        base = timed(m, [rng.integers(0, 151936, 1).astype(np.int32)], 1, sampling, a.runs)
        long = timed(m, [rng.integers(0, 151936, PROMPT_POSITIONS - 2).astype(np.int32)], 1, sampling, a.runs)
        rec["prompt"] = {"positions": PROMPT_POSITIONS, "call_ms_1_token": round(long, 3), "call_ms_1_token_3_positions": round(base, 3),
                         "prompt_pass_ms": round(long - base, 3), "positions_per_second": round(PROMPT_POSITIONS / ((long - base) * 1e-3), 1)}
        print(rec["prompt"], flush=True)
    finally:
        m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

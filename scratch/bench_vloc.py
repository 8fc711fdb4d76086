"""Times VoxCPM2's local networks (qasr.voxcpm.VoxCPM2Local) on the device with synthetic bf16 weights on the real geometry at depth 12
and writes profiles/vloc_bench.json: the 10-step solve at B = 1, 4, 16 and 32 and encode at n = 1 and n = 63 patches (a 10 s prompt).
Device time from the HIP events of qasr_vloc_timing (the call's own copies included), after --warm warm passes (the first solve of a shape
runs launch by launch, the second captures the graph), the median of --runs reads.  Reported: ms per call and per patch, patches per second,
and the achieved bytes per second of weight bytes an estimator call must stream (12 layers x 34.6 MB, 9 calls per solve; one stack per
encode).  Nothing gates on these figures.

Every figure is taken under each value of the knob vloc_skinny_rows given (default 0: every Linear on the gemm.h tile, and 256: the
skinny kernel up to 256 rows).

    python scratch/bench_vloc.py [--runs 5] [--warm 2] [--batches 1 4 16 32] [--knob 0 256] [--out profiles/vloc_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-asr-swift_amd"))
import numpy as np                                                        # noqa: E402
from qasr import synth, voxcpm, _lib                                      # noqa: E402
from qasr.voxcpm import VoxCPM2Local                                      # noqa: E402


def stack_bytes(g):
    """bf16 bytes of one stack's Linears"""
    H, F, q, kv = g["hidden_dim"], g["ffn_dim"], g["num_heads"] * 128, 2 * 128
    return 2 * g["num_layers"] * (H * (q + 2 * kv) + q * H + 3 * H * F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--patches", type=int, nargs="+", default=[1, 63])
    ap.add_argument("--knob", type=int, nargs="+", default=[0, 256], help="values of vloc_skinny_rows to run under")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vloc_bench.json"))
    a = ap.parse_args()
    geom = synth.voxcpm2_local_geometry()
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        synth.write_voxcpm2_local_safetensors(synth.synth_voxcpm2_local_state_dict(geom, seed=0), d, geom)
        m = VoxCPM2Local.from_pretrained(d, max_seqs=max(max(a.batches), max(a.patches)))
    calls = a.steps - voxcpm.zero_steps(a.steps)
    rows = []
    for knob in a.knob:
        assert _lib.load(strict=True).qasr_set_tuning(b"vloc_skinny_rows", knob) == 0
        measure(a, m, geom, calls, rng, knob, rows)
    m.close()
    out = {"geometry": geom, "stack_weight_bytes": stack_bytes(geom["dit"]), "runs": a.runs, "warm": a.warm, "results": rows}
    for r in rows:
        print(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


def measure(a, m, geom, calls, rng, knob, rows):
    for B in a.batches:
        mu, cond, z = (rng.standard_normal(s).astype(np.float32) for s in ((B, m.mu_dim), (B, 4, 64), (B, 4, 64)))
        ms = []
        for i in range(a.warm + a.runs):
            m.solve(mu, cond, z, a.steps, 2.0)
            if i >= a.warm:
                ms.append(m.timing()["solve"])
        t = statistics.median(ms)
        rows.append({"what": "solve", "vloc_skinny_rows": knob, "B": B, "n_steps": a.steps, "estimator_calls": calls, "ms": t, "ms_min": min(ms), "ms_max": max(ms),
                     "ms_per_patch": t / B, "patches_per_s": 1e3 * B / t, "ms_per_estimator_call": t / calls,
                     "weight_GB_per_s": calls * stack_bytes(geom["dit"]) / t / 1e6})
    for n in a.patches:
        f = rng.standard_normal((n, 4, 64)).astype(np.float32)
        ms = []
        for i in range(a.warm + a.runs):
            m.encode(f)
            if i >= a.warm:
                ms.append(m.timing()["encode"])
        t = statistics.median(ms)
        rows.append({"what": "encode", "vloc_skinny_rows": knob, "n": n, "ms": t, "ms_min": min(ms), "ms_max": max(ms), "ms_per_patch": t / n, "patches_per_s": 1e3 * n / t,
                     "weight_GB_per_s": stack_bytes(geom["enc"]) / t / 1e6})


if __name__ == "__main__":
    main()

"""The cases that tests/test_flow_cpu.py measures on the twin and tests/test_gpu_flow.py runs on the device, and the twin's measured
distances from the float64 oracle (max |d| / peak of the oracle's result).  The device's bound on a case is MARGIN x the twin's figure:
4 x, the Talker's choice for a bf16 path.  test_twin_distance recomputes every figure and fails when one has moved."""
import numpy as np

MARGIN = 4.0
SEED, DEPTH_SWEEP, DEPTH_FULL = 5, 2, 22
VEL_T = (2, 4, 30, 32, 62, 64, 66, 126, 128, 130, 258)      # the k = 31 reach, the 64-key attention block, the 128-row GEMM tile at -2 / 0 / +2
VEL_TIMES = (0.0, 0.3, 1.0)
SOLVE_T, SOLVE_STEPS = 66, (1, 2, 10)
FULL_T, FULL_TIME = 66, 0.3                                  # the depth-22 velocity case
GEN_TOKENS, GEN_PROMPT, GEN_SEED = 5, 2, 1234                                # the depth-22 generate case: T = 14


def variant(i, T):
    """(with spks, prompt frames Tp) of velocity case i: every combination of the issue's list comes up with every length class"""
    return [(False, 0), (True, 2), (True, T - 2), (True, T), (False, T), (True, 0)][i % 6]


def velocity_cases():
    out = []
    for i, T in enumerate(VEL_T):
        for j, t in enumerate(VEL_TIMES):
            spk, Tp = variant(i + 2 * j, T)
            out.append((T, t, spk, Tp))
    return out


def inputs(T, spk, Tp, seed=0):
    """x, mu, spks, cond of a case: unit-variance x (noise at t = 0), mu and prompt mel of the size the mu path and a log-mel give"""
    g = np.random.default_rng(1000 * seed + 7 * T + Tp + (1 if spk else 0))
    x = g.standard_normal((T, 80)).astype(np.float32)
    mu = (0.8 * g.standard_normal((T, 80))).astype(np.float32)
    spks = (0.7 * g.standard_normal(80)).astype(np.float32) if spk else None
    cond = None
    if Tp:
        cond = np.zeros((T, 80), dtype=np.float32)
        cond[:Tp] = (1.5 * g.standard_normal((Tp, 80)) - 2.0).astype(np.float32)
    return x, mu, spks, cond


def generate_inputs():
    """tokens, prompt tokens, prompt mel [80, 2 p], speaker vector [192] of the depth-22 generate case, and its x0 [T, 80]: the host twin
    of the device's noise (qasr_hift_noise at counters 80 t + m), seed GEN_SEED, temperature 1"""
    from qasr import vocoder
    g = np.random.default_rng(77)
    tok, ptok = g.integers(0, 6561, GEN_TOKENS).astype(np.int32), g.integers(0, 6561, GEN_PROMPT).astype(np.int32)
    feat = (1.5 * g.standard_normal((80, 2 * GEN_PROMPT)) - 2.0).astype(np.float32)
    emb = g.standard_normal(192).astype(np.float32)
    T = 2 * (GEN_TOKENS + GEN_PROMPT)
    z = vocoder.noise(GEN_SEED, np.arange(80 * T, dtype=np.uint64))[1].reshape(T, 80)
    return tok, ptok, feat, emb, z


def case_key(T, t, spk, Tp):
    return f"T{T}_t{t:g}_s{int(spk)}_p{Tp}"


# measured by test_flow_cpu.py::test_twin_distance (printed with -s), copied here
TWIN_VELOCITY = {
    "T2_t0_s0_p0": 5.08e-03, "T2_t0.3_s1_p0": 4.91e-03, "T2_t1_s0_p2": 3.93e-03, "T4_t0_s1_p2": 3.67e-03, "T4_t0.3_s1_p4": 3.67e-03, "T4_t1_s1_p0": 5.31e-03,
    "T30_t0_s1_p28": 4.26e-03, "T30_t0.3_s0_p30": 4.02e-03, "T30_t1_s0_p0": 3.87e-03, "T32_t0_s1_p32": 3.83e-03, "T32_t0.3_s1_p0": 6.15e-03, "T32_t1_s1_p2": 5.29e-03,
    "T62_t0_s0_p62": 4.03e-03, "T62_t0.3_s0_p0": 5.39e-03, "T62_t1_s1_p60": 2.88e-03, "T64_t0_s1_p0": 4.01e-03, "T64_t0.3_s1_p2": 4.77e-03, "T64_t1_s1_p64": 4.27e-03,
    "T66_t0_s0_p0": 4.06e-03, "T66_t0.3_s1_p64": 4.60e-03, "T66_t1_s0_p66": 3.43e-03, "T126_t0_s1_p2": 4.35e-03, "T126_t0.3_s1_p126": 3.79e-03, "T126_t1_s1_p0": 4.75e-03,
    "T128_t0_s1_p126": 4.20e-03, "T128_t0.3_s0_p128": 4.65e-03, "T128_t1_s0_p0": 3.68e-03, "T130_t0_s1_p130": 4.05e-03, "T130_t0.3_s1_p0": 5.52e-03, "T130_t1_s1_p2": 4.08e-03,
    "T258_t0_s0_p258": 4.14e-03, "T258_t0.3_s0_p0": 5.81e-03, "T258_t1_s1_p256": 3.48e-03,
}
TWIN_VELOCITY_FULL = 8.32e-03
TWIN_SOLVE = {1: 6.35e-03, 2: 5.06e-03, 10: 2.21e-03}
TWIN_GENERATE_FULL = 2.88e-03
TWIN_VELOCITY_8BIT = 5.11e-03

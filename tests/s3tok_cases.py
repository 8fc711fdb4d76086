"""Cases, inputs and the twin's measured distances for the CosyVoice3 speech tokenizer tests (tests/test_s3tok_cpu.py measures and checks
the figures below on these very inputs; tests/test_gpu_s3tok.py bounds the device by MARGIN x them).  DESIGN.md section 24."""
import functools

import numpy as np

import s3tok_oracle as O
from qasr import synth

MARGIN = 4.0                                           # the project's figure for a bf16 path
SEED = 5
# tokens per clip: the FSMN reach of 15 (under, at, past, twice), the 64-key attention tile and the 128-row GEMM tile at -1 / 0 / +1 (+2)
TOKENS = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 130)
FULL_TOKENS = 66                                       # the one clip of the 12-block geometry
BATCH_TOKENS = (2, 130, 4, 66, 30)
THREE_PASSES = 130                                     # max_tokens that holds (2) | (130) | (4, 66, 30)
FLOW_SAMPLES = (480, 481, 720, 721, 959, 960, 1441, 24000, 31337)     # the 720-sample reflect reach, the 480 step, 1 s, an odd 1.3 s
UNDECIDED_MAX = 0.15


def mel_frames(n_tokens, i):
    """A mel length of n tokens; over i the lengths before each stem are odd and even in turn."""
    t1 = 2 * n_tokens - (i & 1)
    return 2 * t1 - ((i >> 1) & 1)


def token_cases():
    return [(n, mel_frames(n, i)) for i, n in enumerate(TOKENS)]


def mel_input(n_tokens, T):
    return synth.synth_s3tok_mel(100 + n_tokens, T)


def pcm(seed, n, sr=16000):
    """n samples: white noise under two tones, peak about 0.6."""
    rng = np.random.default_rng(4242 + seed)
    t = np.arange(n) / sr
    return (0.12 * rng.standard_normal(n) + 0.25 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 3100.0 * t + 1.0)).astype(np.float32)


def whisper_samples():
    """16 kHz sample counts: every token case's mel length, with 0, 37 or 159 samples over the last whole hop."""
    return [160 * T + (0, 37, 159)[i % 3] for i, (_, T) in enumerate(token_cases())]


def batch_pcm():
    return [pcm(50 + i, 160 * mel_frames(n, i) + 11 * i) for i, n in enumerate(BATCH_TOKENS)]


@functools.lru_cache(maxsize=None)
def state_dict(depth):
    return synth.synth_cosyvoice_s3tok_state_dict(SEED, dict(depth=depth), bf16_values=depth > 2)


@functools.lru_cache(maxsize=None)
def oracle(depth, twin=False):
    return O.S3Oracle(state_dict(depth), twin=twin)


@functools.lru_cache(maxsize=None)
def reference(depth, n_tokens, T):
    """(hidden, projections) of the float64 oracle on mel_input(n_tokens, T): computed once, shared, never written to."""
    h, p = oracle(depth).both(mel_input(n_tokens, T))
    h.setflags(write=False)
    p.setflags(write=False)
    return h, p


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def undecided(proj64, tol):
    """Mask of the digits whose oracle projection lies within tol of +-atanh(0.5 / 0.999)."""
    return np.abs(np.abs(proj64) - O.FSQ_EDGE) <= tol


# ---- the twin's distance from float64 (max |d| / peak; for the projections also max |d|), as test_twin_distance measured it ------------
TWIN_HIDDEN = {1: 4.55e-03, 2: 4.84e-03, 15: 5.01e-03, 16: 5.62e-03, 17: 3.68e-03, 31: 5.27e-03, 33: 3.95e-03, 63: 4.91e-03, 64: 4.99e-03, 65: 4.91e-03,
               127: 5.36e-03, 129: 4.82e-03, 130: 4.71e-03}
TWIN_PROJ = {1: 5.83e-03, 2: 6.53e-03, 15: 7.78e-03, 16: 1.06e-02, 17: 5.57e-03, 31: 6.96e-03, 33: 5.05e-03, 63: 5.54e-03, 64: 5.24e-03, 65: 5.83e-03,
             127: 5.88e-03, 129: 5.98e-03, 130: 5.64e-03}
TWIN_PROJ_ABS = {1: 1.15e-02, 2: 1.53e-02, 15: 2.00e-02, 16: 2.66e-02, 17: 1.85e-02, 31: 2.29e-02, 33: 1.72e-02, 63: 1.85e-02, 64: 2.09e-02, 65: 1.96e-02,
                 127: 2.35e-02, 129: 2.13e-02, 130: 2.02e-02}
TWIN_HIDDEN_FULL = 5.67e-03
TWIN_PROJ_FULL = 4.70e-03
# the mel twins: numpy float32 restatements with a plain float32 DFT (the Whisper one on csrc/mel_core.h's table arithmetic), keyed by sample count
TWIN_WHISPER = {640: 4.65e-06, 997: 1.05e-05, 9599: 1.07e-05, 9760: 1.20e-05, 10917: 1.20e-05, 19679: 1.31e-05, 20960: 1.12e-05, 39877: 1.33e-05,
                41119: 1.64e-05, 41280: 1.19e-05, 81157: 1.36e-05, 82239: 1.32e-05, 83200: 1.33e-05}
TWIN_FLOW = {480: 1.38e-06, 481: 1.31e-06, 720: 8.48e-07, 721: 7.52e-07, 959: 9.86e-07, 960: 1.27e-06, 1441: 1.64e-06, 24000: 1.86e-06, 31337: 1.57e-06}

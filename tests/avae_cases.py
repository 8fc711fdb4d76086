"""Geometries and inputs shared by tests/test_avae_cpu.py and tests/test_gpu_avae.py (the VoxCPM2 AudioVAE, qasr_avae_*).

All three geometries keep the reference's rates, so the 54-row reach of the dilation-9 unit and every stride are the real ones; only
the widths shrink.  tiny: encoder widths 8 .. 128, decoder 256 .. 4.  mid: encoder 32 .. 512, decoder 512 .. 8; it crosses the
default vae_fuse_c (128) in both directions and its decoder holds a 64-wide condition layer, the [n, 8, 8] table.  real: the defaults."""
import numpy as np

from qasr import synth

RATES = {"encoder_rates": [2, 5, 8, 8], "decoder_rates": [8, 6, 5, 2, 2, 2], "sr_bin_boundaries": [20000, 30000, 40000]}
GEOMS = {
    "tiny": dict(RATES, encoder_dim=8, latent_dim=8, decoder_dim=256),
    "mid": dict(RATES, encoder_dim=32, latent_dim=16, decoder_dim=512),
    "real": dict(synth.VOXCPM2_AUDIOVAE_REAL),
}
SEEDS = {"tiny": 1, "mid": 2, "real": 3}
HOP, SPF = 640, 1920

# T = 1: 8 rows at decoder stage 1, less than every dilated reach | 8, 9: one 64-row tile of that stage exactly, and one row over
DECODE_T = (1, 2, 3, 8, 9, 17)
ENCODE_N = (1, 639, 640, 641, 1281, 6400, 6401)
REAL_T, REAL_N = 2, 1281
SR_CONDS = (16000, 48000)
FUSE = (0, 64, 128)                                    # the values of the knob vae_fuse_c the tests run under: never fused | the default | up to 128


def stored(name: str) -> dict:
    """The checkpoint of a geometry as written to disk: weight-norm pairs, [n, 8, 8] tables, fc_logvar; mid without the audio_vae. prefix."""
    return synth.synth_voxcpm2_audiovae_state_dict(GEOMS[name], SEEDS[name], weight_norm=True, prefixed=name != "mid")


def make_z(seed: int, T: int, latent: int) -> np.ndarray:
    """Latent frames [T, latent]: unit normal, what the LM side hands over after its own normalisation."""
    return np.random.default_rng(9100 + seed).standard_normal((T, latent)).astype(np.float32)


def clip_z(T: int, latent: int) -> np.ndarray:
    """The first T frames of one long latent clip: clip_z(k) is a prefix of clip_z(T), which the causal tests rely on."""
    return np.ascontiguousarray(make_z(0, 32, latent)[:T])


def make_pcm(seed: int, n: int) -> np.ndarray:
    """16 kHz PCM [n]: three partials under a slow envelope plus a little noise, peak about 0.5."""
    rng = np.random.default_rng(9200 + seed)
    t = np.arange(n) / 16000.0
    f = rng.uniform(90.0, 400.0) * np.array([1.0, 2.0, 3.0])
    x = sum(a * np.sin(2 * np.pi * fk * t + p) for a, fk, p in zip((0.3, 0.15, 0.08), f, rng.uniform(0, 6.28, 3)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.1 * t)) + 0.02 * rng.standard_normal(n)
    return x.astype(np.float32)


def clip_pcm(n: int) -> np.ndarray:
    return np.ascontiguousarray(make_pcm(0, 8000)[:n])

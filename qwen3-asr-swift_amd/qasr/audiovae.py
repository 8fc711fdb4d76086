"""The VoxCPM2 AudioVAE on the GPU over the C ABI (include/qasr.h, qasr_avae_*).

Reference: Sources/VoxCPM2TTS/AudioVAE.swift and VoxCPM2TTS.swift:1040-1074 (encodeAudio), :1434-1446 (the decode at the end of
generateVoxCPM2).  encode() turns float32 16 kHz PCM [n] into latent frames [ceil(n / 640), 64]; decode() turns latent frames [T, 64] into
1920 T samples of 48 kHz PCM.  Every conv is causal, so decode(z[:k]) is the first 1920 k samples of decode(z).  The batch forms run clips
of any lengths in one call, each bit-identical to the single form.  f32 throughout; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
TIMING_SLOTS, DECODER_TIMING_AT = 20, 10


def _fptr(a):
    return a.ctypes.data_as(_F)


def num_frames(n: int, hop: int = 640) -> int:
    """Latent frames of a clip of n samples: ceil(n / hop) (AudioVAE.preprocess pads with zero samples to a whole frame)."""
    return (int(n) + hop - 1) // hop


def sr_index(sr_cond: int, boundaries=(20000, 30000, 40000)) -> int:
    """SampleRateConditionLayer.getSrIdx: how many boundaries sr_cond has reached."""
    return sum(1 for b in boundaries if int(sr_cond) >= b)


def sanitize(weights: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """AudioVAE.sanitize (AudioVAE.swift:646-686) on {key: array}: weight_g / weight_v pairs fuse to g v / (|v| + 1e-9) with the norm over
    everything but the first axis (formed in float64, rounded to float32 once, as the loader does), fc_logvar is dropped, a bare encoder. /
    decoder. prefix gains audio_vae.; a table [n, 8, 8] is flattened to [n, 64] (TableEmbedding)."""
    fused = {}
    for key in sorted(weights):
        if "fc_logvar" in key or key.endswith(".weight_v"):
            continue
        if key.endswith(".weight_g") and key[:-9] + ".weight_v" in weights:
            g = np.asarray(weights[key], dtype=np.float64)
            v = np.asarray(weights[key[:-9] + ".weight_v"], dtype=np.float64)
            norm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(axis=1)).reshape(g.shape)
            fused[key[:-9] + ".weight"] = (g * (v / (norm + 1e-9))).astype(np.float32)
            continue
        fused[key] = np.asarray(weights[key], dtype=np.float32)
    out = {}
    for key, value in fused.items():
        if key.startswith("encoder.") or key.startswith("decoder."):
            key = "audio_vae." + key
        if key.endswith("_embed.weight") and value.ndim == 3:
            value = value.reshape(value.shape[0], -1)
        out[key] = value
    return out


class AudioVAE:
    """AudioVAE.encode / decode on the device."""

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle
        lib = self.lib
        self.latent_dim = int(lib.qasr_avae_latent_dim(handle))
        self.sample_rate = int(lib.qasr_avae_in_sample_rate(handle))
        self.out_sample_rate = int(lib.qasr_avae_out_sample_rate(handle))
        self.hop = int(lib.qasr_avae_hop(handle))
        self.samples_per_frame = int(lib.qasr_avae_samples_per_frame(handle))
        self.encoder_blocks = int(lib.qasr_avae_num_blocks(handle, 0))
        self.decoder_blocks = int(lib.qasr_avae_num_blocks(handle, 1))

    @classmethod
    def from_pretrained(cls, model_dir, max_frames=0, order_with=None, device=0):
        """model_dir holds the *.safetensors with the audio_vae.* tensors and, optionally, config.json with audio_vae_config.
        max_frames: latent frames one device pass holds (0 = 1024); a longer clip is refused, a longer batch runs in several passes
        with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_avae_create(int(device), str(model_dir).encode(), int(max_frames), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_avae_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_avae_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_avae_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_avae_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_avae_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_avae_memory_footprint(self.h))

    def num_frames(self, n: int) -> int:
        return int(self.lib.qasr_avae_num_frames(self.h, int(n)))

    def stage_shape(self, decoder: bool, k: int):
        """(rows per latent frame, width) of stage k's output."""
        r, w = C.c_int32(), C.c_int32()
        self._check(self.lib.qasr_avae_stage_shape(self.h, int(bool(decoder)), int(k), C.byref(r), C.byref(w)))
        return r.value, w.value

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last call per stage: enc_conv_in, enc_block<i>, enc_fc_mu, dec_conv_in, dec_block<i>, dec_conv_out."""
        ms = (C.c_float * TIMING_SLOTS)()
        self._check(self.lib.qasr_avae_timing(self.h, ms))
        names = ["enc_conv_in"] + [f"enc_block{i}" for i in range(self.encoder_blocks)] + ["enc_fc_mu"]
        out = dict(zip(names, (float(v) for v in ms)))
        names = ["dec_conv_in"] + [f"dec_block{i}" for i in range(self.decoder_blocks)] + ["dec_conv_out"]
        out.update(zip(names, (float(v) for v in ms[DECODER_TIMING_AT:])))
        return out

    @staticmethod
    def _pcm(pcm):
        a = np.ascontiguousarray(pcm, dtype=np.float32)
        if a.ndim != 1:
            raise QasrError("qasr error 1: pcm is [n]")
        return a

    def _z(self, z):
        a = np.ascontiguousarray(z, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.latent_dim:
            raise QasrError(f"qasr error 1: z is [T, {self.latent_dim}]")
        return a

    # ---- whole paths ----
    def encode(self, pcm) -> np.ndarray:
        """pcm [n] at 16 kHz -> z [ceil(n / 640), 64]."""
        a = self._pcm(pcm)
        out = np.zeros((self.num_frames(a.size), self.latent_dim), dtype=np.float32)
        self._check(self.lib.qasr_avae_encode(self.h, _fptr(a), a.size, _fptr(out)))
        return out

    def decode(self, z, sr_cond: int = 0) -> np.ndarray:
        """z [T, 64] -> pcm [1920 T] at 48 kHz.  sr_cond: the sample rate the decoder is conditioned on (0 = 48000)."""
        a = self._z(z)
        out = np.zeros(self.samples_per_frame * a.shape[0], dtype=np.float32)
        self._check(self.lib.qasr_avae_decode(self.h, _fptr(a), a.shape[0], int(sr_cond), _fptr(out)))
        return out

    def encode_batch(self, clips: Sequence) -> List[np.ndarray]:
        items = [self._pcm(p) for p in clips]
        B = len(items)
        if B == 0:
            return []
        outs = [np.zeros((self.num_frames(a.size), self.latent_dim), dtype=np.float32) for a in items]
        pp, op = (_F * B)(*[_fptr(a) for a in items]), (_F * B)(*[_fptr(o) for o in outs])
        self._check(self.lib.qasr_avae_encode_batch(self.h, pp, (C.c_size_t * B)(*[a.size for a in items]), B, op))
        return outs

    def decode_batch(self, latents: Sequence, sr_cond: int = 0) -> List[np.ndarray]:
        items = [self._z(z) for z in latents]
        B = len(items)
        if B == 0:
            return []
        outs = [np.zeros(self.samples_per_frame * a.shape[0], dtype=np.float32) for a in items]
        pp, op = (_F * B)(*[_fptr(a) for a in items]), (_F * B)(*[_fptr(o) for o in outs])
        self._check(self.lib.qasr_avae_decode_batch(self.h, pp, (C.c_size_t * B)(*[a.shape[0] for a in items]), B, int(sr_cond), op))
        return outs

    # ---- stages ----
    def enc_stage(self, pcm, k: int) -> np.ndarray:
        """The encoder's rows after conv_in (k = 0) or after block k - 1: [frames x rows per frame, width]."""
        a = self._pcm(pcm)
        r, w = self.stage_shape(False, k)
        out = np.zeros((self.num_frames(a.size) * r, w), dtype=np.float32)
        self._check(self.lib.qasr_avae_enc_stage(self.h, _fptr(a), a.size, int(k), _fptr(out)))
        return out

    def dec_stage(self, z, k: int, sr_cond: int = 0) -> np.ndarray:
        """The decoder's rows after conv_in (k = 0) or after block k - 1, before the next block's scale / bias and Snake."""
        a = self._z(z)
        r, w = self.stage_shape(True, k)
        out = np.zeros((a.shape[0] * r, w), dtype=np.float32)
        self._check(self.lib.qasr_avae_dec_stage(self.h, _fptr(a), a.shape[0], int(sr_cond), int(k), _fptr(out)))
        return out

    def dec_output(self, rows) -> np.ndarray:
        """snake_out, conv_out, tanh on the last decoder stage's rows [1920 T, width] -> pcm [1920 T]."""
        r, w = self.stage_shape(True, self.decoder_blocks)
        a = np.ascontiguousarray(rows, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != w or a.shape[0] % r:
            raise QasrError(f"qasr error 1: rows is [{r} T, {w}]")
        out = np.zeros(a.shape[0], dtype=np.float32)
        self._check(self.lib.qasr_avae_dec_output(self.h, _fptr(a), a.shape[0] // r, _fptr(out)))
        return out

    # ---- VoxCPM2TTSModel's two uses ----
    def encode_audio(self, pcm, sample_rate: int = 16000, patch_size: int = 4, padding: str = "right") -> np.ndarray:
        """encodeAudio (VoxCPM2TTS.swift:1040-1074): pad with zeros to a multiple of patch_size x 640 samples on the chosen side, encode,
        cut to whole patches -> [patches, patch_size, 64].  Audio at another rate is refused (the reference resamples it first)."""
        a = pad_to_patches(self._pcm(pcm), sample_rate, self.sample_rate, patch_size * self.hop, padding)
        z = self.encode(a)
        patches = z.shape[0] // patch_size
        return z[:patches * patch_size].reshape(patches, patch_size, self.latent_dim)

    def decode_patches(self, feat, trim_prefix_patches: int = 0, sr_cond: int = 0) -> np.ndarray:
        """The decode that ends generateVoxCPM2 (:1434-1446): feat [patches, patch_size, 64] -> pcm; with a continuation prefix the
        audio of trim_prefix_patches patches is dropped from the front (only if something is left)."""
        f = np.ascontiguousarray(feat, dtype=np.float32)
        if f.ndim != 3 or f.shape[2] != self.latent_dim:
            raise QasrError(f"qasr error 1: feat is [patches, patch_size, {self.latent_dim}]")
        audio = self.decode(f.reshape(-1, self.latent_dim), sr_cond)
        return trim_prefix(audio, f.shape[1] * self.samples_per_frame * int(trim_prefix_patches))


def pad_to_patches(pcm: np.ndarray, sample_rate: int, want_rate: int, patch_len: int, padding: str) -> np.ndarray:
    """encodeAudio's padding (:1045-1064), host only."""
    if int(sample_rate) != int(want_rate):
        raise QasrError(f"qasr error 7: audio is at {sample_rate} Hz, the AudioVAE reads {want_rate} Hz (resample first)")
    if padding not in ("right", "left"):
        raise QasrError('qasr error 1: padding is "right" or "left"')
    if pcm.size == 0:
        raise QasrError("qasr error 6: reference / prompt audio is empty")
    pad = (-pcm.size) % patch_len
    zeros = np.zeros(pad, dtype=np.float32)
    return np.concatenate([zeros, pcm] if padding == "left" else [pcm, zeros])


def trim_prefix(audio: np.ndarray, trim: int) -> np.ndarray:
    """:1440-1446: the prefix's samples go only if audio is left after them."""
    return audio[trim:] if 0 < trim < audio.size else audio

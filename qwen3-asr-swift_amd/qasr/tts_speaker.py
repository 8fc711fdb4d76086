"""The Qwen3-TTS ECAPA-TDNN speaker encoder on the GPU over the C ABI (include/qasr.h, qasr_xvec_*).

Reference: Sources/Qwen3TTS/SpeakerEncoder.swift (SpeakerMel.compute, SpeakerEncoder) and TTSWeightLoading.swift:385-453.  A 24 kHz mono
float32 clip gives one x-vector of embedding_dim floats (1024 in the reference), not normalised; embed_batch runs clips of any lengths
in one call, each row bit-identical to embed() of it alone.  The stage methods expose the log-mel front end and the network on their
own.  f32 throughout; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
SAMPLE_RATE, N_MELS = 24000, 128
STAGES = ("mel", "conv", "block1", "block2", "block3", "pool")


def _fptr(a):
    return a.ctypes.data_as(_F)


def num_frames(n: int) -> int:
    """Frames of a clip of n samples: n // 256 + 1, 0 for 0 (qasr_xvec_num_frames; host only)."""
    return int(_lib.load(strict=True).qasr_xvec_num_frames(int(n)))


class SpeakerEncoder:
    """SpeakerEncoder(SpeakerMel.compute(audio)) on the device."""
    sample_rate = SAMPLE_RATE

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, max_samples=0, order_with=None, device=0):
        """model_dir: the main model directory; the speaker_encoder.* keys are taken from all its *.safetensors files, other keys are
        left alone.  max_samples: samples one device pass holds (0 = 64 x 10 s); a longer clip is refused, a longer batch runs in several
        passes with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_xvec_create(int(device), str(model_dir).encode(), int(max_samples), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_xvec_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_xvec_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_xvec_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_xvec_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_xvec_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_xvec_memory_footprint(self.h))

    @property
    def embedding_dim(self) -> int:
        return int(self.lib.qasr_xvec_embedding_dim(self.h))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last call per stage."""
        ms = (C.c_float * len(STAGES))()
        self._check(self.lib.qasr_xvec_timing(self.h, ms))
        return dict(zip(STAGES, (float(v) for v in ms)))

    @staticmethod
    def _clips(clips):
        return [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in clips]

    # ---- whole path ----
    def embed(self, pcm, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
        """pcm [n] at 24 kHz -> [embedding_dim]."""
        a = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        out = np.zeros(self.embedding_dim, dtype=np.float32)
        self._check(self.lib.qasr_xvec_embed(self.h, _fptr(a), a.size, int(sample_rate), _fptr(out)))
        return out

    def embed_batch(self, clips: Sequence) -> np.ndarray:
        """Clips of any lengths in one call -> [B, embedding_dim]."""
        items = self._clips(clips)
        B = len(items)
        out = np.zeros((B, self.embedding_dim), dtype=np.float32)
        if B == 0:
            return out
        pp = (_F * B)(*[_fptr(a) for a in items])
        self._check(self.lib.qasr_xvec_embed_batch(self.h, pp, (C.c_size_t * B)(*[a.size for a in items]), B, _fptr(out)))
        return out

    # ---- stages ----
    def mel(self, clips) -> List[np.ndarray]:
        """SpeakerMel.compute of every clip: [n // 256 + 1, 128] each.  A single 1-D array gives a single array."""
        single = isinstance(clips, np.ndarray) and clips.ndim == 1
        items = self._clips([clips] if single else clips)
        B = len(items)
        if B == 0:
            return []
        outs = [np.zeros((num_frames(a.size), N_MELS), dtype=np.float32) for a in items]
        pp = (_F * B)(*[_fptr(a) for a in items])
        op = (_F * B)(*[_fptr(o) for o in outs])
        self._check(self.lib.qasr_xvec_mel(self.h, pp, (C.c_size_t * B)(*[a.size for a in items]), B, op))
        return outs[0] if single else outs

    def embed_mel(self, mel) -> np.ndarray:
        """The network alone: mel [T, 128] -> [embedding_dim]."""
        a = np.ascontiguousarray(mel, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != N_MELS:
            raise QasrError(f"qasr error 1: mel is [T, {N_MELS}]")
        out = np.zeros(self.embedding_dim, dtype=np.float32)
        self._check(self.lib.qasr_xvec_embed_mel(self.h, _fptr(a), a.shape[0], _fptr(out)))
        return out

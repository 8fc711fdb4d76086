"""The CosyVoice3 HiFT vocoder on the GPU over the C ABI (include/qasr.h, qasr_hift_*).

Reference: Sources/CosyVoiceTTS/HiFiGAN.swift (HiFiGANGenerator) and WeightLoading.swift:214-331.  A float32 mel [T, 80] of 20 ms frames
gives 480 T + 16 samples of 24 kHz PCM.  decode() is the whole generator; f0(), source() and decode_source() are its three stages, and
decode(mel, seed) is bit-identical to decode_source(mel, source(f0(mel), seed)).  decode_batch runs clips of any lengths in one call,
each bit-identical to decode() of it alone.  The generator's noise is this library's counter stream, seeded per clip, not MLX's.
f32 throughout; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
SAMPLE_RATE, N_MELS, SAMPLES_PER_FRAME = 24000, 80, 480
STAGES = ("f0", "source", "stft", "conv_pre", "stage0", "stage1", "stage2_tail")


def _fptr(a):
    return a.ctypes.data_as(_F)


def num_samples(T: int) -> int:
    """PCM samples of a clip of T frames: 480 T + 16, 0 for 0 (qasr_hift_num_samples; host only)."""
    return int(_lib.load(strict=True).qasr_hift_num_samples(int(T)))


def noise(seed: int, counters):
    """The host twin of the generator's noise stream (qasr_hift_noise): (uniform, normal) float32 arrays for the given draw counters."""
    c = np.ascontiguousarray(counters, dtype=np.uint64).reshape(-1)
    u, z = np.zeros(c.size, dtype=np.float32), np.zeros(c.size, dtype=np.float32)
    rc = _lib.load(strict=True).qasr_hift_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, c.ctypes.data_as(C.POINTER(C.c_uint64)), c.size, _fptr(u), _fptr(z))
    if rc != 0:
        raise QasrError(f"qasr error {rc}: qasr_hift_noise")
    return u, z


class HiFTVocoder:
    """HiFiGANGenerator.decode(mel:) on the device."""
    sample_rate = SAMPLE_RATE

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, max_frames=0, order_with=None, device=0):
        """model_dir holds hifigan.safetensors.  max_frames: mel frames one device pass holds (0 = 4096); a longer clip is refused, a
        longer batch runs in several passes with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_hift_create(int(device), str(model_dir).encode(), int(max_frames), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_hift_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_hift_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_hift_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_hift_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_hift_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_hift_memory_footprint(self.h))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last call per stage."""
        ms = (C.c_float * len(STAGES))()
        self._check(self.lib.qasr_hift_timing(self.h, ms))
        return dict(zip(STAGES, (float(v) for v in ms)))

    @staticmethod
    def _mel(mel):
        a = np.ascontiguousarray(mel, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != N_MELS:
            raise QasrError(f"qasr error 1: mel is [T, {N_MELS}]")
        return a

    # ---- stages ----
    def f0(self, mel) -> np.ndarray:
        """F0Predictor: mel [T, 80] -> [T] Hz."""
        a = self._mel(mel)
        out = np.zeros(a.shape[0], dtype=np.float32)
        self._check(self.lib.qasr_hift_f0(self.h, _fptr(a), a.shape[0], _fptr(out)))
        return out

    def source(self, f0, seed: int = 0) -> np.ndarray:
        """The harmonic-plus-noise source: f0 [T] -> [480 T]."""
        a = np.ascontiguousarray(f0, dtype=np.float32).reshape(-1)
        out = np.zeros(SAMPLES_PER_FRAME * a.size, dtype=np.float32)
        self._check(self.lib.qasr_hift_source(self.h, _fptr(a), a.size, int(seed), _fptr(out)))
        return out

    def decode_source(self, mel, src) -> np.ndarray:
        """The generator on a given source: mel [T, 80], src [480 T] -> [480 T + 16]."""
        a = self._mel(mel)
        s = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
        if s.size != SAMPLES_PER_FRAME * a.shape[0]:
            raise QasrError(f"qasr error 1: src is [{SAMPLES_PER_FRAME} T]")
        out = np.zeros(num_samples(a.shape[0]), dtype=np.float32)
        self._check(self.lib.qasr_hift_decode_source(self.h, _fptr(a), a.shape[0], _fptr(s), _fptr(out)))
        return out

    # ---- whole path ----
    def decode(self, mel, seed: int = 0) -> np.ndarray:
        """mel [T, 80] -> [480 T + 16]."""
        a = self._mel(mel)
        out = np.zeros(num_samples(a.shape[0]), dtype=np.float32)
        self._check(self.lib.qasr_hift_decode(self.h, _fptr(a), a.shape[0], int(seed), _fptr(out)))
        return out

    def decode_batch(self, mels: Sequence, seeds: Sequence[int]) -> List[np.ndarray]:
        """Clips of any lengths in one call, one seed each -> a list of [480 T + 16]."""
        items = [self._mel(m) for m in mels]
        B = len(items)
        if len(seeds) != B:
            raise QasrError("qasr error 1: one seed per clip")
        if B == 0:
            return []
        outs = [np.zeros(num_samples(a.shape[0]), dtype=np.float32) for a in items]
        pp = (_F * B)(*[_fptr(a) for a in items])
        op = (_F * B)(*[_fptr(o) for o in outs])
        self._check(self.lib.qasr_hift_decode_batch(self.h, pp, (C.c_size_t * B)(*[a.shape[0] for a in items]),
                                                    (C.c_uint64 * B)(*[int(s) for s in seeds]), B, op))
        return outs

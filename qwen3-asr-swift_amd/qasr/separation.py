"""Open-Unmix music source separation on the GPU over the C ABI (include/qasr.h, qasr_sep_*).

Reference: Sources/SourceSeparation (SourceSeparator.fromPretrained / separate, STFTProcessor, OpenUnmixStemModel, WienerFilterMLX).
separate_batch runs many files in one device pass; the stage methods expose the STFT, the four stem networks, the Wiener EM and the
inverse STFT on their own.  f32 throughout; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
SAMPLE_RATE, N_FFT, N_HOP, N_BINS = 44100, 4096, 1024, 2049
TARGETS = ("vocals", "drums", "bass", "other")


def _fptr(a):
    return a.ctypes.data_as(_F)


def num_frames(n: int) -> int:
    """STFT frames of n samples: n / 1024 + 1 (qasr_sep_num_frames)."""
    return int(_lib.load().qasr_sep_num_frames(int(n)))


def target_mask(targets) -> int:
    m = 0
    for t in targets:
        if t not in TARGETS:
            raise QasrError(f"qasr error 1: unknown separation target {t!r}")
        m |= 1 << TARGETS.index(t)
    return m


class SourceSeparator:
    """SourceSeparator (Open-Unmix UMX-HQ / UMX-L) on the device."""
    sample_rate = SAMPLE_RATE

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, device=0, order_with=None, max_batch_samples=0):
        """model_dir/{vocals,drums,bass,other}.safetensors in the reference's keys; the preset follows the checkpoint's shapes.
        max_batch_samples: samples per channel one device pass holds (0 = 64 x 10 s); larger calls are split between files."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_sep_create(int(device), str(model_dir).encode(), int(max_batch_samples), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_sep_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_sep_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_sep_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_sep_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_sep_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_sep_memory_footprint(self.h))

    @property
    def hidden_size(self) -> int:
        return int(self.lib.qasr_sep_hidden_size(self.h))

    def set_recurrence_form(self, form: int):
        self._check(self.lib.qasr_sep_set_recurrence_form(self.h, int(form)))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last call per stage."""
        ms = (C.c_float * 4)()
        self._check(self.lib.qasr_sep_timing(self.h, ms))
        return dict(zip(("stft", "network", "wiener", "istft"), (float(v) for v in ms)))

    def _config(self, wiener, iterations, window):
        c = _lib.QasrSepConfig()
        self.lib.qasr_sep_default_config(C.byref(c))
        c.wiener = 1 if wiener else 0
        if iterations is not None:
            c.wiener_iterations = int(iterations)
        if window is not None:
            c.wiener_window = int(window)
        return c

    @staticmethod
    def _channels(audio):
        a = np.asarray(audio, dtype=np.float32)
        if a.ndim == 1:
            a = a[None]
        if a.ndim != 2 or a.shape[0] not in (1, 2):
            raise QasrError("qasr error 1: audio is [n], [1, n] or [2, n]")
        left = np.ascontiguousarray(a[0])
        return left, (np.ascontiguousarray(a[1]) if a.shape[0] == 2 else None)

    # ---- whole path ----
    def separate_batch(self, audios: Sequence, sample_rate: int = SAMPLE_RATE, targets: Sequence[str] = TARGETS, wiener: bool = True,
                       wiener_iterations: Optional[int] = None, wiener_window: Optional[int] = None) -> List[Dict[str, np.ndarray]]:
        """Files of any lengths ([2, n] stereo, [n] or [1, n] mono) in one call -> per file {target: [2, n]}; each file bit-identical to
        separate() of it alone."""
        mask = target_mask(targets)
        names = [t for t in TARGETS if t in targets]
        chans = [self._channels(a) for a in audios]
        B = len(chans)
        if B == 0:
            return []
        ns = [c[0].shape[0] for c in chans]
        outs = [np.zeros((len(names), 2, n), dtype=np.float32) for n in ns]
        lp = (_F * B)(*[_fptr(c[0]) for c in chans])
        rp = (_F * B)(*[(_fptr(c[1]) if c[1] is not None else _F()) for c in chans])
        op = (_F * B)(*[_fptr(o) for o in outs])
        cfg = self._config(wiener, wiener_iterations, wiener_window)
        self._check(self.lib.qasr_sep_separate_batch(self.h, lp, rp, (C.c_size_t * B)(*ns), B, int(sample_rate), mask, C.byref(cfg), op))
        return [{t: o[i] for i, t in enumerate(names)} for o in outs]

    def separate(self, audio, sample_rate: int = SAMPLE_RATE, targets: Sequence[str] = TARGETS, wiener: bool = True,
                 wiener_iterations: Optional[int] = None, wiener_window: Optional[int] = None) -> Dict[str, np.ndarray]:
        """separate(audio:sampleRate:targets:wiener:) -> {target: [2, n]}."""
        left, right = self._channels(audio)
        names = [t for t in TARGETS if t in targets]
        out = np.zeros((len(names), 2, left.shape[0]), dtype=np.float32)
        cfg = self._config(wiener, wiener_iterations, wiener_window)
        self._check(self.lib.qasr_sep_separate(self.h, _fptr(left), _fptr(right) if right is not None else _F(), left.shape[0],
                                               int(sample_rate), target_mask(targets), C.byref(cfg), _fptr(out)))
        return {t: out[i] for i, t in enumerate(names)}

    # ---- stages ----
    def stft(self, audio):
        """-> (re, im, magnitude), each [T, 2, 2049]."""
        left, right = self._channels(audio)
        T = num_frames(left.shape[0])
        re, im, mag = (np.zeros((max(T, 0), 2, N_BINS), dtype=np.float32) for _ in range(3))
        self._check(self.lib.qasr_sep_stft(self.h, _fptr(left), _fptr(right) if right is not None else _F(), left.shape[0], _fptr(re),
                                           _fptr(im), _fptr(mag)))
        return re, im, mag

    def masks(self, magnitudes):
        """One magnitude [T, 2, 2049] -> [4, T, 2, 2049]; a list of them -> a list, run as one batch."""
        single = isinstance(magnitudes, np.ndarray)
        mags = [magnitudes] if single else list(magnitudes)
        Ts = [int(m.shape[0]) for m in mags]
        cat = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.float32).reshape(t, 2, N_BINS) for m, t in zip(mags, Ts)]))
        out = np.zeros((4, sum(Ts), 2, N_BINS), dtype=np.float32)
        self._check(self.lib.qasr_sep_masks(self.h, _fptr(cat), (C.c_size_t * len(Ts))(*Ts), len(Ts), _fptr(out)))
        cuts = np.cumsum([0] + Ts)
        res = [out[:, cuts[i]:cuts[i + 1]].copy() for i in range(len(Ts))]
        return res[0] if single else res

    def wiener(self, masked, re, im, iterations: int = 1, window: int = 300):
        """masked [J, T, 2, 2049], mixture re / im [T, 2, 2049] -> (re, im) [J, T, 2, 2049]."""
        m = np.ascontiguousarray(masked, dtype=np.float32)
        r, i = np.ascontiguousarray(re, dtype=np.float32), np.ascontiguousarray(im, dtype=np.float32)
        ore, oim = np.zeros_like(m), np.zeros_like(m)
        cfg = self._config(True, iterations, window)
        self._check(self.lib.qasr_sep_wiener(self.h, _fptr(m), m.shape[0], _fptr(r), _fptr(i), m.shape[1], C.byref(cfg), _fptr(ore), _fptr(oim)))
        return ore, oim

    def istft(self, re, im, length: int):
        """re / im [J, T, 2, 2049] (or [T, 2, 2049]) -> [J, 2, length] (or [2, length])."""
        r, i = np.ascontiguousarray(re, dtype=np.float32), np.ascontiguousarray(im, dtype=np.float32)
        single = r.ndim == 3
        if single:
            r, i = r[None], i[None]
        out = np.zeros((r.shape[0], 2, int(length)), dtype=np.float32)
        self._check(self.lib.qasr_sep_istft(self.h, _fptr(r), _fptr(i), r.shape[0], r.shape[1], int(length), _fptr(out)))
        return out[0] if single else out

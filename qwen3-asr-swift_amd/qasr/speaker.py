"""WeSpeaker ResNet34 speaker embeddings on the GPU over the C ABI (include/qasr.h, qasr_spk_*).

Reference: Sources/SpeechVAD/WeSpeaker.swift (WeSpeakerModel: fromPretrained, embed, cosineSimilarity; the SpeakerEmbeddingModel
conformance of Sources/AudioCommon/Protocols.swift:249-256), WeSpeaker+Memory.swift (isLoaded / unload / memoryFootprint).
embed_batch / embed_segments embed many clips in one device pass (the diarization pipeline's per-window loop).  No CPU fallback.
"""
import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
SAMPLE_RATE, EMBEDDING_DIM, N_MELS = 16000, 256, 80


def _fptr(a):
    return a.ctypes.data_as(_F)


def num_frames(n: int) -> int:
    """extractRaw's frame count n / 160 + 1 (qasr_spk_num_frames)."""
    return int(_lib.load().qasr_spk_num_frames(int(n)))


def cosine_similarity(a, b) -> float:
    """WeSpeakerModel.cosineSimilarity (qasr_spk_cosine_similarity, pure CPU): 0 for mismatched or empty input or a zero norm."""
    x = np.ascontiguousarray(a, dtype=np.float32).ravel()
    y = np.ascontiguousarray(b, dtype=np.float32).ravel()
    if x.shape != y.shape or x.size == 0:
        return 0.0
    return float(_lib.load().qasr_spk_cosine_similarity(_fptr(x), _fptr(y), x.size))


class WeSpeakerModel:
    """WeSpeakerModel (MLX engine) on the device; a SpeakerEmbeddingModel (embedding_dimension, input_sample_rate, embed)."""
    embedding_dimension = EMBEDDING_DIM
    input_sample_rate = SAMPLE_RATE

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, device=0, order_with=None, max_batch_samples=0):
        """model_dir/model.safetensors in the reference's keys (WeSpeakerWeightLoading.swift).  order_with: a Qwen3ASRModel (or raw
        engine handle) on the same device whose stream orders this model's work (include/qasr.h, qasr_spk_create).
        max_batch_samples: samples one device pass holds (0 = 64 x 10 s); larger calls are split."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_spk_create(int(device), str(model_dir).encode(), int(max_batch_samples), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_spk_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_spk_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_spk_last_error(self.h).decode()}")

    # ---- ModelMemoryManageable ----
    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_spk_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_spk_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_spk_memory_footprint(self.h))

    # ---- SpeakerEmbeddingModel ----
    def embed(self, audio, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
        """embed(audio:sampleRate:) -> [256] float32, L2-normalised."""
        a = np.ascontiguousarray(audio, dtype=np.float32).ravel()
        out = np.zeros(EMBEDDING_DIM, dtype=np.float32)
        self._check(self.lib.qasr_spk_embed(self.h, _fptr(a), a.shape[0], int(sample_rate), _fptr(out)))
        return out

    @staticmethod
    def cosine_similarity(a, b) -> float:
        return cosine_similarity(a, b)

    # ---- batched ----
    def _rows(self, clips):
        rows = [np.ascontiguousarray(c, dtype=np.float32).ravel() for c in clips]
        B = len(rows)
        ptrs = (_F * B)(*[_fptr(r) for r in rows])
        ns = (C.c_size_t * B)(*[r.shape[0] for r in rows])
        return rows, ptrs, ns

    def embed_batch(self, clips: Sequence) -> np.ndarray:
        """16 kHz clips of any lengths in one call -> [B, 256]; each row bit-identical to embed() of that clip."""
        if len(clips) == 0:
            return np.zeros((0, EMBEDDING_DIM), dtype=np.float32)
        rows, ptrs, ns = self._rows(clips)
        out = np.zeros((len(rows), EMBEDDING_DIM), dtype=np.float32)
        self._check(self.lib.qasr_spk_embed_batch(self.h, ptrs, ns, len(rows), _fptr(out)))
        return out

    def embed_segments(self, audio, segments: Sequence[Tuple[float, float]], sample_rate: int = SAMPLE_RATE) -> np.ndarray:
        """Embeddings of (start, end) second ranges of one recording in one embed_batch call (views into `audio`, no copies)."""
        if int(sample_rate) != SAMPLE_RATE:
            raise QasrError(f"qasr error 7: 16 kHz input only (got {sample_rate})")
        a = np.ascontiguousarray(audio, dtype=np.float32).ravel()
        views = []
        for s, e in segments:
            i0 = max(0, min(a.shape[0], int(round(float(s) * SAMPLE_RATE))))
            i1 = max(i0, min(a.shape[0], int(round(float(e) * SAMPLE_RATE))))
            views.append(a[i0:i1])
        return self.embed_batch(views)

    def fbank(self, clips) -> List[np.ndarray]:
        """Stage entry point: post-CMN log-mel [T, 80] per clip (MelFeatureExtractor.extractRaw)."""
        single = isinstance(clips, np.ndarray) and clips.ndim == 1
        if single:
            clips = [clips]
        rows, ptrs, ns = self._rows(clips)
        if not rows:
            return []
        T = [num_frames(r.shape[0]) for r in rows]
        stride = max(T) * N_MELS
        out = np.zeros((len(rows), stride), dtype=np.float32)
        nf = np.zeros(len(rows), dtype=np.int32)
        self._check(self.lib.qasr_spk_fbank(self.h, ptrs, ns, len(rows), _fptr(out), stride, nf.ctypes.data_as(_I)))
        res = [out[b, :nf[b] * N_MELS].reshape(nf[b], N_MELS).copy() for b in range(len(rows))]
        return res[0] if single else res

    def timing(self) -> float:
        """Device time of the last call in ms."""
        ms = C.c_float()
        self._check(self.lib.qasr_spk_timing(self.h, C.byref(ms)))
        return float(ms.value)

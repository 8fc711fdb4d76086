"""pyannote segmentation, the pyannote VAD and speaker diarization on the GPU over the C ABI (include/qasr.h, qasr_seg_* / qasr_diar_*).

Reference: Sources/SpeechVAD/Segmentation.swift (SegmentationModel), SpeechVAD.swift (PyannoteVADModel.detectSpeech), VADPipeline.swift,
PowersetDecoder.swift, DiarizationPipeline.swift (PyannoteDiarizationPipeline.diarize / extractSpeaker), DiarizationHelpers.swift.
The module-level functions are the pure-CPU pieces of the ABI.  No CPU fallback for the network.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
_L = C.POINTER(C.c_int64)
SAMPLE_RATE, NUM_CLASSES, NUM_SPEAKERS, WINDOW_SAMPLES, FRAMES_PER_WINDOW, EMBEDDING_DIM = 16000, 7, 3, 160000, 589, 256


def _fptr(a):
    return a.ctypes.data_as(_F)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- pure CPU ----
def num_frames(n: int) -> int:
    """Frames of the network for n samples (qasr_seg_num_frames); -1 below 991."""
    return int(_lib.load().qasr_seg_num_frames(int(n)))


def window_positions(n_samples: int, window_samples: int = WINDOW_SAMPLES, step_samples: int = WINDOW_SAMPLES // 2) -> List[Tuple[int, int]]:
    """VADPipeline.windowPositions / DiarizationPipeline.swift:319-332."""
    lib = _lib.load()
    cnt = lib.qasr_seg_window_positions(int(n_samples), int(window_samples), int(step_samples), None, None, 0)
    if cnt < 0:
        raise QasrError(f"qasr error {-cnt}: window and step must be positive")
    st, en = np.zeros(max(cnt, 1), np.int64), np.zeros(max(cnt, 1), np.int64)
    lib.qasr_seg_window_positions(int(n_samples), int(window_samples), int(step_samples), st.ctypes.data_as(_L), en.ctypes.data_as(_L), cnt)
    return [(int(a), int(b)) for a, b in zip(st[:cnt], en[:cnt])]


def aggregate_frames(window_probs, positions, n_samples: int, sample_rate: int = SAMPLE_RATE, window_duration: float = 10.0) -> np.ndarray:
    """VADPipeline.aggregateFrames: window_probs [W, frames]; frameDuration = window_duration / frames."""
    lib = _lib.load()
    p = _f32(window_probs)
    p = p.reshape(len(positions), -1) if len(positions) else p.reshape(0, 1)
    st = np.ascontiguousarray([a for a, _ in positions], dtype=np.int64)
    args = (_fptr(p), p.shape[0], p.shape[1], st.ctypes.data_as(_L), int(n_samples), int(sample_rate), float(window_duration))
    cnt = lib.qasr_seg_aggregate_frames(*args, None, 0)
    if cnt < 0:
        raise QasrError(f"qasr error {-cnt}: aggregate_frames")
    out = np.zeros(max(cnt, 1), np.float32)
    lib.qasr_seg_aggregate_frames(*args, _fptr(out), cnt)
    return out[:cnt]


def binarize(probs, onset: float, offset: float, frame_duration: float, min_speech: Optional[float] = None,
             min_silence: Optional[float] = None) -> List[Tuple[float, float]]:
    """PowersetDecoder.binarize; with min_speech and min_silence given, VADPipeline.binarize (its duration filter applied)."""
    lib = _lib.load()
    p = _f32(probs).ravel()
    filt = min_speech is not None
    cfg = _lib.QasrVadConfig(float(onset), float(offset), float(min_speech or 0.0), float(min_silence or 0.0))
    cap = p.shape[0] // 2 + 2
    seg = np.zeros(2 * cap, np.float32)
    cnt = lib.qasr_seg_binarize(_fptr(p), p.shape[0], float(frame_duration), C.byref(cfg), int(filt), _fptr(seg), cap)
    if cnt < 0:
        raise QasrError(f"qasr error {-cnt}: binarize")
    return [(float(seg[2 * i]), float(seg[2 * i + 1])) for i in range(cnt)]


def cosine_distance(a, b) -> float:
    """DiarizationHelpers.cosineDistance over min(len) elements."""
    x, y = _f32(a).ravel(), _f32(b).ravel()
    n = min(x.size, y.size)
    return float(_lib.load().qasr_diar_cosine_distance(_fptr(x), _fptr(y), n))


def cluster(embeddings, window_index, threshold: float) -> Tuple[List[int], np.ndarray]:
    """constrainedAgglomerativeClustering -> (assignment, centroids [k, dim])."""
    e = _f32(embeddings)
    n = e.shape[0] if e.ndim == 2 else 0
    if n == 0:
        return [], np.zeros((0, 0), np.float32)
    w = np.ascontiguousarray(window_index, dtype=np.int32)
    assign = np.zeros(n, np.int32)
    cen = np.zeros_like(e)
    k = _lib.load().qasr_diar_cluster(_fptr(e), w.ctypes.data_as(_I), n, e.shape[1], float(threshold), assign.ctypes.data_as(_I), _fptr(cen))
    if k < 0:
        raise QasrError(f"qasr error {-k}: cluster")
    return assign.tolist(), cen[:k].copy()


@dataclass
class DiarizedSegment:
    start_time: float
    end_time: float
    speaker_id: int


def _seg_array(segs):
    arr = (_lib.QasrDiarSegment * max(len(segs), 1))()
    for i, s in enumerate(segs):
        arr[i] = _lib.QasrDiarSegment(float(s.start_time), float(s.end_time), int(s.speaker_id))
    return arr


def merge_segments(segments: Sequence[DiarizedSegment], min_silence: float) -> List[DiarizedSegment]:
    """DiarizationHelpers.mergeSegments."""
    a, out = _seg_array(segments), (_lib.QasrDiarSegment * max(len(segments), 1))()
    cnt = _lib.load().qasr_diar_merge_segments(a, len(segments), float(min_silence), out)
    return [DiarizedSegment(out[i].start_time, out[i].end_time, out[i].speaker_id) for i in range(cnt)]


def compact_speaker_ids(segments: Sequence[DiarizedSegment]) -> List[DiarizedSegment]:
    """DiarizationHelpers.compactSpeakerIds."""
    a = _seg_array(segments)
    _lib.load().qasr_diar_compact_speaker_ids(a, len(segments))
    return [DiarizedSegment(a[i].start_time, a[i].end_time, a[i].speaker_id) for i in range(len(segments))]


def default_diarization_config() -> dict:
    c = _lib.QasrDiarConfig()
    _lib.load().qasr_diar_default_config(C.byref(c))
    return {n: float(getattr(c, n)) for n, _ in c._fields_}


def default_vad_config() -> dict:
    c = _lib.QasrSegVadConfig()
    _lib.load().qasr_seg_vad_default_config(C.byref(c))
    return {n: float(getattr(c, n)) for n, _ in c._fields_}


# ---- the network ----
class SegmentationModel:
    """SegmentationModel on the device with both powerset decoders."""

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, device=0, max_windows=0, order_with=None):
        """model_dir/model.safetensors in the reference's keys.  max_windows: windows one device pass holds (0 = 64).  order_with: a
        Qwen3ASRModel (or raw engine handle) on the same device whose stream orders this model's work."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_seg_create(int(device), str(model_dir).encode(), int(max_windows), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_seg_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_seg_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_seg_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_seg_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_seg_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_seg_memory_footprint(self.h))

    num_frames = staticmethod(num_frames)

    def forward(self, pcm):
        """pcm [B, n] (or [n]) -> (posteriors [B, F, 7], speaker_probs [B, F, 3], speech_probs [B, F])."""
        a = _f32(pcm)
        if a.ndim == 1:
            a = a[None]
        B, n = a.shape
        F = max(num_frames(n), 0)
        post, spk, sp = np.zeros((B, F, NUM_CLASSES), np.float32), np.zeros((B, F, NUM_SPEAKERS), np.float32), np.zeros((B, F), np.float32)
        self._check(self.lib.qasr_seg_forward(self.h, _fptr(a), B, n, _fptr(post), _fptr(spk), _fptr(sp)))
        return post, spk, sp

    def windows(self, pcm, window_samples: int = WINDOW_SAMPLES, step_samples: int = WINDOW_SAMPLES // 2):
        """Every window of one buffer in one call -> (positions, posteriors [W, F, 7], speaker_probs [W, F, 3], speech_probs [W, F])."""
        a = _f32(pcm).ravel()
        pos = window_positions(a.shape[0], window_samples, step_samples)
        W, F = len(pos), max(num_frames(window_samples), 0)
        post, spk, sp = np.zeros((W, F, NUM_CLASSES), np.float32), np.zeros((W, F, NUM_SPEAKERS), np.float32), np.zeros((W, F), np.float32)
        st, en = np.zeros(max(W, 1), np.int64), np.zeros(max(W, 1), np.int64)
        cnt = self.lib.qasr_seg_windows(self.h, _fptr(a), a.shape[0], int(window_samples), int(step_samples), _fptr(post), _fptr(spk),
                                        _fptr(sp), st.ctypes.data_as(_L), en.ctypes.data_as(_L), W)
        if cnt < 0:
            self._check(-cnt)
        return [(int(x), int(y)) for x, y in zip(st[:cnt], en[:cnt])], post, spk, sp

    def timing(self) -> float:
        ms = C.c_float()
        self._check(self.lib.qasr_seg_timing(self.h, C.byref(ms)))
        return float(ms.value)


class PyannoteVADModel:
    """PyannoteVADModel: detect_speech over a SegmentationModel."""

    def __init__(self, model: SegmentationModel, **vad_config):
        self.model = model
        self.vad_config = {**default_vad_config(), **vad_config}

    @classmethod
    def from_pretrained(cls, model_dir, device=0, max_windows=0, order_with=None, **vad_config):
        return cls(SegmentationModel.from_pretrained(model_dir, device, max_windows, order_with), **vad_config)

    def close(self):
        self.model.close()

    def detect_speech(self, audio, sample_rate: int = SAMPLE_RATE) -> List[Tuple[float, float]]:
        a = _f32(audio).ravel()
        cfg = _lib.QasrSegVadConfig(*[self.vad_config[n] for n, _ in _lib.QasrSegVadConfig._fields_])
        cap = a.shape[0] // 100 + 16
        seg = np.zeros(2 * cap, np.float32)
        m = self.model
        cnt = m.lib.qasr_seg_detect_speech(m.h, _fptr(a), a.shape[0], int(sample_rate), C.byref(cfg), _fptr(seg), cap)
        if cnt < 0:
            m._check(-cnt)
        return [(float(seg[2 * i]), float(seg[2 * i + 1])) for i in range(cnt)]


@dataclass
class DiarizationResult:
    segments: List[DiarizedSegment]
    num_speakers: int
    speaker_embeddings: np.ndarray                     # [num_speakers, 256]


class PyannoteDiarizationPipeline:
    """PyannoteDiarizationPipeline over a SegmentationModel, a WeSpeakerModel and an optional SileroVADModel pre-filter."""

    def __init__(self, segmentation: SegmentationModel, embedding, vad=None):
        self.segmentation, self.embedding, self.vad = segmentation, embedding, vad

    @classmethod
    def from_models(cls, segmentation, embedding, vad=None):
        return cls(segmentation, embedding, vad)

    def _run(self, audio, sample_rate, config):
        a = _f32(audio).ravel()
        cfg = _lib.QasrDiarConfig(*[{**default_diarization_config(), **config}[n] for n, _ in _lib.QasrDiarConfig._fields_])
        seg = self.segmentation
        r = C.c_void_p()
        seg._check(seg.lib.qasr_diarize(seg.h, self.embedding.h, self.vad.h if self.vad is not None else None, _fptr(a), a.shape[0],
                                        int(sample_rate), C.byref(cfg), C.byref(r)))
        return r

    def _result(self, r) -> DiarizationResult:
        lib = self.segmentation.lib
        cnt = C.c_size_t()
        p = lib.qasr_diar_result_segments(r, C.byref(cnt))
        segs = [DiarizedSegment(p[i].start_time, p[i].end_time, p[i].speaker_id) for i in range(cnt.value)]
        k = lib.qasr_diar_result_num_speakers(r)
        emb = np.ctypeslib.as_array(lib.qasr_diar_result_embeddings(r), (k, EMBEDDING_DIM)).copy() if k else np.zeros((0, EMBEDDING_DIM), np.float32)
        return DiarizationResult(segs, int(k), emb)

    def diarize(self, audio, sample_rate: int = SAMPLE_RATE, **config) -> DiarizationResult:
        r = self._run(audio, sample_rate, config)
        try:
            return self._result(r)
        finally:
            self.segmentation.lib.qasr_diar_result_free(r)

    def extract_speaker(self, audio, target_embedding, sample_rate: int = SAMPLE_RATE, **config) -> List[Tuple[float, float]]:
        """extractSpeaker: the segments of the speaker whose centroid is closest (cosine) to target_embedding."""
        lib = self.segmentation.lib
        t = _f32(target_embedding).ravel()
        if t.shape[0] != EMBEDDING_DIM:
            raise QasrError("qasr error 1: target embedding must have 256 elements")
        r = self._run(audio, sample_rate, config)
        try:
            cnt = C.c_size_t()
            lib.qasr_diar_result_segments(r, C.byref(cnt))
            seg = np.zeros(2 * max(cnt.value, 1), np.float32)
            c = lib.qasr_diar_extract_speaker(r, _fptr(t), _fptr(seg), cnt.value)
            return [(float(seg[2 * i]), float(seg[2 * i + 1])) for i in range(max(c, 0))]
        finally:
            lib.qasr_diar_result_free(r)

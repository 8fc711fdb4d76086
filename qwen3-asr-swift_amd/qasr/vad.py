"""Silero VAD v5 on the GPU over the C ABI (include/qasr.h, qasr_vad_*).

Reference: Sources/SpeechVAD/SileroVAD.swift:39-321 (SileroVADModel: fromPretrained, processChunk, resetState, detectSpeech, the
VoiceActivityDetectionModel / StreamingVADProvider conformances), Sources/SpeechVAD/VADPipeline.swift:117-181 (binarize).
One model object holds `max_streams` independent streams; the single-stream methods of the reference use stream 0.  No CPU fallback.
"""
import ctypes as C
from typing import List, Optional

import numpy as np

from . import _lib
from .model import QasrError
from .streaming import SpeechSegment, VADConfig

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
CHUNK_SIZE, SAMPLE_RATE, CONTEXT_SIZE = 512, 16000, 64


def _fptr(a):
    return a.ctypes.data_as(_F)


def _cfg(config: Optional[VADConfig]):
    c = _lib.QasrVadConfig()
    _lib.load().qasr_vad_default_config(C.byref(c))
    if config is not None:
        c.onset, c.offset = config.onset, config.offset
        c.min_speech_duration, c.min_silence_duration = config.min_speech_duration, config.min_silence_duration
    return c


def binarize(probs, config: Optional[VADConfig] = None) -> List[SpeechSegment]:
    """VADPipeline.binarize with detectSpeech's frame duration (qasr_vad_binarize, pure CPU)."""
    lib = _lib.load()
    p = np.ascontiguousarray(probs, dtype=np.float32)
    cfg = _cfg(config)
    cap = p.shape[0] // 2 + 1
    seg = np.zeros((cap, 2), dtype=np.float32)
    n = lib.qasr_vad_binarize(_fptr(p), p.shape[0], C.byref(cfg), _fptr(seg), cap)
    if n < 0:
        raise QasrError(f"qasr error {-n}: binarize")
    return [SpeechSegment(float(a), float(b)) for a, b in seg[:n]]


class VADPipeline:
    """The binarisation half of VADPipeline (VADPipeline.swift:117-181) as detectSpeech configures it."""

    def __init__(self, config: Optional[VADConfig] = None):
        self.config = config or VADConfig()

    def binarize(self, probs) -> List[SpeechSegment]:
        return binarize(probs, self.config)


class SileroVADModel:
    """SileroVADModel (MLX engine) on the device.  chunk_size / input_sample_rate as the reference's StreamingVADProvider."""
    chunk_size = CHUNK_SIZE
    input_sample_rate = SAMPLE_RATE
    context_size = CONTEXT_SIZE

    def __init__(self, handle, max_streams):
        self.lib, self.h, self.max_streams = _lib.load(strict=True), handle, max_streams

    @classmethod
    def from_pretrained(cls, model_dir, device=0, max_streams=64, order_with=None):
        """model_dir/model.safetensors in the reference's keys (SileroWeightLoading.swift).  order_with: a Qwen3ASRModel (or raw engine
        handle) on the same device whose stream orders the VAD's work (include/qasr.h, qasr_vad_create)."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_vad_create(int(device), str(model_dir).encode(), int(max_streams), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_vad_last_error(None).decode()}")
        return cls(h, int(max_streams))

    def close(self):
        if self.h:
            self.lib.qasr_vad_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_vad_last_error(self.h).decode()}")

    # ---- reference surface (stream 0) ----
    def process_chunk(self, samples) -> float:
        return float(self.process_chunks(np.asarray(samples, dtype=np.float32)[None], [0])[0])

    def reset_state(self, stream=0):
        self._check(self.lib.qasr_vad_reset(self.h, int(stream)))

    def detect_speech(self, audio, sample_rate=SAMPLE_RATE, config: Optional[VADConfig] = None) -> List[SpeechSegment]:
        a = np.ascontiguousarray(audio, dtype=np.float32)
        cfg = _cfg(config)
        cap = a.shape[0] // (2 * CHUNK_SIZE) + 2
        seg = np.zeros((cap, 2), dtype=np.float32)
        n = self.lib.qasr_vad_detect_speech(self.h, _fptr(a), a.shape[0], int(sample_rate), C.byref(cfg), _fptr(seg), cap)
        if n < 0:
            raise QasrError(f"qasr error {-n}: {self.lib.qasr_vad_last_error(self.h).decode()}")
        return [SpeechSegment(float(x), float(y)) for x, y in seg[:n]]

    # ---- many streams ----
    def process_chunks(self, chunks, stream_ids=None) -> np.ndarray:
        """processChunk of B distinct streams: chunks [B, 512] -> probs [B]."""
        c = np.ascontiguousarray(chunks, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] != CHUNK_SIZE:
            raise ValueError("chunks must be [B, 512]")
        B = c.shape[0]
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        out = np.zeros(B, dtype=np.float32)
        self._check(self.lib.qasr_vad_process(self.h, _fptr(c), sid.ctypes.data_as(_I) if sid is not None else None, B, _fptr(out)))
        return out

    def probs(self, buffers, stream_ids=None) -> List[np.ndarray]:
        """detectSpeech's probability loop for whole buffers (each row's stream reset first; rows in groups of max_streams when no
        stream ids are given)."""
        bufs = [np.ascontiguousarray(b, dtype=np.float32) for b in buffers]
        if stream_ids is None and len(bufs) > self.max_streams:
            out = []
            for i in range(0, len(bufs), self.max_streams):
                out += self.probs(bufs[i:i + self.max_streams])
            return out
        B = len(bufs)
        if B == 0:
            return []
        ncs = [-(-b.shape[0] // CHUNK_SIZE) for b in bufs]
        stride = max(1, max(ncs))
        ptrs = (_F * B)(*[_fptr(b) for b in bufs])
        ns = (C.c_size_t * B)(*[b.shape[0] for b in bufs])
        out = np.zeros((B, stride), dtype=np.float32)
        nc = np.zeros(B, dtype=np.int32)
        sid = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        self._check(self.lib.qasr_vad_probs(self.h, ptrs, ns, B, sid.ctypes.data_as(_I) if sid is not None else None, _fptr(out), stride,
                                            nc.ctypes.data_as(_I)))
        return [out[b, :nc[b]].copy() for b in range(B)]

    def state(self, stream=0):
        h, c, ctx = np.zeros(128, np.float32), np.zeros(128, np.float32), np.zeros(CONTEXT_SIZE, np.float32)
        self._check(self.lib.qasr_vad_state(self.h, int(stream), _fptr(h), _fptr(c), _fptr(ctx)))
        return h, c, ctx

    def timing(self):
        ms, g = C.c_float(), C.c_int()
        self._check(self.lib.qasr_vad_timing(self.h, C.byref(ms), C.byref(g)))
        return float(ms.value), bool(g.value)

    def vtable(self, stream=0):
        vt = _lib.ScVadVtable()
        self._check(self.lib.qasr_vad_vtable(self.h, int(stream), C.byref(vt)))
        return vt

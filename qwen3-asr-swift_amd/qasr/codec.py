"""The Qwen3-TTS 12.5 Hz speech tokenizer decoder on the GPU over the C ABI (include/qasr.h, qasr_codec_*).

Reference: Sources/Qwen3TTS/SpeechTokenizerDecoder.swift (SpeechTokenizerDecoder: callAsFunction, chunkedDecode, decode, decodeBatch) and
TTSWeightLoading.swift:190-247.  Codes are int32 [16, T] per utterance; the waveform is 24 kHz float32, 1920 samples per frame.
decode_batch runs every window of every utterance as one batch; the stage methods expose the split RVQ decode and the pre-transformer on
their own.  f32 throughout; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
SAMPLE_RATE, SAMPLES_PER_FRAME = 24000, 1920
STAGES = ("quantizer", "pre_transformer", "upsample", "block1", "block2", "block3", "block4", "output")


def _fptr(a):
    return a.ctypes.data_as(_F)


def _iptr(a):
    return a.ctypes.data_as(_I)


def window_positions(T: int) -> List[Tuple[int, int, int]]:
    """chunkedDecode's windows for T frames as (start, context, end) (qasr_codec_window_positions; host only)."""
    lib = _lib.load(strict=True)
    cap = max(1, int(T) // 25 + 2)
    s, c, e = ((C.c_int32 * cap)() for _ in range(3))
    n = int(lib.qasr_codec_window_positions(int(T), s, c, e, cap))
    if n < 0:
        raise QasrError(f"qasr error {-n}: window_positions({T})")
    return [(int(s[i]), int(c[i]), int(e[i])) for i in range(n)]


def tail_leads(upsample_rates=(8, 5, 4, 3)) -> List[int]:
    """Input rows before the first kept one that decoder.decoder.0, blocks 1..4 and the output conv need (qasr_codec_tail_leads; pure CPU)."""
    r = (C.c_int32 * 4)(*[int(v) for v in upsample_rates])
    out = (C.c_int32 * 6)()
    rc = _lib.load(strict=True).qasr_codec_tail_leads(r, out)
    if rc != 0:
        raise QasrError(f"qasr error {rc}: tail_leads({tuple(upsample_rates)})")
    return [int(v) for v in out]


class SpeechTokenizerDecoder:
    """SpeechTokenizerDecoder on the device."""
    sample_rate = SAMPLE_RATE

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, device=0, order_with=None, max_windows=0):
        """model_dir/model.safetensors in the checkpoint's decoder.* keys (and config.json when the geometry is not the default).
        max_windows: windows one device pass holds (0 = 16); longer inputs run in several passes with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_codec_create(int(device), str(model_dir).encode(), int(max_windows), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_codec_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_codec_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_codec_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_codec_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_codec_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_codec_memory_footprint(self.h))

    @property
    def num_quantizers(self) -> int:
        return int(self.lib.qasr_codec_num_quantizers(self.h))

    @property
    def hidden_size(self) -> int:
        return int(self.lib.qasr_codec_hidden_size(self.h))

    @property
    def latent_dim(self) -> int:
        return int(self.lib.qasr_codec_latent_dim(self.h))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last call per stage."""
        ms = (C.c_float * len(STAGES))()
        self._check(self.lib.qasr_codec_timing(self.h, ms))
        return dict(zip(STAGES, (float(v) for v in ms)))

    def _codes(self, codes, ndim):
        a = np.ascontiguousarray(codes, dtype=np.int32)
        if a.ndim == ndim - 1:
            a = a[None]
        if a.ndim != ndim or a.shape[-2] != self.num_quantizers:
            raise QasrError(f"qasr error 1: codes are [{'B, ' if ndim == 3 else ''}{self.num_quantizers}, T]")
        return a

    # ---- whole path ----
    def forward(self, codes, clip: bool = True) -> np.ndarray:
        """callAsFunction: codes [B, 16, T] (or [16, T]) with T <= 35 -> [B, 1920 T] (or [1920 T]); clip=False: the signal before the clip."""
        single = np.ndim(codes) == 2
        a = self._codes(codes, 3)
        B, _, T = a.shape
        out = np.zeros((B, SAMPLES_PER_FRAME * T), dtype=np.float32)
        self._check(self.lib.qasr_codec_forward(self.h, _iptr(a), B, T, 1 if clip else 0, _fptr(out)))
        return out[0] if single else out

    def forward_tail(self, codes, context: int, clip: bool = True) -> np.ndarray:
        """forward()[..., 1920 * context:], bit for bit, without the vocoder rows only the dropped context needs (qasr_codec_forward_tail)."""
        single = np.ndim(codes) == 2
        a = self._codes(codes, 3)
        B, _, T = a.shape
        if not 0 <= int(context) < T:
            raise QasrError("qasr error 1: the context must be shorter than the window")
        out = np.zeros((B, SAMPLES_PER_FRAME * (T - int(context))), dtype=np.float32)
        self._check(self.lib.qasr_codec_forward_tail(self.h, _iptr(a), B, T, int(context), 1 if clip else 0, _fptr(out)))
        return out[0] if single else out

    def decode(self, codes) -> np.ndarray:
        """decode(codes:): codes [16, T], any T >= 1 -> [1920 T], chunked as the reference's chunkedDecode."""
        a = self._codes(codes, 3)[0]
        out = np.zeros(SAMPLES_PER_FRAME * a.shape[1], dtype=np.float32)
        self._check(self.lib.qasr_codec_decode(self.h, _iptr(a), a.shape[1], _fptr(out)))
        return out

    def decode_batch(self, codes_list: Sequence) -> List[np.ndarray]:
        """decodeBatch: utterances of any lengths in one call; each is bit-identical to decode() of it alone."""
        items = [self._codes(c, 3)[0] for c in codes_list]
        B = len(items)
        if B == 0:
            return []
        outs = [np.zeros(SAMPLES_PER_FRAME * a.shape[1], dtype=np.float32) for a in items]
        cp = (_I * B)(*[_iptr(a) for a in items])
        op = (_F * B)(*[_fptr(o) for o in outs])
        self._check(self.lib.qasr_codec_decode_batch(self.h, cp, (C.c_size_t * B)(*[a.shape[1] for a in items]), B, op))
        return outs

    # ---- stages ----
    def quantizer_decode(self, codes) -> np.ndarray:
        """splitRVQ.decode: codes [B, 16, T] (or [16, T]) -> [B, T, hidden] (or [T, hidden])."""
        single = np.ndim(codes) == 2
        a = self._codes(codes, 3)
        B, _, T = a.shape
        out = np.zeros((B, T, self.hidden_size), dtype=np.float32)
        self._check(self.lib.qasr_codec_quantizer_decode(self.h, _iptr(a), B, T, _fptr(out)))
        return out[0] if single else out

    def pre_transformer(self, x) -> np.ndarray:
        """DecoderTransformer: x [B, T, latent] (or [T, latent]) -> the same shape."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        single = a.ndim == 2
        if single:
            a = a[None]
        if a.ndim != 3 or a.shape[2] != self.latent_dim:
            raise QasrError(f"qasr error 1: x is [B, T, {self.latent_dim}]")
        out = np.zeros_like(a)
        self._check(self.lib.qasr_codec_pre_transformer(self.h, _fptr(a), a.shape[0], a.shape[1], _fptr(out)))
        return out[0] if single else out


ENC_STAGES = ("input", "block1", "block2", "block3", "block4", "downsample", "pre_transformer", "quantizer")


def num_frames(n: int) -> int:
    """Frames of a clip of n samples: ceil(n / 1920) (qasr_codec_enc_num_frames; host only)."""
    return int(_lib.load(strict=True).qasr_codec_enc_num_frames(int(n)))


class SpeechTokenizerEncoder:
    """SpeechTokenizerEncoder on the device (Sources/Qwen3TTS/SpeechTokenizerEncoder.swift; include/qasr.h, qasr_codec_enc_*):
    24 kHz mono float32 PCM -> int32 codes [16, ceil(n / 1920)].  f32 throughout; no CPU fallback."""
    sample_rate = SAMPLE_RATE

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, device=0, order_with=None, max_samples=0):
        """model_dir/model.safetensors in the checkpoint's encoder.* keys (the decoder.* keys may sit beside them) and config.json when
        the geometry is not the default.  max_samples: samples one device pass holds (0 = 720000); a longer clip is refused, a longer
        batch runs in several passes with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_codec_enc_create(int(device), str(model_dir).encode(), int(max_samples), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_codec_enc_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_codec_enc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_codec_enc_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_codec_enc_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_codec_enc_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_codec_enc_memory_footprint(self.h))

    @property
    def num_quantizers(self) -> int:
        return int(self.lib.qasr_codec_enc_num_quantizers(self.h))

    @property
    def hidden_size(self) -> int:
        return int(self.lib.qasr_codec_enc_hidden_size(self.h))

    @property
    def latent_dim(self) -> int:
        return int(self.lib.qasr_codec_enc_latent_dim(self.h))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last call per stage."""
        ms = (C.c_float * len(ENC_STAGES))()
        self._check(self.lib.qasr_codec_enc_timing(self.h, ms))
        return dict(zip(ENC_STAGES, (float(v) for v in ms)))

    def _batch(self, fn, clips, width):
        """clips -> one array per clip: int32 [Q, frames] (width None) or float32 [frames, width]."""
        items = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in clips]
        B = len(items)
        if B == 0:
            return []
        frames = [num_frames(a.size) for a in items]
        if width is None:
            outs = [np.zeros((self.num_quantizers, f), dtype=np.int32) for f in frames]
            op = (_I * B)(*[_iptr(o) for o in outs])
        else:
            outs = [np.zeros((f, width), dtype=np.float32) for f in frames]
            op = (_F * B)(*[_fptr(o) for o in outs])
        pp = (_F * B)(*[_fptr(a) for a in items])
        self._check(fn(self.h, pp, (C.c_size_t * B)(*[a.size for a in items]), B, op))
        return outs

    # ---- whole path ----
    def encode(self, pcm) -> np.ndarray:
        """encode(samples:): pcm [n] -> codes [16, ceil(n / 1920)]."""
        a = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        out = np.zeros((self.num_quantizers, num_frames(a.size)), dtype=np.int32)
        self._check(self.lib.qasr_codec_enc_encode(self.h, _fptr(a), a.size, _iptr(out)))
        return out

    def encode_batch(self, clips: Sequence) -> List[np.ndarray]:
        """Clips of any lengths in one call; each is bit-identical to encode() of it alone."""
        return self._batch(self.lib.qasr_codec_enc_encode_batch, clips, None)

    # ---- stages ----
    def conv(self, pcm) -> np.ndarray:
        """The convolutional front up to post_conv: pcm [n] -> [frames, latent]."""
        return self.conv_batch([pcm])[0]

    def conv_batch(self, clips: Sequence) -> List[np.ndarray]:
        return self._batch(self.lib.qasr_codec_enc_conv_batch, clips, self.latent_dim)

    def latent(self, pcm) -> np.ndarray:
        """... and the unmasked pre-transformer with its final norm: pcm [n] -> [frames, hidden]."""
        return self.latent_batch([pcm])[0]

    def latent_batch(self, clips: Sequence) -> List[np.ndarray]:
        return self._batch(self.lib.qasr_codec_enc_latent_batch, clips, self.hidden_size)

    def quantize(self, h) -> np.ndarray:
        """EncoderRVQ.encode: h [F, hidden] -> codes [16, F]."""
        a = np.ascontiguousarray(h, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != self.hidden_size:
            raise QasrError(f"qasr error 1: h is [F, {self.hidden_size}]")
        out = np.zeros((self.num_quantizers, a.shape[0]), dtype=np.int32)
        self._check(self.lib.qasr_codec_enc_quantize(self.h, _fptr(a), a.shape[0], _iptr(out)))
        return out

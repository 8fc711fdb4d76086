"""The CosyVoice3 speech tokenizer (S3-Tokenizer-v3) and voice profiles on the GPU over the C ABI (include/qasr.h, qasr_s3tok_*).

Reference: Sources/CosyVoiceTTS/SpeechTokenizer.swift, WhisperMelExtractor.swift, FlowMelExtractor.swift, VoiceCloning.swift:69-158
(extractVoiceProfile) and :329-345 (the resampler).  A reference clip at any sample rate gives the prompt speech tokens (25 Hz) and the
prompt mel ([80, frames], 50 Hz) that CosyVoiceTTS.synthesize and CosyVoiceFlow.generate take for zero-shot cloning; the 192-d CAM++
vector stays a caller input.  whisper_mel(), flow_mel(), hidden(), project() are the stages; encode() is the tokenizer and profile() the
whole front end.  bf16 GEMM operands, f32 everywhere else; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
N_MELS, N_STATE, FSQ_DIMS, CODES, FLOW_MELS, SR_TOKENIZER, SR_FLOW = 128, 1280, 8, 6561, 80, 16000, 24000
STAGES = ("mel", "stems", "blocks", "fsq")


def _pcm(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def _fptr(a):
    return a.ctypes.data_as(_F)


def _iptr(a):
    return a.ctypes.data_as(_I)


def whisper_frames(n_samples: int) -> int:
    """Mel frames of n samples at 16 kHz: n // 160, the last frame dropped (host only)."""
    return int(_lib.load(strict=True).qasr_s3tok_whisper_frames(int(n_samples)))


def tokens_of(mel_frames: int) -> int:
    """Tokens of T mel frames: two convs k 3, stride 2, pad 1 (host only)."""
    return int(_lib.load(strict=True).qasr_s3tok_tokens(int(mel_frames)))


def flow_frames(n_samples: int) -> int:
    """Flow mel frames of n samples at 24 kHz: n // 480 for n >= 480, else 0 (host only)."""
    return int(_lib.load(strict=True).qasr_s3tok_flow_frames(int(n_samples)))


def resampled_length(n: int, src: int, dst: int) -> int:
    return int(_lib.load(strict=True).qasr_s3tok_resampled_length(int(n), int(src), int(dst)))


def profile_cut(n_tokens: int, frames: int) -> int:
    """The profile's common length L = min(tokens, frames // 2) (host only)."""
    return int(_lib.load(strict=True).qasr_s3tok_profile_cut(int(n_tokens), int(frames)))


def resample(x, src: int, dst: int) -> np.ndarray:
    """The reference's linear resampler, bit for bit (host only)."""
    x = _pcm(x)
    out = np.zeros(resampled_length(x.size, src, dst), dtype=np.float32)
    if _lib.load(strict=True).qasr_s3tok_resample(_fptr(x), x.size, int(src), int(dst), _fptr(out)) != 0:
        raise QasrError("qasr error 1: sample rates must be positive")
    return out


def fsq_host(proj) -> np.ndarray:
    """Projections [rows, 8] -> codes, the host twin of the device's FSQ lines."""
    p = np.ascontiguousarray(proj, dtype=np.float32).reshape(-1, FSQ_DIMS)
    out = np.zeros(p.shape[0], dtype=np.int32)
    _lib.load(strict=True).qasr_s3tok_fsq_host(_fptr(p), p.shape[0], _iptr(out))
    return out


class SpeechTokenizer:
    """SpeechTokenizerModel, the two mel extractors and extractVoiceProfile on the device."""

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, max_tokens=0, order_with=None, device=0):
        """model_dir holds speech_tokenizer.safetensors.  max_tokens: tokens, summed over clips, one device pass holds (0 = 768, 30 s);
        a longer clip is refused, a longer batch runs in several passes with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_s3tok_create(int(device), str(model_dir).encode(), int(max_tokens), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_s3tok_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_s3tok_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_s3tok_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_s3tok_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_s3tok_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_s3tok_memory_footprint(self.h))

    @property
    def depth(self) -> int:
        return int(self.lib.qasr_s3tok_depth(self.h))

    @property
    def max_tokens(self) -> int:
        return int(self.lib.qasr_s3tok_max_tokens(self.h))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last encode / hidden / project / profile per stage, summed over passes."""
        ms = (C.c_float * len(STAGES))()
        self._check(self.lib.qasr_s3tok_timing(self.h, ms))
        return dict(zip(STAGES, (float(v) for v in ms)))

    # ---- stages ----
    def whisper_mel(self, pcm16k) -> np.ndarray:
        """16 kHz PCM -> [128, n // 160]."""
        x = _pcm(pcm16k)
        out = np.zeros((N_MELS, whisper_frames(x.size)), dtype=np.float32)
        self._check(self.lib.qasr_s3tok_whisper_mel(self.h, _fptr(x), x.size, _fptr(out)))
        return out

    def flow_mel(self, pcm24k) -> np.ndarray:
        """24 kHz PCM -> [80, n // 480]."""
        x = _pcm(pcm24k)
        out = np.zeros((FLOW_MELS, flow_frames(x.size)), dtype=np.float32)
        self._check(self.lib.qasr_s3tok_flow_mel(self.h, _fptr(x), x.size, _fptr(out)))
        return out

    @staticmethod
    def _mel(mel):
        m = np.ascontiguousarray(mel, dtype=np.float32)
        if m.ndim != 2 or m.shape[0] != N_MELS:
            raise QasrError(f"qasr error 1: mel is [{N_MELS}, T]")
        return m

    def hidden(self, mel) -> np.ndarray:
        """mel [128, T] -> the residual stream after the last block, [tokens, 1280]."""
        m = self._mel(mel)
        out = np.zeros((tokens_of(m.shape[1]), N_STATE), dtype=np.float32)
        self._check(self.lib.qasr_s3tok_hidden(self.h, _fptr(m), m.shape[1], _fptr(out)))
        return out

    def project(self, mel) -> np.ndarray:
        """mel [128, T] -> project_down's output before tanh, [tokens, 8]."""
        m = self._mel(mel)
        out = np.zeros((tokens_of(m.shape[1]), FSQ_DIMS), dtype=np.float32)
        self._check(self.lib.qasr_s3tok_project(self.h, _fptr(m), m.shape[1], _fptr(out)))
        return out

    # ---- whole model ----
    def encode(self, pcm16k) -> np.ndarray:
        """16 kHz PCM -> int32 codes at 25 Hz."""
        x = _pcm(pcm16k)
        out = np.zeros(tokens_of(whisper_frames(x.size)), dtype=np.int32)
        self._check(self.lib.qasr_s3tok_encode(self.h, _fptr(x), x.size, _iptr(out)))
        return out

    def encode_batch(self, clips: Sequence) -> List[np.ndarray]:
        """Clips of any lengths in one call; each result is bit-identical to encode() of the clip alone."""
        xs = [_pcm(c) for c in clips]
        B = len(xs)
        if B == 0:
            return []
        outs = [np.zeros(tokens_of(whisper_frames(x.size)), dtype=np.int32) for x in xs]
        self._check(self.lib.qasr_s3tok_encode_batch(self.h, (_F * B)(*[_fptr(x) for x in xs]), (C.c_size_t * B)(*[x.size for x in xs]), B,
                                                     (_I * B)(*[_iptr(o) for o in outs])))
        return outs

    def profile(self, pcm, sample_rate: int, spk_emb=None, prompt_text_ids=None):
        """A reference clip at any sample rate -> a VoiceProfile (qasr.cosyvoice) with tokens [L] and prompt_feat [80, 2 L]."""
        return self.profile_batch([pcm], [sample_rate], [spk_emb], [prompt_text_ids])[0]

    def profile_batch(self, clips: Sequence, sample_rates: Sequence[int], spk_emb=None, prompt_text_ids=None):
        from .cosyvoice import VoiceProfile
        xs = [_pcm(c) for c in clips]
        B = len(xs)
        none = [None] * B
        se, pt = list(spk_emb or none), list(prompt_text_ids or none)
        if not (len(sample_rates) == len(se) == len(pt) == B):
            raise QasrError("qasr error 1: one entry per clip")
        if B == 0:
            return []
        srs = [int(s) for s in sample_rates]
        if any(s <= 0 for s in srs):
            raise QasrError("qasr error 1: sample rates must be positive")
        nt = [tokens_of(whisper_frames(resampled_length(x.size, s, SR_TOKENIZER))) for x, s in zip(xs, srs)]
        nf = [flow_frames(resampled_length(x.size, s, SR_FLOW)) for x, s in zip(xs, srs)]
        tok = [np.zeros(max(n, 1), dtype=np.int32) for n in nt]
        feat = [np.zeros(FLOW_MELS * max(n, 1), dtype=np.float32) for n in nf]
        L, F2, ut, uf = ((C.c_size_t * B)() for _ in range(4))
        self._check(self.lib.qasr_s3tok_profile_batch(
            self.h, (_F * B)(*[_fptr(x) for x in xs]), (C.c_size_t * B)(*[x.size for x in xs]), (C.c_int * B)(*srs), B,
            (_I * B)(*[_iptr(t) for t in tok]), L, (_F * B)(*[_fptr(f) for f in feat]), F2, ut, uf))
        return [VoiceProfile(tokens=tok[b][:L[b]].copy(), prompt_feat=feat[b][:FLOW_MELS * F2[b]].reshape(FLOW_MELS, F2[b]).copy(),
                             spk_emb=None if se[b] is None else np.ascontiguousarray(se[b], dtype=np.float32).reshape(-1),
                             prompt_text_ids=None if pt[b] is None else [int(i) for i in pt[b]],
                             uncut_tokens=int(ut[b]), uncut_frames=int(uf[b])) for b in range(B)]

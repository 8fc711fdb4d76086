"""The Qwen3-TTS Talker + code predictor on the GPU over the C ABI (include/qasr.h, qasr_tts_*).

Reference: Sources/Qwen3TTS/Qwen3TTS.swift (Qwen3TTSModel.synthesize, synthesizeBatch, synthesizeWithVoiceClone in x-vector mode),
Qwen3TTS+ICL.swift (synthesizeWithVoiceCloneICL), Talker.swift, CodePredictor.swift, Sampling.swift, Configuration.swift.  Text -> ids stays with the caller: the wrapper builds the chat
template of prepareTextTokens / prepareInstructTokens around ids it is given.  Codes are int32 [16, n_frames] per row at 12.5 Hz; with a
SpeechTokenizerDecoder (qasr.codec) they become 24 kHz float32 audio, in one piece or streamed in chunks (TtsStreamPool,
synthesize_stream).  No CPU fallback.
"""
import ctypes as C
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
NUM_CODE_GROUPS = 16
IM_START, IM_END, NEWLINE, ASSISTANT, USER = 151644, 151645, 198, 77091, 872


class CodecTokens:
    """Configuration.swift:152-193."""
    codec_pad, codec_bos, codec_eos = 2148, 2149, 2150
    codec_think, codec_nothink, codec_think_bos, codec_think_eos = 2154, 2155, 2156, 2157
    tts_pad, tts_bos, tts_eos = 151671, 151672, 151673
    languages = {"english": 2050, "german": 2052, "chinese": 2055, "japanese": 2058, "spanish": 2054, "french": 2061, "korean": 2064,
                 "russian": 2069, "italian": 2070, "portuguese": 2071, "beijing_dialect": 2074, "sichuan_dialect": 2062}
    short = {"en": "english", "de": "german", "zh": "chinese", "ja": "japanese", "es": "spanish", "fr": "french", "ko": "korean",
             "ru": "russian", "it": "italian", "pt": "portuguese"}

    @classmethod
    def language_id(cls, language: str) -> Optional[int]:
        """languageId(for:): the codec id of a language name or two-letter code, None when unknown."""
        key = str(language).lower()
        return cls.languages.get(cls.short.get(key, key))


@dataclass
class SamplingConfig:
    """Sampling.swift:5-30 (minP is declared and never read there: no field)."""
    temperature: float = 0.9
    top_k: int = 50
    top_p: float = 1.0
    repetition_penalty: float = 1.05
    max_tokens: int = 4096
    eos_logit_bias: float = 0.0

    @classmethod
    def greedy(cls) -> "SamplingConfig":
        return cls(temperature=0.0, top_k=1)

    def c_struct(self) -> _lib.QasrTtsSampling:
        return _lib.QasrTtsSampling(float(self.temperature), int(self.top_k), float(self.top_p), float(self.repetition_penalty),
                                    int(self.max_tokens), float(self.eos_logit_bias))


@dataclass
class StreamingConfig:
    """StreamingConfig (Qwen3TTS.swift): frames of the first chunk, of every later one, and of the codec's left context per chunk."""
    first_chunk_frames: int = 3
    chunk_frames: int = 25
    decoder_left_context: int = 10

    @classmethod
    def default(cls) -> "StreamingConfig":
        return cls()

    @classmethod
    def low_latency(cls) -> "StreamingConfig":
        return cls(1, 15, 10)

    def c_struct(self) -> _lib.QasrTtsStreamConfig:
        return _lib.QasrTtsStreamConfig(int(self.first_chunk_frames), int(self.chunk_frames), int(self.decoder_left_context))


@dataclass
class AudioChunk:
    """AudioChunk: float32 samples [1920 * n_frames] at 24 kHz from frame `frame_index` on; `codes` int32 [16, n_frames] of the chunk and
    `stream` (the pool's name of the stream) beside the reference's fields."""
    samples: np.ndarray
    frame_index: int
    is_final: bool
    codes: Optional[np.ndarray] = None
    stream: int = 0


def stream_chunks(n_frames: int, ended_by_eos: bool, config: Optional[StreamingConfig] = None) -> List[tuple]:
    """The (frame_index, n_frames, is_final) chunks a stream of n_frames frames is cut into (qasr_tts_stream_chunks; pure CPU)."""
    sc = (config or StreamingConfig()).c_struct()
    cap = int(n_frames) + 2
    a, b, c = ((C.c_int32 * cap)() for _ in range(3))
    n = _lib.load(strict=True).qasr_tts_stream_chunks(int(n_frames), int(bool(ended_by_eos)), C.byref(sc), a, b, c, cap)
    if n < 0:
        raise QasrError(f"qasr error {-n}: stream_chunks({n_frames}, {ended_by_eos}, {config})")
    return [(int(a[i]), int(b[i]), bool(c[i])) for i in range(n)]


def prepare_text_tokens(text_ids: Sequence[int]) -> List[int]:
    """prepareTextTokens: <|im_start|>assistant\\n{text}<|im_end|>\\n<|im_start|>assistant\\n around the caller's ids."""
    return [IM_START, ASSISTANT, NEWLINE, *[int(t) for t in text_ids], IM_END, NEWLINE, IM_START, ASSISTANT, NEWLINE]


def prepare_instruct_tokens(instruct_ids: Sequence[int]) -> List[int]:
    """prepareInstructTokens: <|im_start|>user\\n{instruct}<|im_end|>\\n."""
    return [IM_START, USER, NEWLINE, *[int(t) for t in instruct_ids], IM_END, NEWLINE]


def default_config(model: str = "0.6B", bits: int = 4, **over) -> _lib.QasrTtsConfig:
    """Qwen3TTSConfig.config(for:bits:) with the CodecTokens ids; keyword arguments replace fields."""
    cfg = _lib.QasrTtsConfig()
    rc = _lib.load(strict=True).qasr_tts_default_config(model.encode(), int(bits), C.byref(cfg))
    if rc != 0:
        raise QasrError(f"qasr error {rc}: default_config({model!r}, {bits})")
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise QasrError(f"qasr error 1: qasr_tts_config has no field {k}")
        setattr(cfg, k, v)
    return cfg


def sample_host(logits, sampling: SamplingConfig, talker=True, history=(), seed=0, row_index=0, frame=0, group=0, cfg=None) -> int:
    """The host twin of the device sampler on one row of logits (qasr_tts_sample_host; pure CPU)."""
    a = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    h = np.ascontiguousarray(history, dtype=np.int32).reshape(-1)
    s = sampling.c_struct()
    rc = _lib.load(strict=True).qasr_tts_sample_host(C.byref(cfg) if cfg is not None else None, a.ctypes.data_as(_F), a.size, int(bool(talker)),
                                                     C.byref(s), h.ctypes.data_as(_I), h.size, int(seed), int(row_index), int(frame), int(group))
    if rc < 0:
        raise QasrError(f"qasr error {-rc}: sample_host")
    return int(rc)


class _Request:
    """The C request of a batch; keeps the arrays it points to alive."""

    def __init__(self, texts, languages, speakers=None, xvectors=None, instructs=None, row_index=None):
        B = len(texts)
        self.keep = []

        def rows(items):
            arrs = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in items]
            self.keep.append(arrs)
            return (_I * B)(*[a.ctypes.data_as(_I) for a in arrs]), (C.c_int32 * B)(*[a.size for a in arrs])

        if isinstance(languages, (int, np.integer)):
            languages = [languages] * B
        if len(languages) != B:
            raise QasrError("qasr error 1: one language id per row")
        rq = _lib.QasrTtsRequest()
        rq.B = B
        self.text, self.text_len = rows(texts)
        rq.text, rq.text_len = self.text, self.text_len
        self.lang = (C.c_int32 * B)(*[int(v) for v in languages])
        rq.language = self.lang
        if speakers is not None:
            self.spk = (C.c_int32 * B)(*[-1 if v is None else int(v) for v in speakers])
            rq.speaker = self.spk
        if xvectors is not None:
            arrs = [None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in xvectors]
            self.keep.append(arrs)
            self.xv = (_F * B)(*[None if a is None else a.ctypes.data_as(_F) for a in arrs])
            self.xv_sizes = [None if a is None else a.size for a in arrs]
            rq.xvector = self.xv
        if instructs is not None:
            self.ins, self.ins_len = rows([[] if v is None else v for v in instructs])
            rq.instruct, rq.instruct_len = self.ins, self.ins_len
        if row_index is not None:
            self.ridx = (C.c_int64 * B)(*[int(v) for v in row_index])
            rq.row_index = self.ridx
        self.rq = rq


class _Icl:
    """The C ICL side of a batch (qasr_tts_icl); keeps the arrays it points to alive."""

    def __init__(self, ref_texts, ref_codes):
        B = len(ref_codes)
        if len(ref_texts) != B:
            raise QasrError("qasr error 1: one reference text per row")
        self.text = [np.ascontiguousarray([] if t is None else t, dtype=np.int32).reshape(-1) for t in ref_texts]
        self.codes = [np.ascontiguousarray(c, dtype=np.int32) for c in ref_codes]
        for c in self.codes:
            if c.ndim != 2 or c.shape[0] != NUM_CODE_GROUPS:
                raise QasrError("qasr error 1: reference codes are [16, frames] per row")
        self.tp = (_I * B)(*[a.ctypes.data_as(_I) for a in self.text])
        self.tl = (C.c_int32 * B)(*[a.size for a in self.text])
        self.cp = (_I * B)(*[a.ctypes.data_as(_I) for a in self.codes])
        self.cf = (C.c_int32 * B)(*[a.shape[1] for a in self.codes])
        self.icl = _lib.QasrTtsIcl(self.tp, self.tl, self.cp, self.cf)


class TtsStreamPool:
    """Up to max_batch concurrent streams over one Talker and one codec (qasr_tts_pool_*): open() queues a stream, step() runs all of
    them to the next due chunk.  While the pool is open the model's one-shot calls are refused; close_pool() gives the model back."""

    def __init__(self, model: "Qwen3TTSModel", codec, sampling: Optional[SamplingConfig] = None, seed: int = 0):
        self.lib, self.model, self.codec, self.h = model.lib, model, codec, None
        s = (sampling or SamplingConfig()).c_struct()
        h = C.c_void_p()
        model._check(self.lib.qasr_tts_pool_create(model.h, getattr(codec, "h", codec), C.byref(s), int(seed), C.byref(h)))
        self.h = h
        model._pool = weakref.ref(self)                                     # Qwen3TTSModel.close() destroys a pool it still has
        self._chunks = (_lib.QasrTtsChunk * model.cfg.max_batch)()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_tts_pool_last_error(self.h).decode()}")

    def open(self, text, language, config: Optional[StreamingConfig] = None, speaker=None, xvector=None, instruct=None, row_index: int = 0,
             _request=None) -> int:
        """One templated id list (prepare_text_tokens) -> the stream's name, valid until its final chunk or close()."""
        rq = _request or self.model._request([text], [language], None if speaker is None else [speaker], None if xvector is None else [xvector],
                                             None if instruct is None else [instruct], [row_index])
        sc = (config or StreamingConfig()).c_struct()
        stream = C.c_int32(-1)
        self._check(self.lib.qasr_tts_pool_open(self.h, C.byref(rq.rq), C.byref(sc), C.byref(stream)))
        return int(stream.value)

    def step(self) -> List[AudioChunk]:
        """Runs every live stream to the next due chunk; [] only when no stream is live.  The chunks are copies."""
        n = C.c_size_t(0)
        self._check(self.lib.qasr_tts_pool_step(self.h, self._chunks, len(self._chunks), C.byref(n)))
        out = []
        for c in self._chunks[:n.value]:
            f = int(c.n_frames)
            samples = np.ctypeslib.as_array(c.samples, (int(c.n_samples),)).copy() if f else np.zeros(0, dtype=np.float32)
            codes = np.ctypeslib.as_array(c.codes, (NUM_CODE_GROUPS, f)).copy() if f else np.zeros((NUM_CODE_GROUPS, 0), dtype=np.int32)
            out.append(AudioChunk(samples, int(c.frame_index), bool(c.is_final), codes, int(c.stream)))
        return out

    def timing(self) -> dict:
        """Host milliseconds of the last step: admission, frames (with the polls and the code reads), codec."""
        ms = (C.c_float * 3)()
        self._check(self.lib.qasr_tts_pool_timing(self.h, ms))
        return dict(zip(("admission", "frames", "codec"), (float(v) for v in ms)))

    def close(self, stream: int):
        """Cancels a stream; its slot is free at once."""
        self._check(self.lib.qasr_tts_pool_close(self.h, int(stream)))

    @property
    def live(self) -> int:
        return int(self.lib.qasr_tts_pool_live(self.h))

    def close_pool(self):
        if self.h:
            if self.model.h:                                                # never behind the handle it borrows
                self.lib.qasr_tts_pool_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close_pool()

    def __del__(self):
        self.close_pool()


class Qwen3TTSModel:
    """Qwen3TTSModel on the device: ids in, codes (and with a codec, audio) out."""

    def __init__(self, handle, cfg):
        self.lib, self.h, self.cfg = _lib.load(strict=True), handle, cfg
        self._pool = None

    @classmethod
    def from_pretrained(cls, model_dir, cfg=None, max_ref_frames=None, max_ref_text=None, **over):
        """model_dir: the main model directory (talker.* keys in any *.safetensors file).  cfg: a qasr_tts_config (default_config());
        keyword arguments replace fields of it (max_batch, max_frames, max_text, max_instruct, device, ...).  max_ref_frames (and
        max_ref_text, default 0): an ICL handle (qasr_tts_create_icl) that holds reference clips of that many frames and transcript ids."""
        lib = _lib.load(strict=True)
        cfg = cfg if cfg is not None else default_config()
        for k, v in over.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        if max_ref_frames is None and max_ref_text is None:
            rc = lib.qasr_tts_create(str(model_dir).encode(), C.byref(cfg), C.byref(h))
        else:
            rc = lib.qasr_tts_create_icl(str(model_dir).encode(), C.byref(cfg), int(max_ref_frames or 0), int(max_ref_text or 0), C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_tts_last_error(None).decode()}")
        return cls(h, cfg)

    def close(self):
        pool = self._pool() if self._pool is not None else None
        if pool is not None:
            pool.close_pool()                                               # the pool borrows the handle: it goes first
        if self.h:
            self.lib.qasr_tts_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_tts_last_error(self.h).decode()}")

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_tts_memory_footprint(self.h))

    @property
    def device_bytes(self) -> int:
        return int(self.lib.qasr_tts_device_bytes(self.h))

    def _request(self, texts, languages, speakers, xvectors, instructs, row_index):
        rq = _Request(texts, languages, speakers, xvectors, instructs, row_index)
        for n in getattr(rq, "xv_sizes", []):
            if n is not None and n != self.cfg.hidden:
                raise QasrError(f"qasr error 1: an x-vector holds {n} floats, the Talker's hidden size is {self.cfg.hidden}")
        return rq

    # ---- codes ----
    def generate_codes(self, texts, languages, sampling: Optional[SamplingConfig] = None, seed: int = 0, speakers=None, xvectors=None,
                       instructs=None, row_index=None) -> List[np.ndarray]:
        """texts: templated id lists (prepare_text_tokens), one per row -> int32 [16, n_frames] per row."""
        rq = self._request(texts, languages, speakers, xvectors, instructs, row_index)
        s = (sampling or SamplingConfig()).c_struct()
        B, F = len(texts), self.cfg.max_frames
        codes = np.zeros((B, NUM_CODE_GROUPS, F), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        self._check(self.lib.qasr_tts_generate(self.h, C.byref(rq.rq), C.byref(s), int(seed), codes.ctypes.data_as(_I), n.ctypes.data_as(_I)))
        return [codes[b, :, :int(n[b])].copy() for b in range(B)]

    def forced(self, texts, languages, codes, speakers=None, xvectors=None, instructs=None, want=("talker", "cp", "hidden")):
        """Teacher-forced pass on codes [B, 16, T] -> dict of talker logits [B, T, codec_vocab], cp logits [B, T, 15, cp_vocab] and
        post-norm hidden states [B, T, hidden]."""
        rq = self._request(texts, languages, speakers, xvectors, instructs, None)
        c = np.ascontiguousarray(codes, dtype=np.int32)
        B, G, T = c.shape
        if B != len(texts) or G != NUM_CODE_GROUPS:
            raise QasrError("qasr error 1: forced codes are [B, 16, T]")
        out = {}
        if "talker" in want:
            out["talker"] = np.zeros((B, T, self.cfg.codec_vocab), dtype=np.float32)
        if "cp" in want:
            out["cp"] = np.zeros((B, T, NUM_CODE_GROUPS - 1, self.cfg.cp_vocab), dtype=np.float32)
        if "hidden" in want:
            out["hidden"] = np.zeros((B, T, self.cfg.hidden), dtype=np.float32)
        ptr = lambda k: out[k].ctypes.data_as(_F) if k in out else None
        self._check(self.lib.qasr_tts_forced(self.h, C.byref(rq.rq), c.ctypes.data_as(_I), T, ptr("talker"), ptr("cp"), ptr("hidden")))
        return out

    # ---- ICL voice cloning (Qwen3TTS+ICL.swift) ----
    @property
    def icl_capacity(self):
        """(max_ref_frames, max_ref_text) of the handle; (0, 0) on a plain one."""
        f, t = C.c_int32(), C.c_int32()
        self._check(self.lib.qasr_tts_icl_capacity(self.h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def generate_codes_icl(self, texts, languages, xvectors, ref_texts, ref_codes, sampling: Optional[SamplingConfig] = None, seed: int = 0,
                           row_index=None, speakers=None, instructs=None) -> List[np.ndarray]:
        """generate_codes with the ICL prompt: ref_texts = tokenizer.encode(referenceText) per row (no template), ref_codes int32
        [16, frames] per row (qasr.codec SpeechTokenizerEncoder.encode), xvectors [hidden] per row."""
        rq = self._request(texts, languages, speakers, xvectors, instructs, row_index)
        icl = _Icl(ref_texts, ref_codes)
        s = (sampling or SamplingConfig()).c_struct()
        B, F = len(texts), self.cfg.max_frames
        codes = np.zeros((B, NUM_CODE_GROUPS, F), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        self._check(self.lib.qasr_tts_generate_icl(self.h, C.byref(rq.rq), C.byref(icl.icl), C.byref(s), int(seed), codes.ctypes.data_as(_I),
                                                   n.ctypes.data_as(_I)))
        return [codes[b, :, :int(n[b])].copy() for b in range(B)]

    def forced_icl(self, texts, languages, xvectors, ref_texts, ref_codes, codes, want=("talker", "cp", "hidden")):
        """forced with the ICL prompt."""
        rq = self._request(texts, languages, None, xvectors, None, None)
        icl = _Icl(ref_texts, ref_codes)
        c = np.ascontiguousarray(codes, dtype=np.int32)
        B, G, T = c.shape
        if B != len(texts) or G != NUM_CODE_GROUPS:
            raise QasrError("qasr error 1: forced codes are [B, 16, T]")
        out = {}
        if "talker" in want:
            out["talker"] = np.zeros((B, T, self.cfg.codec_vocab), dtype=np.float32)
        if "cp" in want:
            out["cp"] = np.zeros((B, T, NUM_CODE_GROUPS - 1, self.cfg.cp_vocab), dtype=np.float32)
        if "hidden" in want:
            out["hidden"] = np.zeros((B, T, self.cfg.hidden), dtype=np.float32)
        ptr = lambda k: out[k].ctypes.data_as(_F) if k in out else None
        self._check(self.lib.qasr_tts_forced_icl(self.h, C.byref(rq.rq), C.byref(icl.icl), c.ctypes.data_as(_I), T, ptr("talker"), ptr("cp"),
                                                 ptr("hidden")))
        return out

    def icl_prompt(self, texts, languages, xvectors, ref_texts, ref_codes) -> List[np.ndarray]:
        """The ICL prompt rows as the Talker reads them: float32 [P, hidden] per row (bf16 values)."""
        rq = self._request(texts, languages, None, xvectors, None, None)
        icl = _Icl(ref_texts, ref_codes)
        B = len(texts)
        pmax = max(11 + icl.text[b].size + max(len(texts[b]) - 8, 0) + icl.codes[b].shape[1] for b in range(B)) if B else 0
        rows = np.zeros((B, pmax, self.cfg.hidden), dtype=np.float32)
        P = np.zeros(B, dtype=np.int32)
        self._check(self.lib.qasr_tts_icl_prompt(self.h, C.byref(rq.rq), C.byref(icl.icl), rows.ctypes.data_as(_F), P.ctypes.data_as(_I)))
        return [rows[b, :int(P[b])].copy() for b in range(B)]

    def synthesize_batch_icl(self, codec, texts, languages, xvectors, ref_texts, ref_codes, sampling: Optional[SamplingConfig] = None,
                             seed: int = 0, row_index=None, return_codes=False):
        """qasr_tts_synthesize_icl: the ICL codes, then `codec` -> float32 [1920 * n_frames] per row."""
        rq = self._request(texts, languages, None, xvectors, None, row_index)
        icl = _Icl(ref_texts, ref_codes)
        s = (sampling or SamplingConfig()).c_struct()
        B, F = len(texts), self.cfg.max_frames
        pcm = [np.zeros(1920 * F, dtype=np.float32) for _ in range(B)]
        pp = (_F * B)(*[a.ctypes.data_as(_F) for a in pcm])
        ns = (C.c_size_t * B)()
        codes = np.zeros((B, NUM_CODE_GROUPS, F), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        self._check(self.lib.qasr_tts_synthesize_icl(self.h, getattr(codec, "h", codec), C.byref(rq.rq), C.byref(icl.icl), C.byref(s), int(seed),
                                                     pp, ns, codes.ctypes.data_as(_I), n.ctypes.data_as(_I)))
        audio = [pcm[b][:int(ns[b])].copy() for b in range(B)]
        return (audio, [codes[b, :, :int(n[b])].copy() for b in range(B)]) if return_codes else audio

    def clone_batch(self, codec, codec_encoder, speaker_encoder, texts, languages, reference_pcms, ref_texts,
                    sampling: Optional[SamplingConfig] = None, seed: int = 0, row_index=None, return_codes=False):
        """qasr_tts_clone: 24 kHz reference clips -> codes and x-vectors -> the ICL call -> audio, for B rows."""
        rq = self._request(texts, languages, None, None, None, row_index)
        B, F = len(texts), self.cfg.max_frames
        if len(reference_pcms) != B or len(ref_texts) != B:
            raise QasrError("qasr error 1: one reference clip and one reference text per row")
        clips = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in reference_pcms]
        rt = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in ref_texts]
        cp = (_F * B)(*[a.ctypes.data_as(_F) for a in clips])
        cn = (C.c_size_t * B)(*[a.size for a in clips])
        tp = (_I * B)(*[a.ctypes.data_as(_I) for a in rt])
        tl = (C.c_int32 * B)(*[a.size for a in rt])
        s = (sampling or SamplingConfig()).c_struct()
        pcm = [np.zeros(1920 * F, dtype=np.float32) for _ in range(B)]
        pp = (_F * B)(*[a.ctypes.data_as(_F) for a in pcm])
        ns = (C.c_size_t * B)()
        codes = np.zeros((B, NUM_CODE_GROUPS, F), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        self._check(self.lib.qasr_tts_clone(self.h, getattr(codec_encoder, "h", codec_encoder), getattr(speaker_encoder, "h", speaker_encoder),
                                            getattr(codec, "h", codec), C.byref(rq.rq), tp, tl, cp, cn, C.byref(s), int(seed), pp, ns,
                                            codes.ctypes.data_as(_I), n.ctypes.data_as(_I)))
        audio = [pcm[b][:int(ns[b])].copy() for b in range(B)]
        return (audio, [codes[b, :, :int(n[b])].copy() for b in range(B)]) if return_codes else audio

    def synthesize_with_voice_clone_icl(self, codec, codec_encoder, speaker_encoder, text_ids, language, reference_pcm, reference_text_ids,
                                        sampling: Optional[SamplingConfig] = None, seed: int = 0):
        """synthesizeWithVoiceCloneICL: text_ids / reference_text_ids are plain tokenizer ids (the template is added here), language a
        name, a two-letter code or a codec id (an unknown name falls back to english, as the reference does), reference_pcm 24 kHz mono."""
        lang = language if isinstance(language, (int, np.integer)) else (CodecTokens.language_id(language) or CodecTokens.languages["english"])
        return self.clone_batch(codec, codec_encoder, speaker_encoder, [prepare_text_tokens(text_ids)], [int(lang)], [reference_pcm],
                                [reference_text_ids], sampling, seed)[0]

    # ---- audio ----
    def synthesize_batch(self, codec, texts, languages, sampling: Optional[SamplingConfig] = None, seed: int = 0, speakers=None,
                         xvectors=None, instructs=None, row_index=None, return_codes=False):
        """synthesizeBatch: codes, then `codec` (a qasr.codec.SpeechTokenizerDecoder) -> float32 [1920 * n_frames] per row."""
        rq = self._request(texts, languages, speakers, xvectors, instructs, row_index)
        s = (sampling or SamplingConfig()).c_struct()
        B, F = len(texts), self.cfg.max_frames
        pcm = [np.zeros(1920 * F, dtype=np.float32) for _ in range(B)]
        pp = (_F * B)(*[a.ctypes.data_as(_F) for a in pcm])
        ns = (C.c_size_t * B)()
        codes = np.zeros((B, NUM_CODE_GROUPS, F), dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        self._check(self.lib.qasr_tts_synthesize(self.h, getattr(codec, "h", codec), C.byref(rq.rq), C.byref(s), int(seed), pp, ns,
                                                 codes.ctypes.data_as(_I), n.ctypes.data_as(_I)))
        audio = [pcm[b][:int(ns[b])].copy() for b in range(B)]
        if return_codes:
            return audio, [codes[b, :, :int(n[b])].copy() for b in range(B)]
        return audio

    def synthesize(self, codec, text, language, sampling: Optional[SamplingConfig] = None, seed: int = 0, speaker=None, instruct=None):
        """synthesize: one templated id list -> float32 audio at 24 kHz."""
        return self.synthesize_batch(codec, [text], [language], sampling, seed, None if speaker is None else [speaker], None,
                                     None if instruct is None else [instruct])[0]

    def synthesize_stream(self, codec, text, language, sampling: Optional[SamplingConfig] = None, streaming: Optional[StreamingConfig] = None,
                          seed: int = 0, speaker=None, xvector=None, instruct=None, row_index: int = 0):
        """synthesizeStream: a generator of AudioChunk over a pool of one stream; the last chunk has is_final set."""
        with TtsStreamPool(self, codec, sampling, seed) as pool:
            pool.open(text, language, streaming, speaker, xvector, instruct, row_index)
            while pool.live:
                yield from pool.step()

    def synthesize_with_voice_clone(self, codec, text, language, xvector, sampling: Optional[SamplingConfig] = None, seed: int = 0):
        """synthesizeWithVoiceClone in x-vector mode: xvector [hidden] from qasr.tts_speaker.SpeakerEncoder.embed."""
        return self.synthesize_batch(codec, [text], [language], sampling, seed, None, [xvector])[0]

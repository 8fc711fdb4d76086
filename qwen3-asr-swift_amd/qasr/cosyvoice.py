"""The CosyVoice3 speech-token LLM on the GPU over the C ABI (include/qasr.h, qasr_cvlm_*), and the text-ids-to-audio path over it.

Reference: Sources/CosyVoiceTTS/LLM.swift (CosyVoiceLLM.generate, sampleToken), CosyVoiceTTS.swift (synthesize, tokenizeText),
Configuration.swift.  Text -> ids stays with the caller: frame_text / clone_text put <|endofprompt|> where tokenizeText and the
zero-shot path put it.  Speech tokens are int32 at 25 Hz; with a CosyVoiceFlow (qasr.flow) and a HiFTVocoder (qasr.vocoder) they
become 24 kHz float32 audio.  No CPU fallback.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
END_OF_PROMPT = 151646                    # <|endofprompt|> (CosyVoiceTTS.swift:365)
LINEAR_KINDS = {"qkv": 0, "o": 1, "gate_up": 2, "down": 3, "head": 4}


def frame_text(instruction_ids: Sequence[int], content_ids: Sequence[int]) -> List[int]:
    """tokenizeText (CosyVoiceTTS.swift:377-393): instruction + <|endofprompt|> + content."""
    return [int(i) for i in instruction_ids] + [END_OF_PROMPT] + [int(i) for i in content_ids]


def clone_text(prompt_text_ids: Sequence[int], content_ids: Sequence[int]) -> List[int]:
    """The zero-shot path (CosyVoiceTTS.swift:220-223): the reference clip's transcript + <|endofprompt|> + content, no system frame."""
    return [int(i) for i in prompt_text_ids] + [END_OF_PROMPT] + [int(i) for i in content_ids]


def max_tokens_for(content_len: int) -> int:
    """CosyVoiceTTS.swift:240."""
    return max(200, 10 * int(content_len))


@dataclass
class CosySamplingConfig:
    """CosyVoiceSamplingConfig (Configuration.swift:124-133); maxTokenTextRatio is declared and never read there: no field."""
    top_k: int = 25
    top_p: float = 0.8
    win_size: int = 10
    tau_r: float = 0.1
    min_ratio: float = 2.0

    def c_struct(self) -> _lib.QasrCvlmSampling:
        return _lib.QasrCvlmSampling(int(self.top_k), float(self.top_p), int(self.win_size), float(self.tau_r), float(self.min_ratio))


@dataclass
class VoiceProfile:
    """CosyVoiceVoiceProfile (VoiceCloning.swift:152-157) as qasr.s3tok.SpeechTokenizer.profile returns it: tokens [L] int32 at 25 Hz and
    prompt_feat [80, 2 L], cut to the common length; spk_emb [192] (CAM++, the caller's) and the reference clip's transcript ids are
    optional.  uncut_tokens / uncut_frames: what the tokenizer and the mel extractor gave before the cut."""
    tokens: np.ndarray
    prompt_feat: np.ndarray
    spk_emb: Optional[np.ndarray] = None
    prompt_text_ids: Optional[List[int]] = None
    uncut_tokens: int = 0
    uncut_frames: int = 0


def _ivec(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _iptr(a):
    return None if a is None else a.ctypes.data_as(_I)


def _fptr(a):
    return None if a is None else a.ctypes.data_as(_F)


def default_config(bits: int = 4, **over) -> _lib.QasrCvlmConfig:
    cfg = _lib.QasrCvlmConfig()
    _lib.load().qasr_cvlm_default_config(4, C.byref(cfg))
    cfg.bits = int(bits)                   # any other value than 4 or 8 is refused where the config is used
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise QasrError(f"qasr error 1: no config field {k}")
        setattr(cfg, k, v)
    return cfg


def sample_host(logits, history=(), step: int = 0, below_min: bool = False, sampling: Optional[CosySamplingConfig] = None, seed: int = 0,
                row_index: int = 0, cfg: Optional[_lib.QasrCvlmConfig] = None) -> int:
    """The host twin of the device sampler on one row of logits.  Pure CPU."""
    lib = _lib.load()
    lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    h = _ivec(history)
    s = (sampling or CosySamplingConfig()).c_struct()
    rc = lib.qasr_cvlm_sample_host(C.byref(cfg) if cfg is not None else None, _fptr(lg), _iptr(h) if h.size else None, h.size, int(step),
                                   int(bool(below_min)), C.byref(s), int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_index))
    if rc < 0:
        raise QasrError(f"qasr error {-rc}: sampler arguments")
    return int(rc)


class _Request:
    """The ctypes view of a batch of rows; keeps the arrays alive."""

    def __init__(self, texts, prompts=None, content_len=None, max_tokens=None, row_index=None):
        B = len(texts)
        none = [None] * B
        self.text = [_ivec(t) for t in texts]
        self.prompt = [None if p is None or len(p) == 0 else _ivec(p) for p in (prompts or none)]
        if len(self.prompt) != B:
            raise QasrError("qasr error 1: one prompt entry per row")
        self.B = B
        self._tl = (C.c_int32 * B)(*[t.size for t in self.text])
        self._tp = (_I * B)(*[_iptr(t) for t in self.text])
        self._pl = (C.c_int32 * B)(*[0 if p is None else p.size for p in self.prompt])
        self._pp = (_I * B)(*[_iptr(p) for p in self.prompt])
        self._cl = (C.c_int32 * B)(*[-1 if c is None else int(c) for c in (content_len or none)])
        self._mt = (C.c_int32 * B)(*[0 if m is None else int(m) for m in (max_tokens or none)])
        self._ri = (C.c_int64 * B)(*[int(i) for i in (row_index if row_index is not None else range(B))])
        self.c = _lib.QasrCvlmRequest(B, self._tp, self._tl, self._pp, self._pl, self._cl, self._mt, self._ri)


class CosyVoiceLLM:
    """Handle of one LLM (qasr_cvlm).  One object, one thread at a time."""

    def __init__(self, handle, cfg):
        self.lib = _lib.load()
        self.h = handle
        self.cfg = cfg

    @classmethod
    def from_pretrained(cls, model_dir: str, bits: int = 4, cfg: Optional[_lib.QasrCvlmConfig] = None, **over) -> "CosyVoiceLLM":
        """Loads model_dir/llm.safetensors.  `over`: config fields (device, max_batch, max_text, max_prompt_tokens, max_tokens, or a
        reduced geometry)."""
        lib = _lib.load()
        cfg = cfg if cfg is not None else default_config(bits, **over)
        h = C.c_void_p()
        rc = lib.qasr_cvlm_create(str(model_dir).encode(), C.byref(cfg), C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_cvlm_last_error(None).decode()}")
        return cls(h, cfg)

    @staticmethod
    def check(model_dir: str, cfg: _lib.QasrCvlmConfig) -> None:
        """The loader's host checks alone (every key, shape, dtype and the geometry); touches no device."""
        lib = _lib.load()
        rc = lib.qasr_cvlm_check(str(model_dir).encode(), C.byref(cfg))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_cvlm_last_error(None).decode()}")

    def close(self):
        if self.h:
            self.lib.qasr_cvlm_free(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_cvlm_last_error(self.h).decode()}")

    @property
    def vocab(self) -> int:
        return int(self.cfg.speech_tokens + self.cfg.speech_extra)

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_cvlm_memory_footprint(self.h))

    @property
    def device_bytes(self) -> int:
        return int(self.lib.qasr_cvlm_device_bytes(self.h))

    def generate(self, texts, prompts=None, content_len=None, max_tokens=None, sampling: Optional[CosySamplingConfig] = None, seed: int = 0,
                 row_index=None) -> List[np.ndarray]:
        """Rows of text ids (+ prompt speech tokens) -> one int32 array of speech tokens per row."""
        rq = _Request(texts, prompts, content_len, max_tokens, row_index)
        F = int(self.cfg.max_tokens)
        tok = np.full((rq.B, F), -1, dtype=np.int32)
        n = np.zeros(rq.B, dtype=np.int32)
        s = (sampling or CosySamplingConfig()).c_struct()
        self._check(self.lib.qasr_cvlm_generate(self.h, C.byref(rq.c), C.byref(s), int(seed) & 0xFFFFFFFFFFFFFFFF, _iptr(tok), _iptr(n)))
        return [tok[b, :n[b]].copy() for b in range(rq.B)]

    def forced(self, texts, tokens, prompts=None, want_logits=True, want_hidden=True, row_index=None):
        """Teacher-forced pass on tokens [B, T] -> (logits [B, T, V] f32, hidden [B, T, hidden]); an output not wanted is None."""
        rq = _Request(texts, prompts, None, None, row_index)
        tk = np.ascontiguousarray(tokens, dtype=np.int32).reshape(rq.B, -1)
        T = tk.shape[1]
        lg = np.zeros((rq.B, T, self.vocab), dtype=np.float32) if want_logits else None
        hd = np.zeros((rq.B, T, int(self.cfg.hidden)), dtype=np.float32) if want_hidden else None
        self._check(self.lib.qasr_cvlm_forced(self.h, C.byref(rq.c), _iptr(tk), T, _fptr(lg), _fptr(hd)))
        return lg, hd

    def sample(self, logits, histories, steps, below_min, sampling: Optional[CosySamplingConfig] = None, seed: int = 0, row_index=None):
        """The device sampler alone on logits [B, V]: one pick per row."""
        lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, self.vocab)
        B = lg.shape[0]
        hs = [_ivec(h) for h in histories]
        hp = (_I * B)(*[_iptr(h) if h.size else None for h in hs])
        nh = (C.c_int32 * B)(*[h.size for h in hs])
        st = (C.c_int32 * B)(*[int(v) for v in steps])
        bm = (C.c_int32 * B)(*[int(bool(v)) for v in below_min])
        ri = (C.c_int64 * B)(*[int(i) for i in (row_index if row_index is not None else range(B))])
        out = np.zeros(B, dtype=np.int32)
        s = (sampling or CosySamplingConfig()).c_struct()
        self._check(self.lib.qasr_cvlm_sample(self.h, _fptr(lg), hp, nh, st, bm, B, C.byref(s), int(seed) & 0xFFFFFFFFFFFFFFFF, ri, _iptr(out)))
        return out

    def linear_probe(self, kind: str, x, layer: int = 0, resid=None) -> np.ndarray:
        """One linear of the handle alone, as the step runs it (qasr_cvlm_linear_probe): x [B, K] holding bf16 values."""
        c = self.cfg
        nq, nkv = c.heads * c.head_dim, c.kv_heads * c.head_dim
        N = {"qkv": nq + 2 * nkv, "o": c.hidden, "gate_up": c.inter, "down": c.hidden, "head": self.vocab}[kind]
        xa = np.ascontiguousarray(x, dtype=np.float32)
        ra = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
        y = np.zeros((xa.shape[0], N), dtype=np.float32)
        self._check(self.lib.qasr_cvlm_linear_probe(self.h, int(layer), LINEAR_KINDS[kind], _fptr(xa), _fptr(ra), xa.shape[0], _fptr(y)))
        return y


class CosyVoiceTTS:
    """Text ids -> 24 kHz audio: the LLM, the flow decoder and the vocoder (CosyVoiceTTSModel.synthesize behind its tokenizer)."""

    def __init__(self, llm: CosyVoiceLLM, flow, vocoder):
        self.llm, self.flow, self.vocoder = llm, flow, vocoder

    def synthesize(self, texts, content_len=None, prompts=None, prompt_feat=None, spk_emb=None, max_tokens=None,
                   sampling: Optional[CosySamplingConfig] = None, seed: int = 0, row_index=None, return_tokens=False):
        """Rows of framed text ids (frame_text / clone_text) -> one float32 waveform per row.  prompts[b]: the reference clip's speech
        tokens, prompt_feat[b] [80, 2 p] its mel, spk_emb[b] [192] its speaker vector; max_tokens None: max_tokens_for(content_len)."""
        llm = self.llm
        B = len(texts)
        none = [None] * B
        cl = [len(t) if c is None else int(c) for t, c in zip(texts, content_len or none)]
        mt = [min(max_tokens_for(c), int(llm.cfg.max_tokens)) if m is None else int(m) for c, m in zip(cl, max_tokens or none)]
        rq = _Request(texts, prompts, cl, mt, row_index)
        pf = [None if f is None else np.ascontiguousarray(f, dtype=np.float32) for f in (prompt_feat or none)]
        se = [None if e is None else np.ascontiguousarray(e, dtype=np.float32).reshape(-1) for e in (spk_emb or none)]
        F = int(llm.cfg.max_tokens)
        cap = 960 * F + 16
        pcm = [np.zeros(cap, dtype=np.float32) for _ in range(B)]
        ns = (C.c_size_t * B)()
        tok = np.full((B, F), -1, dtype=np.int32)
        n = np.zeros(B, dtype=np.int32)
        s = (sampling or CosySamplingConfig()).c_struct()
        llm._check(llm.lib.qasr_cvlm_synthesize(
            llm.h, self.flow.h, self.vocoder.h, C.byref(rq.c), C.byref(s), int(seed) & 0xFFFFFFFFFFFFFFFF, (_F * B)(*[_fptr(e) for e in se]),
            (_F * B)(*[_fptr(f) for f in pf]), (C.c_size_t * B)(*[0 if f is None else f.shape[1] for f in pf]), (_F * B)(*[_fptr(p) for p in pcm]),
            ns, _iptr(tok), _iptr(n)))
        wav = [pcm[b][:ns[b]].copy() for b in range(B)]
        return (wav, [tok[b, :n[b]].copy() for b in range(B)]) if return_tokens else wav

    def synthesize_with_profile(self, content_ids, profile: VoiceProfile, instruction_ids=(), max_tokens=None,
                                sampling: Optional[CosySamplingConfig] = None, seed: int = 0, return_tokens=False,
                                end_of_prompt: int = END_OF_PROMPT):
        """One row of content ids in the voice of `profile` (VoiceCloning.swift:169-): synthesize() with the profile's tokens, prompt mel
        and speaker vector.  With the clip's transcript the text is clone_text(transcript, content), else frame_text(instruction, content);
        end_of_prompt: the id of <|endofprompt|>, for a model with a reduced text vocabulary."""
        content = [int(i) for i in content_ids]
        head = profile.prompt_text_ids if profile.prompt_text_ids else instruction_ids
        text = [int(i) for i in head] + [int(end_of_prompt)] + content
        r = self.synthesize([text], content_len=[len(content)], prompts=[profile.tokens], prompt_feat=[profile.prompt_feat],
                            spk_emb=[profile.spk_emb], max_tokens=None if max_tokens is None else [max_tokens], sampling=sampling, seed=seed,
                            return_tokens=return_tokens)
        return (r[0][0], r[1][0]) if return_tokens else r[0]

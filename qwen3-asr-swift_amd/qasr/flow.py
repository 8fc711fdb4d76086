"""The CosyVoice3 flow-matching mel decoder on the GPU over the C ABI (include/qasr.h, qasr_flow_*).

Reference: Sources/CosyVoiceTTS/FlowMatching.swift (CosyVoiceFlowModel, ConditionalFlowMatching), DiT.swift and WeightLoading.swift:126-212.
Speech tokens at 25 Hz (prompt tokens then new tokens), optionally a prompt mel and a 192-d speaker vector, give an 80-bin mel at 50 Hz:
what HiFTVocoder.decode takes.  mu(), spks(), velocity() and solve() are the stages; generate() is the whole model and is bit-identical
to solve() on its own noise with the stage outputs.  The noise is this library's counter stream, seeded per clip, not MLX's.
bf16 GEMM operands, f32 everywhere else; no CPU fallback.
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
N_MELS, SPK_DIM, TOKEN_MEL_RATIO, DEFAULT_STEPS, CFG_RATE = 80, 192, 2, 10, 0.7
STAGES = ("modulation", "input_embed", "blocks", "output", "euler")


def _fptr(a):
    return a.ctypes.data_as(_F) if a is not None else None


def _iptr(a):
    return a.ctypes.data_as(_I) if a is not None else None


def mel_frames(n_tokens: int) -> int:
    """Mel frames of n tokens: 2 n (qasr_flow_mel_frames; host only)."""
    return int(_lib.load(strict=True).qasr_flow_mel_frames(int(n_tokens)))


def schedule(n_steps: int = DEFAULT_STEPS) -> np.ndarray:
    """The solver's n_steps + 1 time steps 1 - cos(i / n pi / 2) in float32, as the device uses them (qasr_flow_schedule; host only)."""
    t = np.zeros(int(n_steps) + 1, dtype=np.float32)
    if _lib.load(strict=True).qasr_flow_schedule(int(n_steps), _fptr(t)) != 0:
        raise QasrError("qasr error 1: n_steps in 1..64")
    return t


class CosyVoiceFlow:
    """CosyVoiceFlowModel on the device."""

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle

    @classmethod
    def from_pretrained(cls, model_dir, max_frames=0, order_with=None, device=0):
        """model_dir holds flow.safetensors (MLX 4 / 8 bit).  max_frames: mel frames, summed over clips, one device pass holds (0 = 4096);
        a longer clip is refused, a longer batch runs in several passes with identical results."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_flow_create(int(device), str(model_dir).encode(), int(max_frames), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_flow_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_flow_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_flow_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_flow_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_flow_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_flow_memory_footprint(self.h))

    @property
    def depth(self) -> int:
        return int(self.lib.qasr_flow_depth(self.h))

    def timing(self) -> Dict[str, float]:
        """Device milliseconds of the last solve / generate per stage, summed over steps and passes."""
        ms = (C.c_float * len(STAGES))()
        self._check(self.lib.qasr_flow_timing(self.h, ms))
        return dict(zip(STAGES, (float(v) for v in ms)))

    @staticmethod
    def _rows(a, name, T=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != N_MELS or (T is not None and a.shape[0] != T):
            raise QasrError(f"qasr error 1: {name} is [T, {N_MELS}]")
        return a

    @staticmethod
    def _vec(a, name, n):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        if a.size != n:
            raise QasrError(f"qasr error 1: {name} holds {n} values")
        return a

    @staticmethod
    def _tokens(t):
        return None if t is None else np.ascontiguousarray(t, dtype=np.int32).reshape(-1)

    # ---- stages ----
    def mu(self, tokens) -> np.ndarray:
        """Embedding, the pre-look-ahead convs and the x 2 repeat: tokens [n] -> [2 n, 80]."""
        t = self._tokens(tokens)
        out = np.zeros((TOKEN_MEL_RATIO * t.size, N_MELS), dtype=np.float32)
        self._check(self.lib.qasr_flow_mu(self.h, _iptr(t), t.size, _fptr(out)))
        return out

    def spks(self, emb=None) -> np.ndarray:
        """x / (|x| + 1e-8) and the affine layer: [192] -> [80]; None gives 80 zeros."""
        e = self._vec(emb, "the speaker vector", SPK_DIM)
        out = np.zeros(N_MELS, dtype=np.float32)
        self._check(self.lib.qasr_flow_spks(self.h, _fptr(e), _fptr(out)))
        return out

    def velocity(self, x, mu, t, spks=None, cond=None) -> np.ndarray:
        """One DiT forward on one branch as given: x, mu, cond [T, 80], spks [80] -> [T, 80]."""
        x = self._rows(x, "x")
        T = x.shape[0]
        m, c, s = self._rows(mu, "mu", T), (None if cond is None else self._rows(cond, "cond", T)), self._vec(spks, "spks", N_MELS)
        out = np.zeros((T, N_MELS), dtype=np.float32)
        self._check(self.lib.qasr_flow_velocity(self.h, _fptr(x), _fptr(m), _fptr(s), _fptr(c), T, float(t), _fptr(out)))
        return out

    def solve(self, mu, z, spks=None, cond=None, n_steps=DEFAULT_STEPS, return_velocity=False):
        """The Euler solver with classifier-free guidance from x0 = z: [T, 80].  return_velocity: also the last step's conditioned and
        unconditioned velocities [2, T, 80]."""
        z = self._rows(z, "z")
        T = z.shape[0]
        m, c, s = self._rows(mu, "mu", T), (None if cond is None else self._rows(cond, "cond", T)), self._vec(spks, "spks", N_MELS)
        out = np.zeros((T, N_MELS), dtype=np.float32)
        v = np.zeros((2, T, N_MELS), dtype=np.float32) if return_velocity else None
        self._check(self.lib.qasr_flow_solve(self.h, _fptr(m), _fptr(s), _fptr(c), T, _fptr(z), int(n_steps), _fptr(v), _fptr(out)))
        return (out, v) if return_velocity else out

    # ---- whole model ----
    def generate(self, tokens, prompt_tokens=None, prompt_feat=None, spk_emb=None, n_steps=DEFAULT_STEPS, temperature=1.0, seed=0,
                 strip_prompt=True, return_noise=False):
        """tokens [n] (+ prompt_tokens [p], prompt_feat [80, 2 p], spk_emb [192]) -> mel [80, 2 (n + p)] as the reference returns it, or
        with strip_prompt its last 2 n columns (what the reference's caller keeps).  return_noise: also x0, in the same layout."""
        r = self.generate_batch([tokens], [prompt_tokens], [prompt_feat], [spk_emb], n_steps, temperature, [seed], strip_prompt, return_noise)
        return (r[0][0], r[1][0]) if return_noise else r[0]

    def generate_batch(self, tokens: Sequence, prompt_tokens: Optional[Sequence] = None, prompt_feat: Optional[Sequence] = None,
                       spk_emb: Optional[Sequence] = None, n_steps=DEFAULT_STEPS, temperature=1.0, seeds: Optional[Sequence[int]] = None,
                       strip_prompt=True, return_noise=False):
        """Clips of any lengths in one call, one seed each -> a list of mels; each is bit-identical to generate() of it alone."""
        B = len(tokens)
        none = [None] * B
        tk = [self._tokens(t) for t in tokens]
        pt = [self._tokens(t) for t in (prompt_tokens or none)]
        pf = [None if f is None else np.ascontiguousarray(f, dtype=np.float32) for f in (prompt_feat or none)]
        se = [self._vec(e, "the speaker vector", SPK_DIM) for e in (spk_emb or none)]
        seeds = list(seeds) if seeds is not None else [0] * B
        if not (len(pt) == len(pf) == len(se) == len(seeds) == B):
            raise QasrError("qasr error 1: one entry per clip")
        if B == 0:
            return ([], []) if return_noise else []
        for f in pf:
            if f is not None and (f.ndim != 2 or f.shape[0] != N_MELS):
                raise QasrError(f"qasr error 1: prompt_feat is [{N_MELS}, frames]")
        T = [TOKEN_MEL_RATIO * (t.size + (0 if p is None else p.size)) for t, p in zip(tk, pt)]
        mels = [np.zeros((N_MELS, n), dtype=np.float32) for n in T]
        zs = [np.zeros((N_MELS, n), dtype=np.float32) for n in T] if return_noise else None
        self._check(self.lib.qasr_flow_generate_batch(
            self.h, (_I * B)(*[_iptr(t) for t in tk]), (C.c_size_t * B)(*[t.size for t in tk]), (_I * B)(*[_iptr(p) for p in pt]),
            (C.c_size_t * B)(*[0 if p is None else p.size for p in pt]), (_F * B)(*[_fptr(f) for f in pf]),
            (C.c_size_t * B)(*[0 if f is None else f.shape[1] for f in pf]), (_F * B)(*[_fptr(e) for e in se]), int(n_steps), float(temperature),
            (C.c_uint64 * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]), B, (_F * B)(*[_fptr(z) for z in zs]) if zs else None,
            (_F * B)(*[_fptr(m) for m in mels])))
        if strip_prompt:
            cut = [0 if p is None else TOKEN_MEL_RATIO * p.size for p in pt]
            mels = [np.ascontiguousarray(m[:, c:]) for m, c in zip(mels, cut)]
            zs = [np.ascontiguousarray(z[:, c:]) for z, c in zip(zs, cut)] if zs else None
        return (mels, zs) if return_noise else mels


def synthesize_tokens(flow: CosyVoiceFlow, vocoder, tokens, prompt_tokens=None, prompt_feat=None, spk_emb=None, n_steps=DEFAULT_STEPS,
                      temperature=1.0, seed=0, vocoder_seed=0, return_mel=False):
    """Speech tokens -> 24 kHz PCM: the flow decoder, the prompt frames sliced off as the reference's caller does, the mel transposed to
    the [T, 80] that HiFTVocoder.decode takes, then the vocoder.  480 * 2 n + 16 samples for n tokens."""
    mel = flow.generate(tokens, prompt_tokens, prompt_feat, spk_emb, n_steps, temperature, seed, strip_prompt=True)
    rows = np.ascontiguousarray(mel.T)
    pcm = vocoder.decode(rows, vocoder_seed)
    return (pcm, rows) if return_mel else pcm

"""VoxCPM2's two local networks on the GPU over the C ABI (include/qasr.h, qasr_vloc_*).

Reference: Sources/VoxCPM2TTS/MiniCPM4.swift (VoxCPMLocEnc :480-539, VoxCPMLocDiTV2 :577-652, UnifiedCFM :654-746) and
VoxCPM2TTS.swift:1312, :1368-1371, :1388, :1434-1437.  A patch is [patch_size, feat_dim] latent frames, the rows qasr.audiovae.AudioVAE
encodes to and decodes from.  encode() turns patches into language-model embeddings; mu() joins the two language models' hidden vectors
into the decoder's condition; solve() / sample() run the Euler solve under CFG-zero-star that yields the next patch.  No CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib
from .model import QasrError

_F = C.POINTER(C.c_float)
TIMING = ("encode", "mu", "velocity", "solve")
ENC, DIT = 0, 1


def _fptr(a):
    return a.ctypes.data_as(_F) if a is not None else None


def schedule(n_steps: int) -> np.ndarray:
    """makeUnifiedCFMTimeSpan: t[0 .. n_steps] (pure CPU)."""
    t = np.zeros(int(n_steps) + 1, dtype=np.float32)
    if _lib.load(strict=True).qasr_vloc_schedule(int(n_steps), _fptr(t)) != 0:
        raise QasrError("qasr error 1: n_steps in 1..64")
    return t


def zero_steps(n_steps: int) -> int:
    """The leading steps of a solve whose derivative is zero (CFG-zero-star)."""
    return int(_lib.load(strict=True).qasr_vloc_zero_steps(int(n_steps)))


def rope_table(model_dir, head_dim: int, n_pos: int):
    """(cos, sin) [n_pos, head_dim] of model_dir's config.json, as the handle builds them at load (pure CPU)."""
    lib = _lib.load(strict=True)
    cos, sin = np.zeros((n_pos, head_dim), dtype=np.float32), np.zeros((n_pos, head_dim), dtype=np.float32)
    rc = lib.qasr_vloc_rope_table(str(model_dir).encode(), int(head_dim), int(n_pos), _fptr(cos), _fptr(sin))
    if rc != 0:
        raise QasrError(f"qasr error {rc}: {lib.qasr_vloc_last_error(None).decode()}")
    return cos, sin


def check(model_dir) -> dict:
    """config.json and every tensor of model_dir checked on the host alone; the geometry found."""
    lib = _lib.load(strict=True)
    g = _lib.QasrVlocGeometry()
    rc = lib.qasr_vloc_check(str(model_dir).encode(), C.byref(g))
    if rc != 0:
        raise QasrError(f"qasr error {rc}: {lib.qasr_vloc_last_error(None).decode()}")
    return {n: int(getattr(g, n)) for n, _ in g._fields_}


class VoxCPM2Local:
    """VoxCPMLocEnc + enc_to_lm_proj, lm_to_dit_proj | res_to_dit_proj, and UnifiedCFM over VoxCPMLocDiTV2, on the device."""

    def __init__(self, handle):
        self.lib, self.h = _lib.load(strict=True), handle
        lib = self.lib
        self.patch_size = int(lib.qasr_vloc_patch_size(handle))
        self.feat_dim = int(lib.qasr_vloc_feat_dim(handle))
        self.lm_hidden = int(lib.qasr_vloc_lm_hidden(handle))
        self.mu_dim = int(lib.qasr_vloc_mu_dim(handle))
        self.hidden = (int(lib.qasr_vloc_hidden(handle, ENC)), int(lib.qasr_vloc_hidden(handle, DIT)))
        self.depth = (int(lib.qasr_vloc_depth(handle, ENC)), int(lib.qasr_vloc_depth(handle, DIT)))
        self.max_seqs = int(lib.qasr_vloc_max_seqs(handle))

    @classmethod
    def from_pretrained(cls, model_dir, max_seqs=0, order_with=None, device=0):
        """model_dir holds the *.safetensors with feat_encoder.*, feat_decoder.estimator.* and the three projections and, optionally,
        config.json.  max_seqs: patches one device pass holds (0 = 32)."""
        lib = _lib.load(strict=True)
        eng = getattr(order_with, "h", order_with)
        h = C.c_void_p()
        rc = lib.qasr_vloc_create(int(device), str(model_dir).encode(), int(max_seqs), eng, C.byref(h))
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {lib.qasr_vloc_last_error(None).decode()}")
        return cls(h)

    def close(self):
        if self.h:
            self.lib.qasr_vloc_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise QasrError(f"qasr error {rc}: {self.lib.qasr_vloc_last_error(self.h).decode()}")

    @property
    def is_loaded(self) -> bool:
        return bool(self.lib.qasr_vloc_is_loaded(self.h))

    def unload(self):
        self._check(self.lib.qasr_vloc_unload(self.h))

    @property
    def memory_footprint(self) -> int:
        return int(self.lib.qasr_vloc_memory_footprint(self.h))

    def timing(self) -> dict:
        """Device milliseconds of the last call of each kind, copies included."""
        ms = (C.c_float * len(TIMING))()
        self._check(self.lib.qasr_vloc_timing(self.h, ms))
        return dict(zip(TIMING, (float(v) for v in ms)))

    schedule = staticmethod(schedule)
    zero_steps = staticmethod(zero_steps)

    def _patches(self, a, name):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 3 or a.shape[1:] != (self.patch_size, self.feat_dim):
            raise QasrError(f"qasr error 1: {name} is [n, {self.patch_size}, {self.feat_dim}]")
        return a

    def _rows(self, a, width, name, B=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != width or (B is not None and a.shape[0] != B):
            raise QasrError(f"qasr error 1: {name} is [B, {width}]")
        return a

    def encode(self, feats, want="embed"):
        """feats [n, P, feat_dim] -> embed [n, lm_hidden] (want "embed"), cls [n, hidden] ("cls"), or both ("both": (cls, embed))."""
        f = self._patches(feats, "feats")
        n = f.shape[0]
        cls = np.zeros((n, self.hidden[ENC]), dtype=np.float32) if want in ("cls", "both") else None
        emb = np.zeros((n, self.lm_hidden), dtype=np.float32) if want in ("embed", "both") else None
        if cls is None and emb is None:
            raise QasrError('qasr error 1: want is "embed", "cls" or "both"')
        self._check(self.lib.qasr_vloc_encode(self.h, _fptr(f), n, _fptr(cls), _fptr(emb)))
        return (cls, emb) if want == "both" else (emb if cls is None else cls)

    def mu(self, lm_hidden, res_hidden) -> np.ndarray:
        """lm_to_dit_proj(lm_hidden) || res_to_dit_proj(res_hidden): [B, lm_hidden] twice -> [B, mu_dim]."""
        a = self._rows(lm_hidden, self.lm_hidden, "lm_hidden")
        b = self._rows(res_hidden, self.lm_hidden, "res_hidden", a.shape[0])
        out = np.zeros((a.shape[0], self.mu_dim), dtype=np.float32)
        self._check(self.lib.qasr_vloc_mu(self.h, _fptr(a), _fptr(b), a.shape[0], _fptr(out)))
        return out

    def velocity(self, x, mu, cond, t: float) -> np.ndarray:
        """One estimator call with mu as given: x, cond [B, P, feat_dim], mu [B, mu_dim] -> [B, P, feat_dim]."""
        x = self._patches(x, "x")
        B = x.shape[0]
        c, m = self._patches(cond, "cond"), self._rows(mu, self.mu_dim, "mu", B)
        if c.shape[0] != B:
            raise QasrError("qasr error 1: x and cond differ in B")
        out = np.zeros_like(x)
        self._check(self.lib.qasr_vloc_velocity(self.h, _fptr(x), _fptr(m), _fptr(c), B, float(t), _fptr(out)))
        return out

    def solve(self, mu, cond, z, n_steps: int = 10, cfg: float = 2.0, want_v: bool = False):
        """The Euler solve from noise z [B, P, feat_dim] -> the patches [B, P, feat_dim] (and the last step's derivative)."""
        z = self._patches(z, "z")
        B = z.shape[0]
        c, m = self._patches(cond, "cond"), self._rows(mu, self.mu_dim, "mu", B)
        if c.shape[0] != B:
            raise QasrError("qasr error 1: z and cond differ in B")
        out = np.zeros_like(z)
        v = np.zeros_like(z) if want_v else None
        self._check(self.lib.qasr_vloc_solve(self.h, _fptr(m), _fptr(c), _fptr(z), B, int(n_steps), float(cfg), _fptr(out), _fptr(v)))
        return (out, v) if want_v else out

    def sample(self, mu, cond, n_steps: int = 10, cfg: float = 2.0, temperature: float = 1.0, seed: int = 0, row_index=None, want_z: bool = False):
        """solve() from the project's counter normal stream (MLXRandom is not reproduced): row b draws from counter row_index[b]."""
        c = self._patches(cond, "cond")
        B = c.shape[0]
        m = self._rows(mu, self.mu_dim, "mu", B)
        out = np.zeros_like(c)
        z = np.zeros_like(c) if want_z else None
        idx = None
        if row_index is not None:
            if len(row_index) != B:
                raise QasrError("qasr error 1: row_index holds B values")
            idx = (C.c_uint64 * B)(*[int(i) for i in row_index])
        self._check(self.lib.qasr_vloc_sample(self.h, _fptr(m), _fptr(c), B, int(n_steps), float(cfg), float(temperature), int(seed), idx,
                                              _fptr(z), _fptr(out)))
        return (out, z) if want_z else out

    def stack(self, which: int, x, n_layers: int) -> np.ndarray:
        """The first n_layers layers of a stack (ENC or DIT) on embeddings x [n_seq, S, hidden]; all of them: with the final norm."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != self.hidden[which]:
            raise QasrError(f"qasr error 1: x is [n_seq, S, {self.hidden[which]}]")
        out = np.zeros_like(a)
        self._check(self.lib.qasr_vloc_stack(self.h, int(which), _fptr(a), a.shape[0], a.shape[1], int(n_layers), _fptr(out)))
        return out


def decode_patches(vae, patches, sr_cond: int = 0) -> np.ndarray:
    """VoxCPM2TTS.swift:1434-1437: patches [n, P, feat_dim] -> frames [n P, feat_dim] -> vae.decode -> 1920 n P samples at 48 kHz."""
    p = np.ascontiguousarray(patches, dtype=np.float32)
    if p.ndim != 3 or p.shape[2] != vae.latent_dim:
        raise QasrError(f"qasr error 1: patches is [n, P, {vae.latent_dim}]")
    return vae.decode(p.reshape(-1, vae.latent_dim), sr_cond)

"""CPU checks of the CosyVoice3 HiFT vocoder's oracle (tests/hift_oracle.py) and of the host side of qasr_hift_*.

The float64 oracle is pinned by its shapes (480 T + 16 samples; 8 T, 40 T and 120 T + 1 rows on both sides of every source add), by
STFT -> inverse STFT giving a signal back, by hand-computed draws of the noise stream, and by a torch f32 twin written independently of
it (F.conv1d on padded, repeat_interleave-upsampled rows; torch.cumsum for the phase).  test_f32_distance measures, on the exact
inputs of tests/test_gpu_hift.py, the twin's distance from the oracle per stage: those figures are the F32 table of that file, and each
GPU bound is 10 x its figure.  The source has one figure per kind of F0 track, so that the pure noise path (peak 0.1) is not judged by the
voiced tracks' figure, and the twin keeps its phase in cycles, reduced every frame: radians summed in f32 over 62400 samples drift by
3e-3 of the peak, and ten times that would let a wrong noise counter pass.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hift_oracle as O
from qasr import synth, _lib

F32 = {"f0": 1.5e-06, "source/voiced": 1.6e-04, "source/unvoiced": 1.5e-07, "source/alternating": 1.0e-04, "source/threshold": 1.3e-04,
       "network": 1.2e-05}
TILE = 64                                              # rows of a GEMM tile (csrc/voc_cosyvoice.h)
F0_FRAMES = (1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
SOURCE_FRAMES = (1, 2, 65, 130)
SOURCE_SEEDS = (5, 0xC0FFEE1234567)
DECODE_FRAMES = (1, 2, 3, 5, 8, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 130)
SRC_SEED = 11                                          # of the float32 source the network stage is given


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def given_source(T, W):
    """The float32 source tests/test_gpu_hift.py hands to decode_source for the clip of T frames."""
    return O.source(O.f0(O.clip_mel(T), W).astype(np.float32), SRC_SEED, W).astype(np.float32)


# ---- the torch f32 twin -------------------------------------------------------------------------------------------------------------
class Twin:
    def __init__(self, sd):
        self.w = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}

    def conv(self, x, key, dilation=1, left=None, right=0, stride=1):
        """x [rows, C]: F.conv1d on rows padded with zeros."""
        w = self.w[key + ".weight"].permute(0, 2, 1)
        left = (w.shape[2] - 1) * dilation if left is None else left
        return F.conv1d(F.pad(x.T[None], (left, right)), w, self.w[key + ".bias"], stride=stride, dilation=dilation)[0].T

    def snake(self, x, key):
        a = self.w[key + ".alpha"]
        return x + (1.0 / (a + 1e-9)) * torch.sin(a * x) ** 2

    def resblock(self, x, p):
        h = x
        for d, dil in enumerate(O.DILATIONS):
            xt = self.conv(self.snake(h, "%s.activations1.%d" % (p, d)), "%s.convs1.%d" % (p, d), dilation=dil)
            h = h + self.conv(self.snake(xt, "%s.activations2.%d" % (p, d)), "%s.convs2.%d" % (p, d))
        return h

    def f0(self, mel):
        h = torch.as_tensor(mel, dtype=torch.float32)
        for i in range(5):
            h = F.elu(self.conv(h, "f0_predictor.condnet.%d" % (2 * i), left=0 if i == 0 else None, right=3 if i == 0 else 0))
        return torch.abs(F.linear(h, self.w["f0_predictor.classifier.weight"], self.w["f0_predictor.classifier.bias"]))[:, 0]

    def source(self, f0, seed):
        f = torch.as_tensor(f0, dtype=torch.float32).repeat_interleave(480)
        n = np.arange(f.numel(), dtype=np.uint64)
        h = torch.arange(1, 10, dtype=torch.float32)
        uv = (f > 10.0).float()[:, None]
        # the phase in cycles: an f32 scan over the T frame starts, reduced mod 1 at every frame, then (r + 1) f0 h / 24000 inside the
        # frame.  Radians accumulated over 480 T samples in f32 (the reference's cumsum) drift by 3e-3 of the peak at T = 130, and ten
        # times that would bound nothing.
        T = f.numel() // 480
        inc = (f.view(T, 480)[:, 0, None] * h[None] / 24000.0) * uv.view(T, 480, 1)[:, 0]          # [T, 9] cycles per sample
        base = torch.from_numpy(O.uniform(O.draw(seed, np.arange(9))).astype(np.float32)).clone()
        starts = []
        for t in range(T):
            starts.append(base)
            base = torch.frac(base + 480.0 * inc[t])
        r1 = torch.arange(1, 481, dtype=torch.float32)[None, :, None]
        cyc = torch.frac(torch.stack(starts)[:, None, :] + r1 * inc[:, None, :]).reshape(T * 480, 9)
        phase = cyc * float(2.0 * np.pi)
        hn = O.normal(O.draw(seed, np.uint64(16) + np.uint64(10) * n[:, None] + np.arange(9, dtype=np.uint64)[None]))
        waves = 0.1 * torch.sin(phase) * uv + torch.from_numpy((0.003 * hn).astype(np.float32)) * (1.0 - uv)
        merged = torch.tanh(F.linear(waves, self.w["m_source.l_linear.weight"], self.w["m_source.l_linear.bias"]))[:, 0]
        return merged + torch.from_numpy((0.003 * O.normal(O.draw(seed, np.uint64(16) + np.uint64(10) * n + np.uint64(9)))).astype(np.float32))

    def network(self, mel, src):
        s = torch.as_tensor(src, dtype=torch.float32)
        win = torch.hann_window(16, periodic=True)
        z = torch.stft(F.pad(s[None, None], (8, 8), mode="reflect")[0, 0], 16, 4, window=win, center=False, return_complex=True).T
        spec = torch.cat([z.real, z.imag], dim=1)
        x = self.conv(torch.as_tensor(mel, dtype=torch.float32), "conv_pre", left=0, right=4)
        for i in range(3):
            x = self.conv(F.leaky_relu(x, 0.1).repeat_interleave(O.RATES[i], dim=0), "ups.%d" % i)
            if i == 2:
                x = F.pad(x.T[None], (1, 0), mode="reflect")[0].T
            st = O.DOWN_STRIDE[i]
            x = x + self.resblock(self.conv(spec, "source_downs.%d" % i, left=st - 1, stride=st), "source_resblocks.%d" % i)
            x = (self.resblock(x, "resblocks.%d" % (3 * i)) + self.resblock(x, "resblocks.%d" % (3 * i + 1)) +
                 self.resblock(x, "resblocks.%d" % (3 * i + 2))) / 3.0
        x = self.conv(F.leaky_relu(x, 0.01), "conv_post")
        mag, ph = torch.exp(x[:, :9]), torch.sin(x[:, 9:])
        fr = torch.fft.irfft(torch.polar(mag, ph), n=16, dim=1) * win[None]           # [frames, 16]; overlap-add by fold
        n = 4 * fr.shape[0] + 12
        audio = F.fold(fr.T[None], (1, n), (1, 16), stride=(1, 4))[0, 0, 0]
        wsum = F.fold((win * win)[:, None].expand(16, fr.shape[0])[None], (1, n), (1, 16), stride=(1, 4))[0, 0, 0]
        return torch.clamp(audio / torch.clamp(wsum, min=1e-8), -0.99, 0.99)


@pytest.fixture(scope="module")
def model():
    sd = synth.synth_cosyvoice_hifigan_state_dict(0)
    return sd, O.Weights(sd), Twin(sd)


# ---- shapes, transforms, noise ------------------------------------------------------------------------------------------------------
def test_geometry(model):
    sd = model[0]
    shapes = synth.cosyvoice_hifigan_tensor_shapes()
    assert set(shapes) == set(sd) and all(sd[k].shape == shapes[k] for k in sd)
    assert sd["conv_pre.weight"].shape == (512, 5, 80) and sd["f0_predictor.condnet.0.weight"].shape == (512, 4, 80)
    assert sd["ups.0.weight"].shape == (256, 16, 512) and sd["source_downs.0.weight"].shape == (256, 30, 18)
    assert sd["resblocks.8.convs1.2.weight"].shape == (64, 11, 64) and sd["conv_post.weight"].shape == (18, 7, 64)
    assert 20e6 < sum(v.size for v in sd.values()) < 22e6
    assert [O.num_samples(T) for T in (0, 1, 2, 130)] == [0, 496, 976, 62416]


@pytest.mark.parametrize("T", [1, 2, 8])
def test_shapes(model, T):
    W = model[1]
    mel = O.clip_mel(T)
    f = O.f0(mel, W)
    src = O.source(f.astype(np.float32), 3, W)
    st = {}
    pcm = O.decode_source(mel, src, W, st)
    assert f.shape == (T,) and src.shape == (480 * T,) and O.stft(src).shape == (120 * T + 1, 18) and pcm.shape == (480 * T + 16,)
    assert st["rows0"] == (8 * T, 8 * T) and st["rows1"] == (40 * T, 40 * T) and st["rows2"] == (120 * T + 1, 120 * T + 1)


def test_stft_round_trip():
    """istft(|X|, arg X) of X = stft(x) is x behind the 8 samples of centre padding, away from the ends; the transform itself agrees
    with torch.stft in float64 to the Float tables' rounding."""
    x = np.random.default_rng(3).standard_normal(480)
    X = O.stft(x)
    z = X[:, :9] + 1j * X[:, 9:]
    y = O.istft(np.abs(z), np.angle(z))
    assert X.shape == (121, 18) and y.shape == (496,)
    assert np.abs(y[8 + 16:8 + 480 - 16] - x[16:480 - 16]).max() < 1e-6
    want = torch.stft(torch.from_numpy(x), 16, 4, window=torch.hann_window(16, periodic=True, dtype=torch.float64), center=True,
                      pad_mode="reflect", return_complex=True).numpy().T
    assert np.abs(z - want).max() < 1e-6 * np.abs(want).max()


def test_noise_stream():
    """The spec against draws computed by hand (Python integers) for a fixed seed, and the two values a draw gives."""
    M = (1 << 64) - 1

    def by_hand(seed, c):
        z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    seed = 0xC0FFEE1234567
    cs = [0, 1, 8, 16, 25, 16 + 10 * 62399 + 9]
    got = O.draw(seed, cs)
    assert [int(v) for v in got] == [by_hand(seed, c) for c in cs]
    assert int(O.draw(0, [0])[0]) == 0xE220A8397B1DCDAF                              # splitmix64's first output for seed 0
    assert int(O.draw(M, [3])[0]) == by_hand(M, 3)                                     # the seed wraps
    for r in (int(v) for v in got):
        u1, u2 = ((r >> 40) + 1) / 2.0 ** 24, ((r >> 16) & 0xFFFFFF) / 2.0 ** 24
        assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
        assert O.uniform(np.uint64(r)) == u2
        assert abs(O.normal(np.uint64(r)) - np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)) < 1e-15
    z = O.normal(O.draw(7, np.arange(200000)))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and np.abs(z).max() < 5.77   # sqrt(2 ln 2^24) = 5.768
    u = O.uniform(O.draw(7, np.arange(200000)))
    assert abs(u.mean() - 0.5) < 0.005 and u.min() >= 0.0 and u.max() < 1.0


def test_host_noise_twin():
    """qasr_hift_noise runs on the host the lines the kernels run (csrc/voc_cosyvoice.h): the uniform is the oracle's exactly (24 bits),
    the normal the oracle's to f32 rounding of sqrt, log and cos (its largest value is 5.77)."""
    from qasr.vocoder import noise
    for seed in (0, 5, 0xC0FFEE1234567, (1 << 64) - 1):
        cs = np.concatenate([np.arange(0, 64), 16 + 10 * np.arange(62390, 62400), np.array([1 << 40, (1 << 63) + 7], dtype=np.uint64)]).astype(np.uint64)
        u, z = noise(seed, cs)
        r = O.draw(seed, cs)
        assert u.dtype == z.dtype == np.float32 and np.array_equal(u.astype(np.float64), O.uniform(r))
        assert np.abs(z.astype(np.float64) - O.normal(r)).max() < 4e-6
    u, z = noise(3, [])
    assert u.size == 0 and z.size == 0
    lib = _lib.load(strict=True)
    assert lib.qasr_hift_noise(1, None, 2, None, None) == 1


def test_source_paths(model):
    """Unvoiced frames carry no sine and do not advance the phase; the threshold is a strict >; a seed is a stream of its own."""
    W = model[1]
    quiet = O.source(O.f0_track("unvoiced", 2), 5, W)
    assert np.abs(quiet).max() < 0.2                                                   # tanh(9 terms of 0.003 N w) + 0.003 N
    th = O.f0_track("threshold", 3)
    assert th[0] == 10.0 and th[1] == 0.0 and th[2] > 10.0
    s = O.source(th, 5, W)
    assert np.abs(s[:960]).max() < 0.2 and np.abs(s[960:]).max() > 0.2                 # frames 0, 1 unvoiced, frame 2 voiced
    a, b = O.source(O.f0_track("voiced", 2), 5, W), O.source(O.f0_track("voiced", 2), 6, W)
    assert np.array_equal(a, O.source(O.f0_track("voiced", 2), 5, W)) and np.abs(a - b).max() > 0.05
    # the phase carries through an unvoiced frame: frames 0 and 2 of (200, 0, 200) join as those of (200, 200) do
    x, y = O.source(np.array([200, 0, 200], np.float32), 5, W), O.source(np.array([200, 200], np.float32), 5, W)
    noise = 0.003 * 5.8 * 2
    assert np.abs(x[:480] - y[:480]).max() == 0.0 and np.abs(x[960:965] - y[480:485]).max() < noise


# ---- the twin -----------------------------------------------------------------------------------------------------------------------
def test_oracle_vs_twin_stages(model):
    sd, W, twin = model
    T = 21
    mel = O.clip_mel(T)
    f = O.f0(mel, W)
    src = given_source(T, W)
    with torch.no_grad():
        d0 = rel(twin.f0(mel).numpy(), f)
        d1 = rel(twin.source(f.astype(np.float32), 5).numpy(), O.source(f.astype(np.float32), 5, W))
        d2 = rel(twin.network(mel, src).numpy(), O.decode_source(mel, src, W))
    print("oracle vs torch f32 twin, %d frames: f0 %.2e, source %.2e, network %.2e of peak" % (T, d0, d1, d2))
    assert d0 < 1e-4 and d1 < 1e-4 and d2 < 1e-3


def test_synthetic_weight_conditions(model):
    """What qasr.synth promises of the synthetic weights on the test inputs, in float64."""
    sd, W, twin = model
    for T in DECODE_FRAMES:
        mel = O.clip_mel(T)
        f = O.f0(mel, W)
        st = {}
        pcm = O.decode_source(mel, given_source(T, W), W, st)
        clamped = float((np.abs(pcm) >= 0.99).mean())
        print("T = %d: F0 %.1f .. %.1f Hz, %d unvoiced; |conv_post| <= %.2f; peak %.3f, %.2f %% on the clamp"
              % (T, f.min(), f.max(), int((f <= 10).sum()), np.abs(st["post"]).max(), np.abs(pcm).max(), 100 * clamped))
        assert f.max() <= 450.0 and np.abs(st["post"]).max() <= 4.0 and np.abs(pcm).max() > 0.05 and clamped <= 0.02
        if T >= 8:
            assert (f > 10).any() and (f <= 10).any() and f.max() > 100.0
    assert all(np.all(sd[k] == 1e3) for k in sd if k.endswith(".beta") or k.startswith(("up_activations.", "final_activation.")))


def test_f32_distance(model):
    """The figures of tests/test_gpu_hift.py's F32 table, on its inputs."""
    sd, W, twin = model
    fig = {k: 0.0 for k in F32}
    with torch.no_grad():
        for T in F0_FRAMES:
            mel = O.clip_mel(T)
            fig["f0"] = max(fig["f0"], rel(twin.f0(mel).numpy(), O.f0(mel, W)))
        for T in SOURCE_FRAMES:
            for kind in O.TRACKS:
                for seed in SOURCE_SEEDS:
                    tr = O.f0_track(kind, T)
                    fig["source/" + kind] = max(fig["source/" + kind], rel(twin.source(tr, seed).numpy(), O.source(tr, seed, W)))
        for T in DECODE_FRAMES:
            mel, src = O.clip_mel(T), given_source(T, W)
            fig["network"] = max(fig["network"], rel(twin.network(mel, src).numpy(), O.decode_source(mel, src, W)))
    print("torch f32 twin vs float64 oracle, max |d| / peak: F32 = {" + ", ".join('"%s": %.1e' % kv for kv in fig.items()) + "}")
    for k, v in fig.items():                                                          # the table is what is measured, neither less nor more
        assert 0.5 * F32[k] <= v <= 2 * F32[k], (k, v, F32[k])


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------
def test_host_abi(tmp_path):
    lib = _lib.load(strict=True)
    assert lib.qasr_hift_sample_rate() == 24000
    assert [lib.qasr_hift_num_samples(T) for T in (0, 1, 2, 500)] == [0, 496, 976, 240016]
    fp = (C.c_float * 8)()
    n = (C.c_size_t * 1)(1)
    sd_ = (C.c_uint64 * 1)(0)
    pp = (C.POINTER(C.c_float) * 1)(fp)
    assert lib.qasr_hift_f0(None, fp, 1, fp) == 1 and lib.qasr_hift_source(None, fp, 1, 0, fp) == 1
    assert lib.qasr_hift_decode_source(None, fp, 1, fp, fp) == 1 and lib.qasr_hift_decode(None, fp, 1, 0, fp) == 1
    assert lib.qasr_hift_decode_batch(None, pp, n, sd_, 1, pp) == 1
    assert lib.qasr_hift_unload(None) == 1 and lib.qasr_hift_timing(None, fp) == 1
    assert lib.qasr_hift_is_loaded(None) == 0 and lib.qasr_hift_memory_footprint(None) == 0
    lib.qasr_hift_destroy(None)
    # loader refusals, all before any HIP call
    h = C.c_void_p()
    err = lambda: lib.qasr_hift_last_error(None).decode()
    assert lib.qasr_hift_create(0, None, 0, None, C.byref(h)) == 1 and "model_dir" in err()
    assert lib.qasr_hift_create(0, b".", 0, None, None) == 1
    assert lib.qasr_hift_create(0, str(tmp_path / "none").encode(), 0, None, C.byref(h)) == 4
    assert lib.qasr_hift_create(0, b".", (1 << 17) + 1, None, C.byref(h)) == 1 and "max_frames" in err()
    sd = synth.synth_cosyvoice_hifigan_state_dict(0)
    key = "resblocks.7.convs2.1.weight"
    cases = ((dict(drop=(key,)), 4, key), (dict(reshape={key: (64, 64, 7)}), 1, key), (dict(dtype="F64"), 1, "dtype"),
             (dict(drop=("f0_predictor.condnet.8.bias",)), 4, "f0_predictor.condnet.8.bias"),
             (dict(drop=("source_resblocks.2.activations2.2.alpha",)), 4, "source_resblocks.2.activations2.2.alpha"),
             (dict(reshape={"m_source.l_linear.weight": (9, 1)}), 1, "m_source.l_linear.weight"),
             (dict(reshape={"conv_post.bias": (16,)}), 1, "conv_post.bias"))
    for i, (kw, code, word) in enumerate(cases):
        d = synth.write_cosyvoice_hifigan_safetensors(sd, str(tmp_path / ("m%d" % i)), **kw)
        assert lib.qasr_hift_create(0, d.encode(), 0, None, C.byref(h)) == code, (kw, err())
        assert word in err() and "HiFT vocoder" in err() and not h.value

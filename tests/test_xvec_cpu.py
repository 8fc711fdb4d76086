"""CPU checks of the Qwen3-TTS speaker encoder's oracle (tests/xvec_oracle.py) and of the host side of qasr_xvec_*.

The float64 oracle is pinned three ways: the reference's own known answers (Tests/Qwen3TTSTests/VoiceCloningTests.swift:12-54), its STFT
against torch.stft in float64, and a torch f32 twin written independently of it (torch.stft on the padded signal, F.conv1d with zero
padding and dilation).  test_f32_distance measures, on the exact inputs of tests/test_gpu_xvec.py, the twin's distance from the oracle:
those figures are the reference's own precision, the F32 table of that file, and each GPU bound is 10 x its figure.  Measured here
(max |d| / peak): mel 1.35e-04, embed 2.24e-05.  Both are worst cases over the shortest clips, whose bins sit just above the 1e-5 clamp
where an f32 transform's rounding is the signal, so they say little about a 65-frame clip.  A third figure is therefore kept for the
network alone on a given float32 log-mel of 63, 64, 65 and 129 frames (the tile edges of the device code): network 4.13e-07.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import xvec_oracle as O
from qasr import synth, _lib

F32 = {"mel": 1.35e-04, "embed": 2.24e-05, "network": 4.13e-07}
RES_TILE, RED_TILE = 64, 64                            # rows of a Res2Net tile and of a reduction tile (csrc/xvec_qwen3tts.h)
MEL_LENGTHS = (1, 2, 255, 256, 512, 513, 1023, 1024, 256 * 63 + 17)
EMBED_LENGTHS = MEL_LENGTHS + (256 * 3, 256 * 62, 256 * 63, 256 * 64, 256 * 128, 256 * 299 + 100)
BATCH_N = (1, 513, 256 * 63 + 17, 700, 256 * 20)
NETWORK_FRAMES = tuple(sorted({f for T in (RES_TILE, RED_TILE) for f in (T - 1, T, T + 1, 2 * T + 1)}))


# ---- the torch f32 twin -------------------------------------------------------------------------------------------------------------
class Twin:
    def __init__(self, sd):
        self.w = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
        self.fb = torch.from_numpy(O.filterbank())

    def mel(self, x):
        p = torch.from_numpy(O.padded(x).astype(np.float32))             # the pad only moves samples
        s = torch.stft(p, O.N_FFT, O.HOP, window=torch.hann_window(O.N_FFT, periodic=True), center=False, return_complex=True).abs()
        return torch.log(torch.clamp(s.T @ self.fb, min=1e-5))

    def conv(self, x, key, dilation=1):
        """x [T, C]: F.conv1d with zeros of (k - 1) dilation / 2 on both sides."""
        w = self.w[key + ".weight"].permute(0, 2, 1)
        return F.conv1d(x.T[None], w, self.w[key + ".bias"], padding=(w.shape[2] - 1) * dilation // 2, dilation=dilation)[0].T

    def block(self, x, b):
        p, d = "blocks.%d" % b, O.DILATIONS[b - 1]
        h = F.relu(self.conv(x, p + ".tdnn1.conv"))
        outs = [h[:, :64]]
        for i in range(1, 8):
            c = h[:, 64 * i:64 * (i + 1)]
            outs.append(F.relu(self.conv(c if i == 1 else c + outs[-1], "%s.res2net_block.blocks.%d.conv" % (p, i - 1), d)))
        h = F.relu(self.conv(torch.cat(outs, dim=1), p + ".tdnn2.conv"))
        s = h.mean(dim=0, keepdim=True)
        g = torch.sigmoid(self.conv(F.relu(self.conv(s, p + ".se_block.conv1")), p + ".se_block.conv2"))
        return h * g + x

    def network(self, m):
        h0 = F.relu(self.conv(torch.as_tensor(m, dtype=torch.float32), "blocks.0.conv"))
        o1 = self.block(h0, 1)
        o2 = self.block(o1, 2)
        o3 = self.block(o2, 3)
        x = F.relu(self.conv(torch.cat([o1, o2, o3], dim=1), "mfa.conv"))
        mean = x.mean(dim=0, keepdim=True)
        std = torch.sqrt(torch.clamp(((x - mean) * (x - mean)).mean(dim=0, keepdim=True), min=1e-12))
        a = torch.cat([x, mean.expand_as(x), std.expand_as(x)], dim=1)
        alpha = torch.softmax(self.conv(torch.tanh(self.conv(a, "asp.tdnn.conv")), "asp.conv"), dim=0)
        wm = (alpha * x).sum(dim=0)
        wv = (alpha * (x - wm[None]) * (x - wm[None])).sum(dim=0)
        pooled = torch.cat([wm, torch.sqrt(torch.clamp(wv, min=1e-12))])
        return self.conv(pooled[None], "fc")[0]


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def network_input(frames):
    """The float32 log-mel of a `frames`-frame clip: the input of tests/test_gpu_xvec.py::test_network_at_tile_edges."""
    n = 256 * (frames - 1)
    return np.ascontiguousarray(O.mel(O.make_pcm(n, n)), dtype=np.float32)


def gpu_inputs():
    """(name, pcm) of every clip tests/test_gpu_xvec.py compares against the oracle."""
    return [(n, O.make_pcm(n, n)) for n in EMBED_LENGTHS] + [("batch%d" % i, O.make_pcm(40 + i, n)) for i, n in enumerate(BATCH_N)]


@pytest.fixture(scope="module")
def model():
    sd = synth.synth_tts_speaker_encoder_state_dict(0)
    return sd, O.Weights(sd), Twin(sd)


# ---- the reference's known answers --------------------------------------------------------------------------------------------------
def test_reference_known_answers(model):
    sd = model[0]
    assert O.mel(np.zeros(24000, np.float32)).shape == (94, 128)                        # testMelFilterbankShape
    assert np.all(O.mel(np.zeros(24000, np.float32)) == np.log(1e-5))                   # silence sits on the clamp
    assert sd["blocks.0.conv.weight"].shape == (512, 5, 128) and sd["fc.weight"].shape == (1024, 1, 3072)   # testSpeakerEncoderInit
    assert [O.num_frames(n) for n in (0, 1, 255, 256, 257)] == [0, 1, 1, 2, 2]
    shapes = synth.tts_speaker_encoder_tensor_shapes()
    assert len(shapes) == 2 * (1 + 3 * 11 + 4) and sum(int(np.prod(s)) for s in shapes.values()) == sum(v.size for v in sd.values())
    assert synth.tts_speaker_encoder_tensor_shapes(2048)["fc.weight"] == (2048, 1, 3072)
    assert 8.5e6 < sum(v.size for v in sd.values()) < 9.1e6


def test_padding_clamps():
    """:296, :302: left sample 511 - i is x[min(i + 1, n - 1)], right sample i is x[max(n - 2 - i, 0)]."""
    for n in (1, 2, 3, 512, 513, 700):
        x = np.arange(1, n + 1, dtype=np.float64)
        p = O.padded(x)
        assert p.size == n + 1024 and np.array_equal(p[512:512 + n], x)
        for i in (0, 1, 2, 510, 511):
            assert p[511 - i] == x[min(i + 1, n - 1)] and p[512 + n + i] == x[max(n - 2 - i, 0)]
    assert np.all(O.padded(np.array([3.0])) == 3.0)


@pytest.mark.parametrize("n", [513, 1024, 256 * 63 + 17])
def test_stft_pin(n):
    """The oracle's magnitudes against torch.stft(center=True, pad_mode="reflect", periodic Hann) in float64; torch's own reflect pad
    is valid (and equals the clamped one) from n = 513."""
    x = O.make_pcm(n, n)
    want = torch.stft(torch.from_numpy(x.astype(np.float64)), 1024, 256, window=torch.hann_window(1024, periodic=True, dtype=torch.float64),
                      center=True, pad_mode="reflect", return_complex=True).abs().numpy().T
    got = O.stft_magnitudes(x)
    assert got.shape == want.shape == (n // 256 + 1, 513)
    # the oracle's window is the reference's Float one: 1e-7 of the peak
    assert np.abs(got - want).max() <= 2e-7 * want.max()


def test_filterbank():
    fb, pts = O.filterbank(), O.mel_points().astype(np.float64)
    assert fb.shape == (513, 128) and fb.dtype == np.float32 and fb.min() >= 0.0 and fb.max() <= 1.0
    hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    top = 2595.0 * np.log10(1.0 + 12000.0 / 700.0)
    assert np.allclose(pts, hz(np.arange(130) * top / 129.0), rtol=1e-4, atol=1e-3) and pts[0] == 0.0
    freqs = np.arange(513) * 24000.0 / 1024.0
    for m in range(128):
        inside = np.nonzero((freqs > pts[m] + 1e-2) & (freqs < pts[m + 2] - 1e-2))[0]
        support = np.nonzero(fb[:, m])[0]
        assert set(inside) <= set(support) and all(pts[m] - 1e-2 <= freqs[k] <= pts[m + 2] + 1e-2 for k in support)
        if len(inside):                                                              # the peak is the bin nearest the centre
            k = inside[np.argmax(fb[inside, m])]
            assert abs(freqs[k] - pts[m + 1]) <= 24000.0 / 1024.0
            want = np.minimum((freqs[inside] - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - freqs[inside]) / (pts[m + 2] - pts[m + 1]))
            assert np.allclose(fb[inside, m], want, atol=2e-3)
    # :378-382 at the ends: bin 0 (0 Hz) meets `freq >= fLow` of filter 0 with weight 0; bin 512 (12 kHz) is at most filter 127's end
    assert not fb[0].any() and not fb[512, :127].any() and fb[512, 127] <= 1e-3
    assert np.count_nonzero(fb) <= 2 * 513


def test_oracle_vs_twin_stages(model):
    """Mel and network each on their own input, two independent statements of the reference."""
    sd, W, twin = model
    x = O.make_pcm(5, 256 * 40 + 3)
    m = O.mel(x)
    with torch.no_grad():
        dm = rel(twin.mel(x).numpy(), m)
        de = rel(twin.network(torch.from_numpy(m.astype(np.float32))).numpy(), O.network(m.astype(np.float32).astype(np.float64), W))
    st = {}
    e = O.network(m, W, st)
    print("oracle vs torch f32 twin, 41 frames: mel %.2e, network %.2e of peak" % (dm, de))
    assert m.shape == (41, 128) and e.shape == (1024,) and dm < 1e-4 and de < 1e-4
    for k in ("h0", "o1", "o2", "o3", "mfa"):                                         # the signal is alive and O(1) down the chain
        assert 0.05 < np.abs(st[k]).mean() < 50, (k, np.abs(st[k]).mean())
    assert np.abs(e).max() > 0.05 and rel(O.embed(O.make_pcm(6, 256 * 40 + 3), W), e) > 1e-2


def test_f32_distance(model):
    """The figures of tests/test_gpu_xvec.py's F32 table, on its inputs."""
    sd, W, twin = model
    fig = {"mel": 0.0, "embed": 0.0, "network": 0.0}
    with torch.no_grad():
        for name, x in gpu_inputs():
            m = O.mel(x)
            if name in MEL_LENGTHS:
                fig["mel"] = max(fig["mel"], rel(twin.mel(x).numpy(), m))
            fig["embed"] = max(fig["embed"], rel(twin.network(twin.mel(x)).numpy(), O.network(m, W)))
        for f in NETWORK_FRAMES:                                                      # the network alone, both sides on the same float32 rows
            m32 = network_input(f)
            fig["network"] = max(fig["network"], rel(twin.network(torch.from_numpy(m32)).numpy(), O.network(m32.astype(np.float64), W)))
    print("torch f32 twin vs float64 oracle, max |d| / peak: F32 = {" + ", ".join('"%s": %.2e' % kv for kv in fig.items()) + "}")
    for k, v in fig.items():                                                          # the table is what is measured, neither less nor more
        assert 0.5 * F32[k] <= v <= 2 * F32[k], (k, v, F32[k])


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------
def test_host_abi(tmp_path):
    lib = _lib.load(strict=True)
    assert lib.qasr_xvec_input_sample_rate() == 24000
    assert [lib.qasr_xvec_num_frames(n) for n in (0, 1, 255, 256, 257, 24000)] == [0, 1, 1, 2, 2, 94]
    fp = (C.c_float * 8)()
    n = (C.c_size_t * 1)(4)
    pp = (C.POINTER(C.c_float) * 1)(fp)
    assert lib.qasr_xvec_embed(None, fp, 4, 24000, fp) == 1 and lib.qasr_xvec_embed_batch(None, pp, n, 1, fp) == 1
    assert lib.qasr_xvec_mel(None, pp, n, 1, pp) == 1 and lib.qasr_xvec_embed_mel(None, fp, 1, fp) == 1
    assert lib.qasr_xvec_unload(None) == 1 and lib.qasr_xvec_timing(None, fp) == 1
    assert lib.qasr_xvec_is_loaded(None) == 0 and lib.qasr_xvec_memory_footprint(None) == 0 and lib.qasr_xvec_embedding_dim(None) == 0
    lib.qasr_xvec_destroy(None)
    # loader refusals, all before any HIP call
    h = C.c_void_p()
    err = lambda: lib.qasr_xvec_last_error(None).decode()
    assert lib.qasr_xvec_create(0, None, 0, None, C.byref(h)) == 1 and "model_dir" in err()
    assert lib.qasr_xvec_create(0, b".", 0, None, None) == 1
    assert lib.qasr_xvec_create(0, str(tmp_path / "none").encode(), 0, None, C.byref(h)) == 4
    assert lib.qasr_xvec_create(0, b".", (1 << 28) + 1, None, C.byref(h)) == 1 and "max_samples" in err()
    sd = synth.synth_tts_speaker_encoder_state_dict(0, embedding_dim=64)
    talker = [("talker.model.layers.0.weight", np.zeros((4, 4), np.float32))]
    key = "speaker_encoder.blocks.2.res2net_block.blocks.6.conv.weight"
    cases = ((dict(drop=(key,)), 4, key), (dict(reshape={key: (64, 64, 3)}), 1, key), (dict(dtype="F64"), 1, "dtype"),
             (dict(drop=("speaker_encoder.fc.weight",)), 4, "speaker_encoder.fc.weight"),
             (dict(drop=("speaker_encoder.asp.tdnn.conv.bias",), extra=talker), 4, "speaker_encoder.asp.tdnn.conv.bias"),
             (dict(reshape={"speaker_encoder.fc.bias": (65,)}), 1, "speaker_encoder.fc.bias"))
    for i, (kw, code, word) in enumerate(cases):
        d = synth.write_tts_speaker_encoder_safetensors(sd, str(tmp_path / ("m%d" % i)), **kw)
        assert lib.qasr_xvec_create(0, d.encode(), 0, None, C.byref(h)) == code, (kw, err())
        assert word in err() and "speaker encoder" in err() and not h.value
    none = synth.write_tts_speaker_encoder_safetensors({}, str(tmp_path / "talker_only"), extra=talker)
    assert lib.qasr_xvec_create(0, none.encode(), 0, None, C.byref(h)) == 4 and "speaker_encoder." in err()
    # the state dict holds the reference's 76 tensors without the prefix; the writer adds it
    assert all(not k.startswith("speaker_encoder.") for k in sd) and len(sd) == 76

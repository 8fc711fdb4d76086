"""CPU checks of the WeSpeaker speaker embedding: the float64 oracle's front end against a second numpy statement and its network against
torch.nn.functional.conv2d on NCHW, the reference's unit cases (Tests/SpeechVADTests/WeSpeakerTests.swift:78-219) as known answers,
qasr_spk_cosine_similarity, the loader's error paths (each fails before the device is touched: there is no GPU here, and reaching one
would answer QASR_ERR_HIP), and the synthetic weights' discrimination, which gives the GPU tolerances their meaning."""
import ctypes as C
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import wespeaker_oracle as O
from qasr import _lib, synth
from qasr.model import QasrError
from qasr.speaker import WeSpeakerModel, cosine_similarity, num_frames


@pytest.fixture(scope="module")
def sd():
    return synth.synth_wespeaker_state_dict(0)


def _clips():
    rng = np.random.default_rng(5)
    return [np.array([0.25], np.float32), (0.2 * rng.standard_normal(199)).astype(np.float32), synth.synth_waveform(3, 0.5)]


def _fbank_direct(x):
    """second statement: explicit loops for the pad, a dense DFT matrix for the spectrum, the bank from its own formulas"""
    x = np.asarray(x, np.float64)
    n = len(x)
    e = np.array([x[0]] + [x[i] - 0.97 * x[i - 1] for i in range(1, n)])
    p = np.zeros(n + 400)
    for i in range(200):
        p[i] = e[max(0, min(200 - i, n - 1))]
        p[200 + n + i] = e[max(0, n - 2 - i)]
    p[200:200 + n] = e
    T = (len(p) - 400) // 160 + 1
    k = np.arange(257)[:, None]
    j = np.arange(400)[None, :]
    w = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(400) / 399)
    re, im = np.cos(2 * np.pi * k * j / 512), -np.sin(2 * np.pi * k * j / 512)
    mel = lambda f: 2595 * np.log10(1 + f / 700)
    hz = lambda m: 700 * (10 ** (m / 2595) - 1)
    pts = [hz(mel(20) + i * (mel(8000) - mel(20)) / 81) for i in range(82)]
    fb = np.zeros((80, 257))
    for m in range(80):
        for b in range(257):
            f = b * 16000 / 512
            fb[m, b] = max(0.0, min((f - pts[m]) / (pts[m + 1] - pts[m]), (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1]))) * 2 / (pts[m + 2] - pts[m])
    out = np.zeros((T, 80))
    for t in range(T):
        fr = p[160 * t:160 * t + 400] * w
        pw = (2 * (re @ fr)) ** 2 + (2 * (im @ fr)) ** 2
        out[t] = np.log(np.maximum(fb @ pw, 1e-10))
    return out - out.mean(0)


def _network_nchw(feat, t):
    """the network on NCHW [1, C, F, T] with F.conv2d (weights permuted from MLX [out, kH, kW, in])"""
    cw = lambda k: t[k].permute(0, 3, 1, 2)
    x = torch.as_tensor(feat.T[None, None].copy())
    x = torch.relu(Fn.conv2d(x, cw("conv1.weight"), t["conv1.bias"], padding=1))
    for st, nb in enumerate(O.BLOCKS):
        for i in range(nb):
            p = f"layer{st + 1}.{i}."
            s = 2 if st > 0 and i == 0 else 1
            y = torch.relu(Fn.conv2d(x, cw(p + "conv1.weight"), t[p + "conv1.bias"], stride=s, padding=1))
            y = Fn.conv2d(y, cw(p + "conv2.weight"), t[p + "conv2.bias"], padding=1)
            r = Fn.conv2d(x, cw(p + "shortcut.weight"), t[p + "shortcut.bias"], stride=2) if s == 2 else x
            x = torch.relu(y + r)
    h = x[0].reshape(-1, x.shape[-1]).T                              # [T', C * 10 + f]
    pooled = torch.cat([h.mean(0), torch.sqrt(h.var(0, unbiased=False) + 1e-10)])
    e = pooled @ t["embedding.weight"].T + t["embedding.bias"]
    return (e / torch.sqrt((e * e).sum() + 1e-10)).numpy()


def test_oracle_front_end_second_statement():
    for x in _clips() + [np.zeros(16000, np.float32)]:
        a, b = O.fbank(x), _fbank_direct(x)
        assert a.shape == b.shape == (O.num_frames(len(x)), 80)
        assert np.abs(a - b).max() < 1e-8


def test_oracle_network_against_conv2d(sd):
    W = O.Weights(sd)
    with torch.no_grad():
        for x in _clips():
            f = O.fbank(x)
            e, pooled, _ = O.network(f, W)
            want = _network_nchw(f, W.t)
            assert np.abs(e - want).max() < 1e-10
            assert pooled.shape == (5120,)


def test_reference_mel_cases():
    """WeSpeakerTests.swift:78-157: shape of 1 s of silence, random audio is not -inf, CMN means, the 1 kHz tone's mid frame"""
    m = O.fbank(np.zeros(16000))
    assert m.shape[1] == 80 and 90 < m.shape[0] < 110 and num_frames(16000) == m.shape[0] == 101
    rng = np.random.default_rng(1)
    m = O.fbank(rng.uniform(-0.5, 0.5, 16000).astype(np.float32))
    assert m.max() > -20.0
    tone = (np.sin(np.arange(32000, dtype=np.float32) * np.float32(0.1)) * np.float32(0.3)).astype(np.float32)
    m = O.fbank(tone)
    assert m.shape[0] > 10 and np.abs(m.mean(0)).max() <= 1e-4
    t1k = (np.sin(2 * np.pi * 1000 * np.arange(16000) / 16000) * 0.3).astype(np.float32)
    m = O.fbank(t1k)
    assert m.shape[0] > 50 and np.abs(m[m.shape[0] // 2]).max() < 5.0


def test_reference_network_shapes(sd):
    """WeSpeakerTests.swift:161-199: [1, 256] output with unit norm; BasicBlock shapes ([1, 100, 80, 32] -> [1, 50, 40, 64] after a
    downsampling block, in the reference's [B, H, W, C] with H = 100, W = 80)"""
    W = O.Weights(sd)
    t = W.t
    x = torch.randn(100, 80, 32, dtype=torch.float64)
    y = O.conv(x, t["layer1.0.conv1.weight"], t["layer1.0.conv1.bias"], 1)
    assert tuple(y.shape) == (100, 80, 32)
    y = O.conv(x, t["layer2.0.conv1.weight"], t["layer2.0.conv1.bias"], 2)
    y = O.conv(y, t["layer2.0.conv2.weight"], t["layer2.0.conv2.bias"], 1) + O.conv(x, t["layer2.0.shortcut.weight"], t["layer2.0.shortcut.bias"], 2)
    assert tuple(y.shape) == (50, 40, 64)
    with torch.no_grad():
        e, pooled, last = O.network(np.random.default_rng(2).standard_normal((101, 80)), W)
    assert e.shape == (256,) and abs(float(np.linalg.norm(e)) - 1.0) <= 0.01
    assert tuple(last.shape) == (10, 13, 256)


def test_cosine_similarity_abi():
    """WeSpeakerTests.swift:203-219 through qasr_spk_cosine_similarity, plus the guard cases of cosineSimilarity"""
    assert abs(cosine_similarity([1, 0, 0, 0], [1, 0, 0, 0]) - 1.0) < 1e-3
    assert abs(cosine_similarity([1, 0, 0, 0], [-1, 0, 0, 0]) + 1.0) < 1e-3
    assert abs(cosine_similarity([1, 0, 0, 0], [0, 1, 0, 0])) < 1e-3
    assert cosine_similarity([1, 0], [1, 0, 0]) == 0.0 and cosine_similarity([], []) == 0.0
    assert cosine_similarity([0, 0, 0], [1, 2, 3]) == 0.0
    lib = _lib.load()
    assert lib.qasr_spk_cosine_similarity(None, None, 0) == 0.0
    assert lib.qasr_spk_embedding_dim() == 256 and lib.qasr_spk_input_sample_rate() == 16000
    assert [lib.qasr_spk_num_frames(n) for n in (1, 159, 160, 16000)] == [1, 1, 2, 101]


def _create(d):
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.qasr_spk_create(0, str(d).encode(), 0, None, C.byref(h))
    return rc, lib.qasr_spk_last_error(None).decode()


def test_create_errors_name_the_key(tmp_path, sd):
    """missing file / key -> QASR_ERR_IO, wrong shape, bad dtype or an unknown key -> QASR_ERR_INVALID, the key named (whole messages, as
    the loader worded them before it was shared with the VAD); all before any HIP call"""
    rc, msg = _create(tmp_path / "nope")
    assert rc == 4 and msg == f"wespeaker: cannot open {tmp_path / 'nope'}/model.safetensors"
    synth.write_wespeaker_safetensors(sd, str(tmp_path / "a"), drop=("layer3.0.shortcut.bias",))
    rc, msg = _create(tmp_path / "a")
    assert rc == 4 and msg == "wespeaker: missing tensor layer3.0.shortcut.bias"
    synth.write_wespeaker_safetensors(sd, str(tmp_path / "b"), reshape={"layer2.1.conv1.weight": (64, 64, 3, 3)})
    rc, msg = _create(tmp_path / "b")
    assert rc == 1 and msg == "wespeaker: tensor layer2.1.conv1.weight has shape [64, 64, 3, 3], expected [64, 3, 3, 64]"
    synth.write_wespeaker_safetensors(sd, str(tmp_path / "c"), extra={"layer1.0.shortcut.weight": np.zeros((32, 1, 1, 32))})
    rc, msg = _create(tmp_path / "c")
    assert rc == 1 and msg == "wespeaker: unknown tensor layer1.0.shortcut.weight"
    synth.write_wespeaker_safetensors(sd, str(tmp_path / "d"), dtype="F64")
    rc, msg = _create(tmp_path / "d")
    assert rc == 1 and msg == "wespeaker: tensor conv1.weight has dtype F64 (F32 / F16 / BF16)"
    with pytest.raises(QasrError, match="embedding.weight"):
        synth.write_wespeaker_safetensors(sd, str(tmp_path / "e"), drop=("embedding.weight",))
        WeSpeakerModel.from_pretrained(str(tmp_path / "e"))
    lib = _lib.load()
    assert lib.qasr_spk_create(0, str(tmp_path / "a").encode(), 100, None, C.byref(C.c_void_p())) == 1     # max_batch_samples < 400
    assert lib.qasr_spk_embed(None, None, 0, 16000, None) == 1


def test_synth_weights_discriminate(sd):
    """8 different clips' oracle embeddings: the closest pair has cosine <= 0.9, so a device cosine >= 0.9999 means something; the
    writer round-trips every key and shape"""
    assert {k: v.shape for k, v in sd.items()} == synth.wespeaker_tensor_shapes()
    W = O.Weights(sd)
    rng = np.random.default_rng(0)
    clips = [synth.synth_waveform(k, 0.6) for k in range(4)]
    clips += [(0.1 * rng.standard_normal(9000)).astype(np.float32), (0.3 * np.sin(np.arange(8000) * 0.1)).astype(np.float32),
              (0.3 * rng.standard_normal(8000)).astype(np.float32), synth.synth_waveform(9, 1.0)]
    E = np.array([O.embed(c, W) for c in clips])
    cos = E @ E.T
    off = cos[~np.eye(8, dtype=bool)]
    assert off.min() <= 0.9, off.min()
    assert np.allclose(np.linalg.norm(E, axis=1), 1.0)

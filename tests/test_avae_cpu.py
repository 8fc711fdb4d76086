"""The VoxCPM2 AudioVAE without a device: the float64 oracle (tests/avae_oracle.py) against its torch f32 twin, the properties the device
tests rely on (causality, the two-tap form of the transposed conv, the sanitizer), the host helpers of qasr/audiovae.py, and the C ABI's
refusals, which all come before any HIP call."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import avae_cases as K
import avae_oracle as O
import test_gpu_avae as G
from qasr import audiovae, synth, _lib
from qasr.model import QasrError


@pytest.fixture(scope="module")
def models():
    return {name: O.Weights(K.stored(name), K.GEOMS[name]) for name in ("tiny", "mid")}


def test_f32_distance(models):
    """The figures of tests/test_gpu_avae.py's F32 table, on its inputs: per geometry, direction and stage the largest max |d| / peak
    between the float64 oracle and the torch f32 twin."""
    fig = {}
    for name, W in models.items():
        L = K.GEOMS[name]["latent_dim"]
        for T in K.DECODE_T:
            z = K.clip_z(T, L)
            (s64, p64), (s32, p32) = O.decode(z, W), O.decode(z, W, backend=O.TH)
            for k, (a, b) in enumerate(zip(s32, s64)):
                fig[f"{name}/dec/{k}"] = max(fig.get(f"{name}/dec/{k}", 0.0), O.rel(a, b))
            fig[f"{name}/dec/pcm"] = max(fig.get(f"{name}/dec/pcm", 0.0), O.rel(p32, p64))
        for n in K.ENCODE_N:
            pcm = K.clip_pcm(n)
            (s64, z64), (s32, z32) = O.encode(pcm, W), O.encode(pcm, W, backend=O.TH)
            for k, (a, b) in enumerate(zip(s32, s64)):
                fig[f"{name}/enc/{k}"] = max(fig.get(f"{name}/enc/{k}", 0.0), O.rel(a, b))
            fig[f"{name}/enc/z"] = max(fig.get(f"{name}/enc/z", 0.0), O.rel(z32, z64))
    print("torch f32 twin vs float64 oracle, max |d| / peak: F32 = {")
    for k, v in fig.items():
        print('    "%s": %.1e,' % (k, v))
    print("}")
    for k, v in fig.items():                           # the table is what is measured, neither less nor more
        assert 0.5 * G.F32[k] <= v <= 2 * G.F32[k], (k, v, G.F32[k])


def test_f32_distance_real():
    """The two figures of the real geometry, on the two inputs the device test runs."""
    W = O.Weights(K.stored("real"), K.GEOMS["real"])
    z, pcm = K.clip_z(K.REAL_T, 64), K.clip_pcm(K.REAL_N)
    d = O.rel(O.decode(z, W, backend=O.TH)[1], O.decode(z, W)[1])
    e = O.rel(O.encode(pcm, W, backend=O.TH)[1], O.encode(pcm, W)[1])
    print('real geometry, torch f32 twin vs float64 oracle: "real/dec/pcm": %.1e, "real/enc/z": %.1e' % (d, e))
    assert 0.5 * G.F32["real/dec/pcm"] <= d <= 2 * G.F32["real/dec/pcm"]
    assert 0.5 * G.F32["real/enc/z"] <= e <= 2 * G.F32["real/enc/z"]


def test_signal_stays_in_range(models):
    """The synthetic weights keep every stage O(1) and the waveform off tanh's rails, so a relative bound means something."""
    for name, W in models.items():
        stages, pcm = O.decode(K.clip_z(17, K.GEOMS[name]["latent_dim"]), W)
        for k, s in enumerate(stages):
            assert 0.05 < np.abs(s).max() < 200.0, (name, k, np.abs(s).max())
        assert 0.05 < np.abs(pcm).max() < 0.999 and np.abs(pcm).mean() > 0.01, (name, np.abs(pcm).max())
        stages, z = O.encode(K.clip_pcm(6401), W)
        for k, s in enumerate(stages + [z]):
            assert 0.05 < np.abs(s).max() < 200.0, (name, k, np.abs(s).max())


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_decode_is_causal(models, name):
    """decode(z[:k]) is the first 1920 k samples of decode(z), stage by stage, in float64: no conv looks ahead.  Equal up to the last
    bits only, since a matrix product over more rows may block its sums differently; a row that looked ahead would be off by O(1)."""
    W = models[name]
    L = K.GEOMS[name]["latent_dim"]
    stages, pcm = O.decode(K.clip_z(17, L), W)
    for k in (1, 8, 9):
        s_k, p_k = O.decode(K.clip_z(k, L), W)
        assert p_k.shape == (K.SPF * k,) and O.rel(p_k, pcm[:K.SPF * k]) < 1e-11
        for a, b in zip(s_k, stages):
            assert O.rel(a, b[:a.shape[0]]) < 1e-11


def test_encode_is_causal(models):
    W = models["tiny"]
    _, z = O.encode(K.clip_pcm(6400), W)
    _, z3 = O.encode(K.clip_pcm(1920), W)
    assert z.shape == (10, 8) and O.rel(z3, z[:3]) < 1e-11


@pytest.mark.parametrize("s", [2, 5, 6, 8])
def test_transposed_conv_is_two_taps(s):
    """The trimmed transposed conv = torch's conv_transpose1d with weight[in][out][k] = W[out][k][in], its last s rows cut = the two-tap
    form the device runs as a GEMM; and a strided conv's row t reads input rows (t - 1) s .. (t + 1) s - 1."""
    rng = np.random.default_rng(s)
    L, cin, cout = 7, 5, 3
    x, w, b = rng.standard_normal((L, cin)), rng.standard_normal((cout, 2 * s, cin)), rng.standard_normal(cout)
    want = F.conv_transpose1d(torch.from_numpy(x.T[None]), torch.from_numpy(w).permute(2, 0, 1).contiguous(), torch.from_numpy(b), stride=s)[0].T
    want = want[:L * s].numpy()
    two = O.conv_t_two_tap(x, w, b, s)
    W = type("W", (), {"f64": {"c.weight": w, "c.bias": b}})
    assert np.abs(two - want).max() < 1e-12 and np.abs(O.NP(W).conv_t(x, "c", s) - want).max() < 1e-12
    # the strided conv: L s input rows -> L output rows, row t from rows (t - 1) s .. (t + 1) s - 1
    xs = rng.standard_normal((L * s, cin))
    y = O.NP(W).conv(xs, "c", s, stride=s)
    assert y.shape == (L, cout)
    for t in (0, 1, L - 1):
        acc = b.copy()
        for j in range(2 * s):
            src = (t - 1) * s + j
            if src >= 0:
                acc += w[:, j, :] @ xs[src]
        assert np.abs(acc - y[t]).max() < 1e-12


@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_sanitizer(name):
    """Weight-norm pairs fuse to the weight they were split from, up to f32 rounding; the prefix is completed; fc_logvar goes; a table
    [n, 8, 8] comes back [n, 64]; every key the reference's modules hold is there with its shape."""
    geom = K.GEOMS[name]
    stored = K.stored(name)
    plain = synth.synth_voxcpm2_audiovae_state_dict(geom, K.SEEDS[name], weight_norm=False)
    assert any(k.endswith(".weight_g") for k in stored) and any("fc_logvar" in k for k in stored)
    assert all(k.startswith("audio_vae.") for k in stored) == (name != "mid")
    if name == "mid":
        assert stored["decoder.sr_cond_layers.3.scale_embed.weight"].shape == (4, 8, 8)
    got = audiovae.sanitize(stored)
    shapes = synth.voxcpm2_audiovae_tensor_shapes(geom)
    assert set(got) == set(shapes)
    n_pairs = 0
    for k, shape in shapes.items():
        assert got[k].shape == tuple(shape) and got[k].dtype == np.float32, k
        if k + "_g" in stored or k[len("audio_vae."):] + "_g" in stored:
            n_pairs += 1
            assert np.abs(got[k] - plain[k]).max() <= 4e-7 * np.abs(plain[k]).max(), k
        else:
            assert np.array_equal(got[k], plain[k]), k
    assert n_pairs >= 20


def test_frame_counts_and_buckets():
    assert [audiovae.num_frames(n) for n in (1, 639, 640, 641, 1280, 1281, 6400, 6401)] == [1, 1, 1, 2, 2, 3, 10, 11]
    lib = _lib.load(strict=True)
    assert [lib.qasr_avae_num_frames(None, n) for n in (0, 1, 640, 641, 6401)] == [0, 1, 1, 2, 11]
    assert [audiovae.sr_index(sr) for sr in (19999, 20000, 39999, 40000, 48000)] == [0, 1, 2, 3, 3]
    assert audiovae.sr_index(48000, ()) == 0


def test_sr_cond_buckets_in_the_oracle(models):
    """The decoder's output depends on sr_cond through its bucket alone."""
    W = models["tiny"]
    z = K.clip_z(3, 8)
    out = {sr: O.decode(z, W, sr)[1] for sr in (19999, 20000, 29999, 39999, 40000, 48000)}
    assert np.array_equal(out[20000], out[29999]) and np.array_equal(out[40000], out[48000])
    assert not np.array_equal(out[19999], out[20000]) and not np.array_equal(out[39999], out[40000])


@pytest.mark.parametrize("padding", ["right", "left"])
def test_patch_padding(padding):
    """encode_audio's padding and decode_patches' trim (VoxCPM2TTS.swift:1045-1064, :1440-1446), host only."""
    x = np.arange(1, 2562, dtype=np.float32)            # 2561 samples: one over a patch of 4 x 640
    a = audiovae.pad_to_patches(x, 16000, 16000, 2560, padding)
    assert a.size == 5120 and np.array_equal(a[2559:] if padding == "left" else a[:2561], x)
    assert np.count_nonzero(a) == 2561
    assert audiovae.pad_to_patches(x[:2560], 16000, 16000, 2560, padding).size == 2560
    with pytest.raises(QasrError, match="24000"):
        audiovae.pad_to_patches(x, 24000, 16000, 2560, padding)
    with pytest.raises(QasrError, match="empty"):
        audiovae.pad_to_patches(x[:0], 16000, 16000, 2560, padding)
    with pytest.raises(QasrError, match="padding"):
        audiovae.pad_to_patches(x, 16000, 16000, 2560, "both")
    audio = np.arange(10, dtype=np.float32)
    assert audiovae.trim_prefix(audio, 4).tolist() == list(range(4, 10))
    assert audiovae.trim_prefix(audio, 0) is audio and audiovae.trim_prefix(audio, 10) is audio


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------
def test_host_abi(tmp_path):
    lib = _lib.load(strict=True)
    fp = (C.c_float * 8)()
    n = (C.c_size_t * 1)(1)
    pp = (C.POINTER(C.c_float) * 1)(fp)
    r = C.c_int32()
    assert lib.qasr_avae_encode(None, fp, 1, fp) == 1 and lib.qasr_avae_decode(None, fp, 1, 0, fp) == 1
    assert lib.qasr_avae_encode_batch(None, pp, n, 1, pp) == 1 and lib.qasr_avae_decode_batch(None, pp, n, 1, 0, pp) == 1
    assert lib.qasr_avae_enc_stage(None, fp, 1, 0, fp) == 1 and lib.qasr_avae_dec_stage(None, fp, 1, 0, 0, fp) == 1
    assert lib.qasr_avae_dec_output(None, fp, 1, fp) == 1 and lib.qasr_avae_stage_shape(None, 0, 0, C.byref(r), C.byref(r)) == 1
    assert lib.qasr_avae_unload(None) == 1 and lib.qasr_avae_timing(None, fp) == 1
    assert lib.qasr_avae_is_loaded(None) == 0 and lib.qasr_avae_memory_footprint(None) == 0
    assert lib.qasr_avae_latent_dim(None) == 0 and lib.qasr_avae_hop(None) == 0 and lib.qasr_avae_num_blocks(None, 1) == 0
    lib.qasr_avae_destroy(None)
    # create-time refusals, all before any HIP call
    h = C.c_void_p()
    err = lambda: lib.qasr_avae_last_error(None).decode()
    assert lib.qasr_avae_create(0, None, 0, None, C.byref(h)) == 1 and "model_dir" in err()
    assert lib.qasr_avae_create(0, b".", 0, None, None) == 1
    assert lib.qasr_avae_create(0, str(tmp_path / "none").encode(), 0, None, C.byref(h)) == 4
    assert lib.qasr_avae_create(0, b".", (1 << 14) + 1, None, C.byref(h)) == 1 and "max_frames" in err()
    geom = K.GEOMS["tiny"]
    sd = K.stored("tiny")
    key = "audio_vae.encoder.blocks.layers.0.res1.conv2.weight"
    assert key in sd and "audio_vae.encoder.blocks.layers.0.conv.weight_g" in sd
    cases = (
        (dict(config_extra={"use_noise_block": True}), 1, "use_noise_block"),
        (dict(config_extra={"depthwise": False}), 1, "depthwise"),
        (dict(config_extra={"cond_type": "film"}), 1, "cond_type"),
        (dict(config_extra={"decoder_rates": []}), 1, "decoder_rates"),
        (dict(config_extra={"decoder_dim": 100}), 1, "decoder_dim"),
        (dict(drop=(key,)), 4, key),
        (dict(reshape={key: (8, 1, 4)}), 1, key),
        (dict(dtype="F64"), 1, "dtype"),
        (dict(drop=("audio_vae.decoder.sr_cond_layers.5.bias_embed.weight",)), 4, "sr_cond_layers.5.bias_embed.weight"),
        (dict(reshape={"audio_vae.decoder.sr_cond_layers.0.scale_embed.weight": (3, 256)}), 1, "sr_cond_layers.0.scale_embed.weight"),
        (dict(drop=("audio_vae.encoder.blocks.layers.0.conv.weight_v",)), 4, "encoder.blocks.layers.0.conv.weight"),
        (dict(reshape={"audio_vae.encoder.blocks.layers.0.conv.weight_g": (16,)}), 1, "encoder.blocks.layers.0.conv.weight_g"),
        (dict(reshape={"audio_vae.decoder.snake_out.alpha": (4,)}), 1, "decoder.snake_out.alpha"),
        (dict(drop=("audio_vae.encoder.fc_mu.bias",)), 4, "encoder.fc_mu.bias"),
    )
    for i, (kw, code, word) in enumerate(cases):
        d = synth.write_voxcpm2_audiovae_safetensors(sd, str(tmp_path / ("m%d" % i)), geom, **kw)
        assert lib.qasr_avae_create(0, d.encode(), 0, None, C.byref(h)) == code, (kw, err())
        assert word in err() and "AudioVAE" in err() and not h.value, (kw, err())

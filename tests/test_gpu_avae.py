"""The VoxCPM2 AudioVAE on the MI355X (csrc/vae_voxcpm.hip, csrc/api_avae.cpp) over the C ABI, against the float64 oracle
tests/avae_oracle.py, with synthetic weights (qasr.synth) on the three geometries of tests/avae_cases.py.

Tolerances: the reference runs this model in f32.  The F32 table holds, per geometry, direction and stage, the largest max |d| / peak
between the oracle and its torch f32 twin on these tests' inputs; it is printed (and held to within a factor of two) by
    pytest -s tests/test_avae_cpu.py -k f32_distance
Each bound is 10 x its figure: another f32 summation order through a deep chain, as in DESIGN.md sections 15 to 17 and 21.  No bound is
chosen by hand.  Every accuracy test runs under three values of the knob vae_fuse_c (0: every residual unit as a depthwise launch plus
the shared tile; 128: units up to 128 channels as one launch; 64: the default, which the mid geometry crosses in both directions), all
held to the same bounds.  Every test prints the device's distances; DESIGN.md section 25 holds the parity table they fill."""
import ctypes as C

import numpy as np
import pytest

import avae_cases as K
import avae_oracle as O
from qasr import synth, _lib
from qasr.audiovae import AudioVAE
from qasr.model import QasrError

pytestmark = pytest.mark.gpu

F32 = {
    "tiny/dec/0": 1.3e-07, "tiny/dec/1": 4.5e-07, "tiny/dec/2": 4.1e-07, "tiny/dec/3": 5.0e-07, "tiny/dec/4": 4.2e-07, "tiny/dec/5": 5.5e-07,
    "tiny/dec/6": 4.6e-07, "tiny/dec/pcm": 5.9e-07,
    "tiny/enc/0": 1.3e-07, "tiny/enc/1": 2.7e-07, "tiny/enc/2": 5.7e-07, "tiny/enc/3": 6.5e-07, "tiny/enc/4": 7.0e-07, "tiny/enc/z": 1.1e-06,
    "mid/dec/0": 1.6e-07, "mid/dec/1": 5.0e-07, "mid/dec/2": 5.5e-07, "mid/dec/3": 6.2e-07, "mid/dec/4": 5.3e-07, "mid/dec/5": 6.2e-07,
    "mid/dec/6": 5.9e-07, "mid/dec/pcm": 7.7e-07,
    "mid/enc/0": 1.3e-07, "mid/enc/1": 3.9e-07, "mid/enc/2": 5.4e-07, "mid/enc/3": 6.8e-07, "mid/enc/4": 8.4e-07, "mid/enc/z": 1.1e-06,
    "real/dec/pcm": 7.4e-07, "real/enc/z": 7.2e-07,
}
TOL = {k: 10 * v for k, v in F32.items()}
NAMES = ("tiny", "mid")
BATCH_T = (1, 9, 2, 17, 3)
DEC_THREE_PASSES = 17                                  # holds (1, 9, 2) | (17) | (3)
BATCH_N = (1, 5761, 641, 6401, 1281)                   # 1, 10, 2, 11, 3 frames
ENC_THREE_PASSES = 13                                  # holds (1, 10, 2) | (11) | (3)


@pytest.fixture(scope="module")
def weights():
    return {name: O.Weights(K.stored(name), K.GEOMS[name]) for name in NAMES}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    return {name: synth.write_voxcpm2_audiovae_safetensors(K.stored(name), str(tmp_path_factory.mktemp("avae_" + name)), K.GEOMS[name])
            for name in NAMES}


@pytest.fixture(scope="module")
def vaes(dirs):
    m = {name: AudioVAE.from_pretrained(d, max_frames=64) for name, d in dirs.items()}
    yield m
    for v in m.values():
        v.close()


@pytest.fixture(params=K.FUSE, ids=lambda v: "fuse%d" % v)
def fuse(request):
    """Runs the test under one value of vae_fuse_c and puts the knob back."""
    lib = _lib.load(strict=True)
    old = C.c_int()
    assert lib.qasr_get_tuning(b"vae_fuse_c", C.byref(old)) == 0
    assert lib.qasr_set_tuning(b"vae_fuse_c", request.param) == 0
    yield request.param
    assert lib.qasr_set_tuning(b"vae_fuse_c", old.value) == 0


@pytest.fixture(scope="module")
def dec_ref(weights):
    """(stages, pcm) of the float64 oracle per (geometry, T, sr_cond); computed once."""
    cache = {}

    def get(name, T, sr=48000):
        if (name, T, sr) not in cache:
            cache[name, T, sr] = O.decode(K.clip_z(T, K.GEOMS[name]["latent_dim"]), weights[name], sr)
        return cache[name, T, sr]
    return get


@pytest.fixture(scope="module")
def enc_ref(weights):
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            cache[name, n] = O.encode(K.clip_pcm(n), weights[name])
        return cache[name, n]
    return get


def check(label, got, want, key):
    d = O.rel(got, want)
    print("%s: device vs float64 oracle %.2e of peak (bound %.2e)" % (label, d, TOL[key]))
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), label
    assert d <= TOL[key], (label, d, TOL[key])


def test_knob_default_and_shapes(vaes):
    lib = _lib.load(strict=True)
    v = C.c_int()
    assert lib.qasr_get_tuning(b"vae_fuse_c", C.byref(v)) == 0 and v.value in K.FUSE
    assert lib.qasr_set_tuning(b"vae_fuse_c", 129) != 0 and lib.qasr_set_tuning(b"vae_fuse_c", -1) != 0
    m = vaes["mid"]
    assert (m.latent_dim, m.sample_rate, m.out_sample_rate, m.hop, m.samples_per_frame) == (16, 16000, 48000, K.HOP, K.SPF)
    assert (m.encoder_blocks, m.decoder_blocks) == (4, 6) and [m.num_frames(n) for n in (1, 640, 641)] == [1, 1, 2]
    assert [m.stage_shape(True, k) for k in range(7)] == [(1, 512), (8, 256), (48, 128), (240, 64), (480, 32), (960, 16), (1920, 8)]
    assert [m.stage_shape(False, k) for k in range(5)] == [(640, 32), (320, 64), (64, 128), (8, 256), (1, 512)]
    with pytest.raises(QasrError):
        m.stage_shape(True, 7)


@pytest.mark.parametrize("T", K.DECODE_T)
@pytest.mark.parametrize("name", NAMES)
def test_decode_vs_oracle(vaes, dec_ref, fuse, name, T):
    m, z = vaes[name], K.clip_z(T, K.GEOMS[name]["latent_dim"])
    stages, pcm = dec_ref(name, T)
    for k, want in enumerate(stages):
        check("%s fuse %d T = %d decoder stage %d" % (name, fuse, T, k), m.dec_stage(z, k), want, "%s/dec/%d" % (name, k))
    got = m.decode(z)
    assert got.shape == (K.SPF * T,) and np.abs(got).max() < 1.0
    check("%s fuse %d T = %d waveform" % (name, fuse, T), got, pcm, name + "/dec/pcm")


@pytest.mark.parametrize("name", NAMES)
def test_decode_sr_cond(vaes, dec_ref, fuse, name):
    m, z = vaes[name], K.clip_z(3, K.GEOMS[name]["latent_dim"])
    outs = []
    for sr in K.SR_CONDS:
        stages, pcm = dec_ref(name, 3, sr)
        outs.append(m.decode(z, sr))
        check("%s fuse %d sr_cond %d waveform" % (name, fuse, sr), outs[-1], pcm, name + "/dec/pcm")
        check("%s fuse %d sr_cond %d stage 6" % (name, fuse, sr), m.dec_stage(z, 6, sr), stages[6], name + "/dec/6")
    assert not np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[1], m.decode(z)) and np.array_equal(outs[1], m.decode(z, 40000))     # 0 = out_sample_rate; the same bucket


@pytest.mark.parametrize("n", K.ENCODE_N)
@pytest.mark.parametrize("name", NAMES)
def test_encode_vs_oracle(vaes, enc_ref, fuse, name, n):
    m, pcm = vaes[name], K.clip_pcm(n)
    stages, z = enc_ref(name, n)
    for k, want in enumerate(stages):
        check("%s fuse %d n = %d encoder stage %d" % (name, fuse, n, k), m.enc_stage(pcm, k), want, "%s/enc/%d" % (name, k))
    got = m.encode(pcm)
    assert got.shape == ((n + K.HOP - 1) // K.HOP, K.GEOMS[name]["latent_dim"])
    check("%s fuse %d n = %d latents" % (name, fuse, n), got, z, name + "/enc/z")


@pytest.mark.parametrize("name", NAMES)
def test_decode_bit_for_bit(vaes, dirs, fuse, name):
    """A clip alone = at each place of a ragged batch = under a max_frames that cuts the batch into three passes = a second run."""
    m, L = vaes[name], K.GEOMS[name]["latent_dim"]
    zs = [K.make_z(20 + i, T, L) for i, T in enumerate(BATCH_T)]
    alone = [m.decode(z) for z in zs]
    for order in (range(5), (3, 0, 4, 2, 1)):
        got = m.decode_batch([zs[i] for i in order])
        assert all(np.array_equal(g, alone[i]) for g, i in zip(got, order))
    assert all(np.array_equal(a, b) for a, b in zip(m.decode_batch(zs), alone))
    small = AudioVAE.from_pretrained(dirs[name], max_frames=DEC_THREE_PASSES)
    try:
        assert all(np.array_equal(a, b) for a, b in zip(small.decode_batch(zs), alone))
        with pytest.raises(QasrError, match="max_frames"):
            small.decode(K.make_z(1, DEC_THREE_PASSES + 1, L))
    finally:
        small.close()


@pytest.mark.parametrize("name", NAMES)
def test_encode_bit_for_bit(vaes, dirs, fuse, name):
    m = vaes[name]
    clips = [K.make_pcm(30 + i, n) for i, n in enumerate(BATCH_N)]
    alone = [m.encode(p) for p in clips]
    for order in (range(5), (3, 0, 4, 2, 1)):
        got = m.encode_batch([clips[i] for i in order])
        assert all(np.array_equal(g, alone[i]) for g, i in zip(got, order))
    assert all(np.array_equal(a, b) for a, b in zip(m.encode_batch(clips), alone))
    small = AudioVAE.from_pretrained(dirs[name], max_frames=ENC_THREE_PASSES)
    try:
        assert all(np.array_equal(a, b) for a, b in zip(small.encode_batch(clips), alone))
        with pytest.raises(QasrError, match="max_frames"):
            small.encode(K.make_pcm(1, K.HOP * ENC_THREE_PASSES + 1))
    finally:
        small.close()


@pytest.mark.parametrize("name", NAMES)
def test_decode_is_last_stage_through_output(vaes, fuse, name):
    m, z = vaes[name], K.clip_z(9, K.GEOMS[name]["latent_dim"])
    assert np.array_equal(m.dec_output(m.dec_stage(z, m.decoder_blocks)), m.decode(z))


@pytest.mark.parametrize("name", NAMES)
def test_decode_prefix_bit_for_bit(vaes, fuse, name):
    """The decode of z[:k] is the first 1920 k samples of the decode of z, in bits: nothing reads across the causal edge, and a row's
    sum does not depend on how many rows follow it or on where it falls in a slab or tile."""
    m, L = vaes[name], K.GEOMS[name]["latent_dim"]
    full = m.decode(K.clip_z(17, L))
    for k in (1, 8, 9):
        assert np.array_equal(m.decode(K.clip_z(k, L)), full[:K.SPF * k]), k
    zfull = m.encode(K.clip_pcm(6401))
    for n in (640, 1280, 5760):
        assert np.array_equal(m.encode(K.clip_pcm(n)), zfull[:n // K.HOP]), n


def test_patches(vaes):
    """encode_audio / decode_patches as VoxCPM2TTSModel uses the AudioVAE."""
    m = vaes["tiny"]
    pcm = K.clip_pcm(2561)
    for side in ("right", "left"):
        f = m.encode_audio(pcm, patch_size=4, padding=side)
        pad = np.zeros(5120 - 2561, dtype=np.float32)
        want = m.encode(np.concatenate([pcm, pad] if side == "right" else [pad, pcm]))
        assert f.shape == (2, 4, 8) and np.array_equal(f.reshape(8, 8), want)
    with pytest.raises(QasrError, match="24000"):
        m.encode_audio(pcm, sample_rate=24000)
    feat = K.make_z(5, 8, 8).reshape(2, 4, 8)
    audio = m.decode_patches(feat)
    assert audio.shape == (8 * K.SPF,) and np.array_equal(audio, m.decode(feat.reshape(8, 8)))
    assert np.array_equal(m.decode_patches(feat, trim_prefix_patches=1), audio[4 * K.SPF:])
    assert np.array_equal(m.decode_patches(feat, trim_prefix_patches=2), audio)


# ---- the real geometry ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real(tmp_path_factory):
    """The defaults (no config.json: every field falls back): the 64 KB weight slab of the fused unit at C = 128, N = 8192 in the first
    transposed conv, the loader's real shapes.  Used by the two tests below only."""
    stored = K.stored("real")
    d = synth.write_voxcpm2_audiovae_safetensors(stored, str(tmp_path_factory.mktemp("avae_real")))
    m = AudioVAE.from_pretrained(d, max_frames=8)
    yield m, O.Weights(stored, K.GEOMS["real"])
    m.close()


def test_real_decode(real, fuse):
    m, W = real
    z = K.clip_z(K.REAL_T, 64)
    assert (m.latent_dim, m.hop, m.samples_per_frame, m.decoder_blocks) == (64, K.HOP, K.SPF, 6)
    check("real fuse %d T = %d waveform" % (fuse, K.REAL_T), m.decode(z), O.decode(z, W)[1], "real/dec/pcm")


def test_real_encode(real, fuse):
    m, W = real
    pcm = K.clip_pcm(K.REAL_N)
    check("real fuse %d n = %d latents" % (fuse, K.REAL_N), m.encode(pcm), O.encode(pcm, W)[1], "real/enc/z")


# ---- arguments and lifecycle ----------------------------------------------------------------------------------------------------------
def test_arguments_and_lifecycle(dirs):
    lib = _lib.load(strict=True)
    m = AudioVAE.from_pretrained(dirs["tiny"], max_frames=4)
    try:
        fp = (C.c_float * (4 * K.SPF))()
        assert m.is_loaded and m.memory_footprint > 0
        assert lib.qasr_avae_decode(m.h, fp, 0, 0, fp) == 1 and "no frames" in lib.qasr_avae_last_error(m.h).decode()
        assert lib.qasr_avae_encode(m.h, fp, 0, fp) == 1 and "no samples" in lib.qasr_avae_last_error(m.h).decode()
        assert lib.qasr_avae_decode(m.h, fp, 5, 0, fp) == 1 and "max_frames" in lib.qasr_avae_last_error(m.h).decode()
        assert lib.qasr_avae_encode(m.h, fp, 4 * K.HOP + 1, fp) == 1 and "max_frames" in lib.qasr_avae_last_error(m.h).decode()
        assert lib.qasr_avae_decode(m.h, None, 1, 0, fp) == 1 and lib.qasr_avae_decode(m.h, fp, 1, 0, None) == 1
        assert lib.qasr_avae_decode(m.h, fp, 1, -1, fp) == 1 and lib.qasr_avae_dec_stage(m.h, fp, 1, 0, 7, fp) == 1
        assert lib.qasr_avae_enc_stage(m.h, fp, 1, 5, fp) == 1 and lib.qasr_avae_enc_stage(m.h, fp, 1, -1, fp) == 1
        m.decode(K.clip_z(4, 8))
        t = m.timing()
        assert t["dec_conv_in"] > 0 and t["dec_block5"] > 0 and t["dec_conv_out"] > 0 and t["enc_conv_in"] == 0
        m.encode(K.clip_pcm(641))
        t = m.timing()
        assert t["enc_conv_in"] > 0 and t["enc_block3"] > 0 and t["enc_fc_mu"] > 0 and t["dec_conv_in"] == 0
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        for rc in (lib.qasr_avae_decode(m.h, fp, 1, 0, fp), lib.qasr_avae_encode(m.h, fp, 1, fp), lib.qasr_avae_decode(m.h, None, 0, 0, None),
                   lib.qasr_avae_enc_stage(m.h, fp, 1, 0, fp), lib.qasr_avae_dec_output(m.h, fp, 1, fp)):
            assert rc == 3
        assert "unloaded" in lib.qasr_avae_last_error(m.h).decode()
        m.unload()                                     # a second unload is a no-op
    finally:
        m.close()

"""VoxCPM2's local networks on the device (qasr_vloc_*) against the float64 oracle of tests/vloc_oracle.py, on synthetic weights of the
real widths (tests/vloc_cases.py).

Every oracle-compared case and every bit-for-bit test runs under the knob vloc_skinny_rows at 0 (every Linear on the gemm.h tile) and at
its maximum 256 (the skinny kernel up to 256 rows, then the tile).  The rule: a device figure, max |d| / peak against float64, lies within MARGIN = 4 x the figure of the oracle's twin (the device's precision
plan restated on the CPU) for the same case and output, vloc_cases.TWIN.  mu alone is bounded absolutely, K 2^-24 of the peak: its inputs
hold bfloat16 values, so the only error is the float32 sum over K = lm_hidden products.  Each case prints a VLOC_PARITY line for DESIGN.md
section 26.  The bit-for-bit tests restate the solve in float32 numpy in the kernel's stated order (csrc/loc_voxcpm.h).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import avae_cases as AK
import vloc_cases as K
import vloc_oracle as O
from qasr import synth, voxcpm, _lib
from qasr.audiovae import AudioVAE
from qasr.model import QasrError
from qasr.voxcpm import VoxCPM2Local

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    out = {}
    for name in ("d2", "g2"):
        out[name] = synth.write_voxcpm2_local_safetensors(K.stored(name), str(tmp_path_factory.mktemp("vloc_" + name)), K.GEOMS[name])
    # use_mup is a field of config.json: the same tensors under another configuration
    mup = str(tmp_path_factory.mktemp("vloc_d2mup"))
    os.link(os.path.join(out["d2"], "model.safetensors"), os.path.join(mup, "model.safetensors"))
    with open(os.path.join(mup, "config.json"), "w") as f:
        json.dump(synth.voxcpm2_local_config(K.GEOMS["d2mup"]), f)
    out["d2mup"] = mup
    for name, bits in K.QUANT_BITS.items():
        out[name] = synth.write_voxcpm2_local_quantized_safetensors(K.quantized(name), str(tmp_path_factory.mktemp("vloc_" + name)), K.GEOMS[name], bits)
    return out


KNOB = (0, 256)                                        # vloc_skinny_rows: always the gemm.h tile | the skinny kernel up to its limit, then the tile


@pytest.fixture(params=KNOB, ids=lambda v: "skinny%d" % v)
def knob(request):
    """Runs the test under one value of vloc_skinny_rows and puts the knob back."""
    lib = _lib.load(strict=True)
    old = C.c_int()
    assert lib.qasr_get_tuning(b"vloc_skinny_rows", C.byref(old)) == 0
    assert lib.qasr_set_tuning(b"vloc_skinny_rows", request.param) == 0
    yield request.param
    assert lib.qasr_set_tuning(b"vloc_skinny_rows", old.value) == 0


@pytest.fixture(scope="module")
def nets(dirs):
    """max_seqs 70: encode n = 70 is one pass of 350 rows, over the skinny kernel's 256, so it takes the tile under either knob value"""
    m = {name: VoxCPM2Local.from_pretrained(d, max_seqs=70) for name, d in dirs.items()}
    yield m
    for v in m.values():
        v.close()


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    """The real depth, for the two cases that need it."""
    d = synth.write_voxcpm2_local_safetensors(K.stored("d12"), str(tmp_path_factory.mktemp("vloc_d12")), K.GEOMS["d12"])
    m = VoxCPM2Local.from_pretrained(d, max_seqs=4)
    yield m
    m.close()


def device(m, name):
    """The case on a handle -> {output: array}"""
    kind, _, p = K.CASES[name]
    a = K.inputs(name)
    if kind == "stack":
        return dict(out=m.stack(voxcpm.ENC if p["which"] == "enc" else voxcpm.DIT, a["x"], p["L"]))
    if kind == "encode":
        cls, emb = m.encode(a["feats"], want="both")
        return dict(cls=cls, embed=emb)
    if kind == "mu":
        return dict(mu=m.mu(a["lm"], a["res"]))
    if kind == "velocity":
        return dict(v=m.velocity(a["x"], a["mu"], a["cond"], p["t"]))
    x, d = m.solve(a["mu"], a["cond"], a["z"], p["steps"], p["cfg"], want_v=True)
    return dict(x=x, d=d)


def parity(m, name, knob):
    fig = K.figures(device(m, name), name)
    for k, v in fig.items():
        print("VLOC_PARITY %s skinny_rows %d device %.1e twin %.1e" % (k, knob, v, K.TWIN[k]))
    for k, v in fig.items():
        assert v <= K.MARGIN * K.TWIN[k], (k, v, K.TWIN[k])


SHALLOW = [n for n, c in K.CASES.items() if c[1] in ("d2", "d2mup", "g2", "q8", "q4") and c[0] != "mu"]


@pytest.mark.parametrize("name", SHALLOW)
def test_parity(nets, knob, name):
    parity(nets[K.CASES[name][1]], name, knob)


@pytest.mark.parametrize("name", ["depth12/velocity", "depth12/encode"])
def test_parity_real_depth(deep, knob, name):
    parity(deep, name, knob)


def test_mu(nets, knob):
    got, ref = device(nets["d2"], "mu/B3")["mu"], K.reference("mu/B3")["mu"]
    fig = O.rel(got, ref)
    print("VLOC_PARITY mu/B3/mu skinny_rows %d device %.1e bound %.1e" % (knob, fig, 2048 * 2.0 ** -24))
    assert got.shape == (3, 2048) and fig <= 2048 * 2.0 ** -24


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
def tree_sum(a):
    """csrc/loc_voxcpm.h: padded with zeros to a power of two n, then a[i] += a[i + s] for s = n / 2, n / 4, .. 1"""
    n2 = 1
    while n2 < a.size:
        n2 *= 2
    b = np.zeros(n2, dtype=np.float32)
    b[:a.size] = a
    s = n2 // 2
    while s > 0:
        b[:s] = b[:s] + b[s:2 * s]
        s //= 2
    return b[0]


def euler_loop(m, mu, cond, z, n_steps, cfg):
    """The solve as a float32 loop over velocity (mu given, then mu zero), in the kernel's order -> (x, last derivative)"""
    t = voxcpm.schedule(n_steps)
    x, d, cfg = z.copy(), np.zeros_like(z), np.float32(cfg)
    for step in range(1, n_steps + 1):
        dt = np.float32(t[step - 1] - t[step])
        if step <= voxcpm.zero_steps(n_steps):
            continue
        pos, neg = m.velocity(x, mu, cond, t[step - 1]), m.velocity(x, np.zeros_like(mu), cond, t[step - 1])
        for b in range(x.shape[0]):
            p, q = pos[b].reshape(-1), neg[b].reshape(-1)
            st = tree_sum(p * q) / (tree_sum(q * q) + np.float32(1e-8))
            a = q * st
            db = a + cfg * (p - a)
            d[b] = db.reshape(d[b].shape)
            x[b] = x[b] - (dt * db).reshape(x[b].shape)
    return x, d


@pytest.mark.parametrize("name,steps,B,cfg", [("d2", 2, 3, 2.0), ("d2", 10, 1, 1.0), ("g2", 3, 2, 2.0)])
def test_solve_is_the_euler_loop_over_velocity(nets, knob, name, steps, B, cfg):
    m, g = nets[name], K.GEOMS[name]
    P, F = g["patch_size"], g["feat_dim"]
    mu, cond, z = K.normal(11, B, m.mu_dim), K.normal(12, B, P, F), K.normal(13, B, P, F)
    want_x, want_d = euler_loop(m, mu, cond, z, steps, cfg)
    x, d = m.solve(mu, cond, z, steps, cfg, want_v=True)
    assert np.array_equal(x, want_x) and np.array_equal(d, want_d)
    x2, d2 = m.solve(mu, cond, z, steps, cfg, want_v=True)      # the captured graph
    x3 = m.solve(mu, cond, z, steps, cfg)                       # its replay
    assert np.array_equal(x2, x) and np.array_equal(d2, d) and np.array_equal(x3, x)


def test_zero_steps_leave_x_unchanged(nets, knob):
    m = nets["d2"]
    mu, cond, z = K.normal(21, 2, m.mu_dim), K.normal(22, 2, 4, 64), K.normal(23, 2, 4, 64)
    for _ in range(2):
        x, d = m.solve(mu, cond, z, 1, 2.0, want_v=True)        # one step, and it is a zero step
        assert np.array_equal(x, z) and not d.any()


def test_sample_is_solve_on_its_own_noise(nets, knob):
    m = nets["d2"]
    mu, cond = K.normal(31, 3, m.mu_dim), K.normal(32, 3, 4, 64)
    x, z = m.sample(mu, cond, 3, 2.0, temperature=0.8, seed=7, row_index=[5, 0, 9], want_z=True)
    assert np.array_equal(x, m.solve(mu, cond, z, 3, 2.0))
    assert 0.5 < z.std() < 1.1 and abs(z.mean()) < 0.2
    # a row's noise follows its row_index, not its place
    _, z1 = m.sample(mu[1:2], cond[1:2], 3, 2.0, temperature=0.8, seed=7, row_index=[0], want_z=True)
    assert np.array_equal(z1[0], z[1])
    _, z2 = m.sample(mu, cond, 3, 2.0, temperature=0.8, seed=8, row_index=[5, 0, 9], want_z=True)
    assert not np.array_equal(z2, z)


def test_a_sequence_alone_in_a_batch_and_again(nets, knob):
    m = nets["d2"]
    B = 3
    mu, cond, x = K.normal(41, B, m.mu_dim), K.normal(42, B, 4, 64), K.normal(43, B, 4, 64)
    v = m.velocity(x, mu, cond, 0.37)
    s = m.solve(mu, cond, x, 3, 2.0)
    assert np.array_equal(v, m.velocity(x, mu, cond, 0.37)) and np.array_equal(s, m.solve(mu, cond, x, 3, 2.0))
    for perm in ([1, 2, 0], [2, 0, 1]):
        assert np.array_equal(m.velocity(x[perm], mu[perm], cond[perm], 0.37), v[perm])
        assert np.array_equal(m.solve(mu[perm], cond[perm], x[perm], 3, 2.0), s[perm])
    for b in range(B):
        assert np.array_equal(m.velocity(x[b:b + 1], mu[b:b + 1], cond[b:b + 1], 0.37), v[b:b + 1])
        assert np.array_equal(m.solve(mu[b:b + 1], cond[b:b + 1], x[b:b + 1], 3, 2.0), s[b:b + 1])
    e = K.normal(44, 2, 11, 1024)
    both = m.stack(voxcpm.DIT, e, 2)
    assert np.array_equal(m.stack(voxcpm.DIT, e[1:], 2), both[1:]) and np.array_equal(m.stack(voxcpm.DIT, e, 2), both)


def test_encode_of_a_patch_alone_is_its_row_of_a_batch(nets, dirs, knob):
    m = nets["d2"]
    feats = K.inputs("encode/n13")["feats"]
    cls, emb = m.encode(feats, want="both")
    for i in (0, 5, 12):
        c1, e1 = m.encode(feats[i:i + 1], want="both")
        assert np.array_equal(c1[0], cls[i]) and np.array_equal(e1[0], emb[i])
    assert np.array_equal(m.encode(feats), emb) and np.array_equal(m.encode(feats, want="cls"), cls)
    # n over max_seqs runs in passes; B over max_seqs is refused
    small = VoxCPM2Local.from_pretrained(dirs["d2"], max_seqs=4)
    try:
        assert small.max_seqs == 4 and np.array_equal(small.encode(feats), emb)
        mu, cond = K.normal(51, 5, small.mu_dim), K.normal(52, 5, 4, 64)
        with pytest.raises(QasrError, match="qasr error 5.*max_seqs"):
            small.solve(mu, cond, cond, 2, 2.0)
        with pytest.raises(QasrError, match="qasr error 5.*max_seqs"):
            small.velocity(cond, mu, cond, 0.5)
    finally:
        small.close()


def test_rows_on_either_side_of_the_skinny_limit(nets, knob):
    """51 patches are 255 rows, 52 are 260: under the knob at 256 the first pass runs on the skinny kernel, the second on the tile.  On one
    side of the limit a patch's bits do not depend on the batch; across it the two forms sum in different orders and agree to the rule's
    bound only.  Under the knob at 0 everything is the tile, whichever of its forms gemm_nt picks for the row count: one set of bits."""
    m = nets["d2"]
    feats = K.normal(81, 70, 4, 64)
    e70, e52, e51, e13 = (m.encode(feats[:n]) for n in (70, 52, 51, 13))
    assert np.array_equal(e52, e70[:52]) and np.array_equal(e13, e51[:13])
    if knob == 0:
        assert np.array_equal(e51, e70[:51]) and np.array_equal(m.encode(feats[:1]), e70[:1])
    else:
        assert O.rel(e51, e52[:51]) < 2 * K.MARGIN * K.TWIN["encode/n70/embed"]
    # a solve has 22 rows a sequence: 11 sequences are 242 rows, 12 are 264
    mu, cond, z = K.normal(82, 12, m.mu_dim), K.normal(83, 12, 4, 64), K.normal(84, 12, 4, 64)
    s12, s11, s2 = m.solve(mu, cond, z, 2, 2.0), m.solve(mu[:11], cond[:11], z[:11], 2, 2.0), m.solve(mu[:2], cond[:2], z[:2], 2, 2.0)
    assert np.array_equal(s2, s11[:2])
    if knob == 0:
        assert np.array_equal(s11, s12[:11])
    else:
        assert O.rel(s11, s12[:11]) < 2 * K.MARGIN * K.TWIN["solve/n2B3cfg1/x"]


# ---- the interface -----------------------------------------------------------------------------------------------------------------
def test_api(dirs):
    lib = _lib.load(strict=True)
    m = VoxCPM2Local.from_pretrained(dirs["d2"], max_seqs=2)
    try:
        assert (m.patch_size, m.feat_dim, m.lm_hidden, m.mu_dim, m.hidden, m.depth) == (4, 64, 2048, 2048, (1024, 1024), (2, 2))
        stored = 2 * sum(int(np.prod(s)) for s in synth.voxcpm2_local_tensor_shapes(K.GEOMS["d2"]).values())
        assert m.is_loaded and m.memory_footprint == stored == voxcpm.check(dirs["d2"])["stored_bytes"]
        f = K.normal(61, 1, 4, 64)
        fp = f.ctypes.data_as(C.POINTER(C.c_float))
        assert lib.qasr_vloc_encode(m.h, fp, 1, None, None) == 1 and "null" in lib.qasr_vloc_last_error(m.h).decode()
        assert lib.qasr_vloc_velocity(m.h, fp, None, fp, 1, 0.5, fp) == 1
        assert lib.qasr_vloc_solve(m.h, None, fp, fp, 1, 10, 2.0, None, None) == 1
        assert lib.qasr_vloc_solve(m.h, fp, fp, fp, 1, 0, 2.0, fp, None) == 1 and "n_steps" in lib.qasr_vloc_last_error(m.h).decode()
        assert lib.qasr_vloc_stack(m.h, 2, fp, 1, 1, 1, fp) == 1
        with pytest.raises(QasrError, match="n_layers"):
            m.stack(voxcpm.ENC, K.normal(62, 1, 3, 1024), 3)
        with pytest.raises(QasrError, match="S in 1..32"):
            m.stack(voxcpm.ENC, K.normal(62, 1, 33, 1024), 1)
        assert m.encode(f).shape == (1, 2048) and m.timing()["encode"] > 0
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        with pytest.raises(QasrError, match="qasr error 3"):
            m.encode(f)
        with pytest.raises(QasrError, match="qasr error 3"):
            m.solve(K.normal(63, 1, 2048), f, f, 2, 2.0)
        m.unload()
    finally:
        m.close()


@pytest.mark.parametrize("name", ["q8", "q4"])
def test_quantised_footprint_is_the_stored_bytes(nets, dirs, name):
    """U32 words + bfloat16 scales and biases per group of 64 for every Linear, float32 for the vectors"""
    bits, want = K.QUANT_BITS[name], 0
    for key, shape in synth.voxcpm2_local_tensor_shapes(K.GEOMS[name]).items():
        n = int(np.prod(shape))
        want += n * bits // 8 + 2 * 2 * (n // 64) if key.endswith(".weight") and len(shape) == 2 else 4 * n
    assert nets[name].memory_footprint == want == voxcpm.check(dirs[name])["stored_bytes"]


def test_decode_patches_through_the_audiovae(tmp_path):
    d = synth.write_voxcpm2_audiovae_safetensors(AK.stored("tiny"), str(tmp_path / "vae"), AK.GEOMS["tiny"])
    vae = AudioVAE.from_pretrained(d, max_frames=16)
    try:
        patches = K.normal(71, 3, 4, 8)
        pcm = voxcpm.decode_patches(vae, patches)
        assert pcm.shape == (1920 * 4 * 3,) and np.array_equal(pcm, vae.decode(patches.reshape(12, 8)))
        with pytest.raises(QasrError):
            voxcpm.decode_patches(vae, K.normal(72, 3, 4, 64))
    finally:
        vae.close()

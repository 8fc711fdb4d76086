"""VoxCPM2's local networks without a device: the float64 oracle (tests/vloc_oracle.py) against its twin, the schedule and RoPE known
answers of the reference's own tests, and the C ABI's refusals, which all come before any HIP call."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import vloc_cases as K
import vloc_oracle as O
from qasr import synth, voxcpm, _lib
from qasr.model import QasrError

SMALL = synth.voxcpm2_local_geometry(
    1, feat_dim=16, enc__hidden_dim=512, enc__ffn_dim=512, enc__num_heads=4, dit__hidden_dim=512, dit__ffn_dim=512, dit__num_heads=4,
    lm__hidden_size=512)


@pytest.fixture(scope="module")
def small_sd():
    return synth.synth_voxcpm2_local_state_dict(SMALL, seed=5)


def test_twin_distance():
    """The figures of vloc_cases.TWIN: per case and output the distance between the float64 oracle and the twin."""
    fig = {}
    for name, (kind, mname, _) in K.CASES.items():
        fig.update(K.figures(K.run(K.model(mname, True), name), name))
    print("twin vs float64 oracle, max |d| / peak: TWIN = {")
    for k, v in fig.items():
        print('    "%s": %.1e,' % (k, v))
    print("}")
    assert set(fig) == set(K.TWIN)
    for k, v in fig.items():                           # the table is what is measured, neither less nor more
        assert 0.5 * K.TWIN[k] <= v <= 2 * K.TWIN[k], (k, v, K.TWIN[k])


def test_neg_norm_is_far_from_the_floor():
    """st = <pos, neg> / (|neg|^2 + 1e-8): the cases' |neg|^2 stays far above the floor, so st is a ratio of O(1) sums."""
    for name, (kind, _, p) in K.CASES.items():
        if kind == "solve" and p["steps"] > O.zero_steps(p["steps"]):
            assert K.reference(name)["least"] > 1.0, (name, K.reference(name)["least"])


def test_signal_stays_in_range():
    for name in ("velocity/B2t0.37", "encode/n2", "depth12/velocity", "depth12/encode"):
        for k, v in K.reference(name).items():
            assert 0.05 < np.abs(v).max() < 100.0, (name, k, np.abs(v).max())


def test_schedule_known_answer():
    """testUnifiedCFMTimeSpanMatchesUpstreamSwaySchedule: n = 10, to 1e-6"""
    want = [np.float32((1.0 - s / 10.0) + (math.cos(math.pi / 2.0 * (1.0 - s / 10.0)) - 1.0 + (1.0 - s / 10.0))) for s in range(11)]
    got = voxcpm.schedule(10)
    assert got.shape == (11,) and np.abs(got - np.array(want)).max() <= 1e-6
    assert np.abs(O.schedule(10) - np.array(want)).max() <= 1e-6
    assert got[0] == 1.0 and abs(got[10]) < 1e-7 and np.all(np.diff(got) < 0)
    for n in (1, 2, 24, 49):
        assert np.array_equal(voxcpm.schedule(n), O.schedule(n))


def test_zero_steps():
    assert [voxcpm.zero_steps(n) for n in (10, 24, 49)] == [1, 1, 2]
    assert [O.zero_steps(n) for n in (10, 24, 49)] == [1, 1, 2]


def test_rope_known_answer(tmp_path):
    """The reference's LongRoPE test: head_dim 2, max_pos 32768, rope_scaling original 8192, long factor [2.0].  cos[1][0] = cos(0.5) s.
    The amplitude s reads LMConfig.originalMaxPositionEmbeddings, which config.json cannot set: s = 1 for every checkpoint; the
    reference's test sets the property by hand and expects sqrt(1 + ln 4 / ln 8192).  The oracle restates both, the device table is the
    config.json-reachable one."""
    scaling = {"original_max_position_embeddings": 8192, "short_factor": [1.0], "long_factor": [2.0]}
    by_hand, _ = O.rope_tables(2, 3, 10000.0, 32768, scaling, lm_original=8192)
    assert abs(by_hand[1, 0] - math.cos(0.5) * math.sqrt(1.0 + math.log(4.0) / math.log(8192.0))) < 1e-12
    reachable, rsin = O.rope_tables(2, 3, 10000.0, 32768, scaling)
    assert abs(reachable[1, 0] - math.cos(0.5)) < 1e-12
    d = tmp_path / "kat"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"lm_config": {"max_position_embeddings": 32768, "rope_theta": 10000.0, "rope_scaling": scaling}}))
    cos, sin = voxcpm.rope_table(d, 2, 3)
    assert abs(cos[1, 0] - np.float32(math.cos(0.5))) <= 1e-7 and abs(cos[1, 1] - cos[1, 0]) == 0
    assert np.abs(cos - reachable).max() <= 1e-7 and np.abs(sin - rsin).max() <= 1e-7
    # the short factors when max_pos does not exceed the scaling's original; an empty list is ones; length 1 broadcasts
    (d / "config.json").write_text(json.dumps({"lm_config": {"max_position_embeddings": 8192, "rope_scaling": scaling}}))
    cos, _ = voxcpm.rope_table(d, 2, 3)
    assert abs(cos[1, 0] - np.float32(math.cos(1.0))) <= 1e-7
    (d / "config.json").write_text(json.dumps({"lm_config": {"rope_scaling": {"long_factor": [2.0] * 64, "original_max_position_embeddings": 8192}}}))
    cos, sin = voxcpm.rope_table(d, 128, 32)
    want = O.rope_tables(128, 32, scaling={"long_factor": [2.0] * 64, "original_max_position_embeddings": 8192})
    assert np.abs(cos - want[0]).max() <= 1e-7 and np.abs(sin - want[1]).max() <= 1e-7


def _create_error(model_dir):
    lib = _lib.load(strict=True)
    h = C.c_void_p()
    rc = lib.qasr_vloc_create(0, str(model_dir).encode(), 0, None, C.byref(h))
    assert rc != 0 and not h
    return rc, lib.qasr_vloc_last_error(None).decode()


@pytest.mark.parametrize("config,field", [
    ({"dit_config": {"kv_channels": 64}}, "dit_config.kv_channels"),
    ({"encoder_config": {"kv_channels": None, "hidden_dim": 1024, "num_heads": 4}}, "encoder_config.kv_channels"),
    ({"dit_config": {"mean_mode": True}}, "dit_config.mean_mode"),
    ({"patch_size": 9}, "patch_size"),
    ({"feat_dim": 60}, "feat_dim"),
    ({"lm_config": {"num_key_value_heads": 3}}, "lm_config.num_key_value_heads"),
    ({"lm_config": {"hidden_size": 1000}}, "lm_config.hidden_size"),
    ({"encoder_config": {"hidden_dim": 1000}}, "encoder_config.hidden_dim"),
    ({"dit_config": {"ffn_dim": 4000}}, "dit_config.ffn_dim"),
    ({"dit_config": {"num_layers": 0}}, "dit_config.num_layers"),
    ({"lm_config": {"max_position_embeddings": 65536, "rope_scaling": {"long_factor": [1.0, 2.0, 3.0]}}}, "lm_config.rope_scaling.long_factor"),
    ({"lm_config": {"rope_scaling": {"short_factor": "x"}}}, "rope_scaling.short_factor"),
])
def test_config_refusals_name_the_field(tmp_path, config, field):
    (tmp_path / "config.json").write_text(json.dumps(config))
    rc, msg = _create_error(tmp_path)
    assert rc == 1 and field in msg, msg


def test_loader_refusals_name_the_tensor(tmp_path, small_sd):
    key = "feat_decoder.estimator.decoder.layers.0.mlp.down_proj.weight"
    d = synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "missing"), SMALL, drop=(key,))
    rc, msg = _create_error(d)
    assert rc == 4 and key in msg, msg
    d = synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "shape"), SMALL, reshape={key: (512, 256)})
    rc, msg = _create_error(d)
    assert rc == 1 and key in msg, msg
    d = synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "dtype"), SMALL, dtype="F64")
    rc, msg = _create_error(d)
    assert rc == 1, msg
    d = synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "mu"), SMALL, drop=("lm_to_dit_proj.weight",))
    rc, msg = _create_error(d)
    assert rc == 4 and "lm_to_dit_proj.weight" in msg, msg
    d = synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "murows"), SMALL, reshape={"res_to_dit_proj.weight": (256, 512)})
    rc, msg = _create_error(d)
    assert rc == 1 and "res_to_dit_proj.weight" in msg, msg
    rc, msg = _create_error(tmp_path / "nothing_here")
    assert rc == 4, msg
    lib = _lib.load(strict=True)
    assert lib.qasr_vloc_create(0, None, 0, None, C.byref(C.c_void_p())) == 1
    assert lib.qasr_vloc_create(0, d.encode(), 4096, None, C.byref(C.c_void_p())) == 1 and "max_seqs" in lib.qasr_vloc_last_error(None).decode()


def test_quantised_loader_refusals(tmp_path, small_sd):
    """A Linear with .scales is an MLX triplet: U32 words of 4 or 8 bits, scales and biases per group of 64"""
    q = synth.quantize_voxcpm2_local_state_dict(small_sd, 4)
    stem = "feat_decoder.estimator.decoder.layers.0.self_attn.o_proj"
    d = synth.write_voxcpm2_local_quantized_safetensors(q, str(tmp_path / "good"), SMALL, 4)
    g = voxcpm.check(d)
    assert g["mu_dim"] == 1024 and 0 < g["stored_bytes"] < sum(int(np.prod(s)) for s in synth.voxcpm2_local_tensor_shapes(SMALL).values())
    d = synth.write_voxcpm2_local_quantized_safetensors(q, str(tmp_path / "nobias"), SMALL, 4, drop=(stem + ".biases",))
    rc, msg = _create_error(d)
    assert rc == 4 and stem + ".biases" in msg, msg
    d = synth.write_voxcpm2_local_quantized_safetensors(q, str(tmp_path / "words"), SMALL, 4, reshape={stem + ".weight": (512, 48)})
    rc, msg = _create_error(d)
    assert rc == 1 and stem + ".weight" in msg, msg
    d = synth.write_voxcpm2_local_quantized_safetensors(q, str(tmp_path / "group"), SMALL, 4, reshape={stem + ".scales": (512, 4)})
    rc, msg = _create_error(d)
    assert rc == 1 and stem + ".scales" in msg, msg


def test_host_only_create_checks_a_good_checkpoint(tmp_path, small_sd):
    """qasr_vloc_check is the host half of create: configuration, keys, shapes, dtypes, the mu token count from the projections' rows."""
    d = synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "good"), SMALL)
    g = voxcpm.check(d)
    assert (g["patch_size"], g["feat_dim"], g["lm_hidden"], g["enc_hidden"], g["dit_hidden"]) == (4, 16, 512, 512, 512)
    assert (g["enc_layers"], g["dit_layers"], g["mu_dim"], g["kv_heads"]) == (1, 1, 1024, 2)
    assert g["stored_bytes"] == 2 * sum(int(np.prod(s)) for s in synth.voxcpm2_local_tensor_shapes(SMALL).values())
    with pytest.raises(QasrError, match="mean_mode"):
        cfg = synth.voxcpm2_local_config(SMALL)
        cfg["dit_config"]["mean_mode"] = True
        voxcpm.check(synth.write_voxcpm2_local_safetensors(small_sd, str(tmp_path / "mean"), config=cfg))
    # without config.json the reference's defaults hold, which this checkpoint does not fit
    os.remove(os.path.join(d, "config.json"))
    with pytest.raises(QasrError):
        voxcpm.check(d)


def test_null_handles_are_refused():
    lib = _lib.load(strict=True)
    assert lib.qasr_vloc_encode(None, None, 1, None, None) == 1
    assert lib.qasr_vloc_solve(None, None, None, None, 1, 10, 2.0, None, None) == 1
    assert lib.qasr_vloc_memory_footprint(None) == 0 and lib.qasr_vloc_is_loaded(None) == 0
    assert lib.qasr_vloc_schedule(0, None) == 1 and lib.qasr_vloc_schedule(65, (C.c_float * 66)()) == 1

"""The checked weight loader the Talker and the CosyVoice3 LLM share (csrc/qlm_weights.cpp), through the two create entries, without a
device: one case per refusal of the loader on the tiny synthetic checkpoints of test_talker_cpu.py and test_cvlm_cpu.py.

The return code and the whole message of every case are literals.  They were recorded by running these same cases on the library
built from the commit before the loader was shared, when each model had its own copy of it: the shared loader has to say what both
copies said, byte for byte, and refuse in the same order."""
import ctypes as C

import numpy as np
import pytest
import torch

import cvlm_cases as KC
import talker_cases as KT
from qasr import _lib, cosyvoice as cv, synth, tts

GT, GC = KT.GEOMETRIES["small4"], KC.GEOMETRIES["tiny4"]
T0, C0 = "talker.model.layers.0.", "layers.0."          # the key prefix of a layer, per model
CP1 = "talker.code_predictor.model.layers.1."


def _resized(v, shape):
    a = v.to(torch.float32).numpy() if v.dtype != torch.int32 else v.numpy()
    return torch.from_numpy(np.resize(a, shape)).to(v.dtype)


def rows(stem, n, bias=False):
    """The Linear `stem` cut to n rows: weight, scales and biases alike (and its Linear bias)."""
    def f(sd):
        for part in ("weight", "scales", "biases") + (("bias",) if bias else ()):
            k = f"{stem}.{part}"
            sd[k] = _resized(sd[k], (n,) + tuple(sd[k].shape[1:]))
    return f


def widen(key, by=1):
    return lambda sd: sd.__setitem__(key, _resized(sd[key], tuple(sd[key].shape[:-1]) + (sd[key].shape[-1] + by,)))


def as_float(key, shape):
    return lambda sd: sd.__setitem__(key, torch.zeros(shape, dtype=torch.bfloat16))


def as_int(key):
    return lambda sd: sd.__setitem__(key, torch.zeros(tuple(sd[key].shape), dtype=torch.int32))


def f32_copy(key):
    """`key` leaves the bf16 tensors and comes back as F32: its stem's scales and biases then differ in dtype."""
    return lambda sd: ("extra", key, sd.pop(key).to(torch.float32).numpy())


def drop(key):
    return lambda sd: sd.__delitem__(key)


def both(*changes):
    return lambda sd: [c(sd) for c in changes] and None


# (model, case, change of the state dict, return code, message)
CASES = [
    ("talker", "weight_missing", drop(T0 + "self_attn.o_proj.weight"), 4,
     "talker: missing tensor talker.model.layers.0.self_attn.o_proj.weight"),
    ("talker", "scales_missing", drop(CP1 + "mlp.down_proj.scales"), 4,
     "talker: missing tensor talker.code_predictor.model.layers.1.mlp.down_proj.scales"),
    ("talker", "biases_missing", drop("talker.codec_head.biases"), 4, "talker: missing tensor talker.codec_head.biases"),
    ("talker", "bias_missing", drop("talker.text_projection.linear_fc1.bias"), 4,
     "talker: missing tensor talker.text_projection.linear_fc1.bias"),
    ("talker", "weight_float", as_float(T0 + "self_attn.o_proj.weight", (256, 512)), 1,
     "talker: tensor talker.model.layers.0.self_attn.o_proj.weight is float (BF16): a float (unquantised) checkpoint is not served, "
     "only MLX affine 4 / 8 bit"),
    ("talker", "weight_width", widen(T0 + "self_attn.o_proj.weight"), 1,
     "talker: tensor talker.model.layers.0.self_attn.o_proj.weight has dtype U32 shape [256, 65], expected U32 [N, 64] (bits / width mismatch)"),
    ("talker", "scales_shape", widen(T0 + "mlp.down_proj.scales"), 1,
     "talker: talker.model.layers.0.mlp.down_proj scales / biases have shape [256, 9], expected [256, 8]"),
    ("talker", "biases_shape", widen(T0 + "mlp.down_proj.biases"), 1,
     "talker: talker.model.layers.0.mlp.down_proj scales / biases have shape [256, 9], expected [256, 8]"),
    ("talker", "scales_not_float", as_int(T0 + "mlp.down_proj.scales"), 1,
     "talker: talker.model.layers.0.mlp.down_proj scales / biases have dtype U32"),
    ("talker", "scales_biases_dtype", f32_copy(T0 + "mlp.down_proj.biases"), 1,
     "talker: talker.model.layers.0.mlp.down_proj scales / biases differ in dtype"),
    ("talker", "gate_up_rows", rows(T0 + "mlp.up_proj", 496), 1,
     "talker: talker.model.layers.0.mlp.gate_proj: gate / up row counts do not interleave"),
    ("talker", "gate_up_not_by_16", both(rows(T0 + "mlp.gate_proj", 504), rows(T0 + "mlp.up_proj", 504)), 1,
     "talker: talker.model.layers.0.mlp.gate_proj: gate / up row counts do not interleave"),
    ("talker", "bias_shape", widen("talker.text_projection.linear_fc2.bias"), 1,
     "talker: tensor talker.text_projection.linear_fc2.bias has shape [257] dtype BF16, expected float [256]"),
    ("talker", "bias_not_float", as_int("talker.text_projection.linear_fc2.bias"), 1,
     "talker: tensor talker.text_projection.linear_fc2.bias has shape [256] dtype U32, expected float [256]"),
    ("talker", "norm_shape", widen(T0 + "input_layernorm.weight"), 1,
     "talker: tensor talker.model.layers.0.input_layernorm.weight has shape [257], expected [256]"),
    ("talker", "norm_not_float", as_int(CP1 + "post_attention_layernorm.weight"), 1,
     "talker: tensor talker.code_predictor.model.layers.1.post_attention_layernorm.weight has dtype U32 (F32 / F16 / BF16)"),
    ("talker", "qkv_rows", rows(T0 + "self_attn.k_proj", 128), 1,
     "talker: talker.model.layers.0.self_attn q/k/v_proj hold 896 rows, expected 1024"),
    ("talker", "o_rows", rows(T0 + "self_attn.o_proj", 240), 1,
     "talker: talker.model.layers.0. o_proj / mlp row counts do not match the geometry"),
    ("cosyvoice llm", "weight_missing", drop(C0 + "self_attn.o_proj.weight"), 4,
     "cosyvoice llm: missing tensor layers.0.self_attn.o_proj.weight"),
    ("cosyvoice llm", "scales_missing", drop("layers.2.mlp.down_proj.scales"), 4, "cosyvoice llm: missing tensor layers.2.mlp.down_proj.scales"),
    ("cosyvoice llm", "biases_missing", drop("speech_head.biases"), 4, "cosyvoice llm: missing tensor speech_head.biases"),
    ("cosyvoice llm", "bias_missing", drop(C0 + "self_attn.v_proj.bias"), 4, "cosyvoice llm: missing tensor layers.0.self_attn.v_proj.bias"),
    ("cosyvoice llm", "weight_float", as_float(C0 + "self_attn.o_proj.weight", (384, 384)), 1,
     "cosyvoice llm: tensor layers.0.self_attn.o_proj.weight is float (BF16): a float (unquantised) checkpoint is not served, "
     "only MLX affine 4 / 8 bit"),
    ("cosyvoice llm", "weight_width", widen(C0 + "self_attn.o_proj.weight"), 1,
     "cosyvoice llm: tensor layers.0.self_attn.o_proj.weight has dtype U32 shape [384, 49], expected U32 [N, 48] (bits / width mismatch)"),
    ("cosyvoice llm", "scales_shape", widen(C0 + "mlp.down_proj.scales"), 1,
     "cosyvoice llm: layers.0.mlp.down_proj scales / biases have shape [384, 11], expected [384, 10]"),
    ("cosyvoice llm", "biases_shape", widen(C0 + "mlp.down_proj.biases"), 1,
     "cosyvoice llm: layers.0.mlp.down_proj scales / biases have shape [384, 11], expected [384, 10]"),
    ("cosyvoice llm", "scales_not_float", as_int(C0 + "mlp.down_proj.scales"), 1,
     "cosyvoice llm: layers.0.mlp.down_proj scales / biases have dtype U32"),
    ("cosyvoice llm", "scales_biases_dtype", f32_copy(C0 + "mlp.down_proj.biases"), 1,
     "cosyvoice llm: layers.0.mlp.down_proj scales / biases differ in dtype"),
    ("cosyvoice llm", "gate_up_rows", rows(C0 + "mlp.up_proj", 624), 1,
     "cosyvoice llm: layers.0.mlp.gate_proj: gate / up row counts do not interleave"),
    ("cosyvoice llm", "bias_shape", widen(C0 + "self_attn.k_proj.bias"), 1,
     "cosyvoice llm: tensor layers.0.self_attn.k_proj.bias has shape [129] dtype BF16, expected float [128]"),
    ("cosyvoice llm", "bias_not_float", as_int(C0 + "self_attn.q_proj.bias"), 1,
     "cosyvoice llm: tensor layers.0.self_attn.q_proj.bias has shape [384] dtype U32, expected float [384]"),
    ("cosyvoice llm", "norm_shape", widen(C0 + "input_layernorm.weight"), 1,
     "cosyvoice llm: tensor layers.0.input_layernorm.weight has shape [385], expected [384]"),
    ("cosyvoice llm", "norm_not_float", as_int("norm.weight"), 1, "cosyvoice llm: tensor norm.weight has dtype U32 (F32 / F16 / BF16)"),
    ("cosyvoice llm", "qkv_rows", rows(C0 + "self_attn.k_proj", 64, bias=True), 1,
     "cosyvoice llm: layers.0.self_attn q/k/v_proj hold 576 rows, expected 640"),
    ("cosyvoice llm", "o_rows", rows(C0 + "self_attn.o_proj", 368), 1,
     "cosyvoice llm: layers.0. o_proj / mlp row counts do not match the geometry"),
    ("cosyvoice llm", "head_rows", rows("speech_head", 20), 1, "cosyvoice llm: speech_head holds 20 rows, expected 21"),
]


@pytest.fixture(scope="module")
def state_dicts():
    return {"talker": synth.synth_tts_talker_state_dict(GT, 0), "cosyvoice llm": synth.synth_cosyvoice_llm_state_dict(GC, 0)}


def create(model, model_dir):
    """(return code, message) of the model's create entry; a handle that a machine with a device does create is freed."""
    lib = _lib.load(strict=True)
    if model == "talker":
        kw = {k: v for k, v in GT.items() if k != "bits"}
        cfg = tts.default_config("0.6B", 4, **kw)
        cfg.bits = GT["bits"]
        h = C.c_void_p()
        rc = lib.qasr_tts_create(str(model_dir).encode(), C.byref(cfg), C.byref(h))
        if h.value:
            lib.qasr_tts_free(h)
        return rc, lib.qasr_tts_last_error(None).decode()
    cfg = cv.default_config(**{**GC, **dict(max_text=KC.MAX_TEXT, max_prompt_tokens=KC.MAX_PROMPT, max_tokens=KC.MAX_TOKENS)})
    rc = lib.qasr_cvlm_check(str(model_dir).encode(), C.byref(cfg))        # qasr_cvlm_create's host half: the same constructor, host_only
    return rc, lib.qasr_cvlm_last_error(None).decode()


def write(model, sd, model_dir, extra=()):
    w = synth.write_tts_talker_safetensors if model == "talker" else synth.write_cosyvoice_llm_safetensors
    return w(sd, str(model_dir), extra=extra)


def run_case(model, change, sd, model_dir):
    sd = dict(sd)
    r = change(sd)
    extra = {r[1]: r[2]} if isinstance(r, tuple) and r and r[0] == "extra" else ()
    return create(model, write(model, sd, model_dir, extra))


@pytest.mark.parametrize("model,name,change,code,message", CASES, ids=[f"{c[0].split()[0]}-{c[1]}" for c in CASES])
def test_refusal(state_dicts, tmp_path, model, name, change, code, message):
    rc, msg = run_case(model, change, state_dicts[model], tmp_path)
    print(model, name, rc, repr(msg))
    assert (rc, msg) == (code, message)


def test_talker_reads_past_keys_it_does_not_name(state_dicts, tmp_path):
    """The Talker's checkpoint holds other sub-models: unknown keys are not refused, also not ones that look like its own."""
    extra = {"speaker_encoder.fc.weight": np.zeros((4, 4), dtype=np.float32), "talker.model.layers.0.self_attn.q_norm.bias": np.zeros(4, dtype=np.float32),
             "talker.lm_head.weight": np.zeros(4, dtype=np.float32)}
    rc, msg = create("talker", write("talker", state_dicts["talker"], tmp_path, extra))
    # the loader's host pass is over: either the handle exists, or the first HIP call has failed on a machine without a device
    assert rc == 0 or (rc == 2 and not msg.startswith("talker: ")), (rc, msg)


def test_cosyvoice_refuses_unknown_keys_but_q_k_norm(state_dicts, tmp_path):
    sd = state_dicts["cosyvoice llm"]
    norms = {f"layers.{l}.self_attn.{n}_norm.weight": np.ones(64, dtype=np.float32) for l in range(GC["layers"]) for n in "qk"}
    assert create("cosyvoice llm", write("cosyvoice llm", sd, tmp_path / "norms", norms))[0] == 0
    rc, msg = create("cosyvoice llm", write("cosyvoice llm", sd, tmp_path / "head", {"lm_head.weight": np.zeros(4, dtype=np.float32)}))
    assert (rc, msg) == (1, "cosyvoice llm: unexpected tensor lm_head.weight")
    # map order: the first unknown key is named, behind every check of the keys that are read
    two = {"zz.weight": np.zeros(4, dtype=np.float32), "layers.0.self_attn.q_norm.bias": np.zeros(4, dtype=np.float32)}
    rc, msg = create("cosyvoice llm", write("cosyvoice llm", sd, tmp_path / "two", two))
    assert (rc, msg) == (1, "cosyvoice llm: unexpected tensor layers.0.self_attn.q_norm.bias")

"""The CosyVoice3 speech-token LLM without a GPU: the torch twin against the float64 oracle (tests/cvlm_oracle.py), the host sampler twin
(csrc/cvlm_sampler.cpp) against a numpy restatement, the prefix plan, and every create-time refusal (the loader's host checks)."""
import ctypes as C

import numpy as np
import pytest

import cvlm_cases as K
import cvlm_oracle as O
from qasr import _lib, cosyvoice as cv, synth
from qasr.model import QasrError


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def config_of(g, **over):
    return cv.default_config(**{**g, **dict(max_text=K.MAX_TEXT, max_prompt_tokens=K.MAX_PROMPT, max_tokens=K.MAX_TOKENS), **over})


# ---- the twin against the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(K.TWIN))
def net(request):
    g = K.GEOMETRIES[request.param]
    return request.param, g, O.Weights(synth.synth_cosyvoice_llm_state_dict(g, 0), g)


def test_twin_distance(net):
    name, g, W = net
    n = K.N_ROWS[name]
    rows, toks = K.make_rows(n, g), K.forced_tokens(n, K.FORCED_T, g)
    assert [K.prefix_len(r) for r in rows[:len(K.EDGE_PREFIX)]] == list(K.EDGE_PREFIX)[:n]
    worst = {}
    for i, row in enumerate(rows):
        a, b = O.forced_pass(row, toks[i], W, O.F64), O.forced_pass(row, toks[i], W, O.TWIN)
        for k in a:
            worst[k] = max(worst.get(k, 0.0), rel(b[k], a[k]))
    print(name, {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert K.TWIN[name][k] / 2 <= v <= K.TWIN[name][k] * 2, (name, k, v)


def test_twin_greedy_free_run_within_the_cap():
    g = K.GEOMETRIES["real4"]
    W = O.Weights(synth.synth_cosyvoice_llm_state_dict(g, 0), g)
    rows = K.make_rows(max(K.GREEDY_ROWS) + 1, g)
    second = total = 0
    for i in K.GREEDY_ROWS:
        toks = O.greedy_run(rows[i], K.GREEDY_T, W, O.TWIN)
        ref = O.forced_pass(rows[i], toks, W, O.F64)["logits"]
        s, t = K.margin_rule(toks, ref, K.MARGIN * K.TWIN["real4"]["logits"] * np.abs(ref).max(), g["speech_tokens"])
        second, total = second + s, total + t
    print("second clause", second, "/", total)
    assert second <= 0.02 * total


# ---- the host sampler twin against numpy ------------------------------------------------------------------------------------------
def host_pick(logits, kw, seed, row=0):
    s = cv.CosySamplingConfig(top_k=kw.get("top_k", 25), top_p=kw.get("top_p", 0.8), win_size=kw.get("win_size", 10), tau_r=kw.get("tau_r", 0.1))
    return cv.sample_host(logits, kw.get("history", ()), kw.get("step", 0), kw.get("below_min", False), s, seed, row)


def test_sampler_twin_equals_numpy_on_crafted_logits():
    ST = 6561
    differing = 0
    for name, logits, kw in K.sampler_cases():
        for seed in (1, 2, 3):
            want, pert, gap = O.sample(logits, ST, seed=seed, return_info=True, **kw)
            assert gap > 1e-4, (name, gap)                       # no top-p boundary near top_p: f32 and f64 sums decide alike
            got = host_pick(logits, kw, seed)
            if got != want:
                assert K.ulp_close(pert, got, want), (name, seed, got, want)
                differing += 1
            assert got < ST + 3, (name, got)                     # the suppressed tail is never picked
            if name.startswith("stop_masked") or name == "suppressed_tail" and kw.get("step", 0) == 0:
                assert got < ST, (name, got)
    assert differing <= 1


def test_sampler_rules():
    ST = 6561
    cases = {n: (lg, kw) for n, lg, kw in K.sampler_cases()}
    lg, kw = cases["ties_at_threshold"]
    seen = {host_pick(lg, kw, s) for s in range(200)}
    assert seen == {10, 20, 30, 40}                              # ties at the threshold survive top_k = 2
    lg, kw = cases["resample_one_repeat"]
    assert all(host_pick(lg, kw, s) != 77 for s in range(20))    # one repeat in the window: max(Int(10 * 0.1), 1) = 1 -> resampled
    lg, kw = cases["no_repeat_no_resample"]
    assert all(host_pick(lg, kw, s) == 77 for s in range(20))
    lg, kw = cases["repeat_outside_window"]
    assert all(host_pick(lg, kw, s) == 77 for s in range(20))    # the repeat is 11 tokens back, the window holds 10
    lg, kw = cases["win_size_zero"]
    assert all(host_pick(lg, kw, s) == 77 for s in range(20))
    lg, kw = cases["stop_live_at_min"]
    assert all(host_pick(lg, kw, s) == ST + 1 for s in range(20))
    for n in ("stop_masked_below_min", "stop_masked_at_token_0"):
        lg, kw = cases[n]
        assert all(host_pick(lg, kw, s) < ST for s in range(20)), n
    # the resample draws from the full distribution (no top-k, no top-p): over seeds it leaves the top-25
    lg, kw = cases["resample_one_repeat"]
    top25 = set(np.argsort(-O.mask_logits(lg, ST, False))[:25].tolist())
    assert any(host_pick(lg, kw, s) not in top25 for s in range(50))


def test_seed_row_and_step_key_the_stream():
    lg = K.sampler_cases()[1][1]
    a = [host_pick(lg, dict(step=f, history=[1]), 5, row=2) for f in range(1, 17)]
    assert a == [host_pick(lg, dict(step=f, history=[1]), 5, row=2) for f in range(1, 17)]
    assert a != [host_pick(lg, dict(step=f, history=[1]), 6, row=2) for f in range(1, 17)]
    assert a != [host_pick(lg, dict(step=f, history=[1]), 5, row=3) for f in range(1, 17)]
    with pytest.raises(QasrError, match="qasr error 1"):
        cv.sample_host(lg, sampling=cv.CosySamplingConfig(win_size=65))


# ---- the prefix plan --------------------------------------------------------------------------------------------------------------
def plan_of(cfg, text, prompt=()):
    lib = _lib.load()
    t, p = np.asarray(text, dtype=np.int32), np.asarray(prompt, dtype=np.int32)
    out = np.zeros(2 + t.size + p.size, dtype=np.int32)
    n = lib.qasr_cvlm_plan_prefix(C.byref(cfg), t.ctypes.data_as(cv._I), t.size, p.ctypes.data_as(cv._I) if p.size else None, p.size,
                                  out.ctypes.data_as(cv._I))
    assert n == out.size
    return out.tolist()


def test_prefix_plan_and_text_frames():
    cfg = cv.default_config(4)
    sos, task = -1 - 6561, -1 - 6563
    assert plan_of(cfg, [7]) == [sos, 7, task]                                           # the minimum: 3 positions
    assert plan_of(cfg, [7, 151646, 9]) == [sos, 7, 151646, 9, task]
    assert plan_of(cfg, [4, 5], [0, 6560, 12]) == [sos, 4, 5, task, -1, -6561, -13]      # prompt speech tokens behind task_id
    g = K.GEOMETRIES["tiny4"]
    assert plan_of(config_of(g), [1], [3]) == [-1 - 13, 1, -1 - 15, -4]
    for row in K.make_rows(12, K.GEOMETRIES["real4"]):                                   # the C plan is the oracle's plan
        want = [(-1 - i if kind == "speech" else i) for kind, i in O.prefix_plan(row["text"], row.get("prompt"), 6561)]
        assert plan_of(cfg, row["text"], row.get("prompt") or ()) == want
    assert cv.frame_text([1, 2], [3]) == [1, 2, 151646, 3]
    assert cv.clone_text([8], [3, 4]) == [8, 151646, 3, 4]
    assert [cv.max_tokens_for(n) for n in (0, 20, 21, 100)] == [200, 200, 210, 1000]
    assert _lib.load().qasr_cvlm_poll_interval() == 8
    assert _lib.load().qasr_cvlm_context(C.byref(config_of(g))) == 320                   # 2 + 256 + 24 + 32 = 314, rounded up to 64


# ---- create-time refusals: the loader runs with host checks alone ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    g = K.GEOMETRIES["tiny4"]
    sd = synth.synth_cosyvoice_llm_state_dict(g, 0)
    return g, sd, synth.write_cosyvoice_llm_safetensors(sd, str(tmp_path_factory.mktemp("cvlm_tiny")))


def refused(code, match, model_dir, cfg):
    with pytest.raises(QasrError, match=f"qasr error {code}.*{match}"):
        cv.CosyVoiceLLM.check(model_dir, cfg)


def test_loader_accepts_the_checkpoint_and_ignores_q_k_norm(tiny, tmp_path):
    g, sd, d = tiny
    cv.CosyVoiceLLM.check(d, config_of(g))
    extra = {f"layers.{l}.self_attn.{n}_norm.weight": np.ones(64, dtype=np.float32) for l in range(g["layers"]) for n in "qk"}
    cv.CosyVoiceLLM.check(synth.write_cosyvoice_llm_safetensors(sd, str(tmp_path / "norms"), extra=extra), config_of(g))
    for dt in ("F32", "F16"):
        cv.CosyVoiceLLM.check(synth.write_cosyvoice_llm_safetensors(sd, str(tmp_path / dt), scales_dtype=dt), config_of(g))


def test_geometry_refusals(tiny):
    g, sd, d = tiny
    for over, match in ((dict(head_dim=128), "head_dim must be 64"), (dict(hidden=512), "heads \\* 64"), (dict(kv_heads=4), "multiple of kv_heads"),
                        (dict(group_size=32), "group size 64"), (dict(bits=3), "bits must be 4 or 8"), (dict(inter=704), "multiples of 128"),
                        (dict(max_batch=65), "max_batch"), (dict(max_batch=0), "max_batch"), (dict(speech_extra=2), "speech_extra"),
                        (dict(speech_tokens=8000, speech_extra=200), "over 8192"), (dict(inter=10368), "not served"),
                        (dict(max_tokens=40000), "over the limit"), (dict(layers=0), "layers")):
        refused(1, match, d, config_of(g, **over))
    refused(1, "16 query heads", d, config_of(dict(g, heads=34, kv_heads=2, hidden=34 * 64)))
    refused(1, "multiples of 128", d, config_of(dict(g, heads=3, kv_heads=1, hidden=192)))


def test_checkpoint_refusals(tiny, tmp_path):
    g, sd, d = tiny
    cfg = config_of(g)
    refused(4, "", str(tmp_path / "nowhere"), cfg)
    w = lambda name, **kw: synth.write_cosyvoice_llm_safetensors(sd, str(tmp_path / name), **kw)
    refused(4, "missing tensor norm.weight", w("a", drop=("norm.weight",)), cfg)
    refused(4, "missing tensor layers.1.self_attn.k_proj.bias", w("b", drop=("layers.1.self_attn.k_proj.bias",)), cfg)
    refused(4, "missing tensor speech_head.scales", w("c", drop=("speech_head.scales",)), cfg)
    refused(1, "unexpected tensor lm_head.weight", w("d", extra={"lm_head.weight": np.zeros(4, dtype=np.float32)}), cfg)
    refused(1, "unexpected tensor layers.0.self_attn.q_norm.bias", w("e", extra={"layers.0.self_attn.q_norm.bias": np.zeros(4, dtype=np.float32)}), cfg)
    refused(1, "speech_embedding.weight has shape", w("f", reshape={"speech_embedding.weight": (20, g["hidden"])}), cfg)
    refused(1, "bits / width mismatch", d, config_of(dict(g, bits=8)))
    refused(1, "layers.2.input_layernorm", w("g", reshape={"layers.2.input_layernorm.weight": (g["hidden"] + 1,)}), cfg)
    refused(4, "missing tensor layers.3", d, config_of(dict(g, layers=4)))
    refused(1, "unexpected tensor layers.2", d, config_of(dict(g, layers=2)))
    fl = synth.synth_cosyvoice_llm_state_dict(g, 0, quantized=False)
    refused(1, "float \\(unquantised\\) checkpoint", synth.write_cosyvoice_llm_safetensors(fl, str(tmp_path / "float")), cfg)
    refused(1, "o_proj / mlp row counts|expected U32", d, config_of(dict(g, inter=768)))

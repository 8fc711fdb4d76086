"""CPU checks of the Qwen3-TTS Talker + code predictor: the prefill builder against cases written out by hand from the doc comment of
buildPrefillEmbeddings, the CodecTokens ids, the host sampler (qasr_tts_sample_host) against the numpy restatement and its rules, the
twin's distance from the float64 oracle on the inputs of tests/test_gpu_talker.py (pinned within a factor of two: the GPU bounds are
MARGIN x these figures), the twin's greedy free run under the margin rule, and the refusals that need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import talker_cases as K
import talker_oracle as O
from qasr import synth, _lib, tts
from qasr.model import QasrError

T = K.TOKENS
PAD, BOS, EOS = T["tts_pad"], T["tts_bos"], T["tts_eos"]
THINK, TBOS, TEOS, CPAD, CBOS = T["codec_think"], T["codec_think_bos"], T["codec_think_eos"], T["codec_pad"], T["codec_bos"]


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


# ---- prefill builder ------------------------------------------------------------------------------------------------------------
def test_prefix_six_and_seven_tokens():
    assert O.codec_prefix(T, 2050) == [THINK, TBOS, 2050, TEOS, CPAD, CBOS]
    assert O.codec_prefix(T, 2055, speaker=3001) == [THINK, TBOS, 2055, TEOS, 3001, CPAD, CBOS]


def test_prefill_plan_plain_many_trailing():
    text = [1, 2, 3, 40, 41, 42, 43, 5, 6, 7, 8, 9]
    plan, trailing = O.prefill_plan(text, T, 2050)
    assert plan == [(1, None), (2, None), (3, None),                                       # role
                    (PAD, THINK), (PAD, TBOS), (PAD, 2050), (PAD, TEOS), (BOS, CPAD),      # tts_pad x 4, tts_bos over the prefix but its last
                    (40, CBOS)]                                                            # first text + codec_bos
    assert trailing == [41, 42, 43, EOS]


def test_prefill_plan_speaker_xvector_instruct_and_short_texts():
    nine = [1, 2, 3, 40, 5, 6, 7, 8, 9]
    plan, trailing = O.prefill_plan(nine, T, 2050, speaker=3001)
    assert plan[3:] == [(PAD, THINK), (PAD, TBOS), (PAD, 2050), (PAD, TEOS), (PAD, 3001), (BOS, CPAD), (40, CBOS)]
    assert trailing == [EOS]                                                               # trailing empty: tts_eos alone
    plan, trailing = O.prefill_plan(nine[:4] + [41] + nine[4:], T, 2050, xvector=True)
    assert plan[3:] == [(PAD, THINK), (PAD, TBOS), (PAD, 2050), (PAD, TEOS), (PAD, "xvec"), (BOS, CPAD), (40, CBOS)]   # after index 3
    assert trailing == [41, EOS]                                                           # one trailing token
    plan, _ = O.prefill_plan(nine, T, 2050, instruct=[70, 71])
    assert plan[:5] == [(70, None), (71, None), (1, None), (2, None), (3, None)] and len(plan) == 11


def test_codec_tokens_fixture():
    with open(os.path.join(os.path.dirname(__file__), "golden", "tts_codec_tokens.json")) as f:
        gold = json.load(f)
    for name, want in gold["languages"].items():
        assert tts.CodecTokens.language_id(name) == want, name
    cfg = tts.default_config("0.6B", 4)
    for k, v in gold.items():
        if k != "languages":
            assert getattr(cfg, k) == v, k
            if hasattr(tts.CodecTokens, k):
                assert getattr(tts.CodecTokens, k) == v
    big = tts.default_config("Qwen3-TTS-12Hz-1.7B-Base-MLX-8bit", 8)
    assert (big.hidden, big.inter, big.cp_embedding_dim, big.cp_hidden, big.bits) == (2048, 6144, 2048, 1024, 8)
    assert (cfg.hidden, cfg.layers, cfg.cp_layers, cfg.max_frames) == (1024, 28, 5, 500)
    assert tts.prepare_text_tokens([7, 8]) == [151644, 77091, 198, 7, 8, 151645, 198, 151644, 77091, 198]
    assert tts.prepare_instruct_tokens([7]) == [151644, 872, 198, 7, 151645, 198]


# ---- host sampler ---------------------------------------------------------------------------------------------------------------
def logits_of(seed, V=3072, scale=3.0):
    return (scale * np.random.default_rng(seed).standard_normal(V)).astype(np.float32)


@pytest.mark.parametrize("talker", (True, False))
def test_host_sampler_equals_numpy(talker):
    V = 3072 if talker else 2048
    for seed in range(12):
        lg = logits_of(seed, V)
        hist = [int(v) for v in np.random.default_rng(100 + seed).integers(0, 2048, 9)]
        s = tts.SamplingConfig(eos_logit_bias=0.5 if seed % 2 else 0.0)
        got = tts.sample_host(lg, s, talker=talker, history=hist, seed=seed, row_index=3, frame=seed, group=0 if talker else 5)
        want = O.sample(lg, eos_logit_bias=s.eos_logit_bias, history=hist, talker=talker, seed=seed, row=3, frame=seed,
                        group=0 if talker else 5)
        assert got == want, seed


def test_greedy_is_first_maximum_and_suppress_range():
    lg = np.zeros(3072, dtype=np.float32)
    lg[[700, 1500]] = 4.0                                              # two equal maxima: the first wins
    lg[2500] = 9.0                                                     # suppressed
    assert tts.sample_host(lg, tts.SamplingConfig.greedy()) == 700
    lg[2150] = 9.0                                                     # EOS lies in the range and is exempt
    assert tts.sample_host(lg, tts.SamplingConfig.greedy()) == 2150
    for seed in range(20):                                             # sampled: the range never wins, except EOS
        t = tts.sample_host(logits_of(seed) + np.where(np.arange(3072) >= 2048, 5, 0).astype(np.float32), tts.SamplingConfig(), seed=seed)
        assert t < 2048 or t == 2150


def test_penalty_is_sign_aware():
    lg = np.full(2048 + 1024, -5.0, dtype=np.float32)
    lg[10], lg[11] = 2.0, 1.95                                         # 10 in the history: 2.0 / 1.05 < 1.95
    assert tts.sample_host(lg, tts.SamplingConfig.greedy(), history=[10, 10]) == 11
    assert tts.sample_host(lg, tts.SamplingConfig(temperature=0, top_k=1, repetition_penalty=1.0), history=[10]) == 10
    neg = np.full(3072, -9.0, dtype=np.float32)
    neg[20], neg[21] = -2.0, -2.05                                     # negative logits multiply: -2.0 x 1.05 < -2.05
    assert tts.sample_host(neg, tts.SamplingConfig.greedy(), history=[20]) == 21


def test_top_k_ties_eos_and_membership():
    V, k = 3072, 5
    for seed in range(30):
        lg = logits_of(seed)
        s = tts.SamplingConfig(top_k=k, repetition_penalty=1.0)
        t = tts.sample_host(lg, s, seed=seed)
        masked = lg.copy()
        masked[2048:] = -1e9
        top = set(np.argsort(-masked, kind="stable")[:k].tolist())
        assert t in top or t == 2150, seed
    # ties with the threshold survive: 8 equal values at the top with k = 3 are all reachable
    lg = np.full(V, -20.0, dtype=np.float32)
    lg[100:108] = 1.0
    seen = {tts.sample_host(lg, tts.SamplingConfig(top_k=3, repetition_penalty=1.0), seed=s) for s in range(200)}
    assert seen <= set(range(100, 108)) | {2150} and len(seen & set(range(100, 108))) > 3
    # EOS survives top-k and takes the bias
    lg = logits_of(3)
    lg[2150] = -30.0
    s = tts.SamplingConfig(top_k=2, eos_logit_bias=1000.0)
    assert tts.sample_host(lg, s, seed=1) == 2150
    assert all(tts.sample_host(lg, tts.SamplingConfig(top_k=2), seed=q) != 2150 for q in range(20))


def test_seed_and_counter():
    lg = logits_of(9)
    s = tts.SamplingConfig()
    a = [tts.sample_host(lg, s, seed=5, row_index=2, frame=f) for f in range(16)]
    assert a == [tts.sample_host(lg, s, seed=5, row_index=2, frame=f) for f in range(16)]
    assert a != [tts.sample_host(lg, s, seed=6, row_index=2, frame=f) for f in range(16)]
    assert a != [tts.sample_host(lg, s, seed=5, row_index=3, frame=f) for f in range(16)]
    with pytest.raises(QasrError, match="qasr error 7"):
        tts.sample_host(lg, tts.SamplingConfig(top_p=0.9))


# ---- the twin against the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(K.GEOMETRIES))
def net(request):
    g = K.GEOMETRIES[request.param]
    return request.param, g, O.Weights(synth.synth_tts_talker_state_dict(g, 0), g)


def test_twin_distance(net):
    name, g, W = net
    n = K.N_ROWS[name]
    rows, codes = K.make_rows(n, g["hidden"]), K.forced_codes(n, K.FORCED_T)
    worst = {}
    for i, row in enumerate(rows):
        a, b = O.forced_pass(row, codes[i], W, O.F64, T), O.forced_pass(row, codes[i], W, O.TWIN, T)
        for k in a:
            worst[k] = max(worst.get(k, 0.0), rel(b[k], a[k]))
    print(name, {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert K.TWIN[name][k] / 2 <= v <= K.TWIN[name][k] * 2, (name, k, v)


def test_twin_greedy_free_run_within_the_cap(net):
    name, g, W = net
    rows = K.make_rows(max(K.GREEDY_SEEDS) + 1, g["hidden"])
    second = total = 0
    for i in K.GREEDY_SEEDS:
        codes = O.greedy_run(rows[i], K.GREEDY_T, W, O.TWIN, T)
        assert codes.shape == (16, K.GREEDY_T)
        ref = O.forced_pass(rows[i], codes, W, O.F64, T)
        s, t = K.margin_rule(codes, ref, K.MARGIN * K.TWIN[name]["talker"] * np.abs(ref["talker"]).max(),
                           K.MARGIN * K.TWIN[name]["cp"] * np.abs(ref["cp"]).max())
        second, total = second + s, total + t
    print(name, "second clause", second, "/", total)
    assert second <= 0.02 * total


# ---- refusals without a device --------------------------------------------------------------------------------------------------
def test_create_refusals(tmp_path):
    lib = _lib.load(strict=True)
    g = K.GEOMETRIES["small4"]

    def create(model_dir, **over):
        kw = dict(g, **over)
        cfg = tts.default_config("0.6B", 4, **{k: v for k, v in kw.items() if k != "bits"})
        cfg.bits = kw["bits"]
        h = C.c_void_p()
        rc = lib.qasr_tts_create(str(model_dir).encode(), C.byref(cfg), C.byref(h))
        assert not h.value
        return rc, lib.qasr_tts_last_error(None).decode()

    rc, msg = create(tmp_path / "missing")
    assert rc == 4 and msg.startswith("talker: ")
    for over, word in ((dict(head_dim=64), "head_dim"), (dict(hidden=160), "multiple of 64"), (dict(max_batch=65), "max_batch"),
                       (dict(max_frames=501), "max_frames"), (dict(heads=4, kv_heads=4), "2 query heads"), (dict(bits=3), "bits")):
        rc, msg = create(tmp_path, **over)
        assert rc == 1 and word in msg, (over, msg)
    # a float (unquantised) checkpoint is refused with a clear message, before any device call
    d = synth.write_tts_talker_safetensors(synth.synth_tts_talker_state_dict(g, 0, quantized=False), str(tmp_path / "float"))
    rc, msg = create(d)
    assert rc == 1 and "float (unquantised) checkpoint" in msg, msg
    sd = synth.synth_tts_talker_state_dict(g, 0)
    d = synth.write_tts_talker_safetensors(sd, str(tmp_path / "drop"), drop=("talker.code_predictor.lm_head.7.scales",))
    rc, msg = create(d)
    assert rc == 4 and "missing tensor talker.code_predictor.lm_head.7.scales" in msg, msg
    rc, msg = create(synth.write_tts_talker_safetensors(sd, str(tmp_path / "bits")), bits=8)
    assert rc == 1 and "bits / width mismatch" in msg, msg

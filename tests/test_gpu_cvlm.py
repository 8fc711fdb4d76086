"""The CosyVoice3 speech-token LLM on the MI355X (csrc/llm_cosyvoice.hip, csrc/api_cvlm.cpp) over the C ABI, against the float64 oracle
tests/cvlm_oracle.py, with synthetic MLX 4 / 8 bit weights (qasr.synth) on the reduced geometries of tests/cvlm_cases.py.

Tolerances.  Forced logits and hidden: the device computes in bf16 between ops, like the oracle's torch twin;
tests/test_cvlm_cpu.py::test_twin_distance measures, on these inputs, the twin's max |d| / peak from the oracle (cvlm_cases.TWIN); each
GPU bound is MARGIN = 4 x its figure, the project's margin for a bf16 path (argued in the docstring of tests/test_gpu_talker.py: the
device and the twin differ in summation order and in the SwiGLU's exp / rcp instructions, the twin's own figure moves by a factor of
three between rows, a wrong position, head or table moves the output by its whole peak).  One linear alone (qasr_cvlm_linear_probe): the
bound is the worst case of the number formats, element by element, computed from the float64 terms: the RMSNorm prologue rounds every
input twice to bf16 (2 x 2^-8 of sum |w x|: half an ulp of 8 significant bits), the output is rounded once (2^-8 |y|), the q|k|v bias adds one more rounding, the residual
form rounds the product and the sum, SwiGLU rounds gate, up, silu(gate) and the product (first-order propagation with |silu'| <= 1.1)
and its exp / rcp instructions are good to 2^-20; f32 accumulation over K <= 4864 terms adds K x 2^-24 of sum |w x|.
Contexts: the attention sweeps rounds of 256 keys, 64 per wave; rows 2 .. 8 put the prefix so that the 24 forced tokens start on either
side of 64 keys and cross 128, 192 and 256.  Every test prints the device's distances; DESIGN.md section 23 holds the parity table."""
import ctypes as C

import numpy as np
import pytest
import torch

import cvlm_cases as K
import cvlm_oracle as O
from qasr import _lib, cosyvoice as cv, synth
from qasr.flow import CosyVoiceFlow
from qasr.model import QasrError
from qasr.vocoder import HiFTVocoder

pytestmark = pytest.mark.gpu
LIMITS = dict(max_text=K.MAX_TEXT, max_prompt_tokens=K.MAX_PROMPT, max_tokens=K.MAX_TOKENS)
GREEDY = cv.CosySamplingConfig(top_k=1, top_p=1.0, win_size=0, min_ratio=1000.0)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def open_model(model_dir, g, max_batch):
    return cv.CosyVoiceLLM.from_pretrained(model_dir, **{**g, **LIMITS, "max_batch": max_batch})


class Net:
    def __init__(self, name, tmp, max_batch, with_ref=True):
        self.name, self.g = name, K.GEOMETRIES[name]
        self.sd = synth.synth_cosyvoice_llm_state_dict(self.g, 0)
        self.W = O.Weights(self.sd, self.g)
        self.dir = synth.write_cosyvoice_llm_safetensors(self.sd, str(tmp.mktemp(name)))
        self.m = open_model(self.dir, self.g, max_batch)
        n = K.N_ROWS[name]
        self.rows, self.tokens = K.make_rows(n, self.g), K.forced_tokens(n, K.FORCED_T, self.g)
        self.ref = [O.forced_pass(r, self.tokens[i], self.W, O.F64) for i, r in enumerate(self.rows)] if with_ref else None   # once, shared

    def args(self, idx):
        return dict(texts=[self.rows[i]["text"] for i in idx], prompts=[self.rows[i].get("prompt") for i in idx])


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    n = Net("real4", tmp_path_factory, 33)
    yield n
    n.m.close()


@pytest.fixture(scope="module")
def odd(tmp_path_factory):
    n = Net("odd8", tmp_path_factory, 64)
    yield n
    n.m.close()


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    n = Net("tiny4", tmp_path_factory, 17, with_ref=False)
    yield n
    n.m.close()


# ---- 1. forced logits and hidden against the oracle ------------------------------------------------------------------------------------
def check_forced(net, idx):
    lg, hd = net.m.forced(tokens=net.tokens[idx], **net.args(idx))
    worst = {}
    for j, i in enumerate(idx):
        for k, out in (("logits", lg), ("hidden", hd)):
            assert np.isfinite(out[j]).all()
            d = rel(out[j], net.ref[i][k])
            worst[k] = max(worst.get(k, 0.0), d)
            assert d <= K.MARGIN * K.TWIN[net.name][k], (net.name, len(idx), i, k, d)
    print(net.name, "B", len(idx), {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("B", (1, 15, 16, 17, 33))
def test_forced_logits_against_the_oracle(real, B):
    check_forced(real, list(range(33 - B, 33)) if B < 9 else list(range(B)))
    if B == 1:
        for i in K.EDGE_ROWS:                                            # the shortest prefixes and every context edge, alone
            check_forced(real, [i])


def test_forced_logits_8_bit(odd):
    check_forced(odd, list(range(5)))


# ---- 2. one linear alone against float64 -----------------------------------------------------------------------------------------------
U = 2.0 ** -8                                                            # half an ulp of bf16 (8 significant bits), relative


def bf16_values(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def linear_reference(net, kind, layer, x, resid):
    """(y, bound) in float64, element by element: see the module docstring."""
    W, g = net.W, net.g
    w = lambda key: W.get(key, O.F64).numpy()
    p = f"layers.{layer}."
    K_ = x.shape[1]
    acc_slack = K_ * 2.0 ** -24

    def normed(norm_key):
        inv = 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + O.EPS)
        return x * inv * w(norm_key)[None]

    def dot(h, mat):
        return h @ mat.T, np.abs(h) @ np.abs(mat).T                      # sum w x, sum |w x|

    if kind == "qkv":
        mat = np.concatenate([w(p + f"self_attn.{n}_proj.weight") for n in "qkv"])
        b = np.concatenate([w(p + f"self_attn.{n}_proj.bias") for n in "qkv"])
        y, a = dot(normed(p + "input_layernorm.weight"), mat)
        return y + b[None], (2 * U + acc_slack) * a + U * np.abs(y) + U * np.abs(y + b[None]) + 1e-30
    if kind in ("o", "down"):
        y, a = dot(x, w(p + ("self_attn.o_proj" if kind == "o" else "mlp.down_proj") + ".weight"))
        return resid + y, acc_slack * a + U * np.abs(y) + U * np.abs(resid + y) + 1e-30
    if kind == "gate_up":
        h = normed(p + "post_attention_layernorm.weight")
        gt, ga = dot(h, w(p + "mlp.gate_proj.weight"))
        up, ua = dot(h, w(p + "mlp.up_proj.weight"))
        dg, du = (2 * U + acc_slack) * ga + U * np.abs(gt), (2 * U + acc_slack) * ua + U * np.abs(up)
        sg = gt / (1.0 + np.exp(-gt))
        return sg * up, 1.1 * np.abs(up) * dg + np.abs(sg) * du + (2 * U + 2.0 ** -19) * np.abs(sg * up) + 1.1 * dg * du + 1e-30
    y, a = dot(normed("norm.weight"), w("speech_head.weight"))
    return y, (2 * U + acc_slack) * a + 2.0 ** -22 * np.abs(y) + 1e-30


@pytest.mark.parametrize("kind", ("qkv", "o", "gate_up", "down", "head"))
@pytest.mark.parametrize("which", ("real4", "odd8"))
def test_linear_probe_against_float64(real, odd, which, kind):
    net = real if which == "real4" else odd
    g = net.g
    layer = g["layers"] - 1
    Kin = {"qkv": g["hidden"], "o": g["heads"] * 64, "gate_up": g["hidden"], "down": g["inter"], "head": g["hidden"]}[kind]
    rng = np.random.default_rng(41)
    x = bf16_values(rng.standard_normal((64, Kin)))
    x[3] *= 40.0                                                         # rows of very different scale: the norm prologue is per row
    x[5] *= 0.02
    x = bf16_values(x)
    resid = bf16_values(rng.standard_normal((64, g["hidden"]))) if kind in ("o", "down") else None
    want, bound = linear_reference(net, kind, layer, x, resid)
    first = {}
    for B in (1, 16, 17, 64):
        y = net.m.linear_probe(kind, x[:B], layer, None if resid is None else resid[:B]).astype(np.float64)
        assert y.shape == want[:B].shape and np.isfinite(y).all()
        d = np.abs(y - want[:B])
        print(which, kind, "B", B, "max |d| / peak %.2e" % (d.max() / np.abs(want[:B]).max()), "max d / bound %.3f" % (d / bound[:B]).max())
        assert (d <= bound[:B]).all(), (which, kind, B, float((d / bound[:B]).max()))
        if kind == "head":                                               # the rows behind the last whole 16-row tile of the padded image
            V = g["speech_tokens"] + g["speech_extra"]
            assert (d[:, V - 9:] <= bound[:B, V - 9:]).all() and np.abs(y[:, V - 9:]).max() > 0
        for r in range(B):                                               # a row's bits do not depend on the batch
            if r in first:
                assert np.array_equal(first[r], y[r]), (which, kind, B, r)
            else:
                first[r] = y[r].copy()


# ---- 3. prompt chunking ------------------------------------------------------------------------------------------------------------------
def test_prompt_chunking_gives_the_same_bits(real):
    lib = _lib.load()
    idx = [0, 1, 2, 4, 5, 8, 12]
    old = C.c_int()
    assert lib.qasr_get_tuning(b"cvlm_prompt_chunk", C.byref(old)) == 0 and old.value == 64
    try:
        a = real.m.forced(tokens=real.tokens[idx], **real.args(idx))
        assert lib.qasr_set_tuning(b"cvlm_prompt_chunk", 1) == 0
        b = real.m.forced(tokens=real.tokens[idx], **real.args(idx))
        assert lib.qasr_set_tuning(b"cvlm_prompt_chunk", 2) != 0                          # 64 | 1 only
    finally:
        assert lib.qasr_set_tuning(b"cvlm_prompt_chunk", old.value) == 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 4. bit identity: alone, in a batch at another slot, under another max_batch ---------------------------------------------------------
def test_a_row_is_the_same_bits_alone_and_in_any_batch(real):
    idx = list(range(16, -1, -1))                                        # 17 rows; row i sits at slot 16 - i
    s = cv.CosySamplingConfig(min_ratio=1000.0)                          # default sampling, stops masked: every row runs its 12 tokens
    lg, hd = real.m.forced(tokens=real.tokens[idx], **real.args(idx))
    gen = real.m.generate(max_tokens=[12] * 17, sampling=s, seed=7, row_index=idx, **real.args(idx))
    other = open_model(real.dir, real.g, 3)
    try:
        for i in (0, 2, 8, 11):
            j = idx.index(i)
            for m in (real.m, other):
                l1, h1 = m.forced(tokens=real.tokens[[i]], **real.args([i]))
                assert np.array_equal(l1[0], lg[j]) and np.array_equal(h1[0], hd[j]), i
                g1 = m.generate(max_tokens=[12], sampling=s, seed=7, row_index=[i], **real.args([i]))
                assert len(g1[0]) == 12 and np.array_equal(g1[0], gen[j]), i
    finally:
        other.close()


# ---- 5. the device sampler against the host twin ----------------------------------------------------------------------------------------
def test_device_sampler_equals_host_twin(real):
    ST, V = 6561, 6761
    rows = []                                                            # (logits, kwargs, seed)
    for name, logits, kw in K.sampler_cases():
        rows += [(logits, kw, seed) for seed in (1, 2, 3)]
    rng = np.random.default_rng(3)
    for i in range(64):
        lg = (rng.standard_normal(V) * (1.0 + 3.0 * rng.random())).astype(np.float32)
        n = int(rng.integers(0, 13))
        kw = dict(history=[int(t) for t in rng.integers(0, ST, n)], step=n, below_min=bool(i % 2))
        if n and i % 4 == 0:
            lg[kw["history"][-1]] = 25.0                                 # the likely pick is in the window: the resample route
        rows += [(lg, kw, seed) for seed in (11, 12, 13)]
    differing = 0
    by_setting = {}
    for r in rows:
        kw = r[1]
        by_setting.setdefault((kw.get("top_k", 25), kw.get("top_p", 0.8), kw.get("win_size", 10), r[2]), []).append(r)
    for (top_k, top_p, win, seed), group in by_setting.items():
        s = cv.CosySamplingConfig(top_k=top_k, top_p=top_p, win_size=win)
        for at in range(0, len(group), 33):
            part = group[at:at + 33]
            got = real.m.sample(np.stack([p[0] for p in part]), [p[1].get("history", ()) for p in part], [p[1].get("step", 0) for p in part],
                                [p[1].get("below_min", False) for p in part], s, seed, row_index=list(range(100, 100 + len(part))))
            for j, (lg, kw, _) in enumerate(part):
                want = cv.sample_host(lg, kw.get("history", ()), kw.get("step", 0), kw.get("below_min", False), s, seed, 100 + j)
                if int(got[j]) != want:
                    _, pert, gap = O.sample(lg, ST, seed=seed, row=100 + j, return_info=True, **kw)
                    assert gap > 1e-4 and K.ulp_close(pert, int(got[j]), want), (kw, seed, int(got[j]), want)
                    differing += 1
    print("picks that differ within 4 ulp:", differing, "/", len(rows))
    assert differing <= 1


# ---- 6. greedy free run ------------------------------------------------------------------------------------------------------------------
def test_greedy_free_run_against_the_oracle(real):
    idx = list(K.GREEDY_ROWS)
    got = real.m.generate(max_tokens=[K.GREEDY_T] * len(idx), sampling=GREEDY, **real.args(idx))
    second = total = 0
    for j, i in enumerate(idx):
        assert got[j].shape == (K.GREEDY_T,)
        ref = O.forced_pass(real.rows[i], got[j], real.W, O.F64)["logits"]
        s, t = K.margin_rule(got[j], ref, K.MARGIN * K.TWIN["real4"]["logits"] * np.abs(ref).max(), real.g["speech_tokens"])
        second, total = second + s, total + t
    print("second clause", second, "/", total)
    assert second <= 0.02 * total


# ---- 7. sampled free run with natural stops --------------------------------------------------------------------------------------------
def test_sampled_free_run_stops_and_the_twin_reproduces_it(tiny):
    g, ST = tiny.g, tiny.g["speech_tokens"]
    idx = list(range(17))
    caps = [7, 8, 9] + [K.MAX_TOKENS] * 14                               # rows 0 1 2 end at their max_tokens, around the poll interval of 8,
    content = [100] * 3 + [2] * 14                                       # their stops masked throughout (min_len = 200); the others: min_len = 4
    min_len = [int(np.float32(c) * np.float32(2.0)) for c in content]
    s = cv.CosySamplingConfig(min_ratio=2.0)
    cfg = cv.default_config(**{**g, **LIMITS})
    got = tiny.m.generate(content_len=content, max_tokens=caps, sampling=s, seed=K.SAMPLED_SEED, **tiny.args(idx))
    n = [len(t) for t in got]
    print("tokens per row", n)
    assert n[:3] == [7, 8, 9]
    stops = {}
    differing = 0
    for b in idx:
        T = min(n[b] + 1, K.MAX_TOKENS)
        fed = np.concatenate([got[b], np.zeros(T - n[b], dtype=np.int32)])[None]
        lg, _ = tiny.m.forced(tokens=fed, want_hidden=False, **tiny.args([b]))
        for f in range(T):
            want = cv.sample_host(lg[0, f], got[b][:f], f, f < min_len[b], s, K.SAMPLED_SEED, b, cfg)
            if f < n[b]:
                if want != int(got[b][f]):
                    _, pert, gap = O.sample(lg[0, f], ST, history=got[b][:f], step=f, below_min=f < min_len[b], seed=K.SAMPLED_SEED, row=b, return_info=True)
                    assert gap > 1e-4 and K.ulp_close(pert, want, int(got[b][f])), (b, f, want, int(got[b][f]))
                    differing += 1
                assert int(got[b][f]) < ST                               # a stop token is never stored
            elif n[b] < caps[b]:                                         # the step behind the row's last token: the twin names the stop
                assert ST <= want < ST + 3, (b, f, want)
                assert f >= min_len[b]                                   # no stop before min_len
                stops.setdefault(want, []).append(b)
    print("rows ended by each stop token", stops, "picks within 4 ulp", differing)
    assert differing <= 1
    assert sorted(stops) == [ST, ST + 1, ST + 2]                         # each of the three stop tokens ends at least one row
    ended = [n[b] for b in idx[3:] if n[b] < caps[b]]
    assert len(set(ended)) >= 3                                          # rows end at different steps
    for b in idx:
        assert n[b] <= caps[b]


# ---- 8. text ids to audio ----------------------------------------------------------------------------------------------------------------
def test_synthesize_equals_its_stages(real, tmp_path_factory):
    flow = CosyVoiceFlow.from_pretrained(synth.write_cosyvoice_flow_safetensors(synth.synth_cosyvoice_flow_state_dict(0, depth=2),
                                                                                str(tmp_path_factory.mktemp("flow2"))), max_frames=512)
    voc = HiFTVocoder.from_pretrained(synth.write_cosyvoice_hifigan_safetensors(synth.synth_cosyvoice_hifigan_state_dict(0),
                                                                                str(tmp_path_factory.mktemp("hift"))), max_frames=512)
    try:
        idx = [2, 3]                                                     # row 2 has prompt speech tokens, row 3 has none
        a = real.args(idx)
        rng = np.random.default_rng(9)
        p = len(a["prompts"][0])
        feat = [rng.standard_normal((80, 2 * p)).astype(np.float32), None]
        spk = [rng.standard_normal(192).astype(np.float32), None]
        s = cv.CosySamplingConfig(min_ratio=1000.0)
        tts = cv.CosyVoiceTTS(real.m, flow, voc)
        wav, tok = tts.synthesize(a["texts"], prompts=a["prompts"], prompt_feat=feat, spk_emb=spk, max_tokens=[10, 6], sampling=s, seed=21,
                                  return_tokens=True)
        gen = real.m.generate(max_tokens=[10, 6], sampling=s, seed=21, **a)
        assert [len(t) for t in tok] == [10, 6] and all(np.array_equal(x, y) for x, y in zip(tok, gen))
        mels = flow.generate_batch(gen, a["prompts"], feat, spk, seeds=[21, 22], strip_prompt=False)
        pcm = voc.decode_batch([np.ascontiguousarray(m.T) for m in mels], [21, 22])
        want = [pcm[0][480 * 2 * p:], pcm[1]]
        assert wav[0].size == 480 * 2 * 10 + 16 and wav[1].size == 480 * 2 * 6 + 16
        for x, y in zip(wav, want):
            assert np.array_equal(x, y) and np.isfinite(x).all() and np.abs(x).max() > 0
    finally:
        flow.close()
        voc.close()


# ---- 9. run-time refusals ----------------------------------------------------------------------------------------------------------------
def test_run_time_refusals(tiny):
    m, g = tiny.m, tiny.g
    ok = dict(texts=[[1, 2, 3]], prompts=[[4, 5]])
    with pytest.raises(QasrError, match="qasr error 1: .*row 1: text id 1024"):
        m.generate(texts=[[1], [5, g["text_vocab"]]])
    with pytest.raises(QasrError, match="qasr error 1: .*row 0: text id -1"):
        m.generate(texts=[[-1]])
    with pytest.raises(QasrError, match="qasr error 1: .*row 0: prompt speech token 13"):
        m.generate(texts=[[1]], prompts=[[13]])                          # a special token is no prompt speech token
    with pytest.raises(QasrError, match="qasr error 1: .*row 0: an empty text"):
        m.generate(texts=[[]])
    with pytest.raises(QasrError, match="qasr error 5: .*max_text"):
        m.generate(texts=[[1] * (K.MAX_TEXT + 1)])
    with pytest.raises(QasrError, match="qasr error 5: .*max_prompt_tokens"):
        m.generate(texts=[[1]], prompts=[[1] * (K.MAX_PROMPT + 1)])
    with pytest.raises(QasrError, match="qasr error 5: .*max_tokens"):
        m.generate(max_tokens=[K.MAX_TOKENS + 1], **ok)
    with pytest.raises(QasrError, match="qasr error 5: .*max_batch"):
        m.generate(texts=[[1]] * 18)
    with pytest.raises(QasrError, match="qasr error 1: .*win_size"):
        m.generate(sampling=cv.CosySamplingConfig(win_size=65), **ok)
    with pytest.raises(QasrError, match="qasr error 1: .*forced token 21"):
        m.forced(tokens=[[0, 21]], **ok)
    with pytest.raises(QasrError, match="qasr error 5: .*forced tokens"):
        m.forced(tokens=[[0] * (K.MAX_TOKENS + 1)], **ok)
    with pytest.raises(QasrError, match="qasr error 1: .*kind"):
        m._check(m.lib.qasr_cvlm_linear_probe(m.h, 0, 9, np.zeros(384, dtype=np.float32).ctypes.data_as(cv._F), None, 1,
                                              np.zeros(640, dtype=np.float32).ctypes.data_as(cv._F)))
    with pytest.raises(QasrError, match="qasr error 1: .*resid"):
        m.linear_probe("o", np.zeros((1, 384), dtype=np.float32))
    lib = m.lib
    s = cv.CosySamplingConfig().c_struct()
    rq = cv._Request([[1, 2]])
    tok, n = np.zeros((1, K.MAX_TOKENS), dtype=np.int32), np.zeros(1, dtype=np.int32)
    assert lib.qasr_cvlm_generate(m.h, None, C.byref(s), 0, cv._iptr(tok), cv._iptr(n)) == 1
    assert lib.qasr_cvlm_generate(m.h, C.byref(rq.c), None, 0, cv._iptr(tok), cv._iptr(n)) == 1
    assert lib.qasr_cvlm_generate(m.h, C.byref(rq.c), C.byref(s), 0, None, cv._iptr(n)) == 1
    assert lib.qasr_cvlm_forced(m.h, C.byref(rq.c), None, 1, None, None) == 1
    assert lib.qasr_cvlm_generate(None, C.byref(rq.c), C.byref(s), 0, cv._iptr(tok), cv._iptr(n)) == 1
    assert lib.qasr_cvlm_synthesize(m.h, None, None, C.byref(rq.c), C.byref(s), 0, None, None, None, None, None, None, None) == 1
    # the handle still works after every refusal; a closed handle refuses
    assert len(m.generate(max_tokens=[3], sampling=GREEDY, **ok)[0]) == 3
    other = open_model(tiny.dir, g, 1)
    other.close()
    assert other.h is None
    with pytest.raises(QasrError, match="qasr error 1"):
        other.generate(**ok)

"""The Qwen3-TTS Talker + code predictor on the MI355X (csrc/tts_talker.hip, csrc/api_tts.cpp) over the C ABI, against the float64
oracle tests/talker_oracle.py, with synthetic MLX 4 / 8 bit weights (qasr.synth) on the reduced geometries of tests/talker_cases.py.

Tolerances: the device computes in bf16 between ops, like the oracle's torch twin.  tests/test_talker_cpu.py::test_twin_distance measures,
on these inputs, the twin's max |d| / peak from the oracle (talker_cases.TWIN); each GPU bound is MARGIN = 4 x its figure.  The device and
the twin are two realisations of the same rounding points that differ in summation order, in the attention's P (bf16 on the matrix cores
for the Talker) and in the SwiGLU's exp / rcp instructions; the twin's own figure moves by a factor of three between rows and geometries
(3.4e-3 .. 1.0e-2 for the Talker's logits), so a factor below that would test the draw, while a wrong position, head or table moves the
output by its whole peak, 25 x the bound.  Contexts: the Talker's attention sweeps 32-key chunks, eight per round; rows 4 .. 8 put the
prompt's end so that the 24 forced frames cross 31 | 32 | 33, 63 | 64 | 65 and 255 | 256 | 257 keys.  A text longer than the frames
(rows of up to 40 tokens against 24 frames) and one that runs out (rows 0 and 1: tts_pad from frame 1 or 2 on) are part of the forced cases.
Every test prints the device's distances; DESIGN.md section 18 holds the parity table they fill."""
import numpy as np
import pytest

import talker_cases as K
import talker_oracle as O
from qasr import synth, tts, _lib
from qasr.codec import SpeechTokenizerDecoder
from qasr.model import QasrError

pytestmark = pytest.mark.gpu
T = K.TOKENS
POLL = 8
MAX_FRAMES = 32
CFG = dict(max_frames=MAX_FRAMES, max_text=64, max_instruct=K.MAX_INSTRUCT, tts_pad=T["tts_pad"], tts_bos=T["tts_bos"], tts_eos=T["tts_eos"])


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def open_model(model_dir, g, max_batch):
    cfg = tts.default_config("0.6B", 4, **{k: v for k, v in g.items() if k != "bits"})
    cfg.bits = g["bits"]
    return tts.Qwen3TTSModel.from_pretrained(model_dir, cfg, max_batch=max_batch, **{k: v for k, v in CFG.items() if k.startswith("max")})


class Net:
    def __init__(self, name, tmp, max_batch):
        self.name, self.g = name, K.GEOMETRIES[name]
        self.sd = synth.synth_tts_talker_state_dict(self.g, 0)
        self.W = O.Weights(self.sd, self.g)
        self.dir = synth.write_tts_talker_safetensors(self.sd, str(tmp.mktemp(name)))
        self.m = open_model(self.dir, self.g, max_batch)
        n = K.N_ROWS[name]
        self.rows, self.codes = K.make_rows(n, self.g["hidden"]), K.forced_codes(n, K.FORCED_T)
        self.ref = [O.forced_pass(r, self.codes[i], self.W, O.F64, T) for i, r in enumerate(self.rows)]      # computed once, shared

    def args(self, idx):
        rows = [self.rows[i] for i in idx]
        return dict(texts=[r["text"] for r in rows], languages=[r["language"] for r in rows], speakers=[r.get("speaker") for r in rows],
                    xvectors=[r.get("xvector") for r in rows], instructs=[r.get("instruct") for r in rows])


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    n = Net("small4", tmp_path_factory, 33)
    yield n
    n.m.close()


@pytest.fixture(scope="module", params=("small8", "large4"))
def other(request, tmp_path_factory):
    n = Net(request.param, tmp_path_factory, 5)
    yield n
    n.m.close()


def check_forced(net, idx):
    out = net.m.forced(codes=net.codes[idx], **net.args(idx))
    worst = {}
    for j, i in enumerate(idx):
        for k, ref in net.ref[i].items():
            assert np.isfinite(out[k][j]).all()
            d = rel(out[k][j], ref)
            worst[k] = max(worst.get(k, 0.0), d)
            assert d <= K.MARGIN * K.TWIN[net.name][k], (net.name, len(idx), i, k, d)
    print(net.name, "B", len(idx), {k: "%.2e" % v for k, v in worst.items()})


@pytest.mark.parametrize("B", (1, 15, 16, 17, 33))
def test_forced_logits_against_the_oracle(small, B):
    check_forced(small, list(range(33 - B, 33)) if B < 9 else list(range(B)))
    if B == 1:
        for i in (0, 1, 4, 5, 6, 7, 8):                                  # the shortest texts and every context edge, alone
            check_forced(small, [i])


def test_forced_logits_8_bit_and_projection(other):
    check_forced(other, list(range(5)))


def test_greedy_free_run_against_the_oracle(small):
    idx = list(K.GREEDY_SEEDS)
    got = small.m.generate_codes(sampling=tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=K.GREEDY_T), **small.args(idx))
    second = total = 0
    for j, i in enumerate(idx):
        assert got[j].shape == (16, K.GREEDY_T)
        ref = O.forced_pass(small.rows[i], got[j], small.W, O.F64, T)
        s, t = K.margin_rule(got[j], ref, K.MARGIN * K.TWIN["small4"]["talker"] * np.abs(ref["talker"]).max(),
                             K.MARGIN * K.TWIN["small4"]["cp"] * np.abs(ref["cp"]).max())
        second, total = second + s, total + t
    print("second clause", second, "/", total)
    assert second <= 0.02 * total


def ulp_close(pert, a, b):
    return abs(float(pert[a]) - float(pert[b])) <= 4 * np.spacing(np.float32(max(abs(float(pert[a])), abs(float(pert[b])))))


@pytest.mark.parametrize("temperature", (0.0, 0.9))
def test_device_sampler_equals_host_twin(small, temperature):
    idx = list(range(17))
    a = small.args(idx)
    logits = small.m.forced(codes=small.codes[idx][:, :, :1], want=("talker",), **a)["talker"][:, 0]      # frame 0 depends on no code
    diff = 0
    for seed in (1, 2, 3):
        s = tts.SamplingConfig(temperature=temperature, top_k=50, max_tokens=1, eos_logit_bias=0.25)
        got = small.m.generate_codes(sampling=s, seed=seed, row_index=[100 + i for i in idx], **a)
        forced = small.codes[idx][:, :, :1].copy()
        for j in idx:
            want = tts.sample_host(logits[j], s, talker=True, seed=seed, row_index=100 + j, frame=0, group=0)
            have = int(got[j][0, 0]) if got[j].shape[1] else T["codec_eos"]
            if have != want:
                diff += 1
                pert = O.sample(logits[j], temperature, 50, eos_logit_bias=0.25, seed=seed, row=100 + j, return_perturbed=True)
                assert temperature > 0 and ulp_close(pert, have, want), (seed, j, have, want)
            forced[j, 0, 0] = min(have, 2047)
        # code 1: the code predictor's first logits given the device's code 0
        cp = small.m.forced(codes=forced, want=("cp",), **a)["cp"][:, 0, 0]
        for j in idx:
            if got[j].shape[1] == 0:
                continue
            want = tts.sample_host(cp[j], s, talker=False, seed=seed, row_index=100 + j, frame=0, group=1)
            if int(got[j][1, 0]) != want:
                diff += 1
                pert = O.sample(cp[j], temperature, 50, talker=False, seed=seed, row=100 + j, group=1, return_perturbed=True)
                assert temperature > 0 and ulp_close(pert, int(got[j][1, 0]), want), (seed, j)
    print("picks decided by the last ulp of logf:", diff)


def test_bit_identity(small, tmp_path_factory):
    s = tts.SamplingConfig(max_tokens=12)
    row, fill = [2], list(range(9, 25))
    one = small.m.generate_codes(sampling=s, seed=7, row_index=[55], **small.args(row))[0]
    assert one.shape[0] == 16 and one.shape[1] > 0
    again = small.m.generate_codes(sampling=s, seed=7, row_index=[55], **small.args(row))[0]
    assert np.array_equal(one, again)
    other_seed = small.m.generate_codes(sampling=s, seed=8, row_index=[55], **small.args(row))[0]
    assert other_seed.shape != one.shape or not np.array_equal(one, other_seed)
    first = small.m.generate_codes(sampling=s, seed=7, row_index=[55] + fill, **small.args(row + fill))
    last = small.m.generate_codes(sampling=s, seed=7, row_index=fill + [55], **small.args(fill + row))
    assert len(first) == 17 and np.array_equal(first[0], one) and np.array_equal(last[16], one)
    for mb in (17, 64):
        m = open_model(small.dir, small.g, mb)
        try:
            got = m.generate_codes(sampling=s, seed=7, row_index=fill + [55], **small.args(fill + row))
            assert np.array_equal(got[16], one), mb
        finally:
            m.close()


def test_loop_edges(small):
    a = small.args([3])
    long = small.m.generate_codes(sampling=tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=POLL + 1), **a)[0]
    assert long.shape == (16, POLL + 1)
    for n in (1, POLL - 1, POLL, POLL + 1):                               # the host reads the finished flags every POLL frames
        got = small.m.generate_codes(sampling=tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=n), **a)[0]
        assert got.shape == (16, n) and np.array_equal(got, long[:, :n]), n
    # EOS as the first token
    got = small.m.generate_codes(sampling=tts.SamplingConfig(eos_logit_bias=1e4, max_tokens=5), **small.args([3, 4]))
    assert [g.shape for g in got] == [(16, 0), (16, 0)]
    assert _lib.load().qasr_tts_poll_interval() == POLL


def test_rows_finish_at_different_frames(small):
    idx = list(range(17))
    a = small.args(idx)
    logits = small.m.forced(codes=small.codes[idx][:, :, :1], want=("talker",), **a)["talker"][:, 0]
    bias = float(np.median([(l[:2048].max() - l[T["codec_eos"]]) / 0.9 for l in logits]))      # EOS wins about every other frame
    s = tts.SamplingConfig(eos_logit_bias=bias, max_tokens=POLL + 4)
    ridx = [200 + i for i in idx]
    got = small.m.generate_codes(sampling=s, seed=3, row_index=ridx, **a)
    lens = [g.shape[1] for g in got]
    print("frames per row", lens)
    assert len(set(lens)) >= 2 and min(lens) < POLL + 4                # rows that finish at different frames
    for j in (0, 5, 11, 16, int(np.argmin(lens)), int(np.argmax(lens))):      # finished rows do not disturb the others, nor the others them
        alone = small.m.generate_codes(sampling=s, seed=3, row_index=[ridx[j]], **small.args([j]))[0]
        assert np.array_equal(alone, got[j]), j
    for g in got:
        assert (g[0] != T["codec_eos"]).all() and (g >= 0).all()


def test_synthesize_with_a_reduced_codec(small, tmp_path_factory):
    geo = dict(synth.CODEC_REDUCED, semantic_codebook_size=2048, acoustic_codebook_size=2048)
    d = synth.write_speech_tokenizer_safetensors(synth.synth_speech_tokenizer_state_dict(0, geo), str(tmp_path_factory.mktemp("codec")), geo)
    codec = SpeechTokenizerDecoder.from_pretrained(d)
    try:
        s = tts.SamplingConfig(max_tokens=5)
        audio, codes = small.m.synthesize_batch(codec, sampling=s, seed=4, return_codes=True, **small.args([1, 2]))
        for w, c in zip(audio, codes):
            assert c.shape == (16, 5) and w.shape == (1920 * 5,)
            assert np.array_equal(w, codec.decode(c))
        empty = small.m.synthesize_batch(codec, sampling=tts.SamplingConfig(eos_logit_bias=1e4), **small.args([1]))
        assert empty[0].shape == (0,)
        one = small.m.synthesize(codec, small.rows[1]["text"], small.rows[1]["language"], s, seed=4)
        assert one.shape == (1920 * 5,)
    finally:
        codec.close()


def test_refusals(small):
    ok = small.args([0])
    cases = [
        (dict(texts=[small.rows[0]["text"]] * 34, languages=[2050] * 34), "qasr error 5", "max_batch"),
        (dict(texts=[[1, 2, 3, 4, 5, 6, 7, 8]], languages=[2050]), "qasr error 1", "shorter than the 9 template tokens"),
        (dict(texts=[[1, 2, 3, 4, 5, 6, 7, 8, 512]], languages=[2050]), "qasr error 1", "outside the text vocabulary"),
        (dict(texts=[small.rows[0]["text"]], languages=[3072]), "qasr error 1", "outside the codec vocabulary"),
        (dict(texts=[small.rows[0]["text"]], languages=[2050], instructs=[[600]]), "qasr error 1", "outside the text vocabulary"),
        (dict(texts=[list(range(1, 70))], languages=[2050]), "qasr error 5", "max_text"),
        (dict(ok, sampling=tts.SamplingConfig(top_p=0.9)), "qasr error 7", "top_p"),
    ]
    base = small.m.generate_codes(sampling=tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=3), **ok)[0]
    for kw, code, word in cases:
        with pytest.raises(QasrError) as e:
            small.m.generate_codes(**kw)
        assert code in str(e.value) and word in str(e.value), (str(e.value), word)
        again = small.m.generate_codes(sampling=tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=3), **ok)[0]
        assert np.array_equal(again, base)                                # the handle stays usable
    with pytest.raises(QasrError, match="outside its vocabulary"):
        small.m.forced(codes=np.full((1, 16, 2), 2048, dtype=np.int32), **ok)

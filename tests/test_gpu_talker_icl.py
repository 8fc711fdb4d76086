"""Qwen3-TTS ICL voice cloning on the MI355X (csrc/tts_talker.hip: the ICL plan and the packed prompt pass; csrc/api_tts.cpp: qasr_tts_*_icl,
qasr_tts_clone) over the C ABI, against the float64 oracle tests/talker_icl_oracle.py, with synthetic MLX 4 / 8 bit weights on the reduced
geometries of tests/talker_cases.py and the rows of tests/talker_icl_cases.py.

Tolerances: as in tests/test_gpu_talker.py -- the device and the oracle's torch twin are two realisations of the same rounding points, and
each GPU bound is MARGIN = 4 x the twin's own pinned distance from the oracle (talker_icl_cases.TWIN, measured by
tests/test_talker_icl_cpu.py::test_twin_distance_icl).  The two values of tts_packed_prompt round at different points (the packed pass
multiplies by bf16-rounded weights), so each has its own twin figure.  Prompt rows are one f32 sum rounded once: a plan error (a wrong id,
table or position) moves a row by its whole peak.  The packed positions P - 1 of the rows sit at 12, 63 | 64 | 65 (the prompt attention's
tile), 127 | 128 | 129 and 255 | 256 | 257 (one round of the decode sweep, crossed by the 12 forced frames).
Every test prints the device's distances; DESIGN.md section 19 holds the parity table they fill."""
import ctypes as C

import numpy as np
import pytest

import talker_cases as K
import talker_icl_cases as IC
import talker_icl_oracle as IO
import talker_oracle as O
from qasr import synth, tts, _lib
from qasr.codec import SpeechTokenizerDecoder, SpeechTokenizerEncoder
from qasr.model import QasrError
from qasr.tts_speaker import SpeakerEncoder

pytestmark = pytest.mark.gpu
T = IC.TOKENS
CFG = dict(max_frames=IC.MAX_FRAMES, max_text=IC.MAX_TEXT, max_instruct=8)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def open_model(model_dir, g, max_batch, icl=True):
    cfg = tts.default_config("0.6B", 4, **{k: v for k, v in g.items() if k != "bits"})
    cfg.bits = g["bits"]
    for k in ("tts_pad", "tts_bos", "tts_eos"):
        setattr(cfg, k, T[k])
    kw = dict(max_ref_frames=IC.MAX_REF_FRAMES, max_ref_text=IC.MAX_REF_TEXT) if icl else {}
    return tts.Qwen3TTSModel.from_pretrained(model_dir, cfg, max_batch=max_batch, **CFG, **kw)


def args(rows):
    return dict(texts=[r["text"] for r in rows], languages=[r["language"] for r in rows], xvectors=[r["xvector"] for r in rows],
                ref_texts=[r["ref_text"] for r in rows], ref_codes=[r["ref_codes"] for r in rows])


class Knob:
    """tts_packed_prompt for the length of a with block, restored afterwards."""

    def __init__(self, value):
        self.lib, self.value = _lib.load(strict=True), value

    def __enter__(self):
        v = C.c_int()
        assert self.lib.qasr_get_tuning(b"tts_packed_prompt", C.byref(v)) == 0
        self.old = v.value
        assert self.lib.qasr_set_tuning(b"tts_packed_prompt", int(self.value)) == 0

    def __exit__(self, *exc):
        assert self.lib.qasr_set_tuning(b"tts_packed_prompt", self.old) == 0


class Net:
    def __init__(self, name, tmp, max_batch, n_rows=None):
        self.name, self.g = name, IC.GEOMETRIES[name]
        self.sd = synth.synth_tts_talker_state_dict(self.g, 0)
        self.W = O.Weights(self.sd, self.g)
        self.dir = synth.write_tts_talker_safetensors(self.sd, str(tmp.mktemp(name)))
        self.m = open_model(self.dir, self.g, max_batch)
        self.rows = IC.make_rows(self.g["hidden"], n=n_rows) if name == "small4" else IC.rows_of(name, self.g["hidden"])
        self.codes = IC.forced_codes(len(self.rows))
        self.ref = [IO.forced_pass(r, self.codes[i], self.W, IO.F64, T) for i, r in enumerate(self.rows)]      # computed once, shared


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    n = Net("small4", tmp_path_factory, 17, n_rows=17)
    yield n
    n.m.close()


@pytest.fixture(scope="module", params=("small8", "large4"))
def other(request, tmp_path_factory):
    n = Net(request.param, tmp_path_factory, 3)
    yield n
    n.m.close()


def test_default_knob_and_capacity(small):
    v = C.c_int()
    assert _lib.load().qasr_get_tuning(b"tts_packed_prompt", C.byref(v)) == 0 and v.value in (0, 1)
    assert small.m.icl_capacity == (IC.MAX_REF_FRAMES, IC.MAX_REF_TEXT)
    assert small.m.device_bytes > 0


def test_icl_prompt_against_the_oracle(small):
    got = small.m.icl_prompt(**args(small.rows[:10]))
    worst = 0.0
    for i, rows in enumerate(got):
        ref = small.ref[i]["prompt"]
        assert rows.shape == ref.shape and rows.shape[0] == IC.PACKED_LEN[i] + 1, (i, rows.shape)
        per_row = np.abs(rows.astype(np.float64) - ref).max(axis=1) / np.abs(ref).max()
        worst = max(worst, float(per_row.max()))
        assert per_row.max() <= IC.MARGIN * IC.TWIN["small4"]["prompt"], (i, int(per_row.argmax()), float(per_row.max()))
    print("prompt rows", "%.2e" % worst)


def check_forced(net, idx, packed):
    rows = [net.rows[i] for i in idx]
    with Knob(packed):
        out = net.m.forced_icl(codes=net.codes[idx], **args(rows))
    worst = {}
    for j, i in enumerate(idx):
        for k in ("talker", "cp", "hidden"):
            assert np.isfinite(out[k][j]).all()
            d = rel(out[k][j], net.ref[i][k])
            worst[k] = max(worst.get(k, 0.0), d)
            assert d <= IC.MARGIN * IC.TWIN[net.name][packed][k], (net.name, packed, len(idx), i, k, d)
    print(net.name, "packed", packed, "B", len(idx), {k: "%.2e" % v for k, v in worst.items()})
    return out


@pytest.mark.parametrize("packed", (1, 0))
def test_forced_icl_every_row_alone(small, packed):
    for i in range(10):
        check_forced(small, [i], packed)


@pytest.mark.parametrize("packed", (1, 0))
def test_forced_icl_ragged_and_17_rows(small, packed):
    check_forced(small, list(range(10)), packed)
    check_forced(small, list(range(17)), packed)                           # crosses the frame step's 16-row tile with ICL state


@pytest.mark.parametrize("packed", (1, 0))
def test_forced_icl_8_bit_and_projection(other, packed):
    check_forced(other, [0, 1, 2], packed)


@pytest.mark.parametrize("packed", (1, 0))
@pytest.mark.parametrize("i", (9, 3))                                       # F = 2 below; row 3 moves P - 1 from 65 to 64
def test_boundary_shift(small, packed, i):
    """Run A: reference R[:, :F], forced C.  Run B: reference R[:, :F-1], forced [R[:, F-1] | C[:, :T-1]].  A's frames 0 .. T-2 and B's
    frames 1 .. T-1 are the same function with one position moved from the prompt pass to the frame step: within the sum of both bounds."""
    base = dict(small.rows[i])
    if i == 9:
        base["ref_codes"] = base["ref_codes"][:, :2].copy()
    R, Cd = base["ref_codes"], small.codes[i]
    Tn = Cd.shape[1]
    b_row = dict(base, ref_codes=R[:, :-1].copy())
    b_codes = np.concatenate([R[:, -1:], Cd[:, :Tn - 1]], axis=1)
    with Knob(packed):
        A = small.m.forced_icl(codes=Cd[None], **args([base]))
        B = small.m.forced_icl(codes=b_codes[None], **args([b_row]))
    ref = IO.forced_pass(base, Cd, small.W, IO.F64, T)
    for k in ("talker", "cp", "hidden"):
        a, b = A[k][0][:Tn - 1], B[k][0][1:]
        d = float(np.abs(a.astype(np.float64) - b).max() / np.abs(ref[k][:Tn - 1]).max())
        print("shift row", i, "packed", packed, k, "%.2e" % d)
        assert d <= 2 * IC.MARGIN * IC.TWIN["small4"][packed][k], (i, packed, k, d)


@pytest.mark.parametrize("packed", (1, 0))
def test_greedy_free_run_icl_against_the_oracle(small, packed):
    idx = list(IC.GREEDY_ROWS)
    with Knob(packed):
        got = small.m.generate_codes_icl(sampling=tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=IC.GREEDY_T),
                                         **args([small.rows[i] for i in idx]))
    second = total = 0
    for j, i in enumerate(idx):
        assert got[j].shape == (16, IC.GREEDY_T)
        ref = IO.forced_pass(small.rows[i], got[j], small.W, IO.F64, T)
        s, t = IC.margin_rule(got[j], ref, IC.MARGIN * IC.TWIN["small4"][packed]["talker"] * np.abs(ref["talker"]).max(),
                              IC.MARGIN * IC.TWIN["small4"][packed]["cp"] * np.abs(ref["cp"]).max())
        second, total = second + s, total + t
    print("packed", packed, "second clause", second, "/", total)
    assert second <= 0.02 * total


@pytest.mark.parametrize("packed", (1, 0))
def test_independence_of_rows(small, packed):
    s = tts.SamplingConfig(temperature=0.9, max_tokens=10)
    row, fill = [3], [0, 5, 6, 2]
    pick = lambda idx: args([small.rows[i] for i in idx])
    with Knob(packed):
        one = small.m.generate_codes_icl(sampling=s, seed=7, row_index=[55], **pick(row))[0]
        assert one.shape[0] == 16 and one.shape[1] > 0
        five = small.m.generate_codes_icl(sampling=s, seed=7, row_index=[1, 2, 3, 55, 4], **pick(fill[:3] + row + fill[3:]))
        assert np.array_equal(five[3], one)
        m = open_model(small.dir, small.g, 5)
        try:
            got = m.generate_codes_icl(sampling=s, seed=7, row_index=[1, 55], **pick(fill[:1] + row))
            assert np.array_equal(got[1], one)
        finally:
            m.close()


def test_plain_calls_unchanged_on_an_icl_handle(small):
    rows, codes = K.make_rows(4, small.g["hidden"]), K.forced_codes(4, 8)      # the shortest texts, a speaker token, an x-vector
    a = dict(texts=[r["text"] for r in rows], languages=[r["language"] for r in rows], speakers=[r.get("speaker") for r in rows],
             xvectors=[r.get("xvector") for r in rows])
    plain = open_model(small.dir, small.g, 17, icl=False)
    try:
        assert plain.icl_capacity == (0, 0)
        for s, seed in ((tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=8), 0), (tts.SamplingConfig(max_tokens=8), 5)):
            want = plain.generate_codes(sampling=s, seed=seed, **a)
            got = small.m.generate_codes(sampling=s, seed=seed, **a)
            assert all(np.array_equal(x, y) for x, y in zip(want, got))
        want, got = plain.forced(codes=codes, **a), small.m.forced(codes=codes, **a)
        for k in want:
            assert np.array_equal(want[k], got[k]), k
        with pytest.raises(QasrError) as e:                                 # capacity 0
            plain.generate_codes_icl(**args(small.rows[:1]))
        assert "qasr error 5" in str(e.value) and "row 0" in str(e.value) and "max_ref_frames = 0" in str(e.value)
    finally:
        plain.close()


def test_request_refusals(small):
    ok = [small.rows[0], small.rows[1]]
    greedy = tts.SamplingConfig(temperature=0.0, top_k=1, max_tokens=3)
    base = small.m.generate_codes_icl(sampling=greedy, **args(ok))

    def with_row1(**change):
        return args([ok[0], dict(ok[1], **change)])

    big = ok[1]["ref_codes"].copy()
    big[0, 3] = 3072
    big5 = ok[1]["ref_codes"].copy()
    big5[5, 0] = 2048
    cases = [
        (dict(with_row1(), xvectors=[ok[0]["xvector"], None]), "qasr error 1", "needs an x-vector"),
        (dict(with_row1(), speakers=[None, 3001]), "qasr error 1", "speaker token"),
        (dict(with_row1(), instructs=[None, [5, 6]]), "qasr error 1", "instruct prefix"),
        (with_row1(ref_codes=big), "qasr error 1", "reference code 3072 of stream 0 outside its table"),
        (with_row1(ref_codes=big5), "qasr error 1", "reference code 2048 of stream 5 outside its table"),
        (with_row1(ref_codes=np.zeros((16, IC.MAX_REF_FRAMES + 1), np.int32)), "qasr error 5", "max_ref_frames"),
        (with_row1(ref_text=list(range(4, 4 + IC.MAX_REF_TEXT + 1))), "qasr error 5", "max_ref_text"),
        (with_row1(ref_codes=np.zeros((16, 0), np.int32)), "qasr error 1", "at least 1 reference frame"),
        (with_row1(ref_text=[512]), "qasr error 1", "outside the text vocabulary"),
    ]
    for kw, code, word in cases:
        with pytest.raises(QasrError) as e:
            small.m.generate_codes_icl(**kw)
        assert code in str(e.value) and word in str(e.value) and "row 1" in str(e.value), (str(e.value), word)
        again = small.m.generate_codes_icl(sampling=greedy, **args(ok))
        assert all(np.array_equal(x, y) for x, y in zip(again, base))       # the handle stays usable


def test_clone_is_the_composition_of_the_separate_calls(small, tmp_path_factory):
    geo = dict(synth.CODEC_REDUCED, semantic_codebook_size=2048, acoustic_codebook_size=2048)
    both = synth.merge_speech_tokenizer_state_dicts(synth.synth_speech_tokenizer_state_dict(0, geo),
                                                    synth.synth_speech_tokenizer_encoder_state_dict(0, geo))
    cdir = synth.write_speech_tokenizer_safetensors(both, str(tmp_path_factory.mktemp("codec")), geo)
    H = small.g["hidden"]
    xdir = synth.write_tts_speaker_encoder_safetensors(synth.synth_tts_speaker_encoder_state_dict(0, embedding_dim=H),
                                                       str(tmp_path_factory.mktemp("xvec")))
    bad_dir = synth.write_tts_speaker_encoder_safetensors(synth.synth_tts_speaker_encoder_state_dict(1, embedding_dim=192),
                                                          str(tmp_path_factory.mktemp("xvec192")))
    dec, enc = SpeechTokenizerDecoder.from_pretrained(cdir), SpeechTokenizerEncoder.from_pretrained(cdir, max_samples=1920 * 40)
    spk, bad = SpeakerEncoder.from_pretrained(xdir, max_samples=1920 * 40), SpeakerEncoder.from_pretrained(bad_dir, max_samples=1920 * 40)
    try:
        clips = [synth.synth_waveform(3, 1.0, 24000)[:1920 * 9 + 100].astype(np.float32), synth.synth_waveform(4, 1.0, 24000)[:1920 * 6].astype(np.float32)]
        rows = small.rows[1:3]
        texts, langs, rts = [r["text"] for r in rows], [r["language"] for r in rows], [r["ref_text"] for r in rows]
        s = tts.SamplingConfig(max_tokens=5)
        audio, codes = small.m.clone_batch(dec, enc, spk, texts, langs, clips, rts, sampling=s, seed=4, return_codes=True)
        ref_codes, xv = enc.encode_batch(clips), spk.embed_batch(clips)
        assert [c.shape for c in ref_codes] == [(16, 10), (16, 6)]
        want_audio, want_codes = small.m.synthesize_batch_icl(dec, texts, langs, list(xv), rts, ref_codes, sampling=s, seed=4, return_codes=True)
        for a, b, c, d in zip(audio, want_audio, codes, want_codes):
            assert c.shape == (16, 5) and np.array_equal(c, d) and a.shape == (1920 * 5,) and np.array_equal(a, b)
            assert np.array_equal(a, dec.decode(c))
        with pytest.raises(QasrError) as e:
            small.m.clone_batch(dec, enc, bad, texts, langs, clips, rts, sampling=s)
        assert "qasr error 1" in str(e.value) and "192" in str(e.value)
        # the one-row wrapper adds the chat template itself: its real ids (151644 ...) are outside this reduced text vocabulary
        with pytest.raises(QasrError, match="row 0: text id 151644 outside the text vocabulary"):
            small.m.synthesize_with_voice_clone_icl(dec, enc, spk, rows[0]["text"][3:-5], "english", clips[0], rts[0], s, seed=4)
        one = small.m.clone_batch(dec, enc, spk, texts[:1], langs[:1], clips[:1], rts[:1], sampling=s, seed=4)[0]
        assert np.array_equal(one, audio[0])                                # a row's audio does not depend on the batch
    finally:
        for m in (dec, enc, spk, bad):
            m.close()

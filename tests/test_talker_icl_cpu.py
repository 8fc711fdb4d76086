"""CPU checks of Qwen3-TTS ICL voice cloning: the ICL plan against cases written out by hand from the doc comment of
buildICLPrefillEmbeddings (Qwen3TTS+ICL.swift:149-157), the twin of both values of tts_packed_prompt against the float64 oracle (the
figures the GPU bounds of tests/test_gpu_talker_icl.py derive from), and the refusals of qasr_tts_create_icl that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import talker_icl_cases as IC
import talker_icl_oracle as IO
import talker_oracle as O
from qasr import synth, _lib, tts

T = IC.TOKENS
PAD, BOS, EOS = T["tts_pad"], T["tts_bos"], T["tts_eos"]
CPAD, CBOS, THINK, TBOS, TEOS = T["codec_pad"], T["codec_bos"], T["codec_think"], T["codec_think_bos"], T["codec_think_eos"]
ROLE = [1, 2, 3]
TAIL = [5, 6, 7, 8, 9]
PREFIX = [(1, None), (2, None), (3, None), (PAD, THINK), (PAD, TBOS), (PAD, 2050), (PAD, TEOS), (PAD, "xvec"), (BOS, CPAD)]


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def test_plan_minimal_row():
    plan = IO.icl_plan(ROLE + [40] + TAIL, [], 1, T, 2050)
    assert plan == PREFIX + [(40, CPAD), (EOS, CPAD), (PAD, CBOS), (PAD, ("frame", 0))]
    assert len(plan) == 13 == IO.prompt_length(0, 9, 1)


def test_plan_without_reference_text_and_with_it():
    plan = IO.icl_plan(ROLE + [40, 41] + TAIL, [], 2, T, 2050)
    assert plan == PREFIX + [(40, CPAD), (41, CPAD), (EOS, CPAD), (PAD, CBOS), (PAD, ("frame", 0)), (PAD, ("frame", 1))]
    plan = IO.icl_plan(ROLE + [40, 41] + TAIL, [70, 71, 72], 2, T, 2050)
    assert plan == PREFIX + [(70, CPAD), (71, CPAD), (72, CPAD), (40, CPAD), (41, CPAD), (EOS, CPAD), (PAD, CBOS), (PAD, ("frame", 0)),
                             (PAD, ("frame", 1))]                          # reference text first, then the target


def test_plan_xvector_at_index_4_and_the_dropped_codec_bos():
    plan = IO.icl_plan(ROLE + [40] + TAIL, [70], 3, T, 2061)
    codec = [c for _, c in plan[3:]]
    assert codec[4] == "xvec" and codec[2] == 2061                          # index 4 of the codec prefix
    assert codec[:6] == [THINK, TBOS, 2061, TEOS, "xvec", CPAD]            # the prefix's own trailing codec_bos is dropped ...
    assert codec.count(CBOS) == 1 and plan[-4] == (PAD, CBOS)               # ... the only codec_bos stands in front of the frames
    assert [t for t, _ in plan[3:9]] == [PAD] * 5 + [BOS]


@pytest.mark.parametrize("i", range(len(IC.SHAPES)))
def test_length_formula(i):
    tr, tt, f = IC.SHAPES[i]
    row = IC.make_rows(8)[i]
    plan = IO.icl_plan(row["text"], row["ref_text"], row["ref_codes"].shape[1], T, row["language"])
    assert len(row["ref_text"]) == tr and len(row["text"]) == tt + 8 and row["ref_codes"].shape == (16, f)
    assert len(plan) == 11 + tr + tt + f == IO.prompt_length(tr, tt + 8, f) == IC.PACKED_LEN[i] + 1
    assert 11 + IC.MAX_REF_TEXT + IC.MAX_TEXT + IC.MAX_REF_FRAMES >= len(plan)


def test_frame_rows_are_the_next_input_of_their_codes():
    g = IC.GEOMETRIES["small4"]
    W = O.Weights(synth.synth_tts_talker_state_dict(g, 0), g)
    row = IC.make_rows(g["hidden"])[1]
    pf, pad = IO.icl_embeddings(row, W, IO.F64, T)
    want = O.next_input(pad, row["ref_codes"][:, 7], W, IO.F64)
    assert np.array_equal(pf[-40 + 7].numpy(), want.numpy())
    assert np.array_equal(pf[7].numpy(), (pad + torch.as_tensor(row["xvector"], dtype=torch.float64)).numpy())     # tts_pad + the x-vector


@pytest.fixture(scope="module", params=sorted(IC.GEOMETRIES))
def net(request):
    g = IC.GEOMETRIES[request.param]
    return request.param, g, O.Weights(synth.synth_tts_talker_state_dict(g, 0), g)


def test_twin_distance_icl(net):
    name, g, W = net
    rows = IC.rows_of(name, g["hidden"])
    codes = IC.forced_codes(len(rows))
    worst = {0: {}, 1: {}}
    prompt = 0.0
    for i, row in enumerate(rows):
        a = IO.forced_pass(row, codes[i], W, IO.F64, T)
        for pk in (0, 1):
            b = IO.forced_pass(row, codes[i], W, IO.TWIN, T, packed=bool(pk))
            for k in ("talker", "cp", "hidden"):
                worst[pk][k] = max(worst[pk].get(k, 0.0), rel(b[k], a[k]))
            prompt = max(prompt, rel(b["prompt"], a["prompt"]))
    print(name, "prompt %.2e" % prompt, {pk: {k: "%.2e" % v for k, v in worst[pk].items()} for pk in (0, 1)})
    assert IC.TWIN[name]["prompt"] / 2 <= prompt <= IC.TWIN[name]["prompt"] * 2, (name, prompt)
    for pk in (0, 1):
        for k, v in worst[pk].items():
            assert IC.TWIN[name][pk][k] / 2 <= v <= IC.TWIN[name][pk][k] * 2, (name, pk, k, v)


@pytest.mark.parametrize("packed", (0, 1))
def test_twin_greedy_free_run_icl_within_the_cap(packed):
    g = IC.GEOMETRIES["small4"]
    W = O.Weights(synth.synth_tts_talker_state_dict(g, 0), g)
    rows = IC.make_rows(g["hidden"])
    second = total = 0
    for i in IC.GREEDY_ROWS:
        codes = IO.greedy_run(rows[i], IC.GREEDY_T, W, IO.TWIN, T, packed=bool(packed))
        assert codes.shape == (16, IC.GREEDY_T)
        ref = IO.forced_pass(rows[i], codes, W, IO.F64, T)
        s, t = IC.margin_rule(codes, ref, IC.MARGIN * IC.TWIN["small4"][packed]["talker"] * np.abs(ref["talker"]).max(),
                              IC.MARGIN * IC.TWIN["small4"][packed]["cp"] * np.abs(ref["cp"]).max())
        second, total = second + s, total + t
    print("packed", packed, "second clause", second, "/", total)
    assert second <= 0.02 * total


def test_create_icl_refusals(tmp_path):
    lib = _lib.load(strict=True)
    g = IC.GEOMETRIES["small4"]

    def create(model_dir, frames, text, **over):
        kw = dict(g, **over)
        cfg = tts.default_config("0.6B", 4, **{k: v for k, v in kw.items() if k != "bits"})
        cfg.bits = kw["bits"]
        h = C.c_void_p()
        rc = lib.qasr_tts_create_icl(str(model_dir).encode(), C.byref(cfg), frames, text, C.byref(h))
        assert not h.value
        return rc, lib.qasr_tts_last_error(None).decode()

    for frames, text, over, word in ((0, 0, {}, "max_ref_frames"), (-1, 4, {}, "max_ref_frames"), (8, -1, {}, "max_ref_text"),
                                     (32768, 0, {}, "limit of 32768 positions"), (30000, 3000, {}, "limit of 32768 positions"),
                                     (8, 8, dict(head_dim=64), "head_dim")):
        rc, msg = create(tmp_path, frames, text, **over)
        assert rc == 1 and word in msg and msg.startswith("talker: "), (frames, text, msg)
    rc, msg = create(tmp_path / "missing", 8, 8)                            # a servable geometry: the directory is looked at next
    assert rc == 4 and msg.startswith("talker: ")

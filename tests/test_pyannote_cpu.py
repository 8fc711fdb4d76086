"""CPU checks of the pyannote segmentation / diarization slice: the reference's unit cases (tests/golden/kat_diarization.json) through the
pure-CPU ABI functions, those functions against the f32 restatement in tests/pyannote_oracle.py on random inputs, the float64 oracle
against a second statement in torch (nn.Conv1d, max_pool1d, instance_norm, nn.LSTM), qasr_seg_num_frames, what the GPU tests need of the
synthetic weights, and the loader's error paths (each fails before the device is touched: there is no GPU here, and reaching one would
answer QASR_ERR_HIP).

Measured here (test_f32_distance, printed): max |d| between the float64 oracle and an all-f32 torch run of the same weights and clips is
2.74e-6 on the posteriors (n = 160 000, 16 007 and 1 621); tests/test_gpu_pyannote.py takes its bound from that number."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import pyannote_oracle as O
from qasr import synth
from qasr import diarization as D
from qasr.model import QasrError

KAT = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat_diarization.json")))
FD = np.float32(10.0) / np.float32(589)


@pytest.fixture(scope="module")
def sd():
    return synth.synth_pyannote_state_dict(0)


def _probs(spec):
    p = np.full(spec["n"], spec["base"], np.float32)
    for a, b, v in spec["runs"]:
        p[a:b] = v
    return p


# ---- known answers of the reference's unit tests -------------------------------------------------------------------------------------
def test_kat_configs():
    assert D.default_vad_config() == pytest.approx(KAT["vad_config_default"], rel=1e-7)
    assert D.default_diarization_config() == pytest.approx(KAT["diarization_config_default"], rel=1e-7)


def test_kat_window_positions():
    for c in KAT["window_positions"]:
        pos = D.window_positions(c["n"], c["window"], c["step"])
        assert pos == O.window_positions(c["n"], c["window"], c["step"])
        if "count" in c:
            assert len(pos) == c["count"]
        if "first" in c:
            assert list(pos[0]) == c["first"]
        if "min_count" in c:
            assert len(pos) >= c["min_count"] and pos[0][0] == c["first_start"] and pos[-1][1] == c["last_end"]
            assert all(a >= 0 and b <= c["n"] for a, b in pos)


def test_kat_aggregate_frames():
    for c in KAT["aggregate_frames"]:
        probs = (np.arange(c["frames"], dtype=np.float32) / np.float32(c["ramp_div"]))[None]
        pos = [tuple(p) for p in c["positions"]]
        # VADPipeline() keeps framesPerChunk = 589 for the frame duration: window_duration = 10 * frames / 589 gives that duration here
        wd = float(np.float32(10.0) / np.float32(589) * np.float32(c["frames"]))
        got = D.aggregate_frames(probs, pos, c["n"], 16000, wd)
        assert len(got) >= c["min_count"] and got[0] < c["first_below"]


def test_kat_binarize():
    for c in KAT["binarize"]:
        cfg = KAT["vad_config_default"] if c["cfg"] == "default" else c["cfg"]
        p = _probs(c["probs"])
        got = D.binarize(p, cfg["onset"], cfg["offset"], float(FD), cfg["min_speech_duration"], cfg["min_silence_duration"])
        want = O.filter_durations(O.binarize(p, cfg["onset"], cfg["offset"], FD), cfg["min_speech_duration"], cfg["min_silence_duration"])
        assert len(got) == c["count"] == len(want), c["name"]
        assert np.array_equal(np.array(got, np.float32).ravel(), np.array(want, np.float32).ravel())
        if "start_near" in c:
            assert abs(got[0][0] - c["start_near"][0]) <= c["start_near"][1]
        if "start_above" in c:
            assert got[0][0] > c["start_above"] and got[0][1] < c["end_below"]


def test_kat_speech_probability():
    c = KAT["speech_probability"]
    p = np.random.default_rng(0).uniform(0, 1, (1, c["frames"], c["classes"]))
    p /= p.sum(-1, keepdims=True)
    s = O.speech_probability(p)
    assert s.shape == (1, c["frames"]) and (s >= c["range"][0]).all() and (s <= c["range"][1]).all()
    assert np.allclose(O.speaker_probabilities(p).sum(-1) - (p[..., 4] + p[..., 5] + p[..., 6]), s)


def _segs(rows):
    return [D.DiarizedSegment(*r) for r in rows]


def test_kat_merge_and_compact():
    for c in KAT["merge_segments"]:
        got = D.merge_segments(_segs(c["in"]), c["min_silence"])
        if "out" in c:
            assert [(g.start_time, g.end_time, g.speaker_id) for g in got] == [pytest.approx(tuple(o), abs=1e-3) for o in c["out"]]
        else:
            assert len(got) == c["count"]
        if c.get("sorted"):
            assert all(got[i].start_time >= got[i - 1].start_time for i in range(1, len(got)))
    for c in KAT["compact_speaker_ids"]:
        got = D.compact_speaker_ids(_segs(c["in"]))
        assert [g.speaker_id for g in got] == c["ids"]
        if "times" in c:
            assert [(g.start_time, g.end_time) for g in got] == [pytest.approx(tuple(t), abs=1e-3) for t in c["times"]]


def test_kat_cosine_distance_and_clustering():
    for c in KAT["cosine_distance"]:
        assert D.cosine_distance(c["a"], c["b"]) == pytest.approx(c["want"], abs=1e-3)
    for c in KAT["clustering"]:
        assign, cen = D.cluster([e for _, e in c["items"]], [w for w, _ in c["items"]], c["threshold"])
        assert len(cen) == c["clusters"], c["name"]
        if "assignment" in c:
            assert assign == c["assignment"]
        for a, b in c.get("same", []):
            assert assign[a] == assign[b], c["name"]
        for a, b in c.get("differ", []):
            assert assign[a] != assign[b], c["name"]
        if "centroid0" in c:
            assert cen[0] == pytest.approx(c["centroid0"], abs=1e-3)


# ---- the ABI functions against the f32 restatement on random inputs ----------------------------------------------------------------
def test_random_host_logic_matches_restatement():
    rng = np.random.default_rng(1)
    for trial in range(60):
        n = int(rng.integers(1, 700))
        p = np.clip(np.cumsum(rng.normal(0, 0.12, n)) % 1.0, 0, 1).astype(np.float32)
        on, off = float(rng.uniform(0.4, 0.8)), float(rng.uniform(0.1, 0.4))
        ms, msil = float(rng.uniform(0, 0.3)), float(rng.uniform(0, 0.3))
        a = D.binarize(p, on, off, float(FD))
        b = O.binarize(p, on, off, FD)
        assert np.array_equal(np.array(a, np.float32).ravel(), np.array(b, np.float32).ravel())
        a = D.binarize(p, on, off, float(FD), ms, msil)
        b = O.filter_durations(b, ms, msil)
        assert np.array_equal(np.array(a, np.float32).ravel(), np.array(b, np.float32).ravel())
    for trial in range(40):
        n = int(rng.integers(1, 1200000))
        win, step = int(rng.integers(991, 200000)), int(rng.integers(1000, 100000))
        pos = D.window_positions(n, win, step)
        assert pos == O.window_positions(n, win, step)
    for trial in range(12):
        n = int(rng.integers(100000, 500000))
        pos = O.window_positions(n, 160000, int(rng.choice([16000, 80000, 33333])))
        wp = rng.uniform(0, 1, (len(pos), 589)).astype(np.float32)
        got = D.aggregate_frames(wp, pos, n)
        want = O.aggregate_frames(wp, pos, n, 16000, FD)
        assert np.array_equal(got, want)


def test_random_clustering_matches_restatement():
    rng = np.random.default_rng(2)
    for trial in range(120):
        n, dim = int(rng.integers(1, 14)), int(rng.choice([2, 3, 8, 256]))
        base = rng.standard_normal((3, dim))
        emb = (base[rng.integers(0, 3, n)] + rng.uniform(0, 0.6) * rng.standard_normal((n, dim))).astype(np.float32)
        if trial % 3 == 0 and n > 3:                                   # ties in distance: repeated rows
            emb[n // 2:] = emb[:n - n // 2]
        win = rng.integers(0, max(2, n // 2), n)
        thr = float(rng.uniform(0.05, 1.5))
        a, c = D.cluster(emb, win, thr)
        a2, c2 = O.cluster(list(emb), win, thr)
        assert a == a2 and len(c) == len(c2)
        assert np.array_equal(c, np.array(c2, np.float32).reshape(len(c2), dim))
        i, j = rng.integers(0, n, 2)
        assert np.float32(D.cosine_distance(emb[i], emb[j])) == O.cosine_distance(emb[i], emb[j])
    segs = []
    for trial in range(80):
        m = int(rng.integers(1, 20))
        st = np.sort(rng.uniform(0, 30, m)).astype(np.float32)
        if trial % 2:
            st = np.round(st)                                          # equal start times
        rows = [(float(s), float(np.float32(s) + np.float32(rng.uniform(0.05, 2))), int(rng.choice([0, 2, 5, 9]))) for s in st]
        got = D.merge_segments(_segs(rows), 0.15)
        want = O.merge_segments([(np.float32(a), np.float32(b), k) for a, b, k in rows], 0.15)
        assert [(np.float32(g.start_time), np.float32(g.end_time), g.speaker_id) for g in got] == want
        assert [g.speaker_id for g in D.compact_speaker_ids(_segs(rows))] == [s[2] for s in O.compact_speaker_ids(rows)]


# ---- the oracle against torch ------------------------------------------------------------------------------------------------------
def torch_forward(x, sd, dtype):
    """second statement: channels-first torch modules, LSTM gate blocks are already in torch's i, f, g, o order"""
    t = {k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in sd.items()}
    y = torch.as_tensor(np.asarray(x, np.float64)).to(dtype)[None, None]
    y = Fn.instance_norm(y, weight=t["sincnet.wav_norm.weight"], bias=t["sincnet.wav_norm.bias"], eps=1e-5)
    for i in range(3):
        w = t[f"sincnet.conv.{i}.weight"].permute(0, 2, 1).contiguous()
        conv = torch.nn.Conv1d(w.shape[1], w.shape[0], w.shape[2], stride=10 if i == 0 else 1).to(dtype)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(t[f"sincnet.conv.{i}.bias"])
        y = conv(y)
        if i == 0:
            y = y.abs()
        y = Fn.max_pool1d(y, 3, 3)
        y = Fn.leaky_relu(Fn.instance_norm(y, weight=t[f"sincnet.norm.{i}.weight"], bias=t[f"sincnet.norm.{i}.bias"], eps=1e-5), 0.01)
    y = y.permute(0, 2, 1)
    lstm = torch.nn.LSTM(60, 128, num_layers=4, bidirectional=True, batch_first=True).to(dtype)
    with torch.no_grad():
        for l in range(4):
            for d, suf in (("lstm_fwd", ""), ("lstm_bwd", "_reverse")):
                p = f"{d}.layers.{l}."
                getattr(lstm, f"weight_ih_l{l}{suf}").copy_(t[p + "Wx"])
                getattr(lstm, f"weight_hh_l{l}{suf}").copy_(t[p + "Wh"])
                getattr(lstm, f"bias_ih_l{l}{suf}").copy_(t[p + "bias"])
                getattr(lstm, f"bias_hh_l{l}{suf}").zero_()
    y, _ = lstm(y)
    for l in range(2):
        y = Fn.leaky_relu(Fn.linear(y, t[f"linear.{l}.weight"], t[f"linear.{l}.bias"]), 0.01)
    return torch.softmax(Fn.linear(y, t["classifier.weight"], t["classifier.bias"]), -1)[0].detach().double().numpy()


def _parity_clips():
    return [O.turns_clip(5, 10.0), O.turns_clip(6, 10.0)[:16007], O.turns_clip(7, 10.0)[40000:41621]]


@pytest.fixture(scope="module")
def oracle_post(sd):
    with torch.no_grad():
        return [O.forward(x, sd) for x in _parity_clips()]


def test_oracle_matches_torch_float64(sd, oracle_post):
    with torch.no_grad():
        for x, want in zip(_parity_clips()[:2], oracle_post[:2]):
            got = torch_forward(x, sd, torch.float64)
            assert got.shape == want.shape == (O.num_frames(len(x)), 7)
            assert float(np.abs(got - want).max()) <= 1e-9


def test_f32_distance(sd, oracle_post):
    """The reference's own precision: the distance of an all-f32 run from the float64 oracle (the GPU test's bound is taken from it)."""
    worst = 0.0
    with torch.no_grad():
        for x, want in zip(_parity_clips(), oracle_post):
            worst = max(worst, float(np.abs(torch_forward(x, sd, torch.float32) - want).max()))
    print("f32 torch vs float64 oracle: max |d| %.2e" % worst)
    assert worst < 1e-3


def test_num_frames():
    for n, want in ((990, -1), (991, 1), (2971, 8), (16000, 56), (160000, 589)):
        assert D.num_frames(n) == want == O.num_frames(n), n
    st = KAT["segmentation_frames"]
    assert D.num_frames(st["n"]) == st["frames"] == st["stages"][-1]
    for n in range(985, 1200):
        assert D.num_frames(n) == O.num_frames(n)


def test_synthetic_weights_are_informative(sd, oracle_post):
    """What the GPU tests need of their inputs, on the oracle: every class is the argmax somewhere, every speaker track crosses 0.5 and
    0.3 several times, two local speakers of a window reach 0.5 s of solo frames, and layer 0 holds band-passes."""
    p = oracle_post[0]
    assert (np.bincount(p.argmax(1), minlength=7) >= 5).all()
    sp = O.speaker_probabilities(p)
    for s in range(3):
        for thr in (0.5, 0.3):
            assert np.sum(np.diff((sp[:, s] >= thr).astype(int)) != 0) >= 6
    clips, _ = O.solo_clips(_parity_clips()[0], [(0, 160000)], sp[None])
    assert len(clips) >= 2 and all(len(c) >= 8000 for _, _, c in clips)
    H = np.abs(np.fft.rfft(sd["sincnet.conv.0.weight"][:, :, 0], 2048, axis=1))
    peak = H.argmax(1) * 16000 / 2048
    assert (np.diff(peak) > 0).all() and (H[10:, 0] < 0.05 * H[10:].max(1)).all()


# ---- loader error paths --------------------------------------------------------------------------------------------------------------
def test_loader_errors(sd, tmp_path):
    def create(d):
        return D.SegmentationModel.from_pretrained(str(d))
    with pytest.raises(QasrError, match="qasr error 4.*cannot open"):
        create(tmp_path / "nothing")
    synth.write_pyannote_safetensors(sd, str(tmp_path / "a"), drop=("lstm_bwd.layers.2.Wh",))
    with pytest.raises(QasrError, match="qasr error 4.*missing tensor lstm_bwd.layers.2.Wh"):
        create(tmp_path / "a")
    synth.write_pyannote_safetensors(sd, str(tmp_path / "b"), extra={"sincnet.conv.0.filterbank.low_hz_": np.zeros(40)})
    with pytest.raises(QasrError, match="qasr error 1.*unknown tensor sincnet.conv.0.filterbank.low_hz_"):
        create(tmp_path / "b")
    synth.write_pyannote_safetensors(sd, str(tmp_path / "c"), reshape={"sincnet.conv.1.weight": (60, 80, 5)})
    with pytest.raises(QasrError, match="qasr error 1.*sincnet.conv.1.weight has shape"):
        create(tmp_path / "c")
    synth.write_pyannote_safetensors(sd, str(tmp_path / "d"), dtype="F64")
    with pytest.raises(QasrError, match="qasr error 1.*dtype F64"):
        create(tmp_path / "d")
    # optional keys (conv biases, norm weights and biases) are accepted: the load goes on to the device, which is absent here
    synth.write_pyannote_safetensors(sd, str(tmp_path / "e"), drop=("sincnet.conv.0.bias", "sincnet.norm.1.weight", "sincnet.wav_norm.bias"))
    if not torch.cuda.is_available():
        with pytest.raises(QasrError, match="qasr error 2"):
            create(tmp_path / "e")

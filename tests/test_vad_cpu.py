"""CPU checks of the Silero VAD: the reference's unit cases (reflection pad, sileroDefault, binarize), the float64 oracle against a second
statement in torch (nn.Conv1d / nn.LSTMCell), qasr_vad_binarize against the Python restatement, the loader's error paths (no HIP call is
reached: each one fails before the device is touched), and the StreamingASR wiring of a whole-buffer VAD with stand-ins."""
import ctypes as C
import numpy as np
import pytest
import torch

import silero_oracle as O
from qasr import _lib, synth
from qasr import streaming as S
from qasr.model import QasrError
from qasr.vad import SileroVADModel, VADPipeline, binarize
from test_streaming_cpu import FakeASR, _ramp

f32 = np.float32


def test_silero_default_config():
    """VADConfig.sileroDefault (Configuration.swift:84-91; SileroVADTests.swift:11-16)."""
    c = _lib.QasrVadConfig()
    assert _lib.load().qasr_vad_default_config(C.byref(c)) == 0
    assert (c.onset, c.offset, c.min_speech_duration, c.min_silence_duration) == (f32(0.5), f32(0.35), f32(0.25), f32(0.1))
    d = S.VADConfig()
    assert (d.onset, d.offset, d.min_speech_duration, d.min_silence_duration) == (0.5, 0.35, 0.25, 0.1)


def test_reflection_pad_right():
    """reflectionPadRight (SileroModel.swift): [a, b, c, d, e] with padding 2 -> [a, b, c, d, e, d, c]; the network's case appends
    indices T-2 ... T-65 of the 576 samples."""
    assert O.reflection_pad_right(np.array([1., 2, 3, 4, 5]), 2).tolist() == [1, 2, 3, 4, 5, 4, 3]
    x = np.arange(576.0)
    y = O.reflection_pad_right(x, 64)
    assert y.shape == (640,) and y[576:].tolist() == list(range(574, 510, -1))
    assert O.reflection_pad_right(np.arange(3.0), 5).tolist() == [0, 1, 2]          # guard T > padding


def _abi_binarize(probs, cfg=None):
    lib = _lib.load()
    p = np.ascontiguousarray(probs, dtype=np.float32)
    c = None
    if cfg is not None:
        c = _lib.QasrVadConfig(*cfg)
    seg = np.zeros((len(p) + 1, 2), dtype=np.float32)
    n = lib.qasr_vad_binarize(p.ctypes.data_as(C.POINTER(C.c_float)), len(p), C.byref(c) if c else None,
                              seg.ctypes.data_as(C.POINTER(C.c_float)), len(p) + 1)
    assert n >= 0
    return [(float(a), float(b)) for a, b in seg[:n]]


PYANNOTE = (0.767, 0.377, 0.136, 0.067)          # VADConfig.default, what the reference's binarize tests construct


def test_binarize_reference_cases():
    """SpeechVADTests.swift:80-190 (segment counts and rough positions; the frame duration here is detectSpeech's 0.032 s)."""
    assert _abi_binarize([0.1] * 293, PYANNOTE) == []
    s = _abi_binarize([0.9] * 293, PYANNOTE)
    assert len(s) == 1 and s[0][0] == 0.0
    p = [0.1] * 293
    p[50:200] = [0.9] * 150
    s = _abi_binarize(p, PYANNOTE)
    assert len(s) == 1 and s[0][0] > 0.5 and s[0][1] < 8.0
    p = [0.5] * 293
    p[20:50] = [0.9] * 30
    p[55:100] = [0.9] * 45
    p[100:120] = [0.1] * 20
    assert len(_abi_binarize(p, PYANNOTE)) == 1                              # the dip stays above offset
    p = [0.1] * 293
    p[50:53] = [0.9] * 3
    assert _abi_binarize(p, (0.5, 0.3, 1.0, 0.5)) == []                      # shorter than minSpeechDuration
    p = [0.1] * 293
    p[20:80] = [0.9] * 60
    p[85:150] = [0.9] * 65
    assert len(_abi_binarize(p, (0.5, 0.3, 0.0, 2.0))) == 1                  # gap shorter than minSilenceDuration: merged
    assert _abi_binarize([]) == []


def test_binarize_matches_restatement():
    """qasr_vad_binarize == the Python restatement of binarize + filterDurations on 200 random sequences, lengths included whose f32
    frame duration (n * 0.032) / n is not 0.032f."""
    rng = np.random.default_rng(0)
    c = f32(512) / f32(16000)
    odd_lengths = [n for n in range(1, 70000) if (f32(n) * c) / f32(n) != c]          # 4027, 4073, 8021, ...
    odd = 0
    for trial in range(200):
        n = int(rng.choice(odd_lengths)) if trial % 4 == 0 else int(rng.integers(1, 900))
        frame = (f32(n) * (f32(512) / f32(16000))) / f32(n)
        odd += frame != f32(0.032)
        levels = rng.choice([0.05, 0.3, 0.4, 0.5, 0.6, 0.95], size=n // 5 + 1)
        probs = np.repeat(levels, 5)[:n].astype(np.float32) + (0.01 * rng.standard_normal(n)).astype(np.float32)
        cfg = (0.5, 0.35, 0.25, 0.1) if trial % 2 else (float(rng.uniform(0.4, 0.7)), float(rng.uniform(0.2, 0.4)),
                                                         float(rng.uniform(0.0, 0.5)), float(rng.uniform(0.0, 0.3)))
        want = O.binarize(probs, *cfg)
        assert _abi_binarize(probs, cfg) == want, trial
        assert [tuple(s) for s in VADPipeline(S.VADConfig(*cfg)).binarize(probs)] == want
    assert odd > 10
    assert binarize(np.full(10, 0.9, np.float32)) == [S.SpeechSegment(0.0, float(f32(10) * ((f32(10) * f32(0.032)) / f32(10))))]


class TorchSilero(torch.nn.Module):
    """Second statement of the network in torch (channels-first Conv1d, LSTMCell), float64, built from the reference layouts."""

    def __init__(self, sd):
        super().__init__()
        t = {k: torch.tensor(np.asarray(v, dtype=np.float64)) for k, v in sd.items()}
        self.stft = torch.nn.Conv1d(1, 258, 256, stride=128, bias=False).double()
        self.stft.weight.data = t["stft.weight"].permute(0, 2, 1).contiguous()                    # [258, 256, 1] -> [258, 1, 256]
        self.enc = torch.nn.ModuleList()
        for i, (ci, co, s) in enumerate([(129, 128, 1), (128, 64, 2), (64, 64, 2), (64, 128, 1)]):
            c = torch.nn.Conv1d(ci, co, 3, stride=s, padding=1).double()
            c.weight.data = t[f"encoder.{i}.weight"].permute(0, 2, 1).contiguous()               # [out, k, in] -> [out, in, k]
            c.bias.data = t[f"encoder.{i}.bias"]
            self.enc.append(c)
        self.cell = torch.nn.LSTMCell(128, 128).double()                                          # gate order i, f, g, o
        self.cell.weight_ih.data, self.cell.weight_hh.data = t["lstm.Wx"], t["lstm.Wh"]
        self.cell.bias_ih.data, self.cell.bias_hh.data = t["lstm.bias"], torch.zeros(512, dtype=torch.float64)
        self.dec = torch.nn.Conv1d(128, 1, 1).double()
        self.dec.weight.data = t["decoder.weight"].permute(0, 2, 1).contiguous()
        self.dec.bias.data = t["decoder.bias"]

    def forward(self, x576, h, c):
        x = torch.nn.functional.pad(x576[:, None], (0, 64), mode="reflect")
        s = self.stft(x)
        m = torch.sqrt(s[:, :129] ** 2 + s[:, 129:] ** 2)
        for conv in self.enc:
            m = torch.relu(conv(m))
        h, c = self.cell(m[:, :, 0], (h, c))
        return torch.sigmoid(self.dec(torch.relu(h)[:, :, None]))[:, 0, 0], h, c


def test_oracle_second_statement():
    """The float64 oracle == the torch statement over 100 chunks of one stream (probabilities within 1e-6; pins the [out, k, in] layout,
    the gate order and the padding rule)."""
    sd = synth.synth_silero_state_dict(1)
    W, net = O.Weights(sd), TorchSilero(sd)
    rng = np.random.default_rng(3)
    amp = np.repeat(rng.choice([0.0, 0.002, 0.01, 0.1], size=20), 2560)
    pcm = (amp * rng.standard_normal(amp.shape[0])).astype(np.float32)
    want, st = O.probs_rows(W, [pcm])
    x576, _ = O.chunk_inputs(pcm)
    h = c = torch.zeros(1, 128, dtype=torch.float64)
    got = []
    with torch.no_grad():
        for k in range(100):
            p, h, c = net(torch.tensor(x576[k:k + 1], dtype=torch.float64), h, c)
            got.append(float(p[0]))
    assert np.abs(np.array(got) - want[0]).max() <= 1e-6
    assert np.abs(h[0].numpy() - st[0][0]).max() <= 1e-6
    assert 0.05 < min(got) and max(got) < 0.99 and np.ptp(got) > 0.3                # graded, not saturated
    s = O.Stream(W)                                                                  # processChunk form == buffer form
    assert np.allclose([s.process_chunk(x576[k, 64:]) for k in range(100)], want[0], rtol=0, atol=1e-12)


def _create(d):
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.qasr_vad_create(0, str(d).encode(), 4, None, C.byref(h))
    return rc, lib.qasr_vad_last_error(None).decode()


def test_create_errors_name_the_key(tmp_path):
    """Missing directory / file / key -> QASR_ERR_IO, wrong shape or dtype -> QASR_ERR_INVALID, the key named (whole messages, as the
    loader worded them before it was shared with the speaker model); every check runs before the first HIP call (there is no GPU here:
    reaching one would answer QASR_ERR_HIP)."""
    rc, msg = _create(tmp_path / "nope")
    assert rc == 4 and msg == f"silero vad: cannot open {tmp_path / 'nope'}/model.safetensors"
    sd = synth.synth_silero_state_dict(0)
    synth.write_silero_safetensors(sd, str(tmp_path / "a"), drop=("lstm.Wh",))
    rc, msg = _create(tmp_path / "a")
    assert rc == 4 and msg == "silero vad: missing tensor lstm.Wh"
    synth.write_silero_safetensors(sd, str(tmp_path / "b"), reshape={"encoder.2.weight": (64, 64, 3)})
    rc, msg = _create(tmp_path / "b")
    assert rc == 1 and msg == "silero vad: tensor encoder.2.weight has shape [64, 64, 3], expected [64, 3, 64]"
    synth.write_silero_safetensors(sd, str(tmp_path / "d"), dtype="F64")
    rc, msg = _create(tmp_path / "d")
    assert rc == 1 and msg == "silero vad: tensor stft.weight has dtype F64 (F32 / F16 / BF16)"
    with pytest.raises(QasrError, match="stft.weight"):
        synth.write_silero_safetensors(sd, str(tmp_path / "c"), drop=("stft.weight",))
        SileroVADModel.from_pretrained(str(tmp_path / "c"))
    lib = _lib.load()
    assert lib.qasr_vad_create(0, str(tmp_path / "a").encode(), 0, None, C.byref(C.c_void_p())) == 1      # max_streams
    assert lib.qasr_vad_detect_speech(None, None, 0, 16000, None, None, 0) == -1


def test_synth_weights_and_writer(tmp_path):
    """Hann-windowed DFT basis in stft.weight; the writer round-trips f32 / f16 / bf16 headers in the reference's keys and shapes."""
    import json
    sd = synth.synth_silero_state_dict(0)
    for k, shape in synth.SILERO_SHAPES.items():
        assert sd[k].shape == shape and sd[k].dtype == np.float32
    x = np.cos(2 * np.pi * 10 * np.arange(256) / 256)
    mag = np.hypot(sd["stft.weight"][:129, :, 0] @ x, sd["stft.weight"][129:, :, 0] @ x)
    assert mag.argmax() == 10
    for dt in ("F32", "F16", "BF16"):
        p = synth.write_silero_safetensors(sd, str(tmp_path / dt), dtype=dt)
        raw = open(p, "rb").read()
        hdr = json.loads(raw[8:8 + int.from_bytes(raw[:8], "little")])
        assert sorted(hdr) == sorted(sd) and all(hdr[k]["dtype"] == dt and tuple(hdr[k]["shape"]) == sd[k].shape for k in sd)


class ChunkVAD:
    """A whole-buffer VAD stand-in with the SileroVADModel surface: probability from the chunk's first sample (the ramp audio)."""
    max_streams = 3

    @staticmethod
    def f(chunk):
        return 0.9 if (int(chunk[0]) // 512) % 23 < 14 and chunk[0] != 0 else 0.05

    def process_chunk(self, chunk):
        return self.f(chunk)

    def reset_state(self):
        pass

    def probs(self, bufs, stream_ids=None):
        out = []
        for b in bufs:
            nc = -(-len(b) // 512)
            pad = np.zeros(nc * 512, np.float32)
            pad[:len(b)] = b
            out.append(np.array([self.f(pad[i * 512:(i + 1) * 512]) for i in range(nc)], np.float32))
        return out


def test_streams_batched_wiring():
    """with_vad: transcribe_stream, transcribe_stream_batched and transcribe_streams_batched give the same segments (probabilities from
    one whole-buffer call replayed through the walk); many buffers == buffer by buffer."""
    cfg = S.StreamingASRConfig(max_segment_duration=1.5)
    audios = [_ramp(s) + 1 for s in (2.3, 4.1, 0.7, 3.3)]
    st = S.StreamingASR.with_vad(FakeASR(), ChunkVAD())
    seqs = [list(st.transcribe_stream(a, config=cfg)) for a in audios]
    assert sum(len(s) for s in seqs) >= 5
    assert [st.transcribe_stream_batched(a, config=cfg) for a in audios] == seqs
    assert st.transcribe_streams_batched(audios, config=cfg) == seqs
    assert st.transcribe_streams_batched([], config=cfg) == []
    with pytest.raises(ValueError):
        S.StreamingASR(FakeASR(), ChunkVAD.f).transcribe_streams_batched(audios)

"""The CosyVoice3 speech tokenizer and voice profiles on the MI355X (csrc/s3tok_cosyvoice.hip, csrc/api_s3tok.cpp) over the C ABI, against
the float64 oracle tests/s3tok_oracle.py, with synthetic weights (qasr.synth) on the model's widths: the token-count sweep at 2 blocks,
one clip at 12.

Tolerances.  The device runs its GEMMs on bf16 operands; tests/test_s3tok_cpu.py measures, on these very inputs, how far that precision
plan alone (the oracle's twin) lies from float64, as max |d| / peak, and tests/s3tok_cases.py holds the figures.  A device result must
lie within MARGIN = 4 x its case's figure (DESIGN.md sections 18 and 24); the two mels are bounded the same way by their float32 twins.
The FSQ is pinned exactly: encode's codes are fsq_host of the device's own projections.  Against the oracle the codes are compared digit
by digit where the oracle's projection lies farther from a level boundary than MARGIN x the twin's max |d| (a *decided* digit); through
the exact pin, the device's codes of a mel are fsq_host of its projections.  Batching, passes and the profile are pinned bit for bit.
Every test prints S3TOK_PARITY lines; DESIGN.md section 24 holds the table they fill."""
import numpy as np
import pytest

import cvlm_cases as K
import s3tok_cases as SC
import s3tok_oracle as O
from qasr import _lib, cosyvoice as cv, s3tok, synth
from qasr.flow import CosyVoiceFlow
from qasr.model import QasrError
from qasr.s3tok import SpeechTokenizer
from qasr.vocoder import HiFTVocoder

pytestmark = pytest.mark.gpu


def report(case, twin, got):
    print(f"S3TOK_PARITY {case}: twin {twin:.2e} bound {SC.MARGIN * twin:.2e} device {got:.2e}")
    assert got <= SC.MARGIN * twin, (case, got, SC.MARGIN * twin)


@pytest.fixture(scope="module")
def dir2(tmp_path_factory):
    return synth.write_cosyvoice_s3tok_safetensors(SC.state_dict(2), str(tmp_path_factory.mktemp("s3tok2")))


@pytest.fixture(scope="module")
def tok(dir2):
    m = SpeechTokenizer.from_pretrained(dir2, max_tokens=512)
    yield m
    m.close()


# ---- 1. the two mels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SC.whisper_samples())
def test_whisper_mel(tok, n):
    x = SC.pcm(n, n)
    got = tok.whisper_mel(x)
    assert got.shape == (128, n // 160) and np.isfinite(got).all()
    report(f"whisper_mel n={n}", SC.TWIN_WHISPER[n], SC.rel(got, O.whisper_mel(x)))


@pytest.mark.parametrize("n", SC.FLOW_SAMPLES)
def test_flow_mel(tok, n):
    x = SC.pcm(n, n, 24000)
    got = tok.flow_mel(x)
    assert got.shape == (80, n // 480) and np.isfinite(got).all()
    report(f"flow_mel n={n}", SC.TWIN_FLOW[n], SC.rel(got, O.flow_mel(x)))


# ---- 2. hidden state and projections ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", SC.token_cases())
def test_hidden_and_project(tok, n, T):
    mel = SC.mel_input(n, T)
    h64, p64 = SC.reference(2, n, T)
    h, p = tok.hidden(mel), tok.project(mel)
    assert h.shape == (n, 1280) and p.shape == (n, 8) and np.isfinite(h).all() and np.isfinite(p).all()
    report(f"hidden tokens={n}", SC.TWIN_HIDDEN[n], SC.rel(h, h64))
    report(f"project tokens={n}", SC.TWIN_PROJ[n], SC.rel(p, p64))


def test_depth12(tmp_path):
    d = synth.write_cosyvoice_s3tok_safetensors(SC.state_dict(12), str(tmp_path / "s3tok12"), dtype="BF16")
    m = SpeechTokenizer.from_pretrained(d, max_tokens=128)
    try:
        assert m.depth == 12 and m.memory_footprint == 2 * sum(v.size for v in SC.state_dict(12).values())
        T = SC.mel_frames(SC.FULL_TOKENS, 0)
        mel = SC.mel_input(SC.FULL_TOKENS, T)
        h64, p64 = SC.reference(12, SC.FULL_TOKENS, T)
        h, p = m.hidden(mel), m.project(mel)
        report("hidden depth 12", SC.TWIN_HIDDEN_FULL, SC.rel(h, h64))
        report("project depth 12", SC.TWIN_PROJ_FULL, SC.rel(p, p64))
        x = SC.pcm(1, 160 * T)                                                # check 3 on this geometry
        assert np.array_equal(m.encode(x), s3tok.fsq_host(m.project(m.whisper_mel(x))))
    finally:
        m.close()


# ---- 3. the FSQ, exactly ---------------------------------------------------------------------------------------------------------------
def near_half(proj):
    """Digits whose scaled tanh lies within 4 ulp of +-0.5: the only ones a device tanh one ulp off the host's could move."""
    h = np.tanh(proj.astype(np.float64)) * O.FSQ_SCALE
    return np.abs(np.abs(h) - 0.5) <= 4 * 2.0 ** -24


def test_fsq_exact(tok):
    exempt = total = 0
    for n in SC.whisper_samples():
        x = SC.pcm(n, n)
        proj = tok.project(tok.whisper_mel(x))
        codes = tok.encode(x)
        assert codes.dtype == np.int32 and codes.min() >= 0 and codes.max() < 6561
        mask = near_half(proj)
        exempt += int(mask.sum())
        total += mask.size
        assert np.array_equal(O.digits_of(codes)[~mask], O.digits_of(s3tok.fsq_host(proj))[~mask]), n
    print(f"S3TOK_PARITY fsq: {total} digits, {exempt} within 4 ulp of a boundary")
    assert exempt == 0


# ---- 4. codes against the oracle, digit by digit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [c for c in SC.token_cases() if c[0] >= 15])
def test_codes_against_oracle(tok, n, T):
    _, p64 = SC.reference(2, n, T)
    want = O.fsq_digits(p64)
    got = O.digits_of(s3tok.fsq_host(tok.project(SC.mel_input(n, T))))
    und = SC.undecided(p64, SC.MARGIN * SC.TWIN_PROJ_ABS[n])
    share, moved = float(und.mean()), float((got != want).mean())
    print(f"S3TOK_PARITY codes tokens={n}: undecided {share:.3f}, digits off the oracle's {moved:.4f}")
    assert share <= SC.UNDECIDED_MAX
    assert np.array_equal(got[~und], want[~und])
    side = 1 + np.sign(p64).astype(np.int64)                                   # the two levels next to that boundary: the middle one and its side's
    assert ((got == 1) | (got == side))[und].all()


# ---- 5. a clip is the same bits alone, anywhere in a batch and under any max_tokens --------------------------------------------------------
def test_ragged_batch(tok, dir2):
    clips = SC.batch_pcm()
    alone = [tok.encode(x) for x in clips]
    assert [a.size for a in alone] == list(SC.BATCH_TOKENS)
    small = SpeechTokenizer.from_pretrained(dir2, max_tokens=SC.THREE_PASSES)
    try:
        for m in (tok, small):
            for order in (range(5), (4, 3, 2, 1, 0), (1, 0, 3)):
                got = m.encode_batch([clips[i] for i in order])
                assert all(np.array_equal(g, alone[i]) for g, i in zip(got, order)), order
        x = clips[3]
        mel = tok.whisper_mel(x)
        assert np.array_equal(small.whisper_mel(x), mel)
        assert np.array_equal(small.hidden(mel), tok.hidden(mel)) and np.array_equal(small.project(mel), tok.project(mel))
        x24 = SC.pcm(9, 31337, 24000)
        assert np.array_equal(small.flow_mel(x24), tok.flow_mel(x24))
        profs = tok.profile_batch([clips[3], clips[0], clips[4]], [16000] * 3)
        for p, i in zip(profs, (3, 0, 4)):
            q = small.profile(clips[i], 16000)
            assert np.array_equal(p.tokens, q.tokens) and np.array_equal(p.prompt_feat, q.prompt_feat)
    finally:
        small.close()


# ---- 6. the profile ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,n", [(16000, 16160), (44100, 30001), (24000, 24000)])
def test_profile(tok, sr, n):
    lib = _lib.load(strict=True)
    x = SC.pcm(sr, n, sr)
    p = tok.profile(x, sr, spk_emb=np.ones(192), prompt_text_ids=[1, 2])
    x16, x24 = s3tok.resample(x, sr, 16000), s3tok.resample(x, sr, 24000)
    nt, nf = s3tok.tokens_of(s3tok.whisper_frames(x16.size)), s3tok.flow_frames(x24.size)
    L = min(nt, nf // 2)
    assert (p.uncut_tokens, p.uncut_frames) == (nt, nf) and p.tokens.size == L and p.prompt_feat.shape == (80, 2 * L)
    if sr == 16000:
        assert (nt, nf, L) == (26, 50, 25)                                      # 1.01 s: the uncut lengths disagree
    assert np.array_equal(p.tokens, tok.encode(x16)[:L]) and np.array_equal(p.prompt_feat, tok.flow_mel(x24)[:, :2 * L])
    assert p.spk_emb.shape == (192,) and p.prompt_text_ids == [1, 2]
    new = np.zeros(3, dtype=np.int32)
    assert lib.qasr_flow_check_clip(new.ctypes.data_as(s3tok._I), 3, p.tokens.ctypes.data_as(s3tok._I), L, p.prompt_feat.shape[1], 6561, 0) == 0


# ---- 7. end to end: a reference clip and text ids in, cloned audio out ----------------------------------------------------------------------
def test_synthesize_with_profile(tok, tmp_path_factory):
    """At the 2-layer LLM (real4: the geometry of test_gpu_cvlm.py whose speech vocabulary holds all 6561 codes) and the depth-2 flow."""
    g = K.GEOMETRIES["real4"]
    llm = cv.CosyVoiceLLM.from_pretrained(synth.write_cosyvoice_llm_safetensors(synth.synth_cosyvoice_llm_state_dict(g, 0), str(tmp_path_factory.mktemp("llm"))),
                                          **{**g, "max_text": K.MAX_TEXT, "max_prompt_tokens": K.MAX_PROMPT, "max_tokens": K.MAX_TOKENS, "max_batch": 2})
    flow = CosyVoiceFlow.from_pretrained(synth.write_cosyvoice_flow_safetensors(synth.synth_cosyvoice_flow_state_dict(0, depth=2),
                                                                                str(tmp_path_factory.mktemp("flow2"))), max_frames=512)
    voc = HiFTVocoder.from_pretrained(synth.write_cosyvoice_hifigan_safetensors(synth.synth_cosyvoice_hifigan_state_dict(0),
                                                                                str(tmp_path_factory.mktemp("hift"))), max_frames=512)
    try:
        p = tok.profile(SC.pcm(77, 44100 * 8 // 10, 44100), 44100, spk_emb=np.random.default_rng(3).standard_normal(192), prompt_text_ids=[5, 6, 7])
        assert 0 < p.tokens.size <= K.MAX_PROMPT
        tts = cv.CosyVoiceTTS(llm, flow, voc)
        s = cv.CosySamplingConfig(min_ratio=1000.0)
        content = [11, 12, 13, 14]
        wav, toks = tts.synthesize_with_profile(content, p, max_tokens=9, sampling=s, seed=4, return_tokens=True, end_of_prompt=1000)
        by_hand = tts.synthesize([[5, 6, 7, 1000] + content], content_len=[4], prompts=[p.tokens], prompt_feat=[p.prompt_feat], spk_emb=[p.spk_emb],
                                 max_tokens=[9], sampling=s, seed=4)[0]
        assert toks.size == 9 and wav.size == 480 * 2 * 9 + 16                    # the prompt's 480 x prompt_frames samples are dropped
        assert np.array_equal(wav, by_hand) and np.isfinite(wav).all() and np.abs(wav).max() > 0
    finally:
        for m in (llm, flow, voc):
            m.close()


# ---- 8. refusals on a live handle ------------------------------------------------------------------------------------------------------------
def test_refusals(dir2):
    lib = _lib.load(strict=True)
    m = SpeechTokenizer.from_pretrained(dir2, max_tokens=16)
    try:
        assert m.max_tokens == 16 and m.depth == 2 and m.is_loaded and m.memory_footprint == 4 * sum(v.size for v in SC.state_dict(2).values())
        with pytest.raises(QasrError, match="qasr error 1: .*empty"):
            m.encode(np.zeros(159, dtype=np.float32))
        with pytest.raises(QasrError, match="qasr error 1: .*empty"):
            m.flow_mel(np.zeros(479, dtype=np.float32))
        with pytest.raises(QasrError, match="qasr error 1: .*empty"):
            m.profile(np.zeros(100, dtype=np.float32), 16000)
        with pytest.raises(QasrError, match="qasr error 1: .*17 tokens, more than max_tokens = 16"):
            m.encode(SC.pcm(0, 160 * 4 * 17))
        with pytest.raises(QasrError, match="qasr error 1: .*more than max_tokens = 16"):
            m.profile(SC.pcm(0, 160 * 4 * 17), 16000)                            # refused, not cut
        x = SC.pcm(0, 1600)
        assert lib.qasr_s3tok_encode(m.h, x.ctypes.data_as(s3tok._F), x.size, None) == 1 and "null" in lib.qasr_s3tok_last_error(m.h).decode()
        assert lib.qasr_s3tok_whisper_mel(m.h, x.ctypes.data_as(s3tok._F), x.size, None) == 1
        assert m.encode(x).size == 3                                             # the handle still serves
        assert all(v >= 0 for v in m.timing().values())
        m.unload()
        assert not m.is_loaded and m.memory_footprint == 0
        with pytest.raises(QasrError, match="qasr error 3"):
            m.encode(x)
        with pytest.raises(QasrError, match="qasr error 3"):
            m.flow_mel(np.zeros(479, dtype=np.float32))                          # NOT_LOADED before every other refusal
        assert lib.qasr_s3tok_encode(m.h, None, 0, None) == 3
    finally:
        m.close()

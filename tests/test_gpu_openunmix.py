"""Open-Unmix source separation on the MI355X (csrc/sep_openunmix.hip, csrc/api_sep.cpp) over the C ABI, against the float64 oracle
tests/openunmix_oracle.py.

Tolerances: the reference's own precision is f32.  tests/test_openunmix_cpu.py::test_f32_distance measures, per stage, the max |d|
between the oracle and its f32 twin on these clips and weights, normalised by the stage output's peak:
    stft 6.26e-08, masks 9.30e-07 (T = 9) and 9.40e-07 (T = 305), wiener 3.02e-04, istft 1.96e-07, whole path 1.56e-06.
Each bound is 10 x that figure (another f32 summation order through 3 x T recurrent steps), with a floor of
1e-6 of peak for the STFT and a ceiling of 1e-3 of peak for the Wiener stage, the tolerance the reference allows between its own two
Wiener implementations.  The device's measured distances are printed by every test and recorded in DESIGN.md section 14."""
import ctypes as C

import numpy as np
import pytest

import openunmix_oracle as O
from qasr import synth, _lib
from qasr.model import QasrError
from qasr.separation import SourceSeparator, TARGETS

pytestmark = pytest.mark.gpu

F32 = {"stft": 6.26e-08, "masks": 9.30e-07, "masks_long": 9.40e-07, "wiener": 3.02e-04, "istft": 1.96e-07, "separate": 1.56e-06}
TOL_STFT = max(10 * F32["stft"], 1e-6)
TOL_MASKS, TOL_LONG = 10 * F32["masks"], 10 * F32["masks_long"]
TOL_WIENER = min(10 * F32["wiener"], 1e-3)
TOL_ISTFT, TOL_SEP = 10 * F32["istft"], 10 * F32["separate"]
N_MAIN, N_LONG = 8 * 1024 + 37, 304 * 1024 + 11        # T = 9, T = 305


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def sds():
    return synth.synth_openunmix_state_dict(0, 512)


@pytest.fixture(scope="module")
def model_dir(sds, tmp_path_factory):
    return synth.write_openunmix_safetensors(sds, str(tmp_path_factory.mktemp("umxhq")))


@pytest.fixture(scope="module")
def sep(model_dir):
    m = SourceSeparator.from_pretrained(model_dir)
    yield m
    m.close()


@pytest.fixture(scope="module")
def main(sds):
    """The T = 9 clip and its float64 stages, computed once and shared."""
    x = O.clip(0, N_MAIN)
    re, im, mag = O.stft(x.astype(np.float64))
    return dict(x=x, re=re, im=im, mag=mag, masked=np.stack([O.stem_forward(mag, sds[s]) for s in O.STEMS]))


@pytest.fixture(scope="module")
def long(sds):
    x = O.clip(3, N_LONG)
    re, im, mag = O.stft(x.astype(np.float64))
    return dict(x=x, re=re, im=im, mag=mag, masked=np.stack([O.stem_forward(mag, sds[s]) for s in O.STEMS]))


@pytest.mark.parametrize("n", [N_MAIN, 1024, 700])
def test_stft(sep, n):
    x = O.clip(n % 7, n)
    got = sep.stft(x)
    want = O.stft(x.astype(np.float64))
    assert got[0].shape == (O.num_frames(n), 2, 2049)
    d = max(rel(g, w) for g, w in zip(got, want))
    print("stft n = %d: device vs float64 oracle %.2e of peak (bound %.2e)" % (n, d, TOL_STFT))
    assert d <= TOL_STFT


def test_masks_hidden512(sep, sds, main):
    """T = 9, T = 1 and T = 3 as one ragged batch of three files, all four stems."""
    mags = [main["mag"], O.stft(O.clip(1, 700).astype(np.float64))[2], O.stft(O.clip(2, 2 * 1024 + 5).astype(np.float64))[2]]
    got = sep.masks([m.astype(np.float32) for m in mags])
    worst = 0.0
    for b, m in enumerate(mags):
        assert got[b].shape == (4, m.shape[0], 2, 2049)
        want = main["masked"] if b == 0 else np.stack([O.stem_forward(m.astype(np.float32).astype(np.float64), sds[s]) for s in O.STEMS])
        worst = max(worst, max(rel(got[b][j], want[j]) for j in range(4)))
    print("masks hidden 512: device vs float64 oracle %.2e of peak (bound %.2e)" % (worst, TOL_MASKS))
    assert worst <= TOL_MASKS


def test_masks_hidden1024(tmp_path_factory):
    big = synth.synth_openunmix_state_dict(5, 1024)
    m = SourceSeparator.from_pretrained(synth.write_openunmix_safetensors(big, str(tmp_path_factory.mktemp("umxl"))))
    try:
        assert m.hidden_size == 1024
        mag = O.stft(O.clip(4, 4 * 1024 + 3).astype(np.float64))[2].astype(np.float32)
        got = m.masks(mag)
        worst = max(rel(got[j], O.stem_forward(mag.astype(np.float64), big[s])) for j, s in enumerate(O.STEMS))
    finally:
        m.close()
    print("masks hidden 1024: device vs float64 oracle %.2e of peak (bound %.2e)" % (worst, TOL_MASKS))
    assert worst <= TOL_MASKS


def test_recurrence_long(sep, long):
    got = sep.masks(long["mag"].astype(np.float32))
    worst = max(rel(got[j], long["masked"][j]) for j in range(4))
    print("masks T = 305: device vs float64 oracle %.2e of peak (bound %.2e)" % (worst, TOL_LONG))
    assert worst <= TOL_LONG


@pytest.mark.parametrize("case,window", [("main", 4), ("long", 300)])
@pytest.mark.parametrize("iterations", [1, 2])
def test_wiener(sep, main, long, case, window, iterations):
    """The oracle is fed the DEVICE's masked magnitudes and STFT, so the stage is judged alone."""
    c = main if case == "main" else long
    re, im, mag = sep.stft(c["x"])
    masked = sep.masks(mag)
    gre, gim = sep.wiener(masked, re, im, iterations=iterations, window=window)
    wre, wim = O.wiener(masked.astype(np.float64), re.astype(np.float64), im.astype(np.float64), iterations, window)
    peak = max(np.abs(wre).max(), np.abs(wim).max())
    d = float(max(np.abs(gre - wre).max(), np.abs(gim - wim).max()) / peak)
    print("wiener %s window %d x %d: device vs float64 oracle %.2e of peak (bound %.2e)" % (case, window, iterations, d, TOL_WIENER))
    assert d <= TOL_WIENER


def test_istft(sep, main):
    re, im, _ = sep.stft(main["x"])
    got = sep.istft(re, im, N_MAIN)
    d = rel(got, O.istft(re.astype(np.float64), im.astype(np.float64), N_MAIN))
    back = rel(got, main["x"].astype(np.float64))
    print("istft: device vs float64 oracle %.2e of peak (bound %.2e); reconstruction %.2e (bound 1e-5)" % (d, TOL_ISTFT, back))
    assert got.shape == (2, N_MAIN) and d <= TOL_ISTFT and back <= 1e-5


def test_separate(sep, sds, main):
    x = main["x"]
    worst = 0.0
    for kw, okw in ((dict(wiener=True), dict(use_wiener=True)), (dict(wiener=False), dict(use_wiener=False)),
                    (dict(targets=("other", "drums")), dict(targets=("other", "drums"))), (dict(targets=("bass",)), dict(targets=("bass",)))):
        got, want = sep.separate(x, **kw), O.separate(x, sds, **okw)
        assert list(got) == [t for t in TARGETS if t in kw.get("targets", TARGETS)] == list(want)
        for t in got:
            assert got[t].shape == (2, N_MAIN) and got[t].dtype == np.float32
            worst = max(worst, rel(got[t], want[t]))
    single = sep.separate(x, targets=("bass",), wiener=True)                    # a single target takes the no-Wiener path
    assert np.array_equal(single["bass"], sep.separate(x, targets=("bass",), wiener=False)["bass"])
    mono = sep.separate(x[0])                                                    # mono is duplicated
    stereo = sep.separate(np.stack([x[0], x[0]]))
    assert all(np.array_equal(mono[t], stereo[t]) for t in TARGETS)
    worst = max(worst, max(rel(mono[t], w) for t, w in O.separate(x[0], sds).items()))
    print("separate: device vs float64 oracle %.2e of peak (bound %.2e)" % (worst, TOL_SEP))
    assert worst <= TOL_SEP


def test_bit_identity(sep, model_dir):
    ns = [3 * 1024 + 5, 700, 6 * 1024, 1024 + 1, 4 * 1024 + 999]
    clips = [O.clip(10 + k, n) for k, n in enumerate(ns)]
    clips[1] = clips[1][0]                                                        # one mono file
    alone = [sep.separate(c) for c in clips]
    batch = sep.separate_batch(clips)
    rev = sep.separate_batch(clips[::-1])[::-1]
    small = SourceSeparator.from_pretrained(model_dir, max_batch_samples=8 * 1024)  # passes: (3077, 700), (6144, 1025), (5095)
    try:
        split = small.separate_batch(clips)
    finally:
        small.close()
    again = sep.separate_batch(clips)
    for other in (batch, rev, split, again):
        for a, b in zip(alone, other):
            assert all(np.array_equal(a[t], b[t]) for t in TARGETS)
    sep.set_recurrence_form(1)                                                    # the kept alternative sums in the same order
    try:
        alt = sep.separate_batch(clips)
    finally:
        sep.set_recurrence_form(0)
    assert all(np.array_equal(a[t], b[t]) for a, b in zip(alone, alt) for t in TARGETS)


def test_errors(sep, model_dir):
    x = O.clip(0, 2048)
    for call, code in ((lambda: sep.separate(x, sample_rate=48000), 7), (lambda: sep.separate(x[:, :0]), 6)):
        with pytest.raises(QasrError) as e:
            call()
        assert ("qasr error %d:" % code) in str(e.value) and len(str(e.value)) > 16
    small = SourceSeparator.from_pretrained(model_dir, max_batch_samples=1024)
    try:
        with pytest.raises(QasrError) as e:
            small.separate(x)
        assert "qasr error 5:" in str(e.value) and "max_batch_samples" in str(e.value)
        assert small.separate(x[:, :1000])["vocals"].shape == (2, 1000)          # the handle stays usable
        small.unload()
        assert not small.is_loaded and small.memory_footprint == 0
        with pytest.raises(QasrError) as e:
            small.separate(x[:, :1000])
        assert "qasr error 3:" in str(e.value)
    finally:
        small.close()
    lib = _lib.load(strict=True)
    out = np.zeros((4, 2, 2048), np.float32)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.qasr_sep_separate(None, f(x[0]), f(x[1]), 2048, 44100, 15, None, f(out)) == 1
    assert lib.qasr_sep_timing(None, None) == 1 and lib.qasr_sep_hidden_size(None) == 0
    assert sep.separate(x)["other"].shape == (2, 2048) and sep.is_loaded and sep.memory_footprint > 0
    assert set(sep.timing()) == {"stft", "network", "wiener", "istft"}

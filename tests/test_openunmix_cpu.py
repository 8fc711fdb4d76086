"""Open-Unmix source separation on the CPU: the float64 oracle (tests/openunmix_oracle.py) against torch, the reference's padding rule,
the f32 distances that set the GPU tests' tolerances, and the checked loader of qasr_sep_create (no device call is reached)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import openunmix_oracle as O
from qasr import synth

N_MAIN, N_LONG = 8 * 1024 + 37, 304 * 1024 + 11        # T = 9 and T = 305: the GPU tests' clips


@pytest.fixture(scope="module")
def sds():
    return synth.synth_openunmix_state_dict(0, 512)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())


def test_padding_rule():
    """n <= 2048: the clamped rule, by hand.  n = 1: every index 0.  n = 2: left min(2048 - i, 1) = 1, right max(0, -i) = 0.
    n = 700: left 699 (clamped) until 2048 - i < 699, i.e. i > 1349, then 2048 - i; right 698, 697, .., 0, 0, ..."""
    assert (O.pad_indices(1) == 0).all() and O.pad_indices(1).shape == (4097,)
    p = O.pad_indices(2)
    assert (p[:2048] == 1).all() and list(p[2048:2050]) == [0, 1] and (p[2050:] == 0).all()
    p = O.pad_indices(700)
    assert (p[:1350] == 699).all() and p[1350] == 698 and p[2047] == 1 and list(p[2048:2051]) == [0, 1, 2]
    assert list(p[2748:2751]) == [698, 697, 696] and p[2748 + 698] == 0 and (p[2748 + 698:] == 0).all()
    n = 3000                                            # n > 2048: numpy's reflect pad
    assert (O.pad_indices(n) == np.pad(np.arange(n), 2048, mode="reflect")).all()


def test_stft_istft_vs_torch():
    x = O.clip(1, N_MAIN).astype(np.float64)
    re, im, mag = O.stft(x)
    w = torch.hann_window(4096, periodic=True, dtype=torch.float64)
    z = torch.stft(torch.from_numpy(x), 4096, 1024, window=w, center=True, pad_mode="reflect", return_complex=True)   # [2, F, T]
    want = z.permute(2, 0, 1).numpy()
    assert re.shape == (9, 2, 2049)
    assert rel(re, want.real) <= 1e-9 and rel(im, want.imag) <= 1e-9 and rel(mag, np.abs(want)) <= 1e-9
    back = torch.istft(z, 4096, 1024, window=w, center=True, length=N_MAIN).numpy()
    assert rel(O.istft(re, im, N_MAIN), back) <= 1e-9
    assert rel(O.istft(re, im, N_MAIN), x) <= 1e-9


def test_stem_vs_torch(sds):
    sd = sds["drums"]
    H = 512
    mag = O.stft(O.clip(2, N_MAIN).astype(np.float64))[2]
    t = lambda k: torch.from_numpy(np.asarray(sd[k], dtype=np.float64))
    fc1, fc2, fc3 = torch.nn.Linear(2974, H, bias=False), torch.nn.Linear(2 * H, H, bias=False), torch.nn.Linear(H, 4098, bias=False)
    bns = [torch.nn.BatchNorm1d(H), torch.nn.BatchNorm1d(H), torch.nn.BatchNorm1d(4098)]
    lstm = torch.nn.LSTM(H, H // 2, num_layers=3, bidirectional=True)
    mods = torch.nn.ModuleList([fc1, fc2, fc3, lstm] + bns).double().eval()
    with torch.no_grad():
        for i, fc in enumerate((fc1, fc2, fc3)):
            fc.weight.copy_(t(f"fc{i + 1}.weight"))
        for i, bn in enumerate(bns):
            bn.weight.copy_(t(f"bn{i + 1}.weight")); bn.bias.copy_(t(f"bn{i + 1}.bias"))
            bn.running_mean.copy_(t(f"bn{i + 1}.running_mean")); bn.running_var.copy_(t(f"bn{i + 1}.running_var"))
        for l in range(3):
            for d, suf in (("forward", ""), ("backward", "_reverse")):
                for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    getattr(lstm, f"{k}_l{l}{suf}").copy_(t(f"lstm.layers.{l}.{d}.{k}"))
        x = torch.from_numpy(mag)
        h = ((x[:, :, :1487] + t("input_mean")) * t("input_scale")).reshape(-1, 2974)
        h = torch.tanh(bns[0](fc1(h)))
        h = torch.cat([h, lstm(h[:, None])[0][:, 0]], dim=-1)
        h = bns[2](fc3(torch.relu(bns[1](fc2(h))))).reshape(-1, 2, 2049)
        want = (torch.relu(h * t("output_scale") + t("output_mean")) * x).numpy()
    assert mods is not None and rel(O.stem_forward(mag, sd), want) <= 1e-9


def test_masks_are_neither_zero_nor_saturated(sds):
    mag = O.stft(O.clip(0, N_MAIN).astype(np.float64))[2]
    for stem in O.STEMS:
        ratio = O.stem_forward(mag, sds[stem]) / np.maximum(mag, 1e-12)
        frac_zero = float((ratio == 0).mean())
        assert 0.02 < frac_zero < 0.9 and 0.1 < float(np.median(ratio[ratio > 0])) < 10.0, (stem, frac_zero)


def test_f32_distance(sds):
    """max |f32 twin - float64 oracle| / peak of the stage's output, on the GPU tests' clips and weights.  The printed values are the
    yardsticks of tests/test_gpu_openunmix.py (10 x each) and of DESIGN.md section 14."""
    f32, out = np.float32, {}
    d = 0.0
    for n in (N_MAIN, 1024, 700):
        x = O.clip(n % 7, n)
        a, b = O.stft(x, f32), O.stft(x.astype(np.float64))
        d = max(d, max(rel(p, q) for p, q in zip(a, b)))
    out["stft"] = d
    x = O.clip(0, N_MAIN)
    re, im, mag = O.stft(x.astype(np.float64))
    masked = np.stack([O.stem_forward(mag, sds[s]) for s in O.STEMS])
    out["masks"] = max(rel(O.stem_forward(mag.astype(f32), sds[s], f32), masked[i]) for i, s in enumerate(O.STEMS))
    xl = O.clip(3, N_LONG)
    rel_, iml, magl = O.stft(xl.astype(np.float64))
    maskedl = np.stack([O.stem_forward(magl, sds[s]) for s in O.STEMS])
    out["masks_long"] = max(rel(O.stem_forward(magl.astype(f32), sds[s], f32), maskedl[i]) for i, s in enumerate(O.STEMS))
    d = 0.0
    for (m, r, i, win) in ((masked, re, im, 4), (maskedl, rel_, iml, 300)):
        m32, r32, i32 = m.astype(f32), r.astype(f32), i.astype(f32)
        for it in (1, 2):
            want = O.wiener(m32.astype(np.float64), r32.astype(np.float64), i32.astype(np.float64), it, win)
            got = O.wiener(m32, r32, i32, it, win, f32)
            peak = max(np.abs(want[0]).max(), np.abs(want[1]).max())
            d = max(d, float(max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()) / peak))
    out["wiener"] = d
    r32, i32 = re.astype(f32), im.astype(f32)
    out["istft"] = rel(O.istft(r32, i32, N_MAIN, f32), O.istft(r32.astype(np.float64), i32.astype(np.float64), N_MAIN))
    d = 0.0
    for kw in (dict(use_wiener=True), dict(use_wiener=False), dict(targets=("bass",)), ):
        want, got = O.separate(x, sds, **kw), O.separate(x, sds, dtype=f32, **kw)
        d = max(d, max(rel(got[k], want[k]) for k in want))
    out["separate"] = d
    print("f32 distances:", {k: "%.2e" % v for k, v in out.items()})
    # the Wiener condition: the reference allows 1e-3 of peak between its own two implementations (OpenUnmixTests.swift:198-200, 208-257)
    assert out["wiener"] < 1e-3
    assert all(v < 1e-3 for v in out.values())


# ---- loader (qasr_sep_create fails before any HIP call) ----
def _create(model_dir):
    from qasr import _lib
    lib = _lib.load(strict=True)
    h = C.c_void_p()
    rc = lib.qasr_sep_create(0, str(model_dir).encode(), 0, None, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.qasr_sep_last_error(None).decode()


@pytest.fixture(scope="module")
def small_sds():
    """Real shapes are large; the loader tests only need files that fail early, so one valid set is written once."""
    return synth.synth_openunmix_state_dict(1, 512)


def test_loader_missing_key(small_sds, tmp_path):
    synth.write_openunmix_safetensors(small_sds, str(tmp_path), drop=("bn2.running_var",))
    rc, msg = _create(tmp_path)
    assert rc == 4 and "bn2.running_var" in msg and "drums.safetensors" in msg


def test_loader_wrong_shape(small_sds, tmp_path):
    synth.write_openunmix_safetensors(small_sds, str(tmp_path), reshape={"lstm.layers.1.backward.weight_hh": (1024, 255)})
    rc, msg = _create(tmp_path)
    assert rc == 1 and "lstm.layers.1.backward.weight_hh" in msg and "[1024, 256]" in msg


def test_loader_missing_stem_file(small_sds, tmp_path):
    synth.write_openunmix_safetensors(small_sds, str(tmp_path), skip_stems=("bass",))
    rc, msg = _create(tmp_path)
    assert rc == 4 and "bass.safetensors" in msg


def test_loader_detects_umxl(tmp_path):
    """A hidden-1024 directory is taken as umxl: its shape table is the one checked, so a hidden-512 tensor in it is the wrong shape."""
    big = synth.synth_openunmix_state_dict(2, 1024)
    big["drums"]["fc2.weight"] = np.zeros((512, 1024), np.float32)
    synth.write_openunmix_safetensors(big, str(tmp_path))
    rc, msg = _create(tmp_path)
    assert rc == 1 and "fc2.weight" in msg and "[1024, 2048]" in msg


def test_constants():
    from qasr import _lib, separation
    lib = _lib.load(strict=True)
    cfg = _lib.QasrSepConfig()
    assert lib.qasr_sep_default_config(C.byref(cfg)) == 0 and (cfg.wiener, cfg.wiener_iterations, cfg.wiener_window) == (1, 1, 300)
    assert lib.qasr_sep_sample_rate() == 44100 and separation.num_frames(N_MAIN) == 9 and separation.num_frames(700) == 1
    assert lib.qasr_sep_last_error(None) is not None and lib.qasr_sep_is_loaded(None) == 0 and lib.qasr_sep_unload(None) == 1

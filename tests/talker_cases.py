"""Shared inputs of tests/test_talker_cpu.py and tests/test_gpu_talker.py: the reduced geometries, the rows and the twin's pinned
distances from the float64 oracle, which the GPU bounds derive from."""
import numpy as np

from qasr import synth

TOKENS = dict(codec_pad=2148, codec_bos=2149, codec_eos=2150, codec_think=2154, codec_nothink=2155, codec_think_bos=2156,
              codec_think_eos=2157, tts_pad=509, tts_bos=510, tts_eos=511)
GEOMETRIES = {"small4": dict(synth.TTS_TALKER_SMALL, bits=4), "small8": dict(synth.TTS_TALKER_SMALL, bits=8),
              "large4": dict(synth.TTS_TALKER_LARGE_FORM, bits=4)}
FORCED_T = 24                      # frames of the forced pass
ATT_CHUNK, ATT_ROUND = 32, 256     # keys of one chunk of the Talker's attention sweep, and of one round of its 8 waves
MAX_INSTRUCT = 240
# max |d| / peak of the twin from the oracle over the forced cases (test_talker_cpu.py::test_twin_distance pins them within 2 x)
TWIN = {"small4": {"talker": 9.59e-3, "cp": 1.42e-2, "hidden": 1.15e-2},
        "small8": {"talker": 7.10e-3, "cp": 1.17e-2, "hidden": 9.14e-3},
        "large4": {"talker": 6.35e-3, "cp": 1.68e-2, "hidden": 1.01e-2}}
N_ROWS = {"small4": 33, "small8": 5, "large4": 5}
MARGIN = 4                         # GPU bound = MARGIN x TWIN: see the docstring of tests/test_gpu_talker.py
GREEDY_SEEDS = (0, 1, 2)           # rows of the greedy free run (make_rows indices)
GREEDY_T = 12


def make_rows(n, hidden, seed=11):
    """n ragged rows.  Row 0: the 9-token minimum (trailing = tts_eos alone); row 1: 10 tokens (one trailing text token); a speaker
    token on every third row, an x-vector on every fifth; instruct prefixes that put the prompt's end just under one attention chunk
    (rows 4, 5, 6: prompt + frames cross 31 | 32 | 33), two chunks (row 7: 63 | 64 | 65) and one round of the sweep (row 8: 255 | 256 | 257)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        n_text = 1 if i == 0 else 2 if i == 1 else int(rng.integers(3, 40))
        text = [1, 2, 3] + [int(v) for v in rng.integers(4, 500, n_text)] + [5, 6, 7, 8, 9]
        row = dict(text=text, language=2050 + i % 20)
        if i % 3 == 2:
            row["speaker"] = 3000 + i
        if i % 5 == 3:
            row["xvector"] = (0.5 * rng.standard_normal(hidden)).astype(np.float32)
        ins = {4: 12, 5: 13, 6: 14, 7: 44, 8: MAX_INSTRUCT - 4}.get(i)
        if ins is not None:
            row["instruct"] = [int(v) for v in rng.integers(4, 500, ins)]
        rows.append(row)
    return rows


def forced_codes(n, T, seed=23):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2048, (n, 16, T)).astype(np.int32)
    return c


def margin_rule(codes, ref, bound_talker, bound_cp, eos=2150):
    """Positions (frame, stream) at which `codes` is not the oracle's argmax; asserts the oracle's gap there is within the bound."""
    second = total = 0
    hist = set()
    for f in range(codes.shape[1]):
        lg = ref["talker"][f].astype(np.float64).copy()
        lg[2048:eos] = -1e9
        lg[eos + 1:] = -1e9
        for t in hist:
            lg[t] = lg[t] * 1.05 if lg[t] < 0 else lg[t] / 1.05
        hist.add(int(codes[0, f]))
        for j, (l, tok, bound) in enumerate([(lg, codes[0, f], bound_talker)] + [(ref["cp"][f, q], codes[q + 1, f], bound_cp) for q in range(15)]):
            total += 1
            if int(np.argmax(l)) != int(tok):
                second += 1
                assert l.max() - l[tok] <= bound, (f, j, float(l.max() - l[tok]), bound)
    return second, total

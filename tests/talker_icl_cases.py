"""Shared inputs of tests/test_talker_icl_cpu.py and tests/test_gpu_talker_icl.py: the ICL rows and the twin's pinned distances from the
float64 oracle (tests/talker_icl_oracle.py), which the GPU bounds derive from (MARGIN x the figure, as in tests/talker_cases.py)."""
import numpy as np

import talker_cases as K

TOKENS, GEOMETRIES, MARGIN, margin_rule = K.TOKENS, K.GEOMETRIES, K.MARGIN, K.margin_rule
MAX_REF_FRAMES, MAX_REF_TEXT, MAX_FRAMES, MAX_TEXT = 272, 32, 32, 64
FORCED_T = 12
# (reference-text ids, target ids, reference frames) per row; packed positions P - 1 = 10 + Tr + Tt + F.  12 is the minimum; 64 is the key
# and query tile of the prompt attention, 128 two tiles; at 256 the 12 forced frames cross one round of the decode sweep, the other rows
# its 32-key chunks.  Row 0 has one frame, rows 0 and 2 no reference text, rows 5 and 8 are almost all reference frames.
SHAPES = [(0, 1, 1), (4, 9, 40), (0, 14, 40), (5, 10, 40), (8, 20, 89), (3, 5, 110), (10, 30, 79), (12, 20, 213), (2, 4, 240), (32, 43, 172)]
PACKED_LEN = [12, 63, 64, 65, 127, 128, 129, 255, 256, 257]
OTHER_ROWS = (0, 3, 8)             # the rows of small8 and large4
GREEDY_ROWS = (0, 1, 3)            # rows of the greedy free run
GREEDY_T = 12
# max |d| / peak of the twin from the oracle over the forced ICL cases: "prompt" for the prompt rows, then per value of tts_packed_prompt
# (test_talker_icl_cpu.py::test_twin_distance_icl pins them within 2 x; measured on the CPU, printed by that test)
TWIN = {"small4": {"prompt": 3.76e-3, 0: {"talker": 9.78e-3, "cp": 1.26e-2, "hidden": 1.06e-2}, 1: {"talker": 8.19e-3, "cp": 1.15e-2, "hidden": 1.09e-2}},
        "small8": {"prompt": 3.35e-3, 0: {"talker": 7.42e-3, "cp": 1.07e-2, "hidden": 1.07e-2}, 1: {"talker": 6.60e-3, "cp": 8.38e-3, "hidden": 9.58e-3}},
        "large4": {"prompt": 2.46e-3, 0: {"talker": 5.09e-3, "cp": 1.29e-2, "hidden": 8.36e-3}, 1: {"talker": 6.46e-3, "cp": 1.37e-2, "hidden": 8.71e-3}}}


def make_rows(hidden, seed=31, n=None):
    """Row i has SHAPES[i % 10]; rows past the tenth repeat the shapes with other ids, codes and x-vectors."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(len(SHAPES) if n is None else n):
        tr, tt, f = SHAPES[i % len(SHAPES)]
        text = [1, 2, 3] + [int(v) for v in rng.integers(4, 500, tt)] + [5, 6, 7, 8, 9]
        rows.append(dict(text=text, language=2050 + i % 20, xvector=(0.5 * rng.standard_normal(hidden)).astype(np.float32),
                         ref_text=[int(v) for v in rng.integers(4, 500, tr)],
                         ref_codes=rng.integers(0, 2048, (16, f)).astype(np.int32)))
    return rows


def forced_codes(n, T=FORCED_T, seed=37):
    return np.random.default_rng(seed).integers(0, 2048, (n, 16, T)).astype(np.int32)


def rows_of(name, hidden):
    rows = make_rows(hidden)
    return rows if name == "small4" else [rows[i] for i in OTHER_ROWS]

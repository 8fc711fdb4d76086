"""Shared inputs of tests/test_cvlm_cpu.py and tests/test_gpu_cvlm.py: the reduced geometries, the rows, the crafted sampler cases and
the twin's pinned distances from the float64 oracle, which the GPU bounds derive from."""
import numpy as np

# real4: the product's own K (896, 4864), block counts (7 and 38 at 4 bit) and 7 query heads per kv head, at real widths;
# odd8: an odd block count at 8 bit (K = 384: 6 blocks, 640: 10) and 3 query heads per kv head; tiny4: a vocabulary of 21, so that
# stop tokens occur naturally in a sampled run
GEOMETRIES = {
    "real4": dict(hidden=896, heads=14, kv_heads=2, head_dim=64, inter=4864, layers=2, bits=4, text_vocab=1024, speech_tokens=6561, speech_extra=200),
    "odd8": dict(hidden=384, heads=6, kv_heads=2, head_dim=64, inter=640, layers=3, bits=8, text_vocab=1024, speech_tokens=6561, speech_extra=200),
    "tiny4": dict(hidden=384, heads=6, kv_heads=2, head_dim=64, inter=640, layers=3, bits=4, text_vocab=1024, speech_tokens=13, speech_extra=8),
}
FORCED_T = 24                       # tokens of the forced pass
ATT_CHUNK, ATT_ROUND = 64, 256      # keys of one wave in one round of the attention sweep, and of one round (csrc/llm_cosyvoice.h)
MAX_TEXT, MAX_PROMPT, MAX_TOKENS = 256, 24, 32
N_ROWS = {"real4": 33, "odd8": 5, "tiny4": 17}
# prefix lengths of the first rows: the minimum 3 (sos + one text id + task_id) and 4; 63 | 64 | 65 put the first forced positions on
# either side of one chunk; 120, 180 and 250 make the 24 forced tokens cross 127 | 128 | 129, 191 | 192 | 193 and (one round of the
# sweep) 255 | 256 | 257 keys; 129 starts just behind a chunk edge
EDGE_PREFIX = (3, 4, 63, 64, 65, 129, 120, 180, 250)
EDGE_ROWS = tuple(range(len(EDGE_PREFIX)))
# max |d| / peak of the twin from the oracle over the forced cases (test_cvlm_cpu.py::test_twin_distance pins them within 2 x)
TWIN = {"real4": {"logits": 1.46e-2, "hidden": 1.31e-2},
        "odd8": {"logits": 1.36e-2, "hidden": 1.53e-2}}
MARGIN = 4                          # GPU bound = MARGIN x TWIN: the project's margin for a bf16 path (docstring of tests/test_gpu_talker.py)
# rows of the greedy free run (make_rows indices).  With 36 positions the 2 % cap allows no position off the oracle's argmax, so the run
# is only meaningful on rows where the oracle itself is decisive: these are the three rows of the first twelve whose float64 greedy
# trajectory keeps the largest top-2 gap (0.23, 0.29 and 0.17 of the forced bound at its narrowest; every other row has a gap below 0.1)
GREEDY_ROWS = (1, 5, 7)
GREEDY_T = 12
SAMPLED_SEED = 12                   # the sampled free run on tiny4: with this seed each of the three stop tokens ends a row


def make_rows(n, g, seed=17):
    """n ragged rows of prefix length EDGE_PREFIX[i] (then random 5 .. 60); every third row has prompt speech tokens."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        P = EDGE_PREFIX[i] if i < len(EDGE_PREFIX) else int(rng.integers(5, 61))
        n_prompt = int(rng.integers(1, min(MAX_PROMPT, P - 3) + 1)) if i % 3 == 2 and P > 3 else 0
        row = dict(text=[int(v) for v in rng.integers(0, g["text_vocab"], P - 2 - n_prompt)])
        if n_prompt:
            row["prompt"] = [int(v) for v in rng.integers(0, g["speech_tokens"], n_prompt)]
        rows.append(row)
    return rows


def prefix_len(row):
    return 2 + len(row["text"]) + len(row.get("prompt") or [])


def forced_tokens(n, T, g, seed=29):
    return np.random.default_rng(seed).integers(0, g["speech_tokens"], (n, T)).astype(np.int32)


def margin_rule(tokens, ref_logits, bound, speech_tokens):
    """Positions at which `tokens` is not the argmax of the oracle's masked logits; asserts the oracle's gap there is within the bound."""
    second = 0
    for f, tok in enumerate(tokens):
        lg = ref_logits[f].astype(np.float64).copy()
        lg[speech_tokens:] = -1e9                                # steps 1 and 2 with the stops masked (a large min_len)
        if int(np.argmax(lg)) != int(tok):
            second += 1
            assert lg.max() - lg[tok] <= bound, (f, float(lg.max() - lg[tok]), bound)
    return second, len(tokens)


def ulp_close(pert, a, b):
    """The project's rule for a pick that differs between two realisations of the sampler: 4 ulp of the perturbed values."""
    return abs(float(pert[a]) - float(pert[b])) <= 4 * np.spacing(np.float32(max(abs(float(pert[a])), abs(float(pert[b])))))


def sampler_cases(V=6761, ST=6561):
    """Crafted logits for the sampler: (name, logits, kwargs of cvlm_oracle.sample).  Values are spaced so that no top-p boundary lies
    within 1e-4 of top_p (the tests assert it)."""
    rng = np.random.default_rng(5)
    base = (rng.standard_normal(V) * 2.0).astype(np.float32)
    cases = []
    tie = base.copy()
    tie[[10, 20, 30, 40]] = 9.0                                  # four-way tie at the top-k threshold: all survive top_k = 2
    cases.append(("ties_at_threshold", tie, dict(top_k=2, top_p=1.0, win_size=0)))
    heavy = base.copy()                                          # six tokens hold 0.96 of the mass: with every token a survivor the
    heavy[[100, 200, 300, 400, 500, 600]] = [14.0, 13.5, 13.0, 12.5, 12.0, 11.5]     # boundaries near 0.5 and 0.8 lie among them, far apart
    cases.append(("top_k_off", heavy, dict(top_k=0, top_p=0.8, win_size=0)))
    cases.append(("top_k_over_V", heavy, dict(top_k=V, top_p=0.5, win_size=0)))
    cases.append(("top_p_one", base, dict(top_k=25, top_p=1.0, win_size=0)))
    peak = base.copy()
    peak[77] = 30.0                                              # one token holds all the mass: always picked, a repeat in the window resamples
    cases.append(("resample_one_repeat", peak, dict(history=[5, 77, 9], step=3)))
    cases.append(("no_repeat_no_resample", peak, dict(history=[5, 6, 9], step=3)))
    cases.append(("repeat_outside_window", peak, dict(history=[77] + [5] * 10, step=11)))
    cases.append(("win_size_zero", peak, dict(history=[77, 77, 77], step=3, win_size=0)))
    stop = base.copy()
    stop[ST + 1] = 30.0
    cases.append(("stop_masked_below_min", stop, dict(history=[1, 2], step=2, below_min=True)))
    cases.append(("stop_masked_at_token_0", stop, dict(step=0)))
    cases.append(("stop_live_at_min", stop, dict(history=[1, 2], step=2, below_min=False)))
    tail = base.copy()
    tail[ST + 3:] = 50.0                                         # the suppressed tail never wins
    cases.append(("suppressed_tail", tail, dict(history=[1], step=1)))
    return cases

"""The batched decode step's logits, row by row, at 1 to 64 rows (qasr_batch_prefill_logits / qasr_batch_decode_forced: the product's own
prompt pass and decode step with the [B][vocab] logits kept; the forced step is the step qasr_batch_run captures, launched eagerly).

Every other logit comparison in tests/ runs at ONE batch row; rows 1..63 of a batch were seen only as token ids (one value in 151 936).  Here:

  2.1  every row of a ragged batch against the CPU oracle (DEVICE policy) on that clip alone -- prompt pass + 4 teacher-forced steps along the
       oracle's greedy stream, both sides fed the device's stage-call encoder output of the clip -- at 1, 2, 8, 9, 16, 17, 32, 33, 48, 49 and
       64 rows: both sides of every switch of gemv2_nb (batch tiles, row groups, partial tile, early weights), of the fused q|k|v + attention
       launch (<= 32 rows, context split <= 8) and of the LM heads (NB 1..4); bf16, MLX 4-bit and 8-bit checkpoints at the 0.6B widths
       (1 encoder / 3 decoder layers), the tiny preset (generic kernels) at 17 / 64, the 1.7B widths (2 layers; K = 2048 / 6144) at
       1 / 18 / 32 / 33 / 64; and a 41 s clip (549 prompt positions, beyond the 512 keys of the first request round) between two short rows,
       stepped across a 32-key chunk boundary.
  2.2  slot independence without a tolerance: one clip in rows 0, 15, 16, 17, 31, 33, 47, 48, 63 of a 64-row batch -> bit-identical logits.
  2.3  the fused argmax = the FIRST maximum of the logits the same kernel wrote (tokens of the graph path replayed through the forced step),
       and, with the tied head replicated in blocks of P rows so that every maximum is tied, the pick is always the lower copy.
  2.4  the decode-step knobs no other test sets.
  3    the 1.7B widths created for 64 rows serve 33 and 64 rows (the LM head at hidden 2048 holds 32 rows per launch: two launches).

Bars (the project's own): tiny -- max |d| < 0.06 and rel-L2 < 1.5e-2 (test_gpu_decoder.py); 0.6B / 1.7B widths -- 6 bf16 ulps of the largest
|logit| and rel-L2 < 3e-2 (test_gpu_full._tol); quantised -- the same plus the argmax within that margin (test_gpu_quant._check).  Those bars
were sized for 28 layers; each test prints the CPU floor (rel-L2 between the oracle's DEVICE and REFERENCE policies on the same row and tokens)
next to every row's device-vs-DEVICE distance.

Knobs held to BIT equality with the default (tuning.h / the kernels' comments say they only move requests in time or keep the k order):
gemv_xbar, gemv_earlyw, gemv_nt, lmh_nt, lmh_order, da_spec, da_earlyq, da_unr.  Knobs whose instantiation changes how the k range is cut over
waves or how rows are grouped (gemv_w1024 = 4: 4 waves x 8 k-steps; gemv_splitb 0 / 1: all batch tiles in one workgroup; gemv_partial 0;
da_waves 16: other chunk -> wave map) are held to the 2.1 bars against the oracle; the test prints whether they happened to be bit-equal.

Measured on an MI355X (worst row over all batch sizes and positions; rel-L2 device vs DEVICE | largest CPU floor | max |d| in bf16 ulps):
  0.6B widths, 3 layers, bf16   9.9e-3 | 9.9e-3 | 2.8      4-bit  1.35e-2 | 1.05e-2 | 3.2      8-bit  1.32e-2 | 9.9e-3 | 3.2
  tiny                          1.22e-2 | 1.02e-2 | 2.1    1.7B widths, 2 layers, bf16  8.7e-3 | 8.7e-3 | 1.5      8-bit (33 rows)  1.24e-2 | 9.0e-3 | 2.0
  41 s row between short rows, 2 layers, 31 positions   8.0e-3 | 8.1e-3 | 2.0
The floor at 3 layers of stress weights is 1e-2, so the 3e-2 bar is three floors wide here: every comparison is also held to TWICE the largest
CPU floor over its rows (compare()), which the device meets with a factor of 1.5 to 2 to spare.  Slot copies, tie copies and the knobs of the
bit-equal list were bit-identical; of the oracle-bar knobs gemv_splitb 0 / 1, gemv_partial 0 and da_waves 16 also gave the default's bits at
8 / 17 / 32 rows, gemv_w1024 = 4 did not (rel-L2 9.6e-3 against the oracle).  In-batch mel + encoder gave the stage calls' bits as far as the
logits can tell (the one-row batch equals the figures of the 64-row batch's row 0).  Wall time of this module: 170 s (99 tests).
"""
import dataclasses
import numpy as np
import pytest
import torch
from oracle import config as C, decoder, precision as P
from qasr import synth
import gpu_util

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 8, 9, 16, 17, 32, 33, 48, 49, 64)
N_STEPS = 4
# 64 different clips of 0.4 .. 4 s, no two of the same length
CLIPS = [synth.synth_waveform(300 + k, 0.4 + 3.6 * ((k * 37) % 64) / 63.0) for k in range(64)]
assert len({len(c) for c in CLIPS}) == 64


def _ulp_tol(ref, ulps=6.0):
    m = float(np.abs(ref).max())
    return ulps * 2.0 ** (np.floor(np.log2(max(m, 1e-3))) - 7)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Rig:
    """One engine + the oracle on the same weights.  Row b of every batch is CLIPS[b], so the oracle's stream of a clip (DEVICE policy: prompt
    logits, N greedy tokens, the logits behind each; REFERENCE teacher-forced along the same tokens for the floor) is computed once per clip."""

    def __init__(self, name, preset, audio, text, tok, bits=0, tiny_bars=False, seed=0, max_seconds=5, max_new=16, clips=CLIPS, **eng_kw):
        self.name, self.text, self.tok, self.bits, self.tiny_bars, self.clips = name, text, tok, bits, tiny_bars, clips
        sd = synth.synth_state_dict(audio, text, seed=seed, init="stress")
        self.float_sd = sd
        self.sd = synth.quantize_state_dict(sd, bits) if bits else sd
        kw = dict(max_batch=64, max_audio_seconds=max_seconds, max_new_tokens=max_new)
        kw.update(eng_kw)
        if bits:
            kw["bits"] = bits
        self.eng = gpu_util.Engine(preset, **kw)
        self.eng.load_state_dict(self.sd)
        self.W = decoder.Weights(self.sd)
        # the stage entry points reuse the engine's batch buffers: every clip's encoder output is taken BEFORE any batch is prepared
        self.emb = [self.eng.encode(self.eng.mel(pcm)) for pcm in clips]
        self._oracle = {}

    def close(self):
        self.eng.close()

    def oracle(self, k, n_steps=N_STEPS):
        hit = self._oracle.get(k)
        if hit is not None and len(hit[0]) >= n_steps:
            return hit
        emb = torch.from_numpy(self.emb[k])
        with torch.no_grad():
            lg, st, _ = decoder.prefill(emb, self.W, self.text, P.DEVICE, self.tok)
            rf, rst, _ = decoder.prefill(emb, self.W, self.text, P.REFERENCE, self.tok)
            toks, dev, floor = [], [lg.numpy().copy()], [_rel(lg.numpy(), rf.numpy())]
            for _ in range(n_steps):
                toks.append(decoder.argmax_lowest(lg))
                lg = decoder.decode_step(toks[-1], self.W, self.text, st, P.DEVICE)
                rf = decoder.decode_step(toks[-1], self.W, self.text, rst, P.REFERENCE)
                dev.append(lg.numpy().copy())
                floor.append(_rel(lg.numpy(), rf.numpy()))
        self._oracle[k] = (toks, dev, floor)
        return self._oracle[k]

    def check(self, got, ref):
        """(inside the bars?, max |d|, rel-L2) of one row at one position"""
        d, rel = float(np.abs(got - ref).max()), _rel(got, ref)
        if self.tiny_bars:
            ok = d < 0.06 and rel < 1.5e-2
        else:
            ok = d <= _ulp_tol(ref) and rel < 3e-2
            if self.bits:
                ok = ok and ref[int(got.argmax())] >= ref.max() - _ulp_tol(ref)
        return bool(ok), d, rel

    def run(self, rows, n_steps=N_STEPS, tokens=None):
        """Prompt pass + n_steps forced steps of the batch CLIPS[rows]: list of n_steps + 1 arrays [B, vocab].  tokens[s][b] = id fed to row
        b at step s (default: the oracle's greedy stream of each row)."""
        eng = self.eng
        out = [eng.batch_prefill_logits([self.clips[k] for k in rows])]
        for s in range(n_steps):
            fed = tokens[s] if tokens is not None else [self.oracle(k, n_steps)[0][s] for k in rows]
            out.append(eng.batch_decode_forced(fed))
        return out

    def compare(self, rows, got, what):
        """every row, every position against the oracle; prints the worst row per position next to the CPU floor; returns the summary"""
        n = len(got) - 1
        worst_rel, worst_ulp, worst_floor, bad = 0.0, 0.0, 0.0, []
        for s in range(n + 1):
            for b, k in enumerate(rows):
                _, dev, floor = self.oracle(k, n)
                ok, d, rel = self.check(got[s][b], dev[s])
                worst_rel, worst_floor = max(worst_rel, rel), max(worst_floor, floor[s])
                worst_ulp = max(worst_ulp, d / _ulp_tol(dev[s], 1.0))
                if not ok:
                    bad.append((b, s, d, round(d / _ulp_tol(dev[s], 1.0), 2), rel))
        print(f"[{self.name}] {what}: {len(rows)} rows x {n + 1} positions: worst device-vs-DEVICE rel-L2 {worst_rel:.2e}, max|d| {worst_ulp:.1f} ulps; "
              f"CPU floor (DEVICE vs REFERENCE) worst rel-L2 {worst_floor:.2e}")
        assert not bad, (self.name, what, "(row, position, max|d|, ulps, rel-L2) outside the bars:", bad[:8], len(bad))
        # the tighter bar at these few layers: twice the largest CPU floor over the compared rows (the ratio of the 3e-2 bar to its measured
        # 1.5e-2 floor at 28 layers); it comes from the two CPU policies alone, never from the device's output
        assert worst_rel < 2.0 * worst_floor, (self.name, what, worst_rel, worst_floor)
        return worst_rel, worst_ulp, worst_floor


def _small(layers=3):
    return dataclasses.replace(C.AUDIO_SMALL, layers=1), dataclasses.replace(C.TEXT_SMALL, layers=layers)


@pytest.fixture(scope="module")
def small():
    a, t = _small()
    r = Rig("0.6B-bf16", "0.6B", a, t, C.TOKENS, enc_layers=1, dec_layers=3)
    yield r
    r.close()


@pytest.fixture(scope="module", params=[4, 8], ids=["w4", "w8"])
def small_q(request):
    a, t = _small()
    r = Rig(f"0.6B-w{request.param}", "0.6B", a, t, C.TOKENS, bits=request.param, enc_layers=1, dec_layers=3)
    yield r
    r.close()


@pytest.fixture(scope="module")
def tiny():
    r = Rig("tiny", "tiny", C.AUDIO_TINY, C.TEXT_TINY, C.TOKENS_TINY, tiny_bars=True, seed=3)
    yield r
    r.close()


def _large_rig(bits=0):
    a, t = dataclasses.replace(C.AUDIO_LARGE, layers=1), dataclasses.replace(C.TEXT_LARGE, layers=2)
    return Rig("1.7B-bf16" if not bits else f"1.7B-w{bits}", "1.7B", a, t, C.TOKENS, bits=bits, seed=1, enc_layers=1, dec_layers=2)


@pytest.fixture(scope="module")
def large():
    r = _large_rig()
    yield r
    r.close()


def _structure_ok(rig, B):
    """the fused q|k|v + attention launch runs at 32 rows or fewer (where its shape is instantiated) and never above"""
    fused = rig.eng.decode_structure()[0]
    if B > 32:
        assert fused == 0, (rig.name, B)
    elif rig.text.hidden == 1024 and rig.text.head_dim == 128:
        assert fused == 1, (rig.name, B)
    return fused


# ---- 2.1 every row against the oracle -------------------------------------------------------------------------------------------------
def _every_row(rig, B):
    rows = list(range(B))
    got = rig.run(rows)
    fused = _structure_ok(rig, B)
    assert all(g.shape == (B, rig.text.vocab) for g in got)
    rig.compare(rows, got, f"B={B} fused_qa={fused}")


@pytest.mark.parametrize("B", SIZES)
def test_every_row_vs_oracle_bf16(small, B):
    _every_row(small, B)


@pytest.mark.parametrize("B", SIZES)
def test_every_row_vs_oracle_quantised(small_q, B):
    _every_row(small_q, B)


@pytest.mark.parametrize("B", [17, 64])
def test_every_row_vs_oracle_tiny(tiny, B):
    _every_row(tiny, B)


@pytest.mark.parametrize("B", [1, 18, 32, 33, 64])
def test_every_row_vs_oracle_1p7b(large, B):
    """33 and 64 rows: the LM head at hidden 2048 holds two batch tiles per launch, Engine::run_lm_head serves the rows in blocks of 32 (before
    that fix the first batch of 33 clips on a 64-row 1.7B engine failed with 'LM head: batch rows exceed the LDS image at this hidden size')."""
    _every_row(large, B)


def test_long_context_row_between_short_rows():
    """A 41 s clip (16 + 533 prompt positions: beyond the 512 keys of the first request round) in row 1, short clips in rows 0 and 2, one
    launch; 30 forced steps take row 1 from 549 to 579 keys, across the 32-key chunk boundary at 576."""
    a, t = _small(2)
    clips = [synth.synth_waveform(4, 2.0), synth.synth_waveform(3, 41.0), synth.synth_waveform(5, 0.7)]
    r = Rig("0.6B-bf16-long", "0.6B", a, t, C.TOKENS, seed=2, max_seconds=42, max_new=40, clips=clips, max_batch=3, enc_layers=1, dec_layers=2)
    try:
        assert r.emb[1].shape[0] == 533
        got = r.run([0, 1, 2], n_steps=30)
        assert r.eng.decode_structure()[0] == 1
        r.compare([0, 1, 2], got, "41 s row between short rows, 30 steps")
    finally:
        r.close()


# ---- 2.2 slot independence, no tolerance ----------------------------------------------------------------------------------------------
COPIES = (0, 15, 16, 17, 31, 33, 47, 48, 63)


def _slot_independence(rig):
    rows = [7 if b in COPIES else (b if b != 7 else 0) for b in range(64)]         # CLIPS[7] in the probed slots, other clips elsewhere
    toks = [[rig.oracle(7)[0][s]] * 64 for s in range(N_STEPS)]                     # every row is fed the same ids: the copies stay copies
    got = rig.run(rows, tokens=toks)
    for s, lg in enumerate(got):
        for b in COPIES[1:]:
            assert np.array_equal(lg[b], lg[0]), (rig.name, "pos", s, "row", b, float(np.abs(lg[b] - lg[0]).max()))
        assert not np.array_equal(lg[1], lg[0])                                     # and another clip does differ
    rig.compare([7], [g[:1] for g in got], "the copied clip, slot 0 of 64")


def test_slot_independence_bf16(small):
    _slot_independence(small)


def test_slot_independence_quantised(small_q):
    _slot_independence(small_q)


# ---- 2.3 the fused argmax is the first maximum of the logits it wrote ------------------------------------------------------------------
def _replay(rig, B, n_tokens=6):
    """tokens of the greedy (graph) path, then the same tokens through the forced step: (tokens [B][n], logits n x [B, vocab])"""
    clips = [rig.clips[k] for k in range(B)]
    toks = rig.eng.transcribe_batch(clips, max_tokens=n_tokens, ignore_eos=True)
    assert [len(t) for t in toks] == [n_tokens] * B
    logits = [rig.eng.batch_prefill_logits(clips)]
    for s in range(n_tokens - 1):
        logits.append(rig.eng.batch_decode_forced([t[s] for t in toks]))
    return toks, logits


def _argmax_identity(rig, B):
    toks, logits = _replay(rig, B)
    for s, lg in enumerate(logits):
        want = np.argmax(lg, axis=1)                                                # NumPy: the first maximum
        for b in range(B):
            assert toks[b][s] == int(want[b]), (rig.name, B, "row", b, "step", s, toks[b][s], int(want[b]))
    return toks


@pytest.mark.parametrize("B", SIZES)
def test_greedy_token_is_first_maximum_bf16(small, B):
    _argmax_identity(small, B)


@pytest.mark.parametrize("B", SIZES)
def test_greedy_token_is_first_maximum_quantised(small_q, B):
    _argmax_identity(small_q, B)


@pytest.mark.parametrize("B", [17, 64])
def test_greedy_token_is_first_maximum_tiny(tiny, B):
    _argmax_identity(tiny, B)


@pytest.mark.parametrize("B", [1, 18, 32, 33, 64])
def test_greedy_token_is_first_maximum_1p7b(large, B):
    _argmax_identity(large, B)


@pytest.mark.parametrize("knob", ["lmh_order", "use_graph"])
def test_greedy_token_is_first_maximum_other_order_and_eager(small, knob):
    small.eng.set_tuning(knob, 0)
    try:
        _argmax_identity(small, 17)
    finally:
        small.eng.set_tuning(knob, 1)


def _replicated_rows(V, period):
    """source row of every vocabulary row: each block of `period` rows is followed by one copy of itself; a ragged tail keeps its own rows"""
    i = np.arange(V)
    src = i - (i % (2 * period)) + (i % period)
    tail = V - V % (2 * period)
    src[tail:] = i[tail:]
    return src, tail


def _ties(rig, periods, sizes):
    """Every maximum tied with its copy `period` rows further on: the pick must be the lower one, at each of the four places the device decides
    (per lane, across lanes, across waves, across workgroup partials), and a copy's logits are the source's bits (same weights, same order).
    The oracle takes no part: the reference is argmax_lowest's rule itself."""
    eng, V = rig.eng, rig.text.vocab
    key = "model.embed_tokens.weight"
    try:
        for period in periods:
            assert 2 * period <= V, period
            src, tail = _replicated_rows(V, period)
            sd = {key: rig.float_sd[key][torch.from_numpy(src)].contiguous()}
            if rig.bits:                                       # replicated BEFORE quantisation: packed words, scales and biases of a copy are equal too
                sd = synth.quantize_state_dict(sd, rig.bits)
            eng.set_tensors(sd)
            for B in sizes:
                toks, logits = _replay(rig, B, n_tokens=4)
                for s, lg in enumerate(logits):
                    assert np.array_equal(lg, lg[:, src]), (rig.name, period, B, s)
                    want = np.argmax(lg, axis=1)
                    for b in range(B):
                        t = toks[b][s]
                        assert t == int(want[b]), (rig.name, "period", period, "B", B, "row", b, "step", s, t, int(want[b]))
                        assert t % (2 * period) < period or t >= tail, (rig.name, "period", period, "B", B, "row", b, "step", s, t)
                        assert t >= tail or lg[b, t] == lg[b, t + period]              # the maximum is tied
    finally:
        eng.set_tensors({k: v for k, v in rig.sd.items() if k.startswith("model.embed_tokens.")})


def test_ties_pick_the_lower_copy_bf16(small):
    grid = small.eng.get_tuning("lmh_grid")
    _ties(small, (1, 4, 16, 16 * 8 * grid, small.text.vocab // 2), (17, 64))
    small.eng.set_tuning("lmh_order", 0)                       # wave fastest: the same wave's next tile is 16 x waves x workgroups rows on as well
    try:
        _ties(small, (16, 16 * 8 * grid), (17,))
    finally:
        small.eng.set_tuning("lmh_order", 1)


def test_ties_pick_the_lower_copy_quantised(small_q):
    _ties(small_q, (1, 4, 16, 16 * 8 * 256, small_q.text.vocab // 2), (17, 64))    # LMQ_WAVES = 8, LMQ_GRID = 256 (dec_quant.hip)


def test_ties_pick_the_lower_copy_tiny_generic_head(tiny):
    V = tiny.text.vocab
    _ties(tiny, [p for p in (1, 4, 16, 64, V // 2) if 2 * p <= V], (17, 64))


# ---- 2.4 the decode-step knobs nobody sets ----------------------------------------------------------------------------------------------
BIT_EQUAL = [("gemv_xbar", 0), ("gemv_xbar", 1), ("gemv_xbar", 2), ("gemv_xbar", 3), ("gemv_earlyw", 0), ("gemv_earlyw", 2), ("gemv_earlyw", 3),
             ("gemv_nt", 1), ("lmh_nt", 0), ("lmh_order", 0)]
BIT_EQUAL_DA = [("da_unr", 1), ("da_spec", 0), ("da_spec", 1), ("da_spec", 2), ("da_earlyq", 1)]       # stand-alone attention: under qa = 0
ORACLE_BARS = [("gemv_splitb", 0), ("gemv_splitb", 1), ("gemv_w1024", 4), ("gemv_partial", 0)]
ORACLE_BARS_DA = [("da_waves", 16)]
DEFAULTS = {"gemv_xbar": 4, "gemv_splitb": 2, "gemv_w1024": 8, "gemv_partial": 1, "gemv_earlyw": 1, "gemv_nt": 0, "lmh_nt": 1, "lmh_order": 1,
            "da_unr": 2, "da_waves": 8, "da_spec": 3, "da_earlyq": 0, "qa": 1, "decode_split": 1, "decode_gran": 16}


@pytest.mark.parametrize("B", [8, 17, 32])
def test_decode_step_knobs(small, B):
    eng, rows = small.eng, list(range(B))
    for k, v in DEFAULTS.items():
        assert eng.get_tuning(k) == v, (k, v)                  # the table above is the library's
    try:
        base = small.run(rows, n_steps=3)
        eng.set_tuning("qa", 0)
        base_da = small.run(rows, n_steps=3)
        for s in range(4):
            assert np.array_equal(base[s], base_da[s]), ("qa 0 vs 1", s)      # test_gpu_chain.py holds the fused launch to the two launches' bits
        for knobs, qa, bit in ((BIT_EQUAL, 1, True), (BIT_EQUAL_DA, 0, True), (ORACLE_BARS, 1, False), (ORACLE_BARS_DA, 0, False)):
            eng.set_tuning("qa", qa)
            for key, val in knobs:
                eng.set_tuning(key, val)
                try:
                    got = small.run(rows, n_steps=3)
                finally:
                    eng.set_tuning(key, DEFAULTS[key])
                same = all(np.array_equal(got[s], base[s]) for s in range(4))
                if bit:
                    assert same, (key, val, B, max(float(np.abs(got[s] - base[s]).max()) for s in range(4)))
                else:
                    print(f"[knobs] {key} = {val} at {B} rows: {'bit-equal to' if same else 'differs from'} the default")
                    small.compare(rows, got, f"{key}={val} B={B}")
    finally:
        for k, v in DEFAULTS.items():
            eng.set_tuning(k, v)


@pytest.mark.parametrize("B", [17, 32, 64])
def test_decode_row_groups_on_parallel_branches(small, B):
    """decode_split 2 / 4 (decode_gran 16) exist on the greedy path only: same tokens as one row group, and each is the first maximum of the
    logits of its row."""
    eng = small.eng
    want = _argmax_identity(small, B)
    try:
        eng.set_tuning("decode_gran", 16)
        for split in (2, 4):
            eng.set_tuning("decode_split", split)
            assert _argmax_identity(small, B) == want, (split, B)
    finally:
        eng.set_tuning("decode_split", 1)
        eng.set_tuning("decode_gran", 16)


# ---- 3 the 1.7B widths at more than 32 rows, and the entry points' refusals --------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 8], ids=["bf16", "w8"])
def test_1p7b_engine_created_for_64_rows_serves_33_and_64(large, bits):
    r = large if not bits else _large_rig(bits)
    try:
        for B in (33, 64):
            toks = _argmax_identity(r, B)
            assert len({tuple(t) for t in toks}) > 1
            for k in (0, 31, 32, B - 1):                        # a row of each LM-head block equals the clip alone
                assert r.eng.transcribe_batch([r.clips[k]], max_tokens=6, ignore_eos=True)[0] == toks[k], (B, k)
        if bits:
            _every_row(r, 33)
    finally:
        if bits:
            r.close()


def test_entry_points_refuse_what_they_cannot_serve(tiny):
    V = tiny.text.vocab
    fresh = gpu_util.Engine("tiny", max_batch=2, max_audio_seconds=2, max_new_tokens=4)
    try:
        buf = np.zeros((2, V), np.float32)
        tok = np.zeros(2, np.int32)
        assert fresh.lib.qasr_batch_prefill_logits(fresh.h, gpu_util.fptr(buf)) != 0             # nothing loaded
        fresh.load_state_dict(tiny.sd)
        assert fresh.lib.qasr_batch_prefill_logits(fresh.h, gpu_util.fptr(buf)) == 1             # no prepared batch: QASR_ERR_INVALID
        assert fresh.lib.qasr_batch_decode_forced(fresh.h, gpu_util.iptr(tok), gpu_util.fptr(buf)) == 1
        assert fresh.lib.qasr_batch_prefill_logits(fresh.h, None) == 1
        clips = [tiny.clips[1][:16000], tiny.clips[2][:9000]]
        fresh.transcribe_batch(clips, max_tokens=2, ignore_eos=True)
        assert fresh.lib.qasr_batch_decode_forced(fresh.h, gpu_util.iptr(tok), gpu_util.fptr(buf)) == 1   # a greedy run is no prompt pass with logits
        fresh.batch_prefill_logits(clips)
        with pytest.raises(RuntimeError, match="out of range"):
            fresh.batch_decode_forced([3, V])
        with pytest.raises(RuntimeError, match="out of range"):
            fresh.batch_decode_forced([-1, 3])
        with pytest.raises(RuntimeError, match="qasr error 5.*cache capacity"):                     # QASR_ERR_CAPACITY, not a write past the cache
            for _ in range(2048):
                fresh.batch_decode_forced([3, 4])
        a = fresh.batch_prefill_logits(clips)                   # and the engine still serves
        assert np.array_equal(a, fresh.batch_prefill_logits(clips))
    finally:
        fresh.close()

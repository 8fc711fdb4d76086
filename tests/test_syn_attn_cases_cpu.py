"""What the network tests of the synthesis stacks cannot see (step 0), the float64 references of tests/syn_attn_cases.py against the oracles'
own attention, the f32 twins inside the bounds on every GPU case's inputs, and the mutation condition: tests/test_gpu_syn_attn_cases.py
cannot pass while blind to a dropped edge key, a key admitted past the set, the wrong K/V head, a wrong wave's running maximum, a missing
rescale, a wrong RoPE pairing, swapped cos / sin, a misplaced append or a neighbour's norm statistics.  No GPU.

Measured here: STEP0 and MEASURED_CPU below.

Exempt from the mutation condition, because no input can show them:
  * a drop that leaves a row without any key (pos 0, S = 1) gives NaN, which the GPU tests refuse as such: counted as seen;
  * the wrong K/V head `head % kv_heads` equals `head / rep` at rep 1 and at one K/V head: cvlm (2, 2) and (16, 1), cp (2, 2) and (4, 1),
    vl (4, 4) and (8, 1);
  * a wrong wave's maximum needs a head h + 4 (rep > 4: cvlm (14, 2) and (16, 1)) and, like a missing rescale, a second round (pos >= 256);
  * the key admitted past the last row of a cache (cvlm pos = max_ctx - 1 in the last kv head of the last slot, cp pos 15) and past the last
    sequence of a vl launch lies outside every array;
  * RoPE pairing d with d + 1 at position 0, where nothing rotates (cvlm and cp rows at pos 0); any defect of q, and of k in vl, where
    there is one key, whose weight is 1 whatever the score (cp pos 0, vl S = 1);
  * the norm with the neighbouring head's statistics where there is one head (cp k at one K/V head); the append "into slot 0" for a row that
    is in slot 0, "at pos - 1" is checked for every row (pos 0 lands in the cache row before the slot's or kv head's first).
"""
import json
import math
import types
import numpy as np
import pytest
import torch
import attn_cases as A
import syn_attn_cases as S
from gemm_cases import bf16_bits, bf16_from_bits, bf16_round, randn_bf16, ulp_bf16

STEP0 = """max |d| / peak of the float64 oracle against itself with a wrong key set, beside the bound of the stack's network test on the GPU.
CosyVoice LLM (real4, row 8, prefix 250, 24 forced tokens; bound logits 5.8e-2 / hidden 5.2e-2): ALL UNDER THE BOUND (asserted):
    own key dropped at every position             logits 3.1e-2   hidden 4.2e-2
    key 256 dropped for all later queries         logits 3.4e-2   hidden 2.5e-2
    key 255 dropped once a second round exists    logits 2.9e-2   hidden 3.7e-2
    own key dropped when it opens a 64-key chunk  logits 2.1e-3   hidden 7.8e-3
Code predictor (small4, row 0, 24 frames; bound 5.7e-2 of the cp logits' peak): own key dropped at every position 5.2e-1: VISIBLE to
test_gpu_talker.py, nine times its bound (16 keys at most, so one key carries a large share of the weight).
VoxCPM2 stacks (d2; bounds 1.2e-2 .. 1.5e-2): last key dropped 2.4e-1 (LocEnc stack S 11), 2.7e-1 (LocDiT stack), 2.4e-1 (velocity), 4.5e-1 /
5.4e-1 (encode cls / embed); the next sequence's first key admitted 2.3e-1, 2.6e-1, 2.5e-1, 2.0e-1 / 2.3e-1: VISIBLE to test_gpu_vloc.py, 13
to 36 times its bound.  So of the three stacks only the CosyVoice LLM's network test is blind to a wrong key set; what the other two could
not see is a defect on ONE edge (a single position, head, chunk or sequence boundary) of a geometry their checkpoints do not have, and a
wrong byte outside the rows a launch owns: the isolated tests hold both."""
MEASURED_CPU = """f32 twins as fractions of the bound: cvlm attention <= 0.949 (every geometry 0.91 .. 0.95; prompt chunk 0.933), cvlm writer
1.000 (one ulp of the final rounding); cp attention <= 0.918, cp writer 1.000; vl <= 0.008 (the bound grants every one of the 128 fmaf
steps of a score its worst case, 128 x 2^-23 of sum |q k|; roundings that do not conspire stay far below it; the vl twin runs on the
first three sequences of a launch, which are independent and built alike).
Weakest mutation, over all cases, rows and mutations: cvlm 23.2 x the bound (the row behind pos = max_ctx - 1 admitted, where that row is
the next kv head's Gaussian key 0; every dropped edge key, wrong K/V head, wrong wave, missing rescale and writer defect >= 397 x), prompt
chunk 424 x (l not rescaled), cp 112 x, vl 87.7 x."""


def _seen(mv, v, bound):
    """per leading row: the largest |mutated - true| / bound, NaN (no key left, or a NaN admitted) counted as seen"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(mv - v) / bound
    d[np.isnan(d)] = np.inf
    return d.reshape(d.shape[0], -1).max(1)


# ---- step 0: how blind the network tests are --------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def test_step0_cvlm_network_test_is_blind_to_mask_defects():
    """tests/cvlm_oracle.py at float64 against itself with a mutated mask, geometry real4, row 8 of cvlm_cases.make_rows (prefix 250: the 24
    forced tokens cross the 256-key round edge), as max |d| / peak beside the bound of test_forced_logits_against_the_oracle"""
    import cvlm_cases as K
    import cvlm_oracle as O
    from qasr import synth
    g = K.GEOMETRIES["real4"]
    W = O.Weights(synth.synth_cosyvoice_llm_state_dict(g, 0), g)
    n = K.N_ROWS["real4"]
    row, toks = K.make_rows(n, g)[8], K.forced_tokens(n, K.FORCED_T, g)[8]
    assert K.prefix_len(row) == 250
    ref = O.forced_pass(row, toks, W, O.F64)

    def own(m):
        m = m | torch.eye(m.shape[0], dtype=torch.bool)
        m[0, 0] = False
        return m

    def key256(m):
        m = m.clone()
        m[257:, 256] = True
        return m

    def key255(m):
        m = m.clone()
        m[256:, 255] = True
        return m

    def chunk_open(m):
        m = m.clone()
        for i in range(64, m.shape[0], 64):
            m[i, i] = True
        return m
    bound = {k: K.MARGIN * K.TWIN["real4"][k] for k in ("logits", "hidden")}
    for name, edit in (("own key dropped at every position", own), ("key 256 dropped for all later queries", key256),
                       ("key 255 dropped once a second round exists", key255), ("own key dropped when it opens a 64-key chunk", chunk_open)):
        got = O.forced_pass(row, toks, W, O.F64, mask_edit=edit)
        d = {k: _rel(got[k], ref[k]) for k in bound}
        print(f"step 0 cvlm: {name}: logits {d['logits']:.1e} hidden {d['hidden']:.1e} | bound {bound['logits']:.1e} / {bound['hidden']:.1e}")
        assert 0.0 < d["logits"] < bound["logits"] and 0.0 < d["hidden"] < bound["hidden"], (name, d)


def test_step0_talker_and_vloc_figures():
    """the same measurement on the other two oracles, printed beside their suites' GPU bounds; nothing asserted but that a figure exists"""
    import talker_cases as TK
    import talker_oracle as TO
    import vloc_cases as VC
    import vloc_oracle as VO
    from qasr import synth
    g = TK.GEOMETRIES["small4"]
    W = TO.Weights(synth.synth_tts_talker_state_dict(g, 0), g)
    n = TK.N_ROWS["small4"]
    row, codes = TK.make_rows(n, g["hidden"])[0], TK.forced_codes(n, TK.FORCED_T)[0]
    ref = TO.forced_pass(row, codes, W, TO.F64, TK.TOKENS)
    hn = torch.from_numpy(ref["hidden"])

    def own(m):
        m = m | torch.eye(m.shape[0], dtype=torch.bool)
        m[0, 0] = False
        return m
    with torch.no_grad():
        got = TO.cp_pass(hn, np.asarray(codes).T, W, TO.F64, mask_edit=own).numpy()
    d = _rel(got, ref["cp"])
    print(f"step 0 code predictor: own key dropped: cp logits {d:.1e} | bound {TK.MARGIN * TK.TWIN['small4']['cp']:.1e}")
    assert d > 0.0
    for name in ("stack/enc/S11n7L2", "stack/dit/S11n7L2", "velocity/B2t0.37", "encode/n13"):
        ref = VC.reference(name)
        for what, edit in (("last key dropped", lambda k, v: (k[:, :-1], v[:, :-1])),
                           ("next sequence's first key admitted", lambda k, v: (np.concatenate([k, np.roll(k[:, :1], -1, 0)], 1),
                                                                                np.concatenate([v, np.roll(v[:, :1], -1, 0)], 1)))):
            m = VO.Model(VC.stored("d2"), VC.GEOMS["d2"])
            m.kv_edit = edit
            got = VC.run(m, name)
            for k in ref:
                if k != "least":
                    d = VO.rel(got[k], ref[k])
                    print(f"step 0 vloc: {name}/{k}: {what}: {d:.1e} | bound {VC.MARGIN * VC.TWIN[name + '/' + k]:.1e}")
                    assert d > 0.0


# ---- the references against the oracles' own attention ------------------------------------------------------------------------------------------
def test_vl_tables_equal_what_the_product_uploads(tmp_path):
    from qasr import voxcpm
    for long in (False, True):
        lm = {"rope_theta": 10000.0}
        if long:
            lm.update(max_position_embeddings=S.VL_LONG["max_pos"],
                      rope_scaling={"original_max_position_embeddings": S.VL_LONG["orig"], "long_factor": S.VL_LONG["long_factor"], "short_factor": [1.0] * 64})
        d = tmp_path / ("long" if long else "plain")
        d.mkdir()
        (d / "config.json").write_text(json.dumps({"lm_config": lm}))
        cos, sin = voxcpm.rope_table(d, 128, 32)
        want = S.vl_tables(long)
        assert np.array_equal(np.asarray(cos, np.float32), want[0]) and np.array_equal(np.asarray(sin, np.float32), want[1]), long
    assert not np.array_equal(S.vl_tables(True)[0], S.vl_tables(False)[0]) and S.vl_tables(True)[0][0, 0] > 1.0


def test_cvlm_reference_against_the_oracle_formulation():
    """rope_ref against oracle.decoder.rope (no rounding), attn_f32p against torch's float64 attention over the rows' key sets; and the
    round schedule of cvlm_twin in float64 without a defect is the plain softmax"""
    from oracle import decoder
    rng = np.random.default_rng(3)
    pos = np.array([0, 5, 63, 64, 255, 256, 300])
    x = randn_bf16(rng, (len(pos), 3, 64))
    cos, sin = A.rope_tables(S.CVLM_THETA, 32, 320)
    o, bound = S.rope_ref(x, cos[pos][:, None], sin[pos][:, None])
    want = decoder.rope(torch.tensor(x, dtype=torch.float64), torch.tensor(pos), S.CVLM_THETA).numpy()
    mag = np.abs(want) + np.abs(np.roll(want, 32, -1))
    assert (np.abs(o - want) <= 0.5 * ulp_bf16(want) + 320 * 2.0 ** -22 * mag + 1e-12).all()
    assert (bound >= ulp_bf16(o)).all()
    q, K, V = randn_bf16(rng, (7, 64)), randn_bf16(rng, (301, 64)), randn_bf16(rng, (301, 64))
    t = lambda a: torch.tensor(a, dtype=torch.float64)[None]
    for n in (1, 64, 257, 301):
        got, b = S.attn_f32p(q, K[:n], V[:n], 0.125)
        want = torch.nn.functional.scaled_dot_product_attention(t(q), t(K[:n]), t(V[:n]))[0].numpy()
        assert np.abs(got - want).max() <= 1e-13 and (b >= 0.5 * ulp_bf16(got)).all()
        assert np.abs(S.cvlm_twin(q, K[:n], V[:n], None, np.float64) - want).max() <= 1e-13


def test_cp_reference_against_the_oracle_formulation():
    """the code predictor's q / k / attention as tests/talker_oracle.py states them (rms, rope, softmax at float64) lie within the writer's
    three roundings of the reference; the attention over equal q / K / V is the same to 1e-13"""
    import talker_oracle as TO
    rng = np.random.default_rng(4)
    x, w = randn_bf16(rng, (5, 3, 128)), bf16_round(1.0 + 0.1 * rng.standard_normal(128))
    cos, sin = S.cp_tables()
    o, bound, _ = A.norm_rope_ref(x, w, cos[7], sin[7], S.CP_EPS)
    y = TO.rms(torch.tensor(x, dtype=torch.float64), torch.tensor(w, dtype=torch.float64), S.CP_EPS, TO.F64).numpy()
    c64, s64 = (a.numpy()[0] for a in TO.rope_tables(S.CP_THETA, 64, [7], TO.F64))
    want = np.concatenate([y[..., :64] * c64 - y[..., 64:] * s64, y[..., :64] * s64 + y[..., 64:] * c64], -1)
    mag = np.abs(want) + np.abs(np.roll(want, 64, -1))
    assert (np.abs(o - want) <= 2.0 ** -7 * mag + 0.5 * ulp_bf16(want) + 16 * 2.0 ** -22 * mag).all()
    q, K, V = randn_bf16(rng, (1, 128)), randn_bf16(rng, (16, 128)), randn_bf16(rng, (16, 128))
    for n in (1, 2, 16):
        got, _ = S.attn_f32p(q, K[:n], V[:n], 1.0 / math.sqrt(128.0))
        sc = torch.tensor(q @ K[:n].T / math.sqrt(128.0))
        e = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        want = ((e @ torch.tensor(V[:n])) / e.sum(dim=-1, keepdim=True)).numpy()
        assert np.abs(got - want).max() <= 1e-13


def test_vl_reference_against_the_oracle_formulation():
    """vl_expect against the layer of tests/vloc_oracle.py: its rope (rotate-half on [cos | cos]), its head map (np.repeat) and its softmax"""
    import vloc_oracle as VO
    inp = S.vl_inputs(11, 8, 2, 3, "gauss")
    got, bound = S.vl_expect(inp)
    ns = types.SimpleNamespace(cos=inp["cos"].astype(np.float64), sin=inp["sin"].astype(np.float64))
    x = inp["qkv"].astype(np.float64)
    q, k, v = VO.Model.rope(ns, x[:, :, :8]), VO.Model.rope(ns, x[:, :, 8:10]), x[:, :, 10:]
    k, v = np.repeat(k, 4, axis=2), np.repeat(v, 4, axis=2)
    sc = np.einsum("nihd,njhd->nhij", q, k) * float(S.VL_SCALE)
    sc = np.exp(sc - sc.max(axis=-1, keepdims=True))
    want = np.einsum("nhij,njhd->nihd", sc / sc.sum(axis=-1, keepdims=True), v)
    assert np.abs(got - want).max() <= 1e-13 and (bound > 0).all() and (bound < 1e-3).all()


# ---- cvlm: twins and mutations -------------------------------------------------------------------------------------------------------------------
def _cvlm_written(inp):
    """the reference's own writer output as the device's: (q, caches K / V as values with the appended rows, images K / V as bits)"""
    q, _, k, _, v = S.cvlm_writer_expect(inp)
    Kb, Vb = inp["Kbits"].copy(), inp["Vbits"].copy()
    for r in range(len(inp["pos"])):
        Kb[inp["slot"][r], :, inp["pos"][r]], Vb[inp["slot"][r], :, inp["pos"][r]] = bf16_bits(k[r]), bf16_bits(v[r])
    with np.errstate(invalid="ignore"):
        return q, bf16_from_bits(Kb), bf16_from_bits(Vb), Kb, Vb


def _cvlm_case(inp, kind, edge, edges_of, stats, targeted):
    """one input set: twins, and the mutations this set is meant to show.  edges_of(r) = the row's edge-key list; targeted = the edge-list
    index the set spikes (None for gauss: every mutation is evaluated)"""
    rows, heads, kv = len(inp["pos"]), inp["heads"], inp["kv_heads"]
    rep = heads // kv
    q, K, V, Kb, Vb = _cvlm_written(inp)
    want, bound = S.cvlm_attn_expect(inp, q, K, V)
    # twins: the writer and the attention schedule
    _, qb, k, kb, _ = S.cvlm_writer_expect(inp)
    c, s = inp["cos"][inp["pos"]][:, None], inp["sin"][inp["pos"]][:, None]
    stats["writer"] = max(stats.get("writer", 0.0), S.frac(S.rope_twin(inp["qkv"][:, :heads], c, s), q, qb),
                          S.frac(S.rope_twin(inp["qkv"][:, heads:heads + kv], c, s), k, kb))
    for r in range(rows):
        p, sl = int(inp["pos"][r]), int(inp["slot"][r])
        for g in range(kv):
            hs = slice(g * rep, (g + 1) * rep)
            tw = S.cvlm_twin(q[r, hs], K[sl, g, :p + 1], V[sl, g, :p + 1])
            stats["twin"] = max(stats.get("twin", 0.0), S.frac(tw, want[r, hs], bound[r, hs]))
    seen = stats["seen"]

    def note(name, val, rws=None):
        idx = np.arange(rows) if rws is None else np.asarray(rws)
        if name not in seen:                                   # rows the mutation does not apply to are exempt
            seen[name] = np.full(rows, np.inf)
            seen[name][idx] = 0.0
        a = seen[name]
        a[idx] = np.maximum(a[idx], val[idx])
    n_edge = max(len(edges_of(r)) for r in range(rows))
    for m in (range(n_edge) if targeted is None else [targeted]):
        drop = [edges_of(r)[m % len(edges_of(r))] for r in range(rows)]
        drop = [d if isinstance(d, (int, np.integer)) else (int(inp["pos"][r]) if d == "own" else None) for r, d in enumerate(drop)]
        val = _seen(S.cvlm_attn_expect(inp, q, K, V, drop=drop)[0], want, bound)
        for r in range(rows):
            if drop[r] is None or drop[r] > inp["pos"][r]:
                val[r] = np.inf                                # the key is not in this row's set
        note(f"drop{m}", val)
    if targeted is None or (edges_of(0)[targeted % len(edges_of(0))] == "next"):
        mv = S.cvlm_attn_expect(inp, q, K, V, admit=True)[0]
        note("admit", _seen(mv, want, bound))
    big = [r for r in range(rows) if inp["pos"][r] >= S.ROUND]
    if big:
        for mut in (("wave", "no_o", "no_l") if rep > 4 else ("no_o", "no_l")):
            note(mut, _seen(S.cvlm_attn_expect(inp, q, K, V, mut=mut, rows=big)[0], want, bound), big)
    if targeted is None:
        if rep > 1 and kv > 1:
            note("kvmap", _seen(S.cvlm_attn_expect(inp, q, K, V, kvmap="mod")[0], want, bound))
        for mut in ("pair", "swap_hi"):
            mq, _, mk, _, _ = S.cvlm_writer_expect(inp, mut)
            live = [r for r in range(rows) if mut != "pair" or inp["pos"][r] > 0]     # position 0 does not rotate
            note("q " + mut, _seen(mq, q, qb), live)
            note("k " + mut, _seen(mk, k, kb), live)
        # a misplaced append breaks the whole-image comparison
        for name, at in (("pos - 1", (inp["slot"], inp["pos"] - 1)), ("slot 0", (np.zeros_like(inp["slot"]), inp["pos"]))):
            Km, Vm = inp["Kbits"].reshape(-1, 64).copy(), inp["Vbits"].reshape(-1, 64).copy()
            for r in range(rows):
                for g in range(kv):
                    i = (at[0][r] * kv + g) * inp["max_ctx"] + at[1][r]
                    Km[i], Vm[i] = bf16_bits(k[r, g]), bf16_bits(inp["qkv"][r, heads + kv + g])
            wantK, wantV, _ = S.cvlm_cache_expect(inp, Km.reshape(Kb.shape), Vm.reshape(Vb.shape))
            assert not np.array_equal(wantK, Km.reshape(Kb.shape)) or not np.array_equal(wantV, Vm.reshape(Vb.shape)), name
        wantK, wantV, _ = S.cvlm_cache_expect(inp, Kb, Vb)
        assert np.array_equal(wantK, Kb) and np.array_equal(wantV, Vb)


def _cvlm_finish(name, stats):
    weakest = min(float(v.min()) for v in stats["seen"].values())
    print(f"{name}: twin {stats['twin']:.3f}, writer twin {stats['writer']:.3f} of the bound; weakest mutation {weakest:.1f} x the bound "
          f"({min(stats['seen'], key=lambda k: stats['seen'][k].min())})")
    assert stats["twin"] <= 1.0 and stats["writer"] <= 1.0, stats
    for k, v in stats["seen"].items():
        assert (v >= 10.0).all(), (k, v)


@pytest.mark.parametrize("max_ctx", [320, 544])
@pytest.mark.parametrize("heads,kv", S.CVLM_GEOMS)
def test_cvlm_twin_and_mutations(heads, kv, max_ctx):
    for poss in S.cvlm_batches(max_ctx):
        stats = {"seen": {}}
        for kind, edge in S.cvlm_sets(poss):
            inp = S.cvlm_inputs(heads, kv, max_ctx, poss, kind, edge)
            _cvlm_case(inp, kind, edge, lambda r: S.cvlm_edge_keys(int(inp["pos"][r])), stats, None if kind == "gauss" else edge)
        _cvlm_finish(f"cvlm heads {heads} kv {kv} max_ctx {max_ctx} pos {poss}", stats)


def test_cvlm_prompt_chunk_twin_and_mutations():
    stats = {"seen": {}}
    for kind, edge in S.chunk_sets():
        inp = S.chunk_inputs(kind, edge)
        _cvlm_case(inp, kind, edge, lambda r: list(S.CHUNK_EDGES), stats, None if kind == "gauss" else edge)
    stats["seen"].pop("drop1")                                 # "next" is an admitted key, not a dropped one
    stats["seen"]["admit"][-1] = np.inf                        # behind the last row lies a NaN pattern: seen as such
    _cvlm_finish("cvlm prompt chunk", stats)


# ---- code predictor: twins and mutations ---------------------------------------------------------------------------------------------------------
def _cp_written(inp):
    k, kb, v = S.cp_writer_expect(inp)
    Kb, Vb = inp["Kbits"].copy(), inp["Vbits"].copy()
    Kb[:inp["B"], :, inp["pos"]], Vb[:inp["B"], :, inp["pos"]] = bf16_bits(k), bf16_bits(v)
    with np.errstate(invalid="ignore"):
        return bf16_from_bits(Kb), bf16_from_bits(Vb), Kb, Vb


def _cp_case(inp, stats, targeted, seen):
    heads, kv, B, pos = inp["heads"], inp["kv_heads"], inp["B"], inp["pos"]
    rep = heads // kv
    K, V, Kb, Vb = _cp_written(inp)
    want, bound = S.cp_attn_expect(inp, K, V)
    k, kb, _ = S.cp_writer_expect(inp)
    x = inp["qkv"]
    tw_k = A.norm_rope_twin(x[:, heads:heads + kv], inp["kn_w"], inp["cos"][pos], inp["sin"][pos], inp["eps"])
    stats["writer"] = max(stats.get("writer", 0.0), S.frac(tw_k, k, kb))
    tw_q = A.norm_rope_twin(x[:, :heads], inp["qn_w"], inp["cos"][pos], inp["sin"][pos], inp["eps"])
    for b in range(B):
        for h in range(heads):
            tw = S.cp_twin(tw_q[b, h], K[b, h // rep, :pos + 1], V[b, h // rep, :pos + 1])
            stats["twin"] = max(stats.get("twin", 0.0), S.frac(tw, want[b, h], bound[b, h]))

    def note(name, val):
        seen[name] = np.maximum(seen.get(name, np.zeros(B)), val)
    ek = S.cp_edge_keys(pos)
    for m in (range(len(ek)) if targeted is None else [targeted % len(ek)]):
        note(f"drop key {ek[m]}", _seen(S.cp_attn_expect(inp, K, V, drop=m)[0], want, bound))
    if targeted is None:
        if pos < 15:
            note("admit", _seen(S.cp_attn_expect(inp, K, V, admit=True)[0], want, bound))
        if rep > 1 and kv > 1:
            note("kvmap", _seen(S.cp_attn_expect(inp, K, V, kvmap="mod")[0], want, bound))
        for mut in ("pair", "swap_hi", "neighbour"):
            if pos:                                            # with one key the weight is 1 whatever q is
                note("q " + mut, _seen(S.cp_attn_expect(inp, K, V, qmut=mut)[0], want, bound))
            if (mut != "neighbour" or kv > 1) and (mut != "pair" or pos):       # position 0 does not rotate
                note("k " + mut, _seen(S.cp_writer_expect(inp, mut)[0], k, kb))
    return Kb, Vb


@pytest.mark.parametrize("B", S.CP_B)
@pytest.mark.parametrize("heads,kv", S.CP_GEOMS)
def test_cp_twin_and_mutations(heads, kv, B):
    stats, weakest = {}, np.inf
    for pos in range(16):                                      # the single launches: every mutation at every pos
        seen = {}
        for kind, edge in S.cp_sets(pos):
            _cp_case(S.cp_inputs(heads, kv, B, pos, kind, edge), stats, None if kind == "gauss" else edge, seen)
        for k, v in seen.items():
            assert (v >= 10.0).all(), (pos, k, v)
            weakest = min(weakest, float(v.min()))
    for kind, edge in (("gauss", 0), ("spike", "own")):        # the sequence: the twins over the caches the reference writer leaves
        carry = None
        for pos in range(16):
            inp = S.cp_inputs(heads, kv, B, pos, kind, edge, fresh=True)
            if carry is not None:
                inp["Kbits"], inp["Vbits"] = carry
            seen = {}
            carry = _cp_case(inp, stats, len(S.cp_edge_keys(pos)) - 1, seen)        # the last edge key is the row's own
            if kind == "spike":
                assert (seen[f"drop key {pos}"] >= 10.0).all(), (pos, seen)
    print(f"cp heads {heads} kv {kv} B {B}: twin {stats['twin']:.3f}, writer twin {stats['writer']:.3f} of the bound; weakest mutation {weakest:.1f} x the bound")
    assert stats["twin"] <= 1.0 and stats["writer"] <= 1.0, stats


# ---- vl: twins and mutations ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kv", S.VL_GEOMS)
def test_vl_twin_and_mutations(heads, kv):
    worst, weakest = 0.0, np.inf
    for Sq in range(1, 33):
        for n_seq in S.VL_NSEQ:
            seen = {}
            for kind, edge in S.VL_SETS:
                inp = S.vl_inputs(Sq, heads, kv, n_seq, kind, edge)
                want, bound = S.vl_expect(inp)
                worst = max(worst, S.frac(S.vl_twin(inp, 3), want[:3], bound[:3]))     # sequences are independent and built alike: three of nine
                muts = {}
                if kind == "gauss" or edge == 0:
                    muts["drop key 0"] = dict(drop=0)
                if kind == "gauss" or edge == 1:
                    muts["drop key S - 1"] = dict(drop=Sq - 1)
                if n_seq > 1 and (kind == "gauss" or edge == 2):
                    muts["admit"] = dict(admit=True)
                if kind == "gauss":
                    if Sq > 1:                                  # with one key the weight is 1 whatever q and k are
                        muts.update({"pair": dict(rope_mut="pair"), "swap_hi": dict(rope_mut="swap_hi")})
                    if kv > 1 and heads > kv:
                        muts["kvmap"] = dict(kvmap="mod")
                for name, kw in muts.items():
                    mv = S.vl_expect(inp, **kw)[0]
                    if name == "admit":
                        mv, w, b = mv[:-1], want[:-1], bound[:-1]      # the last sequence has nothing behind it
                    else:
                        w, b = want, bound
                    val = _seen(mv.reshape(-1, *mv.shape[2:]), w.reshape(-1, *w.shape[2:]), b.reshape(-1, *b.shape[2:]))
                    seen[name] = np.maximum(seen.get(name, 0.0), val)
            for k, v in seen.items():
                assert (v >= 10.0).all(), (Sq, n_seq, k, float(v.min()))
                weakest = min(weakest, float(v.min()))
    print(f"vl heads {heads} kv {kv}: twin {worst:.3f} of the bound; weakest mutation over all rows {weakest:.1f} x the bound")
    assert worst <= 1.0, worst

"""The float64 references of tests/attn_cases.py against independent formulations, the fragment image's round trip, the f32 twins inside the
bounds on every GPU case's inputs (decode, prompt, hand-over), and the mutation condition: the GPU tests cannot pass while blind to a
dropped edge key, to a key admitted past the context (decode) or to a causal edge off by one (prompt).  No GPU.

Measured here: MEASURED_CPU below.
At a context of 0 the admitted decode row is the token's own key and value a second time, which no input can show: that one entry is
exempt.  So is the prompt's last row with the key after it admitted: that key lies outside the clip, in no input of the reference.
"""
import numpy as np
import pytest
import torch
import attn_cases as A
from gemm_cases import bf16_round, randn_bf16, ulp_bf16
from oracle import decoder, precision as P

MEASURED_CPU = """f32 twins as fractions of the bound: decode <= 0.722 (head_dim 32: 0.33 .. 0.72, head_dim 128: 0.32 .. 0.72,
nine rows x 8 kv heads 0.722), prompt <= 0.920 (head_dim 32: 0.713, head_dim 128: 0.851 at 2 kv heads, 0.920 at 8), hand-over 0.226 / 0.191,
writers 1.000 (one ulp of the final rounding).  Weakest mutation: decode 22.6 x the bound over all cases and edge keys, prompt 129 x over all
cases, mutations and query rows."""
NINE_ROWS = (128, 8, 544, (0, 1, 31, 32, 33, 255, 256, 513, 543))
DECODE_CASES = [(hd, 2, mc, lens) for hd in (32, 128) for mc in (544, 1056) for lens in A.decode_batches(mc)] + [NINE_ROWS]
PROMPT_CASES = [(hd, kv, clips) for hd, kv in ((32, 2), (128, 2), (128, 8)) for clips in A.PROMPT_CLIPS]


def test_vfrag_round_trip_and_append():
    rng = np.random.default_rng(0)
    for hd in (32, 128):
        V = rng.integers(0, 65536, (96, hd)).astype(np.uint16)
        img = A.vfrag_pack(V)
        assert np.array_equal(A.vfrag_unpack(img, hd), V)
        # the layout statement itself, element by element
        for key, d in ((0, 0), (5, 17), (31, hd - 1), (32, 3), (77, 16), (95, hd - 1)):
            r = key % 32
            half, g, j = r // 16, (r % 16) // 4, r % 4
            idx = (((key // 32) * (hd // 16) + d // 16) * 64 + d % 16 + 16 * g) * 8 + half * 4 + j
            assert img[idx] == V[key, d]
        # a prompt of T keys with one key appended = the image of T + 1 keys
        for T in (33, 64):
            a = np.zeros((96, hd), np.uint16)
            a[:T] = V[:T]
            img_t = A.vfrag_pack(a)
            where = A.vfrag_pack(np.arange(96 * hd).reshape(96, hd))
            img_t[np.isin(where, T * hd + np.arange(hd))] = V[T][where[np.isin(where, T * hd + np.arange(hd))] - T * hd]
            a[T] = V[T]
            assert np.array_equal(img_t, A.vfrag_pack(a))


@pytest.mark.parametrize("hd", [32, 128])
def test_norm_rope_against_oracle(hd):
    """oracle.decoder.rms_norm + rope at policy F32 have no inner roundings: the reference lies within the three bf16 roundings of it"""
    rng = np.random.default_rng(hd)
    theta, eps, n = 10000.0, 1e-6, 40
    x, w = randn_bf16(rng, (n, 3, hd)), bf16_round(1.0 + 0.1 * rng.standard_normal(hd))
    pos = rng.integers(0, 1056, n)
    cos, sin = A.rope_tables(theta, hd // 2, 1056)
    o, bound, _ = A.norm_rope_ref(x, w, cos[pos][:, None], sin[pos][:, None], eps)
    y = decoder.rms_norm(torch.tensor(x, dtype=torch.float64), torch.tensor(w, dtype=torch.float64), eps, P.F32)
    want = decoder.rope(y, torch.tensor(pos), theta).numpy()
    mag = np.abs(want) + np.abs(np.roll(want, hd // 2, -1))
    # two inner roundings of 2^-9 relative each on both members of the pair, the final half ulp, and the f32 angles of the oracle (p 2^-23)
    tol = 2.0 ** -7 * mag + 0.5 * ulp_bf16(want) + 1056 * 2.0 ** -22 * mag
    assert (np.abs(o - want) <= tol).all(), float((np.abs(o - want) / tol).max())
    assert (bound >= ulp_bf16(o)).all()


@pytest.mark.parametrize("hd,kv", [(32, 2), (128, 2), (128, 8)])
def test_writer_twin_inside_bound(hd, kv):
    """the f32 twin of norm + rope on every prompt case's inputs, cancelling rotations included (|o| down to 4e-7 beside terms of 1)"""
    worst = 0.0
    for clips in A.PROMPT_CLIPS:
        for kind, spike in A.prompt_sets(clips):
            inp = A.prompt_inputs(hd, kv, clips, kind, spike)
            cos, sin = A.rope_tables(inp["theta"], hd // 2, inp["max_ctx"])
            c, s = cos[inp["pos"]][:, None], sin[inp["pos"]][:, None]
            for lo, hi, w in ((0, inp["heads"], inp["qn_w"]), (inp["heads"], inp["heads"] + kv, inp["kn_w"])):
                o, bound, _ = A.norm_rope_ref(inp["qkv"][:, lo:hi], w, c, s, inp["eps"])
                got = A.norm_rope_twin(inp["qkv"][:, lo:hi], w, c, s, inp["eps"])
                worst = max(worst, float((np.abs(got - o) / bound).max()))
    print(f"writers hd {hd} kv {kv}: twin {worst:.3f} of the bound")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("hd,T", [(32, 1), (32, 65), (128, 129)])
def test_prompt_ref_against_sdpa(hd, T):
    rng = np.random.default_rng(T)
    q, k, v = (randn_bf16(rng, (T, hd)) for _ in range(3))
    got, bound = A.prompt_ref(q, k, v)
    tq, tk, tv = (torch.tensor(a, dtype=torch.float64)[None] for a in (q, k, v))
    want = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv, is_causal=True)[0].numpy()
    s = np.where(np.tril(np.ones((T, T), bool)), (q @ k.T) / np.sqrt(hd), -np.inf)
    w = np.exp(s - s.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    tol = 2.0 ** -7 * (w @ np.abs(v)) * 1.01 + 1e-12            # the P rounding: two half ulps per weight
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())
    assert (bound >= tol / 1.02).all()


@pytest.mark.parametrize("hd,pos", [(32, 0), (32, 33), (128, 513)])
def test_decode_ref_against_sdpa(hd, pos):
    rng = np.random.default_rng(pos)
    q, K, V = randn_bf16(rng, (2, hd)), randn_bf16(rng, (pos + 1, hd)), randn_bf16(rng, (pos + 1, hd))
    got, bound = A.decode_ref(q, K[:pos], V[:pos], K[pos], V[pos])
    t = lambda a: torch.tensor(a, dtype=torch.float64)[None]
    want = torch.nn.functional.scaled_dot_product_attention(t(q), t(K), t(V))[0].numpy()
    s = (q @ K.T) / np.sqrt(hd)
    w = np.exp(s - s.max(1, keepdims=True))
    w /= w.sum(1, keepdims=True)
    tol = 2.0 ** -7 * (w @ np.abs(V)) * 1.01 + 1e-12
    assert (np.abs(got - want) <= tol).all()
    assert (bound >= tol / 1.02).all()


@pytest.mark.parametrize("hd,kv,mc,lens", DECODE_CASES)
def test_decode_twin_and_mutations(hd, kv, mc, lens):
    """the f32 twin stays inside the bound on every input set of the case; and for every edge key the reference with that key dropped, and
    the reference with the row at `pos` admitted as a cached key, differ from the true one by >= 10 x the bound in at least one set"""
    sets = A.decode_sets(lens)
    n_edge = max(len(A.edge_keys(p)) for p in lens)
    seen = np.zeros((len(lens), n_edge + 1))
    worst = 0.0
    cos, sin = A.rope_tables(10000.0, hd // 2, mc)
    for kind, spike in sets:
        inp = A.decode_inputs(hd, kv, mc, len(lens) + 1, lens, kind, spike)
        v, bound, k_new, _, v_new = A.decode_expect(inp)
        q, _, _ = A.norm_rope_ref(inp["qkv"][:, :2 * kv], inp["qn_w"], cos[list(lens)][:, None], sin[list(lens)][:, None], inp["eps"])
        for b, p in enumerate(lens):
            for h in range(2 * kv):
                got = A.decode_twin(q[b, h], inp["K"][b, h // 2, :p], inp["V"][b, h // 2, :p], k_new[b, h // 2], v_new[b, h // 2])
                worst = max(worst, float((np.abs(got - v[b, h]) / bound[b, h]).max()))
        for m in range(n_edge + 1):
            mv = A.decode_expect(inp, drop_edge=m)[0] if m < n_edge else A.decode_expect(inp, admit=True)[0]
            d = np.abs(mv - v) / bound
            d[np.isnan(d)] = np.inf                     # dropping the only key leaves nothing
            seen[:, m] = np.maximum(seen[:, m], d.reshape(len(lens), -1).max(1))
    # at a context of 0 the admitted row is the token's own key and value a second time: v = v_new either way, no input can show it
    seen[[p == 0 for p in lens], n_edge] = np.inf
    print(f"decode hd {hd} kv {kv} max_ctx {mc} lens {lens}: twin {worst:.3f} of the bound, weakest mutation {seen.min():.1f} x the bound")
    assert worst <= 1.0, worst
    assert (seen >= 10.0).all(), seen


@pytest.mark.parametrize("hd,kv,clips", PROMPT_CASES)
def test_prompt_twin_and_mutations(hd, kv, clips):
    """the f32 twin of the prompt attention stays inside the bound on every input set of the case; and for EVERY query row the reference
    with an edge key of its clip dropped, with the row's own key dropped, and with the key after the row admitted, differs from the true one
    by >= 10 x the bound in at least one set"""
    n_edge = max(len(A.prompt_edge_keys(T)) for T in clips)
    muts = [dict(drop_edge=i) for i in range(n_edge)] + [dict(drop_edge="own"), dict(admit=True)]
    n_pos = sum(clips)
    seen = np.zeros((n_pos, len(muts)))
    worst = 0.0
    for kind, spike in A.prompt_sets(clips):
        inp = A.prompt_inputs(hd, kv, clips, kind, spike)
        q, _, k, _, v = A.prompt_writer_expect(inp)
        want, bound = A.prompt_attn_expect(inp, q, k, v)
        for c in range(len(clips)):
            r = slice(inp["cu"][c], inp["cu"][c + 1])
            for h in range(2 * kv):
                got = A.prompt_twin(q[r, h], k[r, h // 2], v[r, h // 2])
                worst = max(worst, float((np.abs(got - want[r, h]) / bound[r, h]).max()))
        for m, mut in enumerate(muts):
            d = np.abs(A.prompt_attn_expect(inp, q, k, v, **mut)[0] - want) / bound
            d[np.isnan(d)] = np.inf                         # dropping a row's only key leaves nothing
            seen[:, m] = np.maximum(seen[:, m], d.reshape(n_pos, -1).max(1))
    cu = np.concatenate([[0], np.cumsum(clips)])
    for c, T in enumerate(clips):                           # a row ahead of the dropped key never saw it; the key after the last row is no input
        ek = A.prompt_edge_keys(T)
        for m in range(n_edge):
            seen[cu[c]:cu[c] + ek[m % len(ek)], m] = np.inf
        seen[cu[c + 1] - 1, n_edge + 1] = np.inf
    print(f"prompt hd {hd} kv {kv} clips {clips}: twin {worst:.3f} of the bound, weakest mutation over all rows {seen.min():.1f} x the bound")
    assert worst <= 1.0, worst
    assert (seen >= 10.0).all(), (seen.min(0), np.argwhere(seen < 10.0)[:8])


@pytest.mark.parametrize("hd", [32, 128])
def test_handover_twin(hd):
    """the decode twin on the hand-over inputs, over the key rows the float64 prompt writer gives"""
    inp = A.handover_prompt(hd)
    dec = A.handover_decode(inp, A.prompt_writer_expect(inp)[2])
    v, bound, k_new, _, v_new = A.decode_expect(dec)
    lens = list(dec["lens"])
    cos, sin = A.rope_tables(dec["theta"], hd // 2, dec["max_ctx"])
    q, _, _ = A.norm_rope_ref(dec["qkv"][:, :4], dec["qn_w"], cos[lens][:, None], sin[lens][:, None], dec["eps"])
    worst = 0.0
    for b, p in enumerate(lens):
        for h in range(4):
            got = A.decode_twin(q[b, h], dec["K"][b, h // 2, :p], dec["V"][b, h // 2, :p], k_new[b, h // 2], v_new[b, h // 2])
            worst = max(worst, float((np.abs(got - v[b, h]) / bound[b, h]).max()))
    print(f"handover hd {hd}: twin {worst:.3f} of the bound")
    assert worst <= 1.0, worst

"""Decoder attention and the K / V cache writers by themselves, through qasr_attn_case_probe (csrc/attn_cases.hip: the product's own launch
entries on a scratch cache of one layer), against the float64 references and derived bounds of tests/attn_cases.py.  No bar comes from a
device run; tests/test_attn_cases_cpu.py proves on the CPU, for every decode and prompt case run here, that a dropped edge key, a key
admitted past the context and a causal edge off by one move an output by >= 10 x the bound (smallest 22 x), and that honest f32 twins
of the kernels stay inside it (decode <= 0.72, prompt <= 0.92).

  decode   every context length of attn_cases.CTX_LENS and max_ctx - 1, three rows of different lengths per launch, head_dim 32 / 128,
           max_ctx 544 / 1056, and nine rows x 8 kv heads; readout / Gaussian / edge-spike inputs; rows past the context hold NaN patterns,
           the spare slot a sentinel.  out within the bound; K row `pos` within the writer bound, V fragment `pos` bit-exact, every other
           byte of both images unchanged; da_spec 0 / 1 / 2, da_earlyq, da_unr give the default's bits; da_waves 16 is held to the bound.
  prompt   ragged batches of three clips in slots [2, 0, 1] of 4, readout / Gaussian / spike inputs (every row's own key, the key after
           every row, key 0 and the keys either side of the last 64-key tile's start): qr and the K rows within the writer bound, V
           bit-exact in the fragment image, K rows from T upward and the other slots untouched, out within the bound of the float64
           attention over the written q / K bits; the narrow, wide and EpiQkHeads writers are bit-equal (the narrow one sums the squares
           in the wide one's order for that).  The two V operands of prefill_attention2_kernel multiply the same P and V in the same MFMA
           k-slot order (keys 4g + j of the even 16-key block, then of the odd one), so they are held bit-equal.
           The fragment image of the keys from T up to the next multiple of 64 is ZERO, not untouched: v_transpose_kernel writes whole
           64-key tiles and prefill_attention2_kernel<.., true> multiplies those entries by P = 0, so they must not be NaN.
  handover the caches a PROMPT returns go unchanged into DECODE at ctx_len = T: writer and reader agree on the fragment layout.
  refusals QASR_ERR_INVALID before any launch.

Every test prints its worst distance as a fraction of its bound (pytest -s).  Worst fractions on the MI355X: see MEASURED below.
"""
import ctypes as C
import numpy as np
import pytest
import attn_cases as A
import gpu_util
from gemm_cases import bf16_bits, bf16_from_bits
from qasr import _lib

pytestmark = pytest.mark.gpu

MEASURED = """worst fractions of the bound on the MI355X (the CPU f32 twins: decode <= 0.72, prompt <= 0.92, writers 1.000 = one ulp of the
final rounding):
decode hd 32: readout 0.719, gauss 0.334, spike 0.417, appended k 0.000; hd 128: readout 0.718, gauss 0.363, spike 0.332, da_waves 16 0.718,
appended k 0.988; 9 rows x 8 kv heads: readout 0.722, gauss 0.398, spike 0.428, appended k 0.000.
prompt: writers 1.000; attention hd 32: readout 0.713, gauss 0.321, spike 0.324; hd 128, 2 kv heads: readout 0.851, gauss 0.322, spike 0.367;
8 kv heads: readout 0.920, gauss 0.322, spike 0.336.  head-tile route: writers 1.000, attention 0.321.
handover 0.226 (hd 32), 0.191 (hd 128), appended k 0.000."""
P16, PI = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
DEFAULTS = {"da_unr": 2, "da_waves": 8, "da_spec": 3, "da_earlyq": 0, "pa_form": 2, "pa_mt": 1, "pa_vfrag": 1, "pa_order": 1, "qknr_wide": 1}
ERR_INVALID = 1
NINE_ROWS = (128, 8, 544, (0, 1, 31, 32, 33, 255, 256, 513, 543))      # the case of the same name in tests/test_attn_cases_cpu.py


@pytest.fixture(scope="module")
def eng():
    e = gpu_util.Engine("tiny", max_audio_seconds=2)
    yield e
    for k, v in DEFAULTS.items():
        e.set_tuning(k, v)
    e.close()


def _knobs(eng, **kw):
    for k, v in {**DEFAULTS, **kw}.items():
        eng.set_tuning(k, v)


def _p(a, t=P16):
    return None if a is None else a.ctypes.data_as(t)


def _call(eng, op, geom, qkv, idx, qn_w, kn_w, K, VF, vt=None, qr=None, x=None, W=None):
    g = _lib.QasrAttnCase(**geom)
    out = np.zeros((geom["n_pos"], geom["heads"] * geom["hd"]), np.uint16)
    cu, soc, pos, slot = (None if a is None else np.ascontiguousarray(a, np.int32) for a in idx)
    rc = eng.lib.qasr_attn_case_probe(eng.h, op, C.byref(g), _p(qkv), _p(x), _p(W), _p(cu, PI), _p(soc, PI), _p(pos, PI), _p(slot, PI),
                                      _p(qn_w), _p(kn_w), _p(K), _p(VF), _p(vt), _p(qr), _p(out))
    return rc, out


def _geom(inp, n_pos, n_clips=0, route=0, hidden=0):
    return dict(n_slots=inp["n_slots"], heads=inp["heads"], kv_heads=inp["kv_heads"], hd=inp["hd"], max_ctx=inp["max_ctx"], n_pos=n_pos,
                n_clips=n_clips, route=route, hidden=hidden, eps=inp["eps"], rope_theta=inp["theta"])


def run_decode(eng, inp):
    """-> (out values [B, heads, hd], K bits, VF bits) after the launch"""
    B = len(inp["lens"])
    K, VF = inp["Kbits"].copy(), inp["VFbits"].copy()
    rc, out = _call(eng, A.DECODE, _geom(inp, B), bf16_bits(inp["qkv"]).reshape(B, -1), (None, None, inp["lens"], None),
                    bf16_bits(inp["qn_w"]), bf16_bits(inp["kn_w"]), K, VF)
    eng.check(rc)
    return out, K, VF


def _frac(got, v, bound):
    assert np.isfinite(got).all()
    return float((np.abs(got - v) / bound).max())


def check_decode(inp, out, K, VF):
    """-> (worst output fraction, worst appended-key fraction)"""
    hd, B = inp["hd"], len(inp["lens"])
    v, bound, k_new, k_bound, v_new = A.decode_expect(inp)
    f_out = _frac(bf16_from_bits(out).reshape(B, inp["heads"], hd), v, bound)
    wantK, wantVF, f_k = inp["Kbits"].copy(), inp["VFbits"].copy(), 0.0
    for b, pos in enumerate(inp["lens"]):
        for h in range(inp["kv_heads"]):
            f_k = max(f_k, _frac(bf16_from_bits(K[b, h, pos]), k_new[b, h], k_bound[b, h]))
            wantK[b, h, pos] = K[b, h, pos]
            img = A.vfrag_unpack(wantVF[b, h], hd)
            img[pos] = bf16_bits(v_new[b, h])
            wantVF[b, h] = A.vfrag_pack(img)
    assert np.array_equal(K, wantK), "K cache: a byte outside the appended rows changed"
    assert np.array_equal(VF, wantVF), "V fragments: the appended key is not where the layout puts it, or another byte changed"
    return f_out, f_k


@pytest.mark.parametrize("max_ctx", [544, 1056])
@pytest.mark.parametrize("hd", [32, 128])
def test_decode(eng, hd, max_ctx):
    worst = {}
    for lens in A.decode_batches(max_ctx):
        for kind, spike in A.decode_sets(lens):
            _knobs(eng)
            inp = A.decode_inputs(hd, 2, max_ctx, 4, lens, kind, spike)
            base = run_decode(eng, inp)
            f_out, f_k = check_decode(inp, *base)
            worst[kind] = max(worst.get(kind, 0.0), f_out)
            worst["k"] = max(worst.get("k", 0.0), f_k)
            if hd == 128 and (kind != "spike" or spike == 0):
                for key, val in (("da_unr", 1), ("da_spec", 0), ("da_spec", 1), ("da_spec", 2), ("da_earlyq", 1)):
                    _knobs(eng, **{key: val})
                    for a, b in zip(base, run_decode(eng, inp)):
                        assert np.array_equal(a, b), (key, val, lens, kind)
                _knobs(eng, da_waves=16)
                f_out, f_k = check_decode(inp, *run_decode(eng, inp))
                worst["waves16"], worst["k"] = max(worst.get("waves16", 0.0), f_out), max(worst["k"], f_k)
    print(f"decode hd {hd} max_ctx {max_ctx}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_decode_nine_rows_eight_kv_heads(eng):
    """B = 9 > 8 rows: the default da_spec 3 resolves to 1 instead of 2"""
    _knobs(eng)
    hd, kv, max_ctx, lens = NINE_ROWS
    worst = {}
    for kind, spike in A.decode_sets(lens):
        inp = A.decode_inputs(hd, kv, max_ctx, len(lens) + 1, lens, kind, spike)
        f_out, f_k = check_decode(inp, *run_decode(eng, inp))
        worst[kind], worst["k"] = max(worst.get(kind, 0.0), f_out), max(worst.get("k", 0.0), f_k)
    print("decode 9 rows x 8 kv heads: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- prompt ---------------------------------------------------------------------------------------------------------------------------------
def run_prompt(eng, inp, route=0, x=None, W=None, qkv_bits=None, nan_fill=False):
    n_pos, hd, kv, ns, mc = inp["qkv"].shape[0], inp["hd"], inp["kv_heads"], inp["n_slots"], inp["max_ctx"]
    K = np.full((ns, kv, mc, hd), A.SENTINEL, np.uint16)
    VF = np.full((ns, kv, mc * hd), A.SENTINEL, np.uint16)
    vt = np.full((ns, kv, hd, mc), 0x7FC0 if nan_fill else A.SENTINEL, np.uint16)
    qr = np.full((n_pos, inp["heads"] * hd), A.SENTINEL, np.uint16)
    qkv = bf16_bits(inp["qkv"]).reshape(n_pos, -1) if qkv_bits is None else qkv_bits.copy()
    hidden = 0 if x is None else x.shape[1]
    idx = (inp["cu"], inp["slot_of_clip"], inp["pos"], inp["slot"])
    rc, out = _call(eng, A.PROMPT, _geom(inp, n_pos, len(inp["clips"]), route, hidden), qkv, idx, bf16_bits(inp["qn_w"]), bf16_bits(inp["kn_w"]),
                    K, VF, vt, qr, None if x is None else bf16_bits(x), None if W is None else bf16_bits(W))
    eng.check(rc)
    return dict(out=out, K=K, VF=VF, qr=qr, qkv=qkv)


def check_prompt_writers(inp, r, qkv=None):
    """-> (writer fraction, the q / k values the device wrote and the v rows it was given, [n_pos, heads or kv_heads, hd])"""
    hd, kv, heads = inp["hd"], inp["kv_heads"], inp["heads"]
    n_pos = inp["pos"].shape[0]
    q, qb, k, kb, v = A.prompt_writer_expect(inp, qkv)
    got_q = bf16_from_bits(r["qr"]).reshape(n_pos, heads, hd)
    f_w = _frac(got_q, q, qb)
    got_k = np.empty_like(k)
    used = set()
    for c, T in enumerate(inp["clips"]):
        sl, rows = int(inp["slot_of_clip"][c]), slice(inp["cu"][c], inp["cu"][c + 1])
        used.add(sl)
        for h in range(kv):
            got_k[rows, h] = bf16_from_bits(r["K"][sl, h, :T])
            assert (r["K"][sl, h, T:] == A.SENTINEL).all(), "K rows from T upward were touched"
            img = A.vfrag_unpack(r["VF"][sl, h], hd)
            assert np.array_equal(img[:T], bf16_bits(v[rows, h])), "V fragments differ from the V rows"
            T64 = (T + 63) // 64 * 64
            assert (img[T:T64] == 0).all() and (img[T64:] == A.SENTINEL).all(), "V fragments past the prompt: zero to the tile's end, then untouched"
    f_w = max(f_w, _frac(got_k, k, kb))
    for sl in set(range(inp["n_slots"])) - used:
        assert (r["K"][sl] == A.SENTINEL).all() and (r["VF"][sl] == A.SENTINEL).all(), "a slot outside the batch was touched"
    return f_w, got_q, got_k, v


def check_prompt(inp, r, qkv=None):
    """-> (writer fraction, attention fraction, the key values the device wrote)"""
    f_w, got_q, got_k, v = check_prompt_writers(inp, r, qkv)
    want, bound = A.prompt_attn_expect(inp, got_q, got_k, v)
    return f_w, _frac(bf16_from_bits(r["out"]).reshape(want.shape), want, bound), got_k


# the first form reads V^T, which the writers fill only under pa_vfrag 0
FORMS = [dict(), dict(pa_vfrag=0), dict(pa_form=1, pa_mt=1, pa_vfrag=0), dict(pa_form=1, pa_mt=2, pa_vfrag=0), dict(pa_order=0), dict(qknr_wide=0)]


@pytest.mark.parametrize("hd,kv", [(32, 2), (128, 2), (128, 8)])
def test_prompt(eng, hd, kv):
    """qk_norm_rope_launch takes the wide writer only where (heads + kv_heads) % 8 == 0: at 2 kv heads (6 heads) the qknr_wide 0 entry of
    FORMS reruns the narrow kernel, and wide against narrow is compared at 8 kv heads alone (and in test_prompt_head_tile_route)."""
    worst = {}
    for clips in A.PROMPT_CLIPS:
        for kind, spike in A.prompt_sets(clips):
            inp = A.prompt_inputs(hd, kv, clips, kind, spike)
            res = {}
            for i, form in enumerate(FORMS):
                _knobs(eng, **form)
                res[i] = run_prompt(eng, inp, nan_fill=i == 0)
            # every writer the same bits, so one reference over the written q / K serves every form
            f_w, got_q, got_k, v = check_prompt_writers(inp, res[0])
            for i in range(1, len(FORMS)):
                for key in ("qr", "K", "VF"):
                    assert np.array_equal(res[0][key], res[i][key]), (FORMS[i], key)
            want, bound = A.prompt_attn_expect(inp, got_q, got_k, v)
            f_a = max(_frac(bf16_from_bits(r["out"]).reshape(want.shape), want, bound) for r in res.values())
            worst["writers"], worst[kind] = max(worst.get("writers", 0.0), f_w), max(worst.get(kind, 0.0), f_a)
            # the two V operands of the second form the same bits; so the two tile orders and, the writers being bit-equal, qknr_wide 0
            assert np.array_equal(res[0]["out"], res[1]["out"]), "pa_vfrag 0 / 1"
            assert np.array_equal(res[0]["out"], res[4]["out"]) and np.array_equal(res[0]["out"], res[5]["out"])
    print(f"prompt hd {hd} kv {kv}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_prompt_head_tile_route(eng):
    """the q|k|v projection as the head-tile GEMM with EpiQkHeads writes the bits of the separate wide and narrow launches"""
    _knobs(eng)
    inp = A.prompt_inputs(128, 8, (64, 65, 127), "gauss")
    rng = np.random.default_rng(5)
    H, n_pos = 64, inp["pos"].shape[0]
    x, W = A.randn_bf16(rng, (n_pos, H)), A.randn_bf16(rng, (32 * 128, H), H ** -0.5)
    sep = run_prompt(eng, inp, 1, x, W)
    fused = run_prompt(eng, inp, 2, x, W)
    _knobs(eng, qknr_wide=0)
    narrow = run_prompt(eng, inp, 1, x, W)
    assert np.array_equal(sep["qkv"], narrow["qkv"])
    nv = 24 * 128
    assert np.array_equal(sep["qkv"][:, nv:], fused["qkv"][:, nv:])
    for key in ("qr", "K", "VF", "out"):
        assert np.array_equal(sep[key], fused[key]) and np.array_equal(sep[key], narrow[key]), key
    f_w, f_a, _ = check_prompt(inp, fused, bf16_from_bits(sep["qkv"]).reshape(n_pos, 32, 128))
    print(f"head-tile route: writers {f_w:.3f}, attention {f_a:.3f} of the bound")
    assert f_w <= 1.0 and f_a <= 1.0


@pytest.mark.parametrize("hd", [32, 128])
def test_handover(eng, hd):
    """PROMPT of T = 33 and 64 keys, its cache images unchanged into DECODE at ctx_len = T"""
    _knobs(eng)
    inp = A.handover_prompt(hd)
    r = run_prompt(eng, inp)
    f_w, f_a, got_k = check_prompt(inp, r)
    assert f_w <= 1.0 and f_a <= 1.0
    dec = A.handover_decode(inp, got_k)                # the reference reads the keys the prompt wrote and the V rows it was given
    dec["Kbits"], dec["VFbits"] = r["K"], r["VF"]
    f_out, f_k = check_decode(dec, *run_decode(eng, dec))
    print(f"handover hd {hd}: {f_out:.3f} of the bound, appended k {f_k:.3f}")
    assert f_out <= 1.0 and f_k <= 1.0


def test_refusals(eng):
    dec = A.decode_inputs(32, 2, 64, 2, (3, 5), "gauss")
    B = 2

    def decode_rc(lens=(3, 5), **over):
        return _call(eng, A.DECODE, {**_geom(dec, B), **over}, bf16_bits(dec["qkv"]).reshape(B, -1), (None, None, lens, None),
                     bf16_bits(dec["qn_w"]), bf16_bits(dec["kn_w"]), dec["Kbits"].copy(), dec["VFbits"].copy())[0]
    assert decode_rc() == 0
    assert decode_rc(heads=6) == ERR_INVALID and decode_rc(hd=64) == ERR_INVALID and decode_rc(max_ctx=48) == ERR_INVALID
    assert decode_rc(lens=(3, 64)) == ERR_INVALID and decode_rc(lens=(-1, 5)) == ERR_INVALID and decode_rc(n_slots=1) == ERR_INVALID
    assert b"attn case" in eng.lib.qasr_last_error(eng.h)
    inp = A.prompt_inputs(32, 2, (3, 4), "gauss", max_ctx=64, n_slots=2)
    inp["slot_of_clip"], inp["slot"] = np.array([1, 0], np.int32), np.array([1] * 3 + [0] * 4, np.int32)

    def prompt_rc(**over):
        i = {**inp, **over}
        n_pos = 7
        z = lambda *s: np.full(s, A.SENTINEL, np.uint16)
        return _call(eng, A.PROMPT, {**_geom(i, n_pos, 2), **over.get("geom", {})}, bf16_bits(inp["qkv"]).reshape(n_pos, -1),
                     (i["cu"], i["slot_of_clip"], i["pos"], i["slot"]), bf16_bits(inp["qn_w"]), bf16_bits(inp["kn_w"]), z(2, 2, 64, 32),
                     z(2, 2, 64 * 32), z(2, 2, 32, 64), z(n_pos, 4 * 32))[0]
    assert prompt_rc() == 0
    i32 = lambda *a: np.array(a, np.int32)
    assert prompt_rc(cu=i32(0, 3, 3)) == ERR_INVALID and prompt_rc(cu=i32(0, 3, 9)) == ERR_INVALID and prompt_rc(cu=i32(1, 3, 7)) == ERR_INVALID
    assert prompt_rc(slot_of_clip=i32(1, 2)) == ERR_INVALID and prompt_rc(slot_of_clip=i32(1, 1)) == ERR_INVALID
    assert prompt_rc(slot=i32(1, 1, 1, 0, 0, 0, 5)) == ERR_INVALID and prompt_rc(pos=i32(0, 1, 2, 0, 1, 2, 64)) == ERR_INVALID
    assert prompt_rc(geom=dict(max_ctx=96)) == ERR_INVALID and prompt_rc(geom=dict(route=2)) == ERR_INVALID

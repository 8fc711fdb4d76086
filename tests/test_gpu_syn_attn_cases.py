"""The attention kernels of the speech-synthesis stacks by themselves, through qasr_syn_attn_case_probe (csrc/syn_attn_cases.hip: one call of
the launch entry the owning class calls), against the float64 references and derived bounds of tests/syn_attn_cases.py.  No bar comes
from a device run; tests/test_syn_attn_cases_cpu.py proves on the CPU, on every case's inputs, that honest f32 twins of the kernels stay
inside the bounds and that the defects a round, chunk, wave, head or sequence boundary produces move an output by >= 10 x the bound or
break an exact check.

  cvlm   (heads, kv heads) (14, 2) / (6, 2) / (16, 1) / (2, 2), max_ctx 320 / 544, the positions of syn_attn_cases.CVLM_POS in launches of
         six to eight rows whose slots are permuted against row order, and one launch shaped like the product's prompt chunk (64 rows of
         one slot at positions 224 .. 287).  Gaussian / readout / spike inputs on every edge key.  qr and K row `pos` within the writer
         bound, V row `pos` bit-exact, every other byte of both caches unchanged (compared whole), qr / out rows past the launch hold the
         sentinel, out within the bound of the float64 attention over the written q / K / V bits; a row alone and a second launch give
         the same bits.
  cp     head_dim 128, rep 1 / 2 / 4, B = 1 / 3 / 17: the product's own sequence pos = 0 .. 15 on one cache that starts as NaN patterns, and
         a single launch at each pos on a pre-filled cache whose entries from pos up are NaN patterns.  Cache entry pos: K within the
         writer bound, V bit-exact, every other entry and the spare cache row unchanged; out within the bound; rows alone, second launch.
  vl     every S in 1 .. 32, (heads, kv heads) (4, 4) / (8, 2) / (8, 1) / (4, 2), n_seq 1 / 3 / 9, plain and long-factor RoPE tables: within
         the bound, rows past n_seq * S hold the sentinel, a sequence alone and a second launch give the same bits.
  refusals  QASR_ERR_INVALID before any launch.

Every test prints its worst distance as a fraction of its bound (pytest -s).  Worst fractions on the MI355X: see MEASURED below.
"""
import ctypes as C
import numpy as np
import pytest
import syn_attn_cases as S
import gpu_util
from gemm_cases import bf16_bits, bf16_from_bits
from qasr import _lib

pytestmark = pytest.mark.gpu

MEASURED = """worst fractions of the bound on the MI355X (the CPU f32 twins: cvlm <= 0.949, cp <= 0.918, vl <= 0.008, writers 1.000 = one ulp of
the final rounding):
cvlm writers 1.000; attention (14, 2): gauss 0.945, readout 0.935, spike 0.949; (6, 2): 0.939, 0.926, 0.946; (16, 1): 0.946, 0.935, 0.948;
(2, 2): 0.936, 0.898, 0.944; prompt chunk: writers 1.000, gauss 0.846, readout 0.933, spike 0.919.
cp sequence: writers 1.000, gauss <= 0.916, own-key spike <= 0.913; single launches: writers 1.000, gauss <= 0.917, readout <= 0.911, spike <= 0.918.
vl: gauss <= 0.006, readout 0.008, spike <= 0.009.
The module's wall time: 18 s (32 tests; 1.0 s at most per cvlm case, 0.5 s per cp case, 3.0 s per vl geometry)."""
P16, PI, PF = C.POINTER(C.c_uint16), C.POINTER(C.c_int32), C.POINTER(C.c_float)
ERR_INVALID = 1


@pytest.fixture(scope="module")
def eng():
    e = gpu_util.Engine("tiny", max_audio_seconds=2)
    yield e
    e.close()


def _p(a, t=P16):
    return None if a is None else a.ctypes.data_as(t)


def _v(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(eng, op, geom, qkv, slot, pos, qn, kn, cos, sin, K, V, qr, out):
    g = _lib.QasrSynAttnCase(**geom)
    return eng.lib.qasr_syn_attn_case_probe(eng.h, op, C.byref(g), _v(qkv), _p(slot, PI), _p(pos, PI), _p(qn), _p(kn), _p(cos, PF), _p(sin, PF),
                                            _p(K), _p(V), _p(qr), _v(out))


_frac = S.frac


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _up(worst, **kw):
    for k, v in kw.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ---- cvlm ---------------------------------------------------------------------------------------------------------------------------------
def cvlm_geom(inp, rows, **over):
    heads, kv = inp["heads"], inp["kv_heads"]
    g = dict(heads=heads, kv_heads=kv, rows=rows, out_rows=rows + 2, n_slots=inp["n_slots"], max_ctx=inp["max_ctx"], pos=0, S=0, n_seq=0,
             n_table=inp["max_ctx"], qkv_elems=rows * (heads + 2 * kv) * 64, cache_elems=inp["Kbits"].size, out_elems=(rows + 2) * heads * 64,
             table_elems=inp["max_ctx"] * 32, eps=0.0)
    return {**g, **over}


def run_cvlm(eng, inp, rows=None, caches=None):
    """rows: indices of the rows to launch (default all); caches: (K, V) images to launch over (default the case's) -> dict of bit images"""
    rows = np.arange(len(inp["pos"])) if rows is None else np.asarray(rows)
    n = len(rows)
    K, V = (inp["Kbits"].copy(), inp["Vbits"].copy()) if caches is None else (caches[0].copy(), caches[1].copy())
    qr = np.full((n + 2, inp["heads"] * 64), S.SENTINEL, np.uint16)
    out = qr.copy()
    qkv = np.ascontiguousarray(bf16_bits(inp["qkv"][rows]).reshape(n, -1))
    slot, pos = np.ascontiguousarray(inp["slot"][rows], np.int32), np.ascontiguousarray(inp["pos"][rows], np.int32)
    eng.check(_call(eng, S.CVLM, cvlm_geom(inp, n), qkv, slot, pos, None, None, _f32(inp["cos"]), _f32(inp["sin"]), K, V, qr, out))
    return dict(out=out, qr=qr, K=K, V=V)


def check_cvlm(inp, r):
    """-> (writer fraction, attention fraction)"""
    rows, heads = len(inp["pos"]), inp["heads"]
    q, qb, k, kb, _ = S.cvlm_writer_expect(inp)
    assert (r["qr"][rows:] == S.SENTINEL).all() and (r["out"][rows:] == S.SENTINEL).all(), "qr / out rows past the launch were written"
    got_q = bf16_from_bits(r["qr"][:rows]).reshape(rows, heads, 64)
    wantK, wantV, got_k = S.cvlm_cache_expect(inp, r["K"], r["V"])
    assert np.array_equal(r["K"], wantK), "K cache: a byte outside the appended rows changed"
    assert np.array_equal(r["V"], wantV), "V cache: the appended row is not bit-exact, or another byte changed"
    f_w = max(_frac(got_q, q, qb), _frac(got_k, k, kb))
    with np.errstate(invalid="ignore"):
        Kv, Vv = bf16_from_bits(r["K"]), bf16_from_bits(r["V"])
    want, bound = S.cvlm_attn_expect(inp, got_q, Kv, Vv)
    return f_w, _frac(bf16_from_bits(r["out"][:rows]).reshape(want.shape), want, bound)


def same_bits_cvlm(eng, inp, r):
    """a second launch, and every row alone over the caches the launch left, give the launch's bits"""
    again = run_cvlm(eng, inp)
    for key in ("out", "qr", "K", "V"):
        assert np.array_equal(again[key], r[key]), ("second launch", key)
    for i in range(len(inp["pos"])):
        one = run_cvlm(eng, inp, rows=[i], caches=(r["K"], r["V"]))
        assert np.array_equal(one["out"][0], r["out"][i]) and np.array_equal(one["qr"][0], r["qr"][i]), ("row alone", i)
        assert np.array_equal(one["K"], r["K"]) and np.array_equal(one["V"], r["V"]), ("row alone: caches", i)


@pytest.mark.parametrize("max_ctx", [320, 544])
@pytest.mark.parametrize("heads,kv", S.CVLM_GEOMS)
def test_cvlm(eng, heads, kv, max_ctx):
    worst = {}
    for poss in S.cvlm_batches(max_ctx):
        for kind, edge in S.cvlm_sets(poss):
            inp = S.cvlm_inputs(heads, kv, max_ctx, poss, kind, edge)
            r = run_cvlm(eng, inp)
            f_w, f_a = check_cvlm(inp, r)
            _up(worst, writers=f_w, **{kind: f_a})
            if kind == "gauss":
                same_bits_cvlm(eng, inp, r)
    print(f"cvlm heads {heads} kv {kv} max_ctx {max_ctx}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_cvlm_prompt_chunk(eng):
    """64 rows of one slot at consecutive positions: the keys behind a row's own position are real data of the later rows"""
    worst = {}
    for kind, edge in S.chunk_sets():
        inp = S.chunk_inputs(kind, edge)
        r = run_cvlm(eng, inp)
        f_w, f_a = check_cvlm(inp, r)
        _up(worst, writers=f_w, **{kind: f_a})
        if kind == "gauss":
            same_bits_cvlm(eng, inp, r)
    print("cvlm prompt chunk: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- code predictor -----------------------------------------------------------------------------------------------------------------------------
def cp_geom(inp, B, n_cache, **over):
    heads, kv = inp["heads"], inp["kv_heads"]
    g = dict(heads=heads, kv_heads=kv, rows=B, out_rows=B + 1, n_slots=n_cache, max_ctx=16, pos=inp["pos"], S=0, n_seq=0, n_table=16,
             qkv_elems=B * (heads + 2 * kv) * 128, cache_elems=n_cache * kv * 16 * 128, out_elems=(B + 1) * heads * 128, table_elems=16 * 64,
             eps=inp["eps"])
    return {**g, **over}


def run_cp(eng, inp, row=None):
    """row: launch that row alone on its own cache row (default: all rows) -> dict of bit images"""
    sel = slice(None) if row is None else slice(row, row + 1)
    qkv = np.ascontiguousarray(bf16_bits(inp["qkv"][sel]).reshape(-1, (inp["heads"] + 2 * inp["kv_heads"]) * 128))
    B = qkv.shape[0]
    K, V = (inp["Kbits"].copy(), inp["Vbits"].copy()) if row is None else (inp["Kbits"][[row, -1]].copy(), inp["Vbits"][[row, -1]].copy())
    out = np.full((B + 1, inp["heads"] * 128), S.SENTINEL, np.uint16)
    eng.check(_call(eng, S.CP, cp_geom(inp, B, K.shape[0]), qkv, None, None, bf16_bits(inp["qn_w"]), bf16_bits(inp["kn_w"]), _f32(inp["cos"]),
                    _f32(inp["sin"]), K, V, None, out))
    return dict(out=out, K=K, V=V)


def check_cp(inp, r):
    """-> (writer fraction, attention fraction)"""
    B, pos, heads = inp["B"], inp["pos"], inp["heads"]
    k, kb, v = S.cp_writer_expect(inp)
    assert (r["out"][B:] == S.SENTINEL).all(), "out rows past the launch were written"
    wantK, wantV = inp["Kbits"].copy(), inp["Vbits"].copy()
    wantK[:B, :, pos] = r["K"][:B, :, pos]
    wantV[:B, :, pos] = bf16_bits(v)
    assert np.array_equal(r["K"], wantK), "K cache: an entry other than pos, or the cache of a row past B, changed"
    assert np.array_equal(r["V"], wantV), "V cache: entry pos is not bit-exact, or another byte changed"
    f_w = _frac(bf16_from_bits(r["K"][:B, :, pos]), k, kb)
    with np.errstate(invalid="ignore"):
        Kv, Vv = bf16_from_bits(r["K"]), bf16_from_bits(r["V"])
    want, bound = S.cp_attn_expect(inp, Kv, Vv)
    return f_w, _frac(bf16_from_bits(r["out"][:B]).reshape(want.shape), want, bound)


def same_bits_cp(eng, inp, r):
    again = run_cp(eng, inp)
    for key in ("out", "K", "V"):
        assert np.array_equal(again[key], r[key]), ("second launch", key)
    for b in range(inp["B"]):
        one = run_cp(eng, inp, row=b)
        assert np.array_equal(one["out"][0], r["out"][b]), ("row alone", b)
        assert np.array_equal(one["K"][0], r["K"][b]) and np.array_equal(one["V"][0], r["V"][b]), ("row alone: cache", b)


@pytest.mark.parametrize("B", S.CP_B)
@pytest.mark.parametrize("heads,kv", S.CP_GEOMS)
def test_cp_sequence(eng, heads, kv, B):
    """the product's own sequence: 16 launches pos = 0 .. 15 on one cache, each checked"""
    worst = {}
    for kind, edge in (("gauss", 0), ("spike", "own")):
        carry = None
        for pos in range(16):
            inp = S.cp_inputs(heads, kv, B, pos, kind, edge, fresh=True)
            if carry is not None:
                inp["Kbits"], inp["Vbits"] = carry
            r = run_cp(eng, inp)
            f_w, f_a = check_cp(inp, r)
            _up(worst, writers=f_w, **{kind: f_a})
            carry = (r["K"], r["V"])
    print(f"cp sequence heads {heads} kv {kv} B {B}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("B", S.CP_B)
@pytest.mark.parametrize("heads,kv", S.CP_GEOMS)
def test_cp_single(eng, heads, kv, B):
    """a single launch at each pos on a pre-filled cache whose entries from pos up are NaN patterns"""
    worst = {}
    for pos in range(16):
        for kind, edge in S.cp_sets(pos):
            inp = S.cp_inputs(heads, kv, B, pos, kind, edge)
            r = run_cp(eng, inp)
            f_w, f_a = check_cp(inp, r)
            _up(worst, writers=f_w, **{kind: f_a})
            if kind == "gauss" and pos in S.CP_ALONE_POS:
                same_bits_cp(eng, inp, r)
    print(f"cp single heads {heads} kv {kv} B {B}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- vl -----------------------------------------------------------------------------------------------------------------------------------------
def vl_geom(inp, n_seq, **over):
    heads, kv, Sq = inp["heads"], inp["kv_heads"], inp["S"]
    rows = n_seq * Sq
    g = dict(heads=heads, kv_heads=kv, rows=rows, out_rows=rows + 2, n_slots=0, max_ctx=0, pos=0, S=Sq, n_seq=n_seq, n_table=32,
             qkv_elems=rows * (heads + 2 * kv) * 128, cache_elems=0, out_elems=(rows + 2) * heads * 128, table_elems=32 * 128, eps=0.0)
    return {**g, **over}


def run_vl(eng, inp, seq=None):
    """seq: launch that sequence alone -> out f32 [rows + 2, heads * 128]"""
    x = np.ascontiguousarray(inp["qkv"] if seq is None else inp["qkv"][seq:seq + 1])
    n = x.shape[0]
    out = np.full((n * inp["S"] + 2, inp["heads"] * 128), S.F32_SENTINEL, np.float32)
    eng.check(_call(eng, S.VL, vl_geom(inp, n), x, None, None, None, None, inp["cos"], inp["sin"], None, None, None, out))
    return out


@pytest.mark.parametrize("heads,kv", S.VL_GEOMS)
def test_vl(eng, heads, kv):
    worst = {}
    for Sq in range(1, 33):
        for n_seq in S.VL_NSEQ:
            for kind, edge in S.VL_SETS:
                inp = S.vl_inputs(Sq, heads, kv, n_seq, kind, edge)
                out = run_vl(eng, inp)
                rows = n_seq * Sq
                assert (out[rows:] == S.F32_SENTINEL).all(), "out rows past n_seq * S were written"
                want, bound = S.vl_expect(inp)
                _up(worst, **{kind: _frac(out[:rows].astype(np.float64).reshape(want.shape), want, bound)})
                if kind == "gauss":
                    assert np.array_equal(run_vl(eng, inp), out), "second launch"
                    for j in range(n_seq):
                        assert np.array_equal(run_vl(eng, inp, seq=j)[:Sq], out[j * Sq:(j + 1) * Sq]), ("sequence alone", Sq, n_seq, j)
    print(f"vl heads {heads} kv {kv}: fractions of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    inp = S.cvlm_inputs(6, 2, 320, (3, 70, 300), "gauss")
    n = 3

    def cvlm_rc(op=S.CVLM, slot=inp["slot"], pos=inp["pos"], drop=(), **over):
        a = dict(qkv=np.ascontiguousarray(bf16_bits(inp["qkv"]).reshape(n, -1)), slot=np.ascontiguousarray(slot, np.int32),
                 pos=np.ascontiguousarray(pos, np.int32), cos=_f32(inp["cos"]), sin=_f32(inp["sin"]), K=inp["Kbits"].copy(), V=inp["Vbits"].copy(),
                 qr=np.full((n + 2, 6 * 64), S.SENTINEL, np.uint16), out=np.full((n + 2, 6 * 64), S.SENTINEL, np.uint16))
        for k in drop:
            a[k] = None
        return _call(eng, op, cvlm_geom(inp, n, **over), a["qkv"], a["slot"], a["pos"], None, None, a["cos"], a["sin"], a["K"], a["V"], a["qr"], a["out"])
    assert cvlm_rc() == 0
    assert cvlm_rc(op=3) == ERR_INVALID and cvlm_rc(op=-1) == ERR_INVALID                              # an unknown op
    for name in ("qkv", "slot", "pos", "cos", "sin", "K", "V", "qr", "out"):                              # null pointers
        assert cvlm_rc(drop=(name,)) == ERR_INVALID, name
    assert cvlm_rc(heads=34, kv_heads=2) == ERR_INVALID and cvlm_rc(heads=7) == ERR_INVALID            # rep 17; rep 3.5
    assert cvlm_rc(slot=(0, 1, 4)) == ERR_INVALID and cvlm_rc(slot=(0, -1, 2)) == ERR_INVALID          # a slot outside the cache
    assert cvlm_rc(pos=(3, 70, 320)) == ERR_INVALID and cvlm_rc(pos=(-1, 70, 300)) == ERR_INVALID      # a position outside the cache
    assert cvlm_rc(n_table=300, table_elems=300 * 32) == ERR_INVALID                                     # ... outside the tables
    assert cvlm_rc(slot=(1, 1, 2), pos=(3, 3, 300)) == ERR_INVALID                                       # two rows on one cache row
    for key in ("qkv_elems", "cache_elems", "out_elems", "table_elems"):                                 # sizes that contradict the geometry
        assert cvlm_rc(**{key: cvlm_geom(inp, n)[key] - 64}) == ERR_INVALID, key
    assert cvlm_rc(max_ctx=288) == ERR_INVALID and cvlm_rc(out_rows=2) == ERR_INVALID
    assert b"syn attn case" in eng.lib.qasr_last_error(eng.h)

    cp = S.cp_inputs(4, 2, 3, 5, "gauss")

    def cp_rc(drop=(), **over):
        a = dict(qkv=np.ascontiguousarray(bf16_bits(cp["qkv"]).reshape(3, -1)), qn=bf16_bits(cp["qn_w"]), kn=bf16_bits(cp["kn_w"]), cos=_f32(cp["cos"]),
                 sin=_f32(cp["sin"]), K=cp["Kbits"].copy(), V=cp["Vbits"].copy(), out=np.full((4, 4 * 128), S.SENTINEL, np.uint16))
        for k in drop:
            a[k] = None
        return _call(eng, S.CP, cp_geom(cp, 3, 4, **over), a["qkv"], None, None, a["qn"], a["kn"], a["cos"], a["sin"], a["K"], a["V"], None, a["out"])
    assert cp_rc() == 0
    for name in ("qkv", "qn", "kn", "cos", "sin", "K", "V", "out"):
        assert cp_rc(drop=(name,)) == ERR_INVALID, name
    assert cp_rc(pos=16) == ERR_INVALID and cp_rc(pos=-1) == ERR_INVALID                                # pos outside the cache
    assert cp_rc(pos=5, n_table=4, table_elems=4 * 64) == ERR_INVALID                                    # ... outside the tables
    assert cp_rc(heads=3) == ERR_INVALID and cp_rc(n_slots=2) == ERR_INVALID and cp_rc(max_ctx=32) == ERR_INVALID
    for key in ("qkv_elems", "cache_elems", "out_elems", "table_elems"):
        assert cp_rc(**{key: cp_geom(cp, 3, 4)[key] + 128}) == ERR_INVALID, key

    vl = S.vl_inputs(5, 4, 2, 3, "gauss")

    def vl_rc(drop=(), **over):
        a = dict(qkv=np.ascontiguousarray(vl["qkv"]), cos=vl["cos"], sin=vl["sin"], out=np.full((17, 4 * 128), S.F32_SENTINEL, np.float32))
        for k in drop:
            a[k] = None
        return _call(eng, S.VL, vl_geom(vl, 3, **over), a["qkv"], None, None, None, None, a["cos"], a["sin"], None, None, None, a["out"])
    assert vl_rc() == 0
    for name in ("qkv", "cos", "sin", "out"):
        assert vl_rc(drop=(name,)) == ERR_INVALID, name
    assert vl_rc(S=0) == ERR_INVALID and vl_rc(S=33) == ERR_INVALID and vl_rc(S=4) == ERR_INVALID      # S outside 1 .. 32; rows != n_seq * S
    assert vl_rc(heads=6, kv_heads=2) == ERR_INVALID and vl_rc(heads=2, kv_heads=2) == ERR_INVALID      # heads x 128 no multiple of 512
    assert vl_rc(heads=4, kv_heads=3) == ERR_INVALID                                                      # rep non-integral
    assert vl_rc(n_table=4, table_elems=4 * 128) == ERR_INVALID                                           # S outside the tables
    for key in ("qkv_elems", "out_elems", "table_elems"):
        assert vl_rc(**{key: vl_geom(vl, 3)[key] + 128}) == ERR_INVALID, key

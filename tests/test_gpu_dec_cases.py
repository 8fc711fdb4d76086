"""The kernels that stream the weights of a decode step by themselves, through qasr_dec_case_probe (csrc/dec_cases.hip: the product's packer and
ONE call of the product's launch entry on host data), against the float64 references and derived bounds of tests/dec_cases.py.  No bar comes
from a device run; tests/test_dec_cases_cpu.py proves on the CPU, on the inputs used here, that honest f32 twins stay inside the bounds and
that a dropped or doubled k-step, a dropped column phase, a leaking or dropped edge row, a row group at group 0's offset, a wrong residual row,
a wrong gate / up pairing, a wrong inv or norm-weight chunk, a neighbour's scale or bias, a dropped bias or 4-bit offset and swapped nibbles
each move an output by >= 10 x the bound or break an exact check.

  gemv     decode_gemv_dense_launch on a bf16 weight: tuned K 1024 / 2048 / 3072 (decode_gemv2_kernel), 6144 (decode_gemv_wide_kernel), generic
           K 96 / 1056 (decode_gemv_kernel: 3 and 33 k-steps); BF16 / RESID at N = 144 (9 tiles against the 8-XCD map), SWIGLU at 288, LOGITS at
           320 (tuned) / 272; the norm prologue at 1024 / 2048; B = 1 .. 64 on both sides of every batch rule; every knob at the batch sizes
           where it changes the instantiation, bit-equal to the defaults where the reduction map is kept (dec_cases.gemv_knob_runs).  Every
           launch reports the kernel it was meant to run (tuned / generic); rows >= B keep the sentinel; a second launch gives the same bits; a
           row alone gives the bits it gives inside the batch; one-hot rows and one-hot weight rows read back weights / activations bit for bit.
  gemvq    decode_gemv_q_launch: bits 4 / 8 x bf16 / f32 scales, RESID at K 1024 .. 6144 (6144 under gemv_wide 0 / 1), norm BF16 / SWIGLU at
           1024 / 2048 (N = 4096 / 6144: two / four tiles per workgroup), the generic kernel at K = 192; gemv_xbar 0 .. 4; the same assertions,
           the readout in the kernel's f32 order.
  heads    lm_head_launch (persistent at N = 65616, K 1024 / 2048; generic at N = 272 / 16448) and lm_head_q_launch (persistent at N = 32848,
           generic at 272): logits within the bound; the partials exact against the device's own logits, part by part; planted equal rows
           (one lane, one wave's first and tail tile, two waves, two workgroups) are each a row's maximum and the lower copy wins; knobs
           lmh_order, lmh_nt, lmh_q_ring; logits and partial rows >= B untouched.
  norm     rmsnorm_rows_launch at widths 96 .. 2048 and row counts around a workgroup's four, element by element against the two candidates.
  tail     greedy_finalize_launch against an exact restatement (dec_cases.finalize_ref): 1 / 256 / 257 / 600 partials per row with every row's
           maximum in two parts (the lower index in the later one); +inf, NaN, all -inf, an index at the vocabulary's end or below zero set
           err on unfinished rows only; EOS with and without ignore_eos, the length cap, n_active, advance_ctx 0 / 1, the cleared words and the
           sequence word, the rope row of the NEXT position at half 16 / 64, the next input row from a bf16 / 4-bit / 8-bit table; every
           array it may write comes back and is compared whole.  embed_splice(_q), gather_rows(_q), quant_dequant_rows at H 64 / 1024.
  refusals QASR_ERR_INVALID before any launch.

Every test prints its worst distance as a fraction of its bound (pytest -s).  Worst fractions on the MI355X: see MEASURED below.
"""
import ctypes as C
import numpy as np
import pytest
import dec_cases as D
import gemm_cases as G
import gpu_util
from gemm_cases import bf16_bits, bf16_from_bits
from qasr import _lib

pytestmark = pytest.mark.gpu

MEASURED = """worst fractions of the bound on the MI355X, beside the CPU f32 twins of tests/test_dec_cases_cpu.py on the same inputs (in
brackets); the half ulp of the output rounding is 0.97 of every bound, so these figures say that the f32 error is where the twins' is.  To
three digits no case lies above its own twin, group by group:
bf16 linear   tuned BF16 0.966 [0.966], RESID 0.968 [0.968], LOGITS 0.966 [0.966]; generic 0.968 / 0.969 / 0.968 [the same]; gemv_w1024 4 and
              gemv_wide 0: the figures of the defaults; coherent SWIGLU 0 bf16 ulps at 8 and at 4 waves [2], bar 3
quantised     4 bit tuned RESID 0.951 [0.951], BF16 behind a norm 0.945 [0.945], generic 0.967 [0.967]; 8 bit tuned 0.963 / 0.950 [the same],
              generic 0.967 [0.967]; coherent SWIGLU 2 ulps (N 6144), 0 elsewhere [2 at 4 bit, 3 at 8 bit]
Gaussian SWIGLU, bf16 and quantised cases pooled: 216 of 692 736 outputs not bit-equal to float64 (0.031 %) [234, 0.034 %]; bar 3 x the twins
LM heads      bf16 persistent K 1024 0.966 [0.966], K 2048 0.962 [0.962], generic N 272 0.964 [0.964], N 16448 0.967 [0.967]
              quantised persistent K 1024: 4 bit 0.929 / 0.927 (bf16 / f32 scales) [0.929 / 0.930], 8 bit 0.955 / 0.955 [0.955 / 0.955];
              K 2048: 4 bit 0.911 [0.913], 8 bit f32 scales 0.949 [0.950]; generic 0.942 / 0.942 [0.942 / 0.943]; partials, planted ties: exact
every knob setting that keeps the reduction map: bit-equal to the defaults
readouts, rmsnorm_rows, greedy tail, embedding lookups: exact.
The tuned four-tile LOGITS form at K 2048 has no instantiation above 48 rows (its LDS image would be 176 KiB): B = 49 and 64 report the generic
kernel, as dec_cases.gemv_route states from gemv2_lds; no product launch takes that form.  The whole module (120 tests) runs in 19 s."""
ERR_INVALID = 1
SENT, SENT_F32 = D.SENTINEL, D.SENTINEL_F32
KNOBS = ("gemv_splitb", "gemv_w1024", "gemv_partial", "gemv_earlyw", "gemv_nt", "gemv_xbar", "gemv_wide", "lmh_order", "lmh_nt", "lmh_q_ring")


@pytest.fixture(scope="module")
def eng():
    e = gpu_util.Engine("tiny", max_audio_seconds=2)
    saved = {k: e.get_tuning(k) for k in KNOBS}
    yield e
    for k, v in saved.items():
        e.set_tuning(k, v)
    e.close()


@pytest.fixture
def knobs(eng):
    """set_tuning that is undone when the test ends"""
    saved = {}

    def set_(key, value):
        saved.setdefault(key, eng.get_tuning(key))
        eng.set_tuning(key, value)
    yield set_
    for k, v in saved.items():
        eng.set_tuning(k, v)


def _ptr(a, t=C.c_void_p):
    return None if a is None else C.cast(a.ctypes.data, t)


def probe(eng, op, X, W=None, scales=None, biases=None, nw=None, out=None, logits=None, pv=None, pi=None, state=None, rope=None, rows=None,
          **geom):
    """-> (status, n_parts, route); out / logits / pv / pi are overwritten in place"""
    g = _lib.QasrDecCase(eps=D.EPS, **geom)
    u16 = C.POINTER(C.c_uint16)
    keep = [None if a is None else np.ascontiguousarray(a) for a in (X, W, scales, biases, nw)]
    for a in (out, logits, pv, pi, state, rope, rows):
        assert a is None or a.flags["C_CONTIGUOUS"]
    fp = C.POINTER(C.c_float)
    rc = eng.lib.qasr_dec_case_probe(eng.h, op, C.byref(g), _ptr(keep[0], u16), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4], u16),
                                     _ptr(out, u16), _ptr(logits, fp), _ptr(pv, fp), _ptr(pi, C.POINTER(C.c_int32)),
                                     _ptr(state, C.POINTER(C.c_int32)), _ptr(rope, fp), _ptr(rows, fp))
    return rc, g.n_parts, g.route


def _report(name, worst):
    print(f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- the linears ---------------------------------------------------------------------------------------------------------------------------------
class Linear:
    """one weight of a case on the host: launches on the first B rows of given activations"""

    def __init__(self, eng, op, epi, K, N, norm, generic, W, nw, scales=None, biases=None, bits=0, sb_f32=0, route=None):
        self.eng, self.op, self.epi, self.K, self.N, self.norm, self.generic = eng, op, epi, K, N, norm, generic
        self.W, self.scales, self.biases, self.bits, self.sb_f32 = W, scales, biases, bits, sb_f32
        self.nw = None if nw is None else bf16_bits(nw)
        self.cols = N // 2 if epi == D.SWIGLU else N
        self.route = route
        self.parts = (N // 64 if N % 64 == 0 else N // 32 if N % 32 == 0 else N // 16) if epi == D.LOGITS else 0

    def __call__(self, X, B, resid=None, wide=1):
        """X [rows >= B, K] values -> out [B, cols] bf16 bits (LOGITS: f32 logits, and the partials are checked here)"""
        extra = 2
        geom = dict(B=B, N=self.N, K=self.K, epi=self.epi, generic=self.generic, bits=self.bits, sb_f32=self.sb_f32, in_extra=1, out_extra=extra)
        xb = D.x_bits(X, B)
        if self.epi == D.LOGITS:
            lg = np.full((B + extra, self.N), SENT_F32, np.float32)
            cap = (B + extra) * self.parts
            pv, pi = np.full(cap, SENT_F32, np.float32), np.full(cap, -77, np.int32)
            rc, n_parts, route = probe(self.eng, self.op, xb, self.W, nw=self.nw, logits=lg, pv=pv, pi=pi, part_cap=cap, **geom)
            self.eng.check(rc)
            assert n_parts == self.parts and (lg[B:] == SENT_F32).all() and (pv[B * n_parts:] == SENT_F32).all() and (pi[B * n_parts:] == -77).all()
            nt = self.N // 16 // n_parts
            bad = D.partials_defects(lg[:B], pv[:B * n_parts].reshape(B, -1), pi[:B * n_parts].reshape(B, -1),
                                     [list(range(p * nt, (p + 1) * nt)) for p in range(n_parts)])
            assert not bad, bad
            out = lg[:B]
        else:
            o = np.full((B + extra, self.cols), SENT, np.uint16)
            if resid is not None:
                o[:B] = bf16_bits(resid[:B])
            rc, _, route = probe(self.eng, self.op, xb, self.W, self.scales, self.biases, self.nw, out=o, **geom)
            self.eng.check(rc)
            assert (o[B:] == SENT).all(), "a row after the last was written"
            out = o[:B]
        want = self.route_at(B) if self.K != 6144 or wide else 0
        assert route == want, f"ran the {'tuned' if route else 'generic'} kernel, meant the {'tuned' if want else 'generic'} one (B {B})"
        return out

    def route_at(self, B):
        return self.route(B) if callable(self.route) else self.route

    def values(self, out):
        return out.astype(np.float64) if self.epi == D.LOGITS else bf16_from_bits(out)


def linear_case(lin, d, expect, kinds, Bs, knob_runs, knobs):
    """every input kind at every B against the reference; launch = launch, row alone = row in the batch, knob settings"""
    epi, worst = lin.epi, {}
    for kind in kinds:
        X, r, exp = d[kind]["X"], d[kind]["r"], expect[kind]
        base = {}
        for B in Bs:
            out = base[B] = lin(X, B, r)
            got = lin.values(out)
            if epi == D.SWIGLU and kind == "gauss":
                assert np.isfinite(got).all()           # held to the reference by test_swiglu_gaussian_share
            else:
                f = D.gemv_frac(epi, exp, got, B)
                worst[kind] = max(worst.get(kind, 0.0), f)
                assert f <= (3 if epi == D.SWIGLU else 1.0), (kind, B, f)
        Bmax = max(b for b in Bs if lin.route_at(b) == lin.route_at(1))     # a row alone and the batch: the same kernel family
        assert np.array_equal(lin(X, Bmax, r), base[Bmax]), "a second launch gave other bits"
        for b in sorted({0, 15, 16, Bmax - 1} & set(range(Bmax))):
            alone = lin(X[b:b + 1], 1, None if r is None else r[b:b + 1])
            assert np.array_equal(alone[0], base[Bmax][b]), f"row {b} alone differs from row {b} of the batch of {Bmax}"
        for key, value, kBs, same in knob_runs:
            default = lin.eng.get_tuning(key)
            knobs(key, value)
            for B in kBs:
                out = lin(X, B, r, wide=value if key == "gemv_wide" else 1)
                if same:
                    assert np.array_equal(out, base[B]), f"{key} {value} at B {B} is not bit-equal to the default"
                elif epi == D.SWIGLU and kind == "gauss":   # other bits than the defaults: held on the coherent kind, under the three ulps
                    assert np.isfinite(lin.values(out)).all()
                else:
                    f = D.gemv_frac(epi, exp, lin.values(out), B)
                    worst[f"{kind} {key} {value}"] = max(worst.get(f"{kind} {key} {value}", 0.0), f)
                    assert f <= (3 if epi == D.SWIGLU else 1.0), (kind, key, value, B, f)
            knobs(key, default)
    return worst


def _gemv_id(c):
    return f"{D.EPI_NAMES[c[0]]}-K{c[1]}-N{c[2]}" + ("-norm" if c[3] else "") + ("-generic" if c[4] else "")


@pytest.mark.parametrize("case", D.gemv_cases(), ids=_gemv_id)
def test_gemv(eng, knobs, case):
    epi, K, N, norm, generic = case
    kinds = D.gemv_kinds(epi, norm)
    d = {k: D.gemv_inputs(epi, K, N, norm, k) for k in kinds}
    expect = {k: D.gemv_expect(epi, K, N, norm, k) for k in kinds}
    worst = {}
    for kind in kinds:              # the weight differs per kind (spike columns, coherent rows): one Linear each
        lin = Linear(eng, D.GEMV, epi, K, N, norm, generic, bf16_bits(d[kind]["W"]), d[kind]["nw"],
                     route=lambda B: D.gemv_route(epi, K, N, norm, generic, B=B))
        worst.update(linear_case(lin, d, expect, (kind,), D.BS, [r for r in D.gemv_knob_runs(epi, K, N, norm, generic) if kind != "coherent" or not r[3]], knobs))
    if not norm and epi in (D.BF16, D.RESID):
        readouts(eng, epi, K, N, generic)
    _report(f"gemv {_gemv_id(case)}: fractions of the bound" + (" (swiglu: bf16 ulps, bar 3)" if epi == D.SWIGLU else ""), worst)


def readouts(eng, epi, K, N, generic):
    """one-hot activation rows read the weight back, one-hot weight rows the activations, bit for bit"""
    rng = np.random.default_rng([K, N, epi, 3])
    W, Xg = G.randn_bf16(rng, (N, K), K ** -0.5), D.x_rows(K, "gauss", 0)
    r = G.bf16_round(rng.standard_normal((D.ROWS, N)) * 2.0 ** -4) if epi == D.RESID else None
    route = D.gemv_route(epi, K, N, 0, generic)
    lin = Linear(eng, D.GEMV, epi, K, N, 0, generic, bf16_bits(W), None, route=route)
    for shift in D.readout_shifts(K, D.ROWS):
        k = np.array([D.readout_k(K, i, shift) for i in range(D.ROWS)])
        X = np.zeros((D.ROWS, K))
        X[np.arange(D.ROWS), k] = 1.0
        for B in (1, 16, 17, 64) if shift == 0 else (64,):
            got = bf16_from_bits(lin(X, B, r))
            assert np.array_equal(got, D.readout_expect(epi, W, k[:B], None if r is None else r[:B])), f"one-hot rows, shift {shift}, B {B}"
    for shift in D.readout_shifts(K, N):
        k = np.array([D.readout_k(K, n, shift) for n in range(N)])
        Wh = np.zeros((N, K))
        Wh[np.arange(N), k] = 1.0
        linw = Linear(eng, D.GEMV, epi, K, N, 0, generic, bf16_bits(Wh), None, route=route)
        for B in (7, 33, 64):
            got = bf16_from_bits(linw(Xg, B, r))
            want = Xg[:B][:, k] if r is None else G.bf16_round(D.f32(r[:B] + Xg[:B][:, k]))
            assert np.array_equal(got, want), f"one-hot weight rows, shift {shift}, B {B}"


def _gemvq_id(c):
    return f"q{c[5]}{'f' if c[6] else 'h'}-" + _gemv_id(c[:5])


@pytest.mark.parametrize("case", D.gemvq_cases(), ids=_gemvq_id)
def test_gemvq(eng, knobs, case):
    epi, K, N, norm, generic, bits, sbf = case
    route = D.gemvq_route(epi, K, N, norm, generic)
    kinds = D.gemvq_kinds(epi)
    Bs = D.BS_Q
    worst = {}
    for kind in kinds:
        d = D.gemvq_inputs(epi, K, N, norm, bits, sbf, kind)
        m = d["m"]
        cast = (lambda a: a.astype(np.float32)) if sbf else bf16_bits
        lin = Linear(eng, D.GEMVQ, epi, K, N, norm, generic, m["words"], d["nw"], cast(m["s"]), cast(m["b"]), bits, sbf, route=route)
        exp = {kind: D.gemvq_expect(epi, K, N, norm, bits, sbf, kind, bool(route))}
        runs = D.gemvq_knob_runs(epi, K, N, norm, generic) if kind == "gauss" else ()
        if runs and runs[0][0] == "gemv_wide":      # the generic kernel multiplies by q and b, not by 16 + q and b': its own reference
            lin0 = Linear(eng, D.GEMVQ, epi, K, N, norm, generic, m["words"], d["nw"], cast(m["s"]), cast(m["b"]), bits, sbf, route=route)
            e0 = D.gemvq_expect(epi, K, N, norm, bits, sbf, kind, False)
            knobs("gemv_wide", 0)
            for B in runs[0][2]:
                f = D.gemv_frac(epi, e0, lin0.values(lin0(d["X"], B, d["r"], wide=0)), B)
                worst["gauss gemv_wide 0"] = max(worst.get("gauss gemv_wide 0", 0.0), f)
                assert f <= 1.0, (B, f)
            knobs("gemv_wide", 1)
            runs = ()
        worst.update(linear_case(lin, {kind: d}, exp, (kind,), Bs, runs, knobs))
    if not norm and N <= 288:
        m = D.quant_matrix(K, N, bits, sbf)
        r = G.bf16_round(np.random.default_rng(K).standard_normal((D.ROWS, N)) * 2.0 ** -4) if epi == D.RESID else None
        cast = (lambda a: a.astype(np.float32)) if sbf else bf16_bits
        lin = Linear(eng, D.GEMVQ, epi, K, N, 0, generic, m["words"], None, cast(m["s"]), cast(m["b"]), bits, sbf, route=route)
        for shift in D.readout_shifts(K, D.ROWS):
            k = np.array([D.readout_k(K, i, shift) for i in range(D.ROWS)])
            X = np.zeros((D.ROWS, K))
            X[np.arange(D.ROWS), k] = 1.0
            for B in (1, 17, 64) if shift == 0 else (64,):
                got = bf16_from_bits(lin(X, B, r))
                want = D.quant_readout_expect(epi, m, bits, bool(route), k[:B], None if r is None else r[:B])
                assert np.array_equal(got, want), f"one-hot rows, shift {shift}, B {B}"
    _report(f"gemvq {_gemvq_id(case)}: fractions of the bound" + (" (swiglu: bf16 ulps, bar 3)" if epi == D.SWIGLU else ""), worst)


def test_swiglu_gaussian_share(eng):
    """over every Gaussian SWIGLU output of the bf16 and the quantised cases (B = 1, 17, 64), the share that is not bit-equal to the float64
    reference is at most 3 x the share of the f32 twins on the same rows"""
    dev = total = twin = 0
    Bs = (1, 17, 64)
    for case in D.gemv_cases() + D.gemvq_cases():
        if case[0] != D.SWIGLU:
            continue
        epi, K, N, norm, generic = case[:5]
        if len(case) == 5:
            d, ref = D.gemv_inputs(epi, K, N, norm, "gauss"), D.gemv_expect(epi, K, N, norm, "gauss")["ref"]
            lin = Linear(eng, D.GEMV, epi, K, N, norm, generic, bf16_bits(d["W"]), d["nw"], route=D.gemv_route(*case))
            tw = D.gemv_twin(epi, d) != ref
        else:
            bits, sbf = case[5:]
            route = D.gemvq_route(*case[:5])
            d, ref = D.gemvq_inputs(epi, K, N, norm, bits, sbf, "gauss"), D.gemvq_expect(epi, K, N, norm, bits, sbf, "gauss", bool(route))["ref"]
            cast = (lambda a: a.astype(np.float32)) if sbf else bf16_bits
            lin = Linear(eng, D.GEMVQ, epi, K, N, norm, generic, d["m"]["words"], d["nw"], cast(d["m"]["s"]), cast(d["m"]["b"]), bits, sbf, route=route)
            tw = D.gemvq_twin(epi, d, bits, bool(route)) != ref
        for B in Bs:
            got = bf16_from_bits(lin(d["X"], B))
            dev, total, twin = dev + int((got != ref[:B]).sum()), total + got.size, twin + int(tw[:B].sum())
    print(f"swiglu, Gaussian inputs: {dev} of {total} outputs differ from float64 ({dev / total * 100:.4f} %), f32 twins {twin} ({twin / total * 100:.4f} %)")
    assert dev <= 3 * twin, (dev, twin, total)


# ---- LM heads ---------------------------------------------------------------------------------------------------------------------------------------
def run_head(eng, op, K, N, generic, d, B, W, scales=None, biases=None, bits=0, sbf=0, order=1):
    """-> logits [B, N] f32; the partials are checked against them here"""
    persistent = not generic
    parts = D.HEAD_GRID if persistent else 1 if op == D.LMHEADQ else (N // 64 if N % 64 == 0 else N // 32 if N % 32 == 0 else N // 16)
    extra = 1
    lg = np.full((B + extra, N), SENT_F32, np.float32)
    cap = (B + extra) * parts
    pv, pi = np.full(cap, SENT_F32, np.float32), np.full(cap, -77, np.int32)
    rc, n_parts, route = probe(eng, op, D.x_bits(d["X"], B), W, scales, biases, bf16_bits(d["nw"]), logits=lg, pv=pv, pi=pi, B=B, N=N, K=K,
                               generic=generic, bits=bits, sb_f32=sbf, in_extra=1, out_extra=extra, part_cap=cap)
    eng.check(rc)
    assert route == int(persistent), f"ran the {'persistent' if route else 'generic'} head (B {B})"
    assert n_parts == parts and (lg[B:] == SENT_F32).all() and (pv[B * parts:] == SENT_F32).all() and (pi[B * parts:] == -77).all()
    tiles = D.head_tiles(N, persistent, order) if op == D.LMHEAD or persistent else [list(range(N // 16))]
    bad = D.partials_defects(lg[:B], pv[:B * parts].reshape(B, parts), pi[:B * parts].reshape(B, parts), tiles)
    assert not bad, (B, bad)
    pairs = D.tie_pairs(N, persistent)[:B]
    first = lg[:B].argmax(1)
    assert [int(a) for a in first[:len(pairs)]] == [p[0] for p in pairs], "a planted pair: the lower copy is not its row's first maximum"
    assert all((lg[:B, lo] == lg[:B, hi]).all() for lo, hi in pairs), "two equal weight rows gave different logits"
    return lg[:B]


@pytest.mark.parametrize("K,N,generic,Bs", D.HEAD_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "B" + "_".join(map(str, v)))
def test_lm_head(eng, knobs, K, N, generic, Bs):
    d = D.head_inputs(K, N, not generic)
    v, mag = D.head_expect(K, N, not generic)
    W = bf16_bits(d["W"])
    worst, base = 0.0, {}
    for B in Bs:
        base[B] = run_head(eng, D.LMHEAD, K, N, generic, d, B, W)
        worst = max(worst, D.frac_bf16(base[B].astype(np.float64), v[:B], mag[:B]))
    assert worst <= 1.0, worst
    assert np.array_equal(run_head(eng, D.LMHEAD, K, N, generic, d, Bs[-1], W), base[Bs[-1]]), "a second launch gave other bits"
    if not generic:                 # request order and cache policy: the same (tile -> k order) sums, so the same bits
        for key, value in (("lmh_order", 0), ("lmh_nt", 0)):
            knobs(key, value)
            for B in Bs[:2]:
                got = run_head(eng, D.LMHEAD, K, N, generic, d, B, W, order=0 if key == "lmh_order" else 1)
                assert np.array_equal(got, base[B]), f"{key} {value} at B {B} is not bit-equal to the default"
            knobs(key, 1)
    print(f"lm head K {K} N {N} {'generic' if generic else 'persistent'} B {Bs}: {worst:.3f} of the bound")


@pytest.mark.parametrize("K,N,generic,bits,sbf,Bs", D.HEADQ_CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "B" + "_".join(map(str, v)))
def test_lm_head_q(eng, knobs, K, N, generic, bits, sbf, Bs):
    d = D.headq_inputs(K, N, bits, sbf, not generic)
    v, mag = D.headq_expect(K, N, bits, sbf, not generic)
    m = d["m"]
    cast = (lambda a: a.astype(np.float32)) if sbf else bf16_bits
    args = (m["words"], cast(m["s"]), cast(m["b"]), bits, sbf)
    worst, base = 0.0, {}
    for B in Bs:
        base[B] = run_head(eng, D.LMHEADQ, K, N, generic, d, B, *args)
        worst = max(worst, D.frac_bf16(base[B].astype(np.float64), v[:B], mag[:B]))
    assert worst <= 1.0, worst
    assert np.array_equal(run_head(eng, D.LMHEADQ, K, N, generic, d, Bs[-1], *args), base[Bs[-1]]), "a second launch gave other bits"
    if not generic and K == 1024:   # the register ring in place of the LDS ring (B <= 32): the same sums
        knobs("lmh_q_ring", 0)
        for B in [b for b in Bs if b <= 32][:2]:
            assert np.array_equal(run_head(eng, D.LMHEADQ, K, N, generic, d, B, *args), base[B]), f"lmh_q_ring 0 at B {B} is not bit-equal"
        knobs("lmh_q_ring", 1)
    print(f"quantised lm head K {K} N {N} {bits} bit {'f32' if sbf else 'bf16'} scales {'generic' if generic else 'persistent'} B {Bs}: "
          f"{worst:.3f} of the bound")


# ---- rmsnorm_rows ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [96, 1024, 1056, 2048, 8, 520])
def test_rmsnorm_rows(eng, K):
    """plain Gaussian rows (ambiguous elements included): every element is one of its two candidates; rows of three scales"""
    rng = np.random.default_rng(K)
    x = G.randn_bf16(rng, (9, K)) * 2.0 ** (np.arange(9) % 3 - 1)[:, None]
    w = D.norm_weight(K)
    _, amb, (lo, hi) = D.rms_stage(x, w)
    for B in (1, 3, 4, 5, 8, 9):
        out = np.full((B + 2, K), SENT, np.uint16)
        rc, _, _ = probe(eng, D.RMSNORM_ROWS, D.x_bits(x, B), nw=bf16_bits(w), out=out, B=B, K=K, in_extra=1, out_extra=2)
        eng.check(rc)
        assert (out[B:] == SENT).all(), "a row after the last was written"
        got = bf16_from_bits(out[:B])
        assert ((got == lo[:B]) | (got == hi[:B])).all(), (K, B)
    print(f"rmsnorm rows K {K}: exact ({int(amb.sum())} of {amb.size} elements have two candidates)")


# ---- greedy tail, embedding lookups -------------------------------------------------------------------------------------------------------------------
def _table(kind, vocab, H):
    """-> (reference table, W, scales, biases, bits, sb_f32)"""
    if kind == "bf16":
        t = G.randn_bf16(np.random.default_rng([vocab, H]), (vocab, H))
        return t, bf16_bits(t), None, None, 0, 0
    bits, sbf = int(kind[1]), int(kind.endswith("f"))
    m = D.quant_matrix(H, vocab, bits, sbf)
    cast = (lambda a: a.astype(np.float32)) if sbf else bf16_bits
    return m, m["words"], cast(m["s"]), cast(m["b"]), bits, sbf


FINALIZE_CONFIGS = ((64, 16, "bf16", 1, 0, 0), (1024, 64, "q4", 0, 1, 40), (1024, 64, "q8f", 1, 0, 5), (1024, 16, "bf16", 1, 1, 40), (64, 64, "q4f", 1, 0, 0))


@pytest.mark.parametrize("n_parts", [1, 256, 257, 600])
@pytest.mark.parametrize("H,half,kind,advance,ignore_eos,clear_words", FINALIZE_CONFIGS)
def test_finalize(eng, H, half, kind, advance, ignore_eos, clear_words, n_parts):
    vocab, max_new, n_rope, extra = 97, 12, 48, 2
    table, W, sc, bi, bits, sbf = _table(kind, vocab, H)
    rng = np.random.default_rng([H, half, n_parts])
    rope = rng.standard_normal((2, n_rope, half)).astype(np.float32)
    for B in (1, 17, 64):
        for scenario in ("plain", "insane", "insane_finished"):
            d = D.finalize_inputs(B, n_parts, vocab, max_new, scenario)
            want = D.finalize_ref(d, table, rope[0], rope[1], advance, ignore_eos)
            R, stride = B + extra, max_new + 1
            tokens = np.full((R, stride), -9, np.int32)
            tokens[:B] = d["tokens"]
            tail = np.concatenate([np.full(clear_words, 0x5eed, np.int32), np.arange(100, 132, dtype=np.int32), [41]]) if clear_words else np.zeros(0, np.int32)
            pad = lambda a: np.concatenate([a, np.full(extra, -9, np.int32)])
            state = np.concatenate([tokens.reshape(-1), pad(d["lens"]), pad(d["finished"]), pad(d["ctx_len"]), [d["n_active"], 0], tail]).astype(np.int32)
            rows = np.full((2, R, half), SENT_F32, np.float32)
            out = np.full((R, H), SENT, np.uint16)
            rc, _, _ = probe(eng, D.FINALIZE, None, W, sc, bi, out=out, pv=d["pv"], pi=d["pi"], state=state, rope=rope, rows=rows, B=B, N=vocab, K=H,
                             bits=bits, sb_f32=sbf, out_extra=extra, n_parts=n_parts, part_cap=B * n_parts, max_new=max_new, max_tokens=d["max_tokens"], eos=d["eos"],
                             ignore_eos=ignore_eos, advance_ctx=advance, clear_words=clear_words, n_rope=n_rope, half=half)
            eng.check(rc)
            what = (B, scenario)
            got_tokens = state[:R * stride].reshape(R, stride)
            lens, fin, ctx = (state[R * stride + i * R:R * stride + (i + 1) * R] for i in range(3))
            assert np.array_equal(got_tokens[:B], want["tokens"]) and (got_tokens[B:] == -9).all(), what
            for name, got in (("lens", lens), ("finished", fin), ("ctx_len", ctx)):
                assert np.array_equal(got[:B], want[name]) and (got[B:] == -9).all(), (name,) + what
            assert state[R * stride + 3 * R] == want["n_active"] and state[R * stride + 3 * R + 1] == want["err"], what
            assert want["err"] == (scenario == "insane")
            if clear_words:
                got_tail = state[R * stride + 3 * R + 2:]
                assert (got_tail[:clear_words] == 0).all() and np.array_equal(got_tail[clear_words:-1], tail[clear_words:-1]) and got_tail[-1] == 42, what
            assert np.array_equal(rows[0, :B], want["cos_rows"]) and np.array_equal(rows[1, :B], want["sin_rows"]) and (rows[:, B:] == SENT_F32).all(), what
            assert np.array_equal(bf16_from_bits(out[:B]), want["x"]) and (out[B:] == SENT).all(), what


@pytest.mark.parametrize("H", [64, 1024])
@pytest.mark.parametrize("kind", ["bf16", "q4", "q4f", "q8", "q8f"])
def test_embed(eng, kind, H):
    vocab, n_audio = 97, 23
    table, W, sc, bi, bits, sbf = _table(kind, vocab, H)
    rng = np.random.default_rng([H, vocab])
    audio = G.randn_bf16(rng, (n_audio, H))
    for B in (1, 17, 64):
        ids = rng.integers(0, vocab, B).astype(np.int32)
        src = np.where(rng.random(B) < 0.4, rng.integers(0, n_audio, B), -1).astype(np.int32)
        src[0], ids[B - 1] = -1, vocab - 1
        if B > 1:
            src[1], src[B - 1], ids[1] = n_audio - 1, -1, -12345          # an audio position's id is never read
        geom = dict(B=B, N=vocab, K=H, bits=bits, sb_f32=sbf, out_extra=1, n_audio=n_audio)
        for epi, state in ((0, np.concatenate([ids, src])), (1, np.where(ids < 0, 0, ids)), (2, np.zeros(1, np.int32))):
            if epi == 2 and (not bits or B > vocab):
                continue
            out = np.full((B + 1, H), SENT, np.uint16)
            r0 = vocab - B if epi == 2 else 0
            eng.check(probe(eng, D.EMBED, bf16_bits(audio), W, sc, bi, out=out, state=np.ascontiguousarray(state, np.int32), epi=epi, r0=r0, **geom)[0])
            if epi == 0:
                want = np.where((src >= 0)[:, None], audio[np.maximum(src, 0)], D.table_rows(table, np.where(src >= 0, 0, ids)))
            else:
                want = D.table_rows(table, np.where(ids < 0, 0, ids) if epi == 1 else np.arange(r0, r0 + B))
            assert np.array_equal(bf16_from_bits(out[:B]), want) and (out[B:] == SENT).all(), (epi, B)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(eng):
    z16, zf, zi = np.zeros(1 << 16, np.uint16), np.zeros(1 << 16, np.float32), np.zeros(1 << 16, np.int32)

    def st(op, **kw):
        geom = dict(B=1, N=16, K=128, in_extra=0, out_extra=0)
        geom.update(kw)
        full = dict(W=z16, scales=z16, biases=z16, nw=z16, out=z16, logits=zf, pv=zf, pi=zi, state=None, rope=None, rows=None)
        for k in [k for k in geom if k in full]:
            full[k] = geom.pop(k)
        return probe(eng, op, z16, **full, **geom)[0]
    q = dict(bits=4)
    assert st(D.GEMV) == 0 and st(D.GEMVQ, **q) == 0 and st(D.RMSNORM_ROWS) == 0
    assert st(D.LMHEAD, part_cap=1) == 0 and st(D.LMHEADQ, part_cap=1, **q) == 0
    assert st(7) == ERR_INVALID
    for B in (0, -1, 65):
        assert st(D.GEMV, B=B) == ERR_INVALID
    assert st(D.GEMV, N=24) == ERR_INVALID and st(D.GEMV, N=48, epi=D.SWIGLU) == ERR_INVALID and st(D.GEMV, N=0) == ERR_INVALID
    assert st(D.GEMV, K=48) == ERR_INVALID and st(D.GEMV, K=16384) == ERR_INVALID and st(D.GEMV, K=4096) == ERR_INVALID    # 4096: behind a norm
    assert st(D.GEMV, epi=4) == ERR_INVALID and st(D.GEMV, generic=2) == ERR_INVALID
    assert st(D.GEMV, epi=D.LOGITS, part_cap=0) == ERR_INVALID and st(D.GEMV, epi=D.LOGITS, part_cap=1) == 0
    assert st(D.GEMV, W=None) == ERR_INVALID and st(D.GEMV, out=None) == ERR_INVALID and st(D.GEMV, epi=D.LOGITS, part_cap=1, pv=None) == ERR_INVALID
    for bits in (0, 2, 3, 16):
        assert st(D.GEMVQ, bits=bits) == ERR_INVALID and st(D.LMHEADQ, bits=bits, part_cap=1) == ERR_INVALID
    assert st(D.GEMVQ, K=96, **q) == ERR_INVALID and st(D.GEMVQ, K=192, **q) == ERR_INVALID and st(D.GEMVQ, K=192, generic=1, **q) == 0
    assert st(D.GEMVQ, epi=D.LOGITS, **q) == ERR_INVALID and st(D.GEMVQ, scales=None, **q) == ERR_INVALID and st(D.GEMVQ, sb_f32=2, **q) == ERR_INVALID
    assert st(D.LMHEAD, nw=None, part_cap=1) == ERR_INVALID and st(D.LMHEAD, epi=1, part_cap=1) == ERR_INVALID
    assert st(D.RMSNORM_ROWS, K=4096) == ERR_INVALID and st(D.RMSNORM_ROWS, K=100) == ERR_INVALID and st(D.RMSNORM_ROWS, nw=None) == ERR_INVALID
    assert st(D.GEMV, in_extra=-1) == ERR_INVALID and st(D.GEMV, out_extra=65) == ERR_INVALID
    # the persistent heads hold 64 rows at K = 1024 and 32 at K = 2048 (lm_head_rows): refused before the launcher would throw; no weight
    # of that size is needed to be refused
    big = dict(N=D.N_HEAD, K=2048, part_cap=1 << 16)
    assert st(D.LMHEAD, B=33, **big) == ERR_INVALID and st(D.LMHEADQ, B=33, bits=4, **dict(big, N=D.N_HEADQ)) == ERR_INVALID
    assert st(D.LMHEAD, B=1, **dict(big, part_cap=100)) == ERR_INVALID       # 256 partials per row
    # FINALIZE / EMBED: ids, rows and positions outside their tables
    i32 = lambda *v: np.array(v, np.int32)
    emb = dict(B=2, N=10, K=64, n_audio=3)
    assert st(D.EMBED, state=i32(1, 9, -1, 2), **emb) == 0
    assert st(D.EMBED, state=i32(1, 10, -1, -1), **emb) == ERR_INVALID and st(D.EMBED, state=i32(-1, 2, -1, -1), **emb) == ERR_INVALID
    assert st(D.EMBED, state=i32(1, 2, 3, -1), **emb) == ERR_INVALID and st(D.EMBED, state=i32(1, 10), epi=1, **emb) == ERR_INVALID
    assert st(D.EMBED, state=i32(0), epi=2, bits=4, r0=9, **emb) == ERR_INVALID and st(D.EMBED, state=i32(0), epi=2, **emb) == ERR_INVALID
    assert st(D.EMBED, state=i32(1, 2, -1, -1), **dict(emb, K=60)) == ERR_INVALID and st(D.EMBED, state=i32(1, 2, -1, -1), bits=4, **dict(emb, K=96)) == ERR_INVALID
    fin = dict(B=1, N=10, K=64, n_parts=1, part_cap=1, max_new=4, max_tokens=4, n_rope=8, half=4, rope=zf, rows=zf)
    ok_state = i32(0, 0, 0, 0, 0, 2, 0, 7, 1, 0)            # tokens [5] | lens | finished | ctx_len | n_active | err
    assert st(D.FINALIZE, state=ok_state.copy(), **fin) == 0
    assert st(D.FINALIZE, state=ok_state.copy(), advance_ctx=1, **fin) == ERR_INVALID                       # position 8 of 8
    assert st(D.FINALIZE, state=i32(0, 0, 0, 0, 0, 5, 0, 0, 1, 0), **fin) == ERR_INVALID                     # lens above max_new
    assert st(D.FINALIZE, state=i32(0, 0, 0, 0, 0, 0, 0, -1, 1, 0), **fin) == ERR_INVALID
    assert st(D.FINALIZE, state=ok_state.copy(), **dict(fin, n_parts=0)) == ERR_INVALID and st(D.FINALIZE, state=ok_state.copy(), **dict(fin, half=257)) == ERR_INVALID
    assert st(D.FINALIZE, state=ok_state.copy(), **dict(fin, part_cap=0)) == ERR_INVALID
    assert st(D.EMBED, state=i32(1, 2, -1, -1), **dict(emb, n_audio=-1)) == ERR_INVALID
    assert st(D.FINALIZE, state=ok_state.copy(), **dict(fin, rope=None)) == ERR_INVALID and st(D.FINALIZE, state=None, **fin) == ERR_INVALID
    assert b"dec case" in eng.lib.qasr_last_error(eng.h)

"""The cases tests/test_gpu_vloc.py compares with the float64 oracle (tests/vloc_oracle.py), their inputs, and TWIN: per case the distance
max |d| / peak between the oracle and its twin (the device's precision plan on the CPU), measured by tests/test_vloc_cpu.py::
test_twin_distance.  The device's distance must lie within MARGIN x that figure.

Weights are synthetic (qasr.synth), bfloat16-valued, on the real widths: "d2" both stacks 2 layers deep, "d12" the real depth, "g2" the
second geometry (patch_size 2, one mu token, 4 K/V heads), "q8" / "q4" the weights of "d2" as an MLX 8-bit / 4-bit checkpoint (the oracle
multiplies by scale q + bias unrounded, as the reference does).  use_mup changes config.json alone.
"""
import functools

import numpy as np

import vloc_oracle as O
from qasr import synth

MARGIN = 4.0

GEOMS = {
    "d2": synth.voxcpm2_local_geometry(2),
    "d2mup": synth.voxcpm2_local_geometry(2, lm__use_mup=True),
    "d12": synth.voxcpm2_local_geometry(12),
    "g2": synth.voxcpm2_local_geometry(2, patch_size=2, mu_tokens=1, lm__num_key_value_heads=4),
}
GEOMS["q8"] = GEOMS["q4"] = GEOMS["d2"]               # "d2" as an MLX 8-bit / 4-bit checkpoint
SEEDS = {"d2": 1, "d2mup": 1, "d12": 2, "g2": 3}
QUANT_BITS = {"q8": 8, "q4": 4}


@functools.lru_cache(maxsize=None)
def stored(name):
    return synth.synth_voxcpm2_local_state_dict(GEOMS[name], seed=SEEDS[name])


@functools.lru_cache(maxsize=None)
def quantized(name):
    """The checkpoint of "q8" / "q4" as stored: triplets of torch tensors"""
    return synth.quantize_voxcpm2_local_state_dict(stored("d2"), QUANT_BITS[name])


@functools.lru_cache(maxsize=None)
def model(name, twin=False):
    if name in QUANT_BITS:
        return O.Model(O.plain(quantized(name)), GEOMS[name], twin=twin)
    return O.Model(stored(name), GEOMS[name], twin=twin)


def normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# name -> (kind, model, parameters)
CASES = {}
for which in ("enc", "dit"):
    for S, n, L, mup in ((1, 1, 1, False), (2, 2, 2, False), (5, 3, 1, True), (11, 7, 2, False), (16, 1, 2, True), (32, 2, 1, False)):
        CASES["stack/%s/S%dn%dL%d%s" % (which, S, n, L, "mup" if mup else "")] = ("stack", "d2mup" if mup else "d2", dict(which=which, S=S, n=n, L=L))
for n in (1, 2, 13, 70):
    CASES["encode/n%d" % n] = ("encode", "d2", dict(n=n))
CASES["mu/B3"] = ("mu", "d2", dict(B=3))
for B, t in ((1, 1.0), (2, 0.37), (3, 0.0)):
    for zero in (False, True):
        CASES["velocity/B%dt%g%s" % (B, t, "zero" if zero else "")] = ("velocity", "d2", dict(B=B, t=t, zero=zero))
for steps, B, cfg in ((1, 1, 2.0), (2, 3, 1.0), (10, 1, 1.0), (10, 3, 2.0)):
    CASES["solve/n%dB%dcfg%g" % (steps, B, cfg)] = ("solve", "d2", dict(steps=steps, B=B, cfg=cfg))
CASES["depth12/velocity"] = ("velocity", "d12", dict(B=1, t=0.37, zero=False))
CASES["depth12/encode"] = ("encode", "d12", dict(n=2))
CASES["geom2/velocity"] = ("velocity", "g2", dict(B=2, t=0.37, zero=False))
CASES["geom2/encode"] = ("encode", "g2", dict(n=3))
for q in ("q8", "q4"):
    CASES["%s/velocity" % q] = ("velocity", q, dict(B=2, t=0.37, zero=False))
    CASES["%s/encode" % q] = ("encode", q, dict(n=3))
CASES["geom2/solve"] = ("solve", "g2", dict(steps=2, B=2, cfg=2.0))


def inputs(name):
    kind, mname, p = CASES[name]
    g = GEOMS[mname]
    P, F, H = g["patch_size"], g["feat_dim"], g["dit"]["hidden_dim"]
    seed = sum(name.encode()) + 1000
    if kind == "stack":
        return dict(x=normal(seed, p["n"], p["S"], g[p["which"]]["hidden_dim"]))
    if kind == "encode":
        return dict(feats=normal(seed, p["n"], P, F))
    if kind == "mu":                                   # bfloat16 values: the load's rounding is then exact and the bound is the f32 sum's
        return dict(lm=synth.bf16_values(normal(seed, p["B"], g["lm"]["hidden_size"])), res=synth.bf16_values(normal(seed + 1, p["B"], g["lm"]["hidden_size"])))
    B = p["B"]
    mu = normal(seed, B, g["mu_tokens"] * H)
    if kind == "velocity":
        return dict(x=normal(seed + 1, B, P, F), mu=np.zeros_like(mu) if p["zero"] else mu, cond=normal(seed + 2, B, P, F))
    return dict(z=normal(seed + 1, B, P, F), mu=mu, cond=normal(seed + 2, B, P, F))


def run(m, name):
    """The case on an oracle model -> {output name: array} (solve: also "least", the smallest |neg|^2 met)."""
    kind, _, p = CASES[name]
    a = inputs(name)
    if kind == "stack":
        return dict(out=m.stack(p["which"], a["x"], p["L"]))
    if kind == "encode":
        cls, emb = m.encode(a["feats"])
        return dict(cls=cls, embed=emb)
    if kind == "mu":
        return dict(mu=m.mu(a["lm"], a["res"]))
    if kind == "velocity":
        return dict(v=m.velocity(a["x"], a["mu"], a["cond"], p["t"]))
    x, d, least, _ = m.solve(a["mu"], a["cond"], a["z"], p["steps"], p["cfg"])
    return dict(x=x, d=d, least=least)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's outputs of a case: computed once, shared, not to be written to."""
    out = run(model(CASES[name][1]), name)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def figures(got, name):
    """{case/output: max |d| / peak} of outputs `got` against the oracle's"""
    ref = reference(name)
    return {"%s/%s" % (name, k): O.rel(got[k], ref[k]) for k in ref if k != "least"}


# measured by test_twin_distance (CPU), which fails when a figure here is off by more than a factor 2
TWIN = {
    "stack/enc/S1n1L1/out": 2.0e-03,
    "stack/enc/S2n2L2/out": 2.5e-03,
    "stack/enc/S5n3L1mup/out": 2.2e-03,
    "stack/enc/S11n7L2/out": 2.9e-03,
    "stack/enc/S16n1L2mup/out": 2.9e-03,
    "stack/enc/S32n2L1/out": 1.7e-03,
    "stack/dit/S1n1L1/out": 2.2e-03,
    "stack/dit/S2n2L2/out": 2.9e-03,
    "stack/dit/S5n3L1mup/out": 2.2e-03,
    "stack/dit/S11n7L2/out": 3.3e-03,
    "stack/dit/S16n1L2mup/out": 2.4e-03,
    "stack/dit/S32n2L1/out": 1.5e-03,
    "encode/n1/cls": 2.9e-03,
    "encode/n1/embed": 3.8e-03,
    "encode/n2/cls": 3.7e-03,
    "encode/n2/embed": 3.9e-03,
    "encode/n13/cls": 3.5e-03,
    "encode/n13/embed": 3.8e-03,
    "encode/n70/cls": 3.6e-03,
    "encode/n70/embed": 3.3e-03,
    "mu/B3/mu": 2.4e-07,
    "velocity/B1t1/v": 4.1e-03,
    "velocity/B1t1zero/v": 5.1e-03,
    "velocity/B2t0.37/v": 3.4e-03,
    "velocity/B2t0.37zero/v": 4.0e-03,
    "velocity/B3t0/v": 4.5e-03,
    "velocity/B3t0zero/v": 3.7e-03,
    "solve/n1B1cfg2/x": 0.0e+00,
    "solve/n1B1cfg2/d": 0.0e+00,
    "solve/n2B3cfg1/x": 1.9e-03,
    "solve/n2B3cfg1/d": 3.9e-03,
    "solve/n10B1cfg1/x": 1.3e-03,
    "solve/n10B1cfg1/d": 3.7e-03,
    "solve/n10B3cfg2/x": 2.3e-03,
    "solve/n10B3cfg2/d": 5.5e-03,
    "depth12/velocity/v": 7.0e-03,
    "depth12/encode/cls": 5.4e-03,
    "depth12/encode/embed": 6.0e-03,
    "geom2/velocity/v": 3.4e-03,
    "geom2/encode/cls": 3.2e-03,
    "geom2/encode/embed": 3.6e-03,
    "q8/velocity/v": 5.1e-03,
    "q8/encode/cls": 3.9e-03,
    "q8/encode/embed": 5.1e-03,
    "q4/velocity/v": 4.7e-03,
    "q4/encode/cls": 4.0e-03,
    "q4/encode/embed": 5.1e-03,
    "geom2/solve/x": 3.5e-03,
    "geom2/solve/d": 6.9e-03,
}

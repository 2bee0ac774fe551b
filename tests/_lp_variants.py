"""Helpers of tests/test_lp_variants.py (TEST INFRASTRUCTURE): models whose tableau is a dense-LP(M, N, seed) with holes, seeded
variants that keep a model's structure, a variant as the LP tuple tests/_lp_batch.py works with (always from
tableau_model(apply_variant(model, variant)), never from the patch), the packing of a model and its variants for
yalps_lpvar_solve, the spelling of a compiled lp_variants kernel symbol."""
import math

import numpy as np

from tests import _census
from yalps_amd.model import apply_variant, entries, tableau_model, tableau_model_with_bounds, variant_patch

KERNEL_LANES = {0: 256, 1: 256, 2: 256, 3: 1024, 4: 1024}  # the class table of wg_queue_host.inc, which lp_variants.hip includes


def kernel_of(cls, check):
    return "lp_variants_kernel<%d%s%s>" % (KERNEL_LANES[cls], ",check" if check else "", ",lds" if cls < 4 else "")


def spelling(symbol):
    """lp_variants_kernel<T[,check][,lds]> | lp_variants_base_kernel of a mangled symbol, as yalps_lpvar_info spells it."""
    name, args = _census.parse(symbol)
    if name == "lp_variants_base_kernel":
        assert not args, symbol
        return name
    assert name == "lp_variants_kernel" and len(args) == 3, (symbol, name, args)
    lanes, check, lds = args
    return "lp_variants_kernel<%d%s%s>" % (lanes, ",check" if check else "", ",lds" if lds else "")


def is_hole(r, j):
    return (3 * r + j) % 11 == 0


def dense_model(oracle, M, N, seed, holes=True):
    """A maximisation whose tableau is dense-LP(M, N, seed) (objective row and right-hand sides positive, coefficients in
    [0, 1)): constraint "c<r>" = {"max": rhs}, variable "x<j>".  holes: the coefficients (r, j) with is_hole are left out of
    the model, so that the base tableau lacks cells a variant can add."""
    m = oracle.dense_lp(M, N, seed).reshape(M + 1, N + 1)
    constraints = {"c%d" % r: {"max": float(m[r, 0])} for r in range(1, M + 1)}
    variables = {}
    for j in range(1, N + 1):
        coefs = {"obj": float(m[0, j])}
        for r in range(1, M + 1):
            if not (holes and is_hole(r, j)):
                coefs["c%d" % r] = float(m[r, j])
        variables["x%d" % j] = coefs
    return {"direction": "maximize", "objective": "obj", "constraints": constraints, "variables": variables}


def shape_variants(M, N):
    """The 8 variants every shape is run with: the empty patch, column 0 only, row 0 only, the last column (with odd N its
    neighbour in the 16-byte unit is the pitch padding), cells the base lacks (dense_model's holes), a mixture, a
    right-hand side below zero (phase 1 runs), right-hand sides of 0."""
    last = "x%d" % N
    holes = [(r, j) for j in range(1, N + 1) for r in range(1, M + 1) if is_hole(r, j)]
    assert N == 0 or M == 0 or holes
    added = {}
    for r, j in holes[:5] + holes[-2:]:
        added.setdefault("x%d" % j, {})["c%d" % r] = 0.5 + 0.01 * r
    rows = sorted({1, max(1, M // 2), M})
    return [
        {},
        {"constraints": {"c%d" % r: {"max": 2.5 + r} for r in rows}},
        {"variables": {"x1": {"obj": 0.75}, last: {"obj": 0.125}}},
        {"variables": {last: dict({"c%d" % r: 0.25 + 0.001 * r for r in range(1, M + 1)}, obj=0.9)}},
        {"variables": added},
        {"constraints": {"c%d" % M: {"max": 1.5}}, "variables": {"x1": {"c1": 0.3, "obj": 0.2}, last: {"c%d" % M: 0.7}}},
        {"constraints": {"c1": {"max": -0.5}}, "variables": {"x1": {"c1": -1.0}}},
        {"constraints": {"c%d" % r: {"max": 0} for r in rows}},
    ]


def kind_of(lower, upper):
    return math.isfinite(lower), math.isfinite(upper)


def seeded_variant(model, rng, n_constraints=3, n_variables=3):
    """A variant of `model` that keeps the structure: replaced bounds with the finite sides of the base's merged bound (0,
    negative and equal values among them), changed and newly added objective and constraint coefficients."""
    tabmod, info = tableau_model_with_bounds(model, sparse=True)
    bounds, objective = info["bounds"], info["objective"]
    variant = {"constraints": {}, "variables": {}}
    keys = list(bounds)
    values = [0, -3.5, 7.25, float(rng.integers(-20, 20)), 0.0]
    for k in rng.permutation(len(keys))[:n_constraints]:
        key, b = keys[k], bounds[keys[k]]
        lo, up = kind_of(b["lower"], b["upper"])
        a = values[int(rng.integers(len(values)))]
        if lo and up:
            pick = int(rng.integers(3))
            variant["constraints"][key] = [{"equal": a}, {"min": a, "max": a}, {"min": a - 2, "max": a + 1.5}][pick]
        elif up:
            variant["constraints"][key] = {"max": a}
        elif lo:
            variant["constraints"][key] = {"min": a}
        else:
            variant["constraints"][key] = {}
    variables = tabmod.variables
    for k in rng.permutation(len(variables))[:n_variables]:
        key, coefs = variables[k]
        have = [c for c, _ in entries(coefs)]
        over = {}
        if have:
            over[have[int(rng.integers(len(have)))]] = float(rng.integers(-9, 9)) / 4  # a changed coefficient (0 among them)
        lacking = [c for c in keys if c not in have]
        if lacking:
            over[lacking[int(rng.integers(len(lacking)))]] = 1.0 + float(rng.random())  # a new one
        if objective is not None:
            over[objective] = float(rng.integers(-5, 6))
        variant["variables"][key] = over
    return variant


def patched_matrix(tabmod, patch):
    """The base tableau's cells with the patch written over them, dense."""
    t = tabmod.tableau
    row, col, val = t.cells
    m = np.zeros(t.width * t.height, np.float64)
    m[row.astype(np.int64) * t.width + col] = val
    prow, pcol, pval = patch
    m[prow.astype(np.int64) * t.width + pcol] = pval
    return m


def variant_lp(model, variant, options=None):
    """The LP a variant stands for, as tests/_lp_batch.py takes it: cells of tableau_model(apply_variant(model, variant))."""
    o = dict(precision=1e-8, maxPivots=8192.0, checkCycles=False)
    o.update(options or {})
    t = tableau_model(apply_variant(model, variant), sparse=True).tableau
    return (t.width, t.height, *t.cells, o["precision"], float(o["maxPivots"]), bool(o["checkCycles"]))


def packed(nat, model, variants, options=None):
    """PackedVariants of a model and its (structure-keeping) variants, patches by variant_patch."""
    tabmod, info = tableau_model_with_bounds(model, sparse=True)
    patches = [variant_patch(tabmod, info, v) for v in variants]
    assert all(p is not None for p in patches)
    options = options if isinstance(options, (list, tuple)) else [options] * len(variants)
    triples = []
    for o in options:
        d = dict(precision=1e-8, maxPivots=8192.0, checkCycles=False)
        d.update(o or {})
        triples.append((d["precision"], d["maxPivots"], d["checkCycles"]))
    t = tabmod.tableau
    return nat.PackedVariants(t.width, t.height, *t.cells, patches, triples)

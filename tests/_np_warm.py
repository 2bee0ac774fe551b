"""Helpers of tests/test_lp_warm.py (TEST INFRASTRUCTURE): the warm tableau of include/yalps_lpwarm.h restated in numpy, the
same in exact arithmetic next to the tableau reached by pivoting, the C oracle started from it, the oracle as the warm backend
of solve._reoptimize_variants_with, the variants and shapes of the tests.

The warm tableau (w = width, F / pos = the base's final matrix and positionOfVariable, b0 = the base's initial tableau, 0
where no cell was written, d = patch value - b0[cell], cells with d == 0.0 dropped, every product and sum rounded alone):
  1. column 0 cells (r, 0), r >= 1, in patch order, p = pos[w + r]:
       p < w: W[i,0] = W[i,0] + d * W[i,p] for every row i;   else: W[p-w,0] += d
  2. row 0 cells (0, c), c >= 1, in patch order, on the column 0 step 1 left, p = pos[c]:
       p < w: W[0,p] += d;   else: W[0,j] = W[0,j] - d * W[p-w,j] for every column j, column 0 included"""
import math
from fractions import Fraction

import numpy as np

from tests import _cases as K
from tests import _lp_batch as LB
from tests import _lp_variants as V
from yalps_amd.model import apply_variant, tableau_model, tableau_model_with_bounds, variant_patch_cells

KERNEL_LANES = V.KERNEL_LANES
IMAGE_KERNEL = "lp_warm_image_kernel"


def kernel_of(cls, check):
    return "lp_warm_kernel<%d%s%s>" % (KERNEL_LANES[cls], ",check" if check else "", ",lds" if cls < 4 else "")


def spelling(symbol):
    """lp_warm_kernel<T[,check][,lds]> | lp_warm_image_kernel | lp_batch_kernel<...> of a mangled symbol."""
    from tests import _census
    name, args = _census.parse(symbol)
    if name == IMAGE_KERNEL:
        return name
    assert name in ("lp_warm_kernel", "lp_batch_kernel") and len(args) == 3, (symbol, name, args)
    lanes, check, lds = args
    return "%s<%d%s%s>" % (name, lanes, ",check" if check else "", ",lds" if lds else "")


# ------------------------------------------------------------------------------------------------ the definition

def edge_cells(cells, w):
    """{flat index: value} of the cells of row 0 and column 0 among (row, col, val)."""
    row, col, val = cells
    keep = (row == 0) | (col == 0)
    return dict(zip((row[keep].astype(np.int64) * w + col[keep]).tolist(), val[keep].tolist()))


def warm_tableau(F, pos, b0, patch, number=float):
    """W of the definition.  F: (h, w) array (float64, or objects of exact numbers); b0: {flat index: value} of the base's
    initial row 0 and column 0; patch: [(flat index, value)] in patch order, row 0 and column 0 only.  A new array."""
    h, w = F.shape
    W = F.copy()
    cells = []
    for k, v in patch:
        r, c = divmod(int(k), w)
        assert (r == 0) != (c == 0), "a warm patch holds cells of row 0 and column 0 only, never (0, 0)"
        d = number(v) - number(b0.get(int(k), 0.0))
        if d == 0:
            continue
        cells.append((r, c, d))
    for r, c, d in cells:
        if c != 0:
            continue
        p = int(pos[w + r])
        if p < w:
            W[:, 0] = W[:, 0] + d * W[:, p]
        else:
            W[p - w, 0] = W[p - w, 0] + d
    for r, c, d in cells:
        if r != 0:
            continue
        p = int(pos[c])
        if p < w:
            W[0, p] = W[0, p] + d
        else:
            W[0, :] = W[0, :] - d * W[p - w, :]
    return W


def exact_pivot(M, pos, var, row, col):
    """src/simplex.ts:5-39 without its flushes, on exact numbers, in place."""
    h, w = M.shape
    q = M[row, col]
    leaving, entering = var[w + row], var[col]
    var[w + row], var[col] = entering, leaving
    pos[leaving], pos[entering] = col, w + row
    M[row, :] = M[row, :] / q
    M[row, col] = 1 / q
    for r in range(h):
        if r == row:
            continue
        coef = M[r, col]
        if coef == 0:
            continue
        M[r, :] = M[r, :] - coef * M[row, :]
        M[r, col] = -coef / q
    return M


def fractions_of(m, w, h):
    return np.array([Fraction(float(x)) for x in m], dtype=object).reshape(h, w)


def exact_along(m, w, h, trace):
    """(matrix of Fractions, pos, var) after pivoting the dense tableau m along trace [(row, col)]."""
    M = fractions_of(m, w, h)
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    for row, col in trace:
        exact_pivot(M, pos, var, int(row), int(col))
    return M, pos, var


# ------------------------------------------------------------------------------------------------ the oracle from a warm start

def dense_of(cells, w, h):
    row, col, val = cells
    m = np.zeros(w * h, np.float64)
    m[row.astype(np.int64) * w + col] = val
    return m


def solve_base(oracle, cells, w, h, precision=1e-8, max_pivots=8192.0, check_cycles=False, trace_cap=0):
    """The base by the oracle: dict(status, result, n_pivots, matrix (flat), pos, var, trace)."""
    m = dense_of(cells, w, h)
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    status, result, npiv, trace = oracle.simplex(m, w, h, pos, var, precision=precision, max_pivots=max_pivots,
                                                 check_cycles=check_cycles, trace_cap=trace_cap)
    return dict(status=status, result=result, n_pivots=npiv, matrix=m, pos=pos, var=var, trace=trace)


def warm_answer(oracle, base, w, h, b0, patch, precision=1e-8, max_pivots=8192.0, check_cycles=False):
    """The oracle started from the warm tableau and the base's permutations, as LB.oracle_answer's dict, plus `start`."""
    with np.errstate(all="ignore"):
        W = warm_tableau(base["matrix"].reshape(h, w), base["pos"], b0, patch)
    m = np.ascontiguousarray(W).reshape(-1).copy()
    pos, var = base["pos"].copy(), base["var"].copy()
    status, result, npiv, _ = oracle.simplex(m, w, h, pos, var, precision=precision, max_pivots=max_pivots, check_cycles=check_cycles)
    return dict(status=status, result=result, n_pivots=npiv, matrix=m, pos=pos, var=var, start=W)


def oracle_warm_backend(oracle, log=None):
    """warm_backend of solve._reoptimize_variants_with by the C oracle and warm_tableau; log (a list) receives every call's
    (patches, options)."""
    def backend(tableau, base_options, patches, options, stats=None):
        w, h = tableau.width, tableau.height
        o = base_options
        base = solve_base(oracle, tableau.cells, w, h, o["precision"], o["maxPivots"], o["checkCycles"])
        if log is not None:
            log.append((patches, options))
        if stats is not None:
            stats.update(launches=0, reruns=0, kernels=[])
        head = (base["status"], base["result"], base["n_pivots"])
        if base["status"] != "optimal":
            return head, None
        b0 = edge_cells(tableau.cells, w)
        out = []
        for patch, o in zip(patches, options):
            a = warm_answer(oracle, base, w, h, b0, patch, o["precision"], o["maxPivots"], o["checkCycles"])
            out.append((a["status"], a["result"], a["n_pivots"], a["matrix"][::w].copy(), a["pos"], a["var"]))
        if stats is not None:
            stats.update(launches=1, kernels=["oracle"])
        return head, out
    return backend


def oracle_cold(oracle):
    """cold_fn of _reoptimize_variants_with: solve_variants with the oracle behind it."""
    from tests.test_lp_variants import oracle_solve_many, oracle_variants_backend
    from yalps_amd import solve as S
    _, many = oracle_solve_many(oracle)
    return lambda model, variants, options, stats: S._solve_variants_with(oracle_variants_backend(oracle), many, model, variants,
                                                                          options, stats)


# ------------------------------------------------------------------------------------------------ the golden models' variants

N_VARIANTS = 24
GOLDEN_LPS, NON_OPTIMAL = 23, 8


def golden_lp_cases(oracle):
    """(cases whose base ends optimal, cases whose base does not): the golden models without integers and within 4 MiB, each
    solved with its own options by the oracle."""
    good, bad = [], []
    for name in K.names():
        case = K.load(name)
        t = tableau_model(case["model"], sparse=True)
        if t.integers or 8 * t.tableau.width * t.tableau.height > LB.MAX_BYTES:
            continue
        o = case["options"]
        base = solve_base(oracle, t.tableau.cells, t.tableau.width, t.tableau.height, o["precision"], o["maxPivots"], o["checkCycles"])
        (good if base["status"] == "optimal" else bad).append(case)
    return good, bad


def objective_only(model, variant):
    """The variant with its "variables" part cut down to the objective key."""
    objective = model.get("objective")
    out = {"constraints": variant.get("constraints") or {}, "variables": {}}
    for key, over in (variant.get("variables") or {}).items():
        if objective is not None and objective in over:
            out["variables"][key] = {objective: over[objective]}
    return out


def golden_variants(model):
    """The 24 structure-keeping variants of one golden model: seeded bounds and objective coefficients."""
    rng = np.random.default_rng(7)
    return [objective_only(model, V.seeded_variant(model, rng, n_constraints=1 + k % 3, n_variables=k % 3)) for k in range(N_VARIANTS)]


def midpoint_moves(model, sens):
    """Single-bound moves of a model whose base is optimal: every finite side of every merged constraint, once towards each
    end of its range in sens = sensitivity(model)["sensitivity"] -- to the midpoint between the bound and the end where the
    end is finite, by -1 / +1 where it is not -- with the other side held.  [(variant, label)]."""
    _, info = tableau_model_with_bounds(model, sparse=True)
    out = []
    for key, entry in sens["constraints"]:
        b = info["bounds"][key]
        for side, name in (("upper", "upper_range"), ("lower", "lower_range")):
            if name not in entry:
                continue
            for end, step in zip(entry[name], (-1.0, 1.0)):
                moved = (b[side] + end) / 2 if math.isfinite(end) else b[side] + step
                if moved == b[side]:
                    continue  # (a range that ends at the bound itself: nothing moves)
                sides = {"upper": b["upper"], "lower": b["lower"], side: moved}
                constraint = {k: v for k, v in (("min", sides["lower"]), ("max", sides["upper"])) if math.isfinite(v)}
                out.append(({"constraints": {key: constraint}}, "%s %s -> %r" % (key, side, moved)))
    return out


# ------------------------------------------------------------------------------------------------ native packing

def packed_cells(nat, base_lp, patches, options=None, base_options=(1e-8, 8192.0, False)):
    """PackedWarm of a base LP (tests/_lp_batch.py's tuple) and per-variant patches [(flat index, value)] in patch order."""
    w, h = base_lp[:2]
    as_arrays = [(np.array([k // w for k, _ in p], np.int32), np.array([k % w for k, _ in p], np.int32),
                  np.array([v for _, v in p], np.float64)) for p in patches]
    return nat.PackedWarm(w, h, *base_lp[2:5], as_arrays, options, base_options=base_options)


def check_variant(lw, i, out, ref, w, h, label=""):
    """Variant i of LpWarm's last solve against warm_answer's dict, bit for bit: status, pivots, result, both permutations,
    column 0 and the kept matrix."""
    LB.check_lp(lw, i, out, ref, (w, h), tableau=True, label=label)


# ------------------------------------------------------------------------------------------------ a handle on a caller's stream

def caller_stream_child(path):
    """tests/test_lp_warm.py::ending_variants through an LpWarm on a stream torch made, its outputs to `path` (.npz).  A process
    of its own, for the reason tests/_variant_shapes.py::caller_stream_child gives: torch has to be loaded before the library."""
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from tests import _oracle, _variant_shapes as VS
    from tests.test_lp_warm import ending_variants
    from yalps_amd import _native as nat
    lp, _, rows, _ = ending_variants(_oracle.load())
    stream = torch.cuda.Stream()
    lw = nat.LpWarm(0, stream=stream.cuda_stream)
    try:
        out = lw.solve(packed_cells(nat, lp, [p for _, p, _ in rows], [o for _, _, o in rows], base_options=(1e-8, math.inf, False)),
                       keep_tableaux=True)
        np.savez(path, **VS.outputs(lw, out, len(rows)))
    finally:
        lw.close()  # (before the stream is dropped)
    del stream


if __name__ == "__main__":
    import sys
    caller_stream_child(sys.argv[1])

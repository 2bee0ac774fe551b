"""Helpers of tests/test_lp_sensitivity.py (TEST INFRASTRUCTURE): the reference of lp_sens_kernel's five arrays -- a plain
numpy restatement of include/yalps_lpsens.h from a final matrix, applied to the matrix the C oracle leaves -- the comparisons,
and the oracle as the backends of yalps_amd.sensitivity._sensitivity_many_with.  Shares no code with the product."""
import numpy as np

from tests import _census
from tests import _lp_batch as LB


def restate(matrix, w, h, p):
    """(row0, col_up, col_dn, row_lo, row_hi) of a final matrix M (flat row-major w * h) at precision p:
         row0[c]   = M[0,c]
         col_up[c] = min{ M[r,0] /  M[r,c] : 1 <= r < h, M[r,c] >  p }      col_dn[c] = min{ M[r,0] / -M[r,c] : M[r,c] < -p }
         row_lo[r] = max{ M[0,c] /  M[r,c] : 1 <= c < w, M[r,c] >  p }      row_hi[r] = min{ M[0,c] /  M[r,c] : M[r,c] < -p }
       an empty set gives +inf (row_lo: -inf), entry 0 of the four ratio arrays is 0.0, a NaN quotient is ignored."""
    M = np.array(matrix[:w * h], np.float64).reshape(h, w)
    row0 = M[0].copy()
    col_up, col_dn = np.zeros(w), np.zeros(w)
    row_lo, row_hi = np.zeros(h), np.zeros(h)
    A, b, k = M[1:, 1:], M[1:, 0][:, None], M[0, 1:][None, :]
    pos, neg = A > p, A < -p
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        masked = lambda num, den, mask, fill: np.where(mask, np.divide(num, den), fill)
        col_up[1:] = np.fmin.reduce(masked(b, A, pos, np.inf), axis=0, initial=np.inf)
        col_dn[1:] = np.fmin.reduce(masked(b, np.negative(A), neg, np.inf), axis=0, initial=np.inf)
        row_lo[1:] = np.fmax.reduce(masked(k, A, pos, -np.inf), axis=1, initial=-np.inf)
        row_hi[1:] = np.fmin.reduce(masked(k, A, neg, np.inf), axis=1, initial=np.inf)
    return row0, col_up, col_dn, row_lo, row_hi


def check_ranges(got, want, tag=""):
    """row0 bit for bit; the four ratio arrays equal as numbers, infinities included (+0.0 == -0.0)."""
    names = ("row0", "col_up", "col_dn", "row_lo", "row_hi")
    assert len(got) == len(want) == 5
    assert LB.same_words(got[0], want[0]), (tag, "row0")
    for name, g, e in zip(names[1:], got[1:], want[1:]):
        assert g.shape == e.shape and not np.isnan(g).any() and not np.isnan(e).any(), (tag, name)
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (tag, name, bad[:5], g[bad[:5]], e[bad[:5]])


def check_lp(sens, i, out, ref, lp, tag=""):
    """LP i of an LpSens solve (keep_tableaux) against the oracle's answer: the solve as _lp_batch.check_lp compares it, then
    the ranges against the restatement on the oracle's matrix -- or, where the LP did not end optimal, no ranges."""
    LB.check_lp(sens, i, out, ref, lp, label=tag)
    if ref["status"] == "optimal":
        check_ranges(sens.ranges(i), restate(ref["matrix"], lp[0], lp[1], lp[5]), (i, tag))
    else:
        no_ranges(sens, i)


def no_ranges(sens, i):
    from yalps_amd import _native
    try:
        sens.ranges(i)
    except _native.NativeError as e:
        assert "error -1" in str(e) and "did not end optimal" in str(e), e  # YALPS_E_ARG
    else:
        raise AssertionError("LP %d did not end optimal and has ranges" % i)


def spelling(symbol):
    """lp_sens_kernel<T[,check][,lds]> of a mangled symbol, as yalps_lpsens_info spells the kernel it launched."""
    name, args = _census.parse(symbol)
    assert name == "lp_sens_kernel" and len(args) == 3, (symbol, name, args)
    lanes, check, lds = args
    return "lp_sens_kernel<%d%s%s>" % (lanes, ",check" if check else "", ",lds" if lds else "")


def oracle_one(oracle, tableau, opt):
    """(status, result, ranges | None) of one sparse-built tableau by the oracle and the restatement; column 0 and the
    permutations of the final tableau are left in it, as the device backends leave them."""
    assert tableau.matrix is None and tableau.cells is not None
    w, h = tableau.width, tableau.height
    row, col, val = tableau.cells
    m = np.zeros(w * h)
    m[row.astype(np.int64) * w + col] = val
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    status, result, _, _ = oracle.simplex(m, w, h, pos, var, precision=opt["precision"], max_pivots=opt["maxPivots"],
                                          check_cycles=opt["checkCycles"])
    tableau.col0, tableau.position_of_variable, tableau.variable_at_position = m[::w][:h].copy(), pos, var
    return status, result, restate(m, w, h, opt["precision"]) if status == "optimal" else None


def oracle_backends(oracle, seen=None):
    """(batch_backend, large_backend) for _sensitivity_many_with; `seen` (a dict) counts what went which way."""
    def batch(tableaux, options, stats=None):
        if seen is not None:
            seen["batch_calls"] = seen.get("batch_calls", 0) + 1
            seen["batched"] = seen.get("batched", 0) + len(tableaux)
        return [oracle_one(oracle, t, o) for t, o in zip(tableaux, options)]

    def large(tableau, opt):
        if seen is not None:
            seen["large"] = seen.get("large", 0) + 1
        return oracle_one(oracle, tableau, opt)
    return batch, large


def oracle_sensitivity(oracle, models, options=None, stats=None):
    from yalps_amd.sensitivity import _sensitivity_many_with
    return _sensitivity_many_with(*oracle_backends(oracle), models, options, stats)

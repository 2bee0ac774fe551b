"""Helpers of tests/test_lp_batch.py (TEST INFRASTRUCTURE): LPs as yalps_lpbatch_solve takes them -- (width, height, row, col,
val, precision, max_pivots, check_cycles) -- made from golden records, edge records, dense-LP(M, N, seed) and models; the C
oracle's answer for one of them; the bit-for-bit comparison; the spelling of a compiled lp_batch_kernel symbol."""
import numpy as np

from tests import _census
from tests import _edges as E
from tests import _golden as G

MAX_BYTES = 4 << 20
SMALL_LDS_MAX = 150 * 1024
BOUNDS = (19 * 1024, 39 * 1024, 79 * 1024, SMALL_LDS_MAX)  # LDS bytes of the classes 0..3; class 4 is the HBM form


def lds_bytes(w, h):
    """small_lds_bytes (yalps_amd/csrc/wg_simplex.cuh), restated: tableau at the LDS pitch, rhs, colbuf, prow, both permutations."""
    lp = ((w - 1 + 1) & ~1) | 2
    return 8 * (h * lp + 2 * h + lp) + 4 * 2 * (w + h + 1)


def size_class(w, h):
    if w < 1 or h < 1 or 8 * w * h > MAX_BYTES:
        return -1
    return next((k for k, b in enumerate(BOUNDS) if lds_bytes(w, h) <= b), len(BOUNDS))


def cells_of(matrix, w, h):
    """Every entry of a dense tableau whose bits are not +0.0, sorted by (row, col)."""
    idx = np.flatnonzero(np.ascontiguousarray(matrix[:w * h]).view(np.int64))
    return (idx // w).astype(np.int32), (idx % w).astype(np.int32), np.ascontiguousarray(matrix[idx])


def scatter(lp):
    """The dense row-major tableau the device assembles from an LP's cells."""
    w, h, row, col, val = lp[:5]
    m = np.zeros(w * h, np.float64)
    m[row.astype(np.int64) * w + col] = val
    return m


def from_dense(matrix, w, h, precision=1e-8, max_pivots=8192.0, check_cycles=False):
    return (w, h, *cells_of(matrix, w, h), precision, float(max_pivots), bool(check_cycles))


def dense_lp(oracle, M, N, seed, **opts):
    return from_dense(oracle.dense_lp(M, N, seed), N + 1, M + 1, **opts)


def record_lp(rec, oracle):
    o = G.options(rec)
    return from_dense(G.initial_matrix(rec, oracle), rec["width"], rec["height"], o["precision"], o["max_pivots"], o["check_cycles"])


def edge_lp(rec, oracle):
    o = G.options(rec)
    return from_dense(E.initial(rec, oracle.dense_lp), rec["width"], rec["height"], o["precision"], o["max_pivots"], o["check_cycles"])


def model_lp(tabmod, options):
    t = tabmod.tableau
    return (t.width, t.height, *t.cells, options["precision"], float(options["maxPivots"]), bool(options["checkCycles"]))


def oracle_answer(oracle, lp):
    w, h, _, _, _, precision, max_pivots, check = lp
    m = scatter(lp)
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    status, result, npiv, _ = oracle.simplex(m, w, h, pos, var, precision=precision, max_pivots=max_pivots, check_cycles=check)
    return dict(status=status, result=result, n_pivots=npiv, matrix=m, pos=pos, var=var)


def same_words(a, b, canonical_nan=False):
    """Bit for bit; canonical_nan: NaN at the same positions (whatever their signs and payloads), bit for bit elsewhere."""
    if canonical_nan:
        a, b = G.canon(a), G.canon(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_lp(batch, i, out, ref, lp, tableau=True, label="", canonical_nan=False):
    """LP i of the batch's last solve against the oracle's answer (or a golden record's: matrix None, final_sha256 set).
    canonical_nan: all NaNs are one value (the oracle's answer only)."""
    assert not canonical_nan or ref.get("matrix") is not None
    statuses, results, pivots = out[:3]
    w, h = lp[0], lp[1]
    tag = "LP %d %s (%dx%d)" % (i, label, h, w)
    assert statuses[i] == ref["status"], (tag, statuses[i], ref["status"])
    assert int(pivots[i]) == ref["n_pivots"], (tag, int(pivots[i]), ref["n_pivots"])
    assert G.same_number(float(results[i]), ref["result"]), (tag, float(results[i]), ref["result"])
    col0, pos, var = batch.solution(i)
    assert np.array_equal(pos, ref["pos"]) and np.array_equal(var, ref["var"]), tag
    if ref.get("matrix") is not None:
        assert same_words(col0, ref["matrix"].reshape(h, w)[:, 0], canonical_nan), tag
    elif ref.get("col0") is not None:
        assert same_words(col0, ref["col0"]), tag
    else:
        assert G.sha256(col0) == ref["col0_sha256"], tag
    if tableau:
        m = batch.tableau(i)
        if ref.get("matrix") is not None:
            assert same_words(m, ref["matrix"], canonical_nan), tag
        else:
            assert G.sha256(m) == ref["final_sha256"], tag
        assert same_words(np.ascontiguousarray(m.reshape(h, w)[:, 0]), col0, canonical_nan), tag


def spelling(symbol):
    """lp_batch_kernel<T[,check][,lds]> of a mangled symbol, as yalps_lpbatch_info spells the kernel it launched."""
    name, args = _census.parse(symbol)
    assert name == "lp_batch_kernel" and len(args) == 3, (symbol, name, args)
    lanes, check, lds = args
    return "lp_batch_kernel<%d%s%s>" % (lanes, ",check" if check else "", ",lds" if lds else "")

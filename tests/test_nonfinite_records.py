"""The non-finite records (tests/golden/simplex_nonfinite.json.gz: the reference's src/simplex.ts run on the tableaux and
options of tests/_nonfinite.py) pin the CPU checkers on NaN and infinite input, every family of them does what it is there
for, and tells a right restatement from one that is wrong only for a NaN or an infinity.

Final tableaux are compared with all NaNs made one value (tests/_golden.sha256_canon); the initial ones by their raw bytes."""
import math

import numpy as np
import pytest

from tests import _edges as E
from tests import _golden as G
from tests import _nonfinite as NF
from tests import _np_simplex as NP

RECORDS = G.records("nonfinite")
ALL = [pytest.param(r, id=NF.label(r)) for r in RECORDS]
SMALL = [r for r in RECORDS if r["width"] * r["height"] <= 2_000_000]

# mutant -> the families (tests/_nonfinite.py) whose records must include one that the mutant gets wrong
TARGETS = {
    "flush_le_row": ("N1",),
    "skip_le_coef": ("N1",),
    "nan_min": ("N1",),
    "rc_not_le": ("N1",),
    "rhs_not_ge": ("N4",),
    "inf_q_skip": ("N2",),
    "sentinel": ("N6",),
}


def test_records_cover_every_family_and_path_shape():
    assert {r["family"] for r in RECORDS} == set(NF.FAMILIES)
    assert {(r["M"], r["N"]) for r in RECORDS} == set(E.SHAPES)
    assert sorted((r["family"], r["M"], r["N"], r["seed"]) for r in RECORDS) == sorted(NF.specs())
    for M, N in E.SHAPES:  # (tests/test_nonfinite_paths.py: every path finds N1, N2 and N6 at its shape)
        assert set(NF.PARTITION_FAMILIES) <= {r["family"] for r in RECORDS if (r["M"], r["N"]) == (M, N)}


@pytest.mark.parametrize("rec", ALL)
def test_generator_reproduces_the_initial_tableau(oracle, rec):
    """init_sha256 is of the raw bytes: the planted NaN payloads reached the reference as they were written."""
    m = NF.initial(rec, oracle.dense_lp)  # (asserts init_sha256)
    got, want = NF.options(rec["family"], rec["M"], rec["N"], rec["seed"]), G.options(rec)
    assert got["check_cycles"] == want["check_cycles"]
    assert G.same_number(got["precision"], want["precision"]) and G.same_number(got["max_pivots"], want["max_pivots"])
    assert rec["layout"] == [list(x) for x in E.default_layout(rec["M"], rec["N"])]
    if rec["family"] == "N6":
        c, q, pc, pr, u, uc = NF.n6_sites(rec["M"], rec["N"])
        U = m.view(np.uint64).reshape(rec["height"], rec["width"])
        assert tuple(U[q, pc]) == tuple(U[pr, c]) == tuple(U[u, uc]) == NF.PATTERNS and U[u, pc[0]] == NF.FLUSHED


def _check(run, rec, m):
    exp = G.expected(rec)
    status, result, npiv, pos, var = run
    assert (status, npiv) == (exp["status"], exp["n_pivots"]) and G.same_number(result, exp["result"])
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
    assert NF.col0_matches(m, rec, exp)
    assert G.sha256_canon(m) == exp["final_canon_sha256"]


@pytest.mark.parametrize("rec", ALL)
def test_every_record_does_what_its_family_is_there_for(oracle, rec):
    """From the reference's own pivot sequence, replayed with the oracle's pivot(): the tableau before each pivot shows
    what the family planted reaching the decisions, and the last one is the reference's final tableau."""
    fam, w, h = rec["family"], rec["width"], rec["height"]
    exp = G.expected(rec)
    assert exp["n_pivots"] >= NF.MIN_PIVOTS[fam], (exp["status"], exp["n_pivots"])
    m = NF.initial(rec, oracle.dense_lp)
    o = G.options(rec)
    if fam == "N7":
        budget = E.options("E1", rec["M"], rec["N"], rec["seed"])["max_pivots"]
        if math.isnan(o["precision"]) or o["precision"] == math.inf:
            assert (exp["status"], exp["n_pivots"]) == ("optimal", 0) and math.isnan(exp["result"])
        elif o["precision"] == -1.0:
            assert (exp["status"], exp["n_pivots"]) == ("cycled", budget)
        else:
            assert math.isnan(o["max_pivots"]) or o["max_pivots"] == -1.0
            assert (exp["status"], exp["n_pivots"]) == ("cycled", 0)
        return
    if fam == "N5":
        assert np.isfinite(m).all()
    pos, var = G.identity_perms(rec)
    nan_rows = nan_cols = inf_q = inf_rows = 0
    for k, (row, col) in enumerate(exp["pivots"].tolist()):
        A = m.reshape(h, w)
        nan_rows += bool(np.isnan(A[row]).any())
        nan_cols += bool(np.isnan(A[1:, col]).any())
        inf_q += bool(np.isinf(A[row, col]))
        inf_rows += bool(np.isinf(A[row]).any())
        if fam == "N6" and k == 0:
            U = A.view(np.uint64)
            assert set(NF.PATTERNS) <= set(U[row].tolist()) and set(NF.PATTERNS) <= set(U[1:, col].tolist())
            assert (row, col) == (NF.n6_sites(rec["M"], rec["N"])[1], NF.n6_sites(rec["M"], rec["N"])[0])
        oracle.pivot(m, w, h, pos, var, row, col)
    assert G.sha256_canon(m) == exp["final_canon_sha256"]
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
    if fam == "N1":
        assert nan_rows >= 1 and nan_cols >= 1
    if fam == "N2":
        assert inf_q >= 1
    if fam == "N4":
        assert inf_rows == exp["n_pivots"]
    if fam == "N5":
        assert not np.isfinite(m).all()


@pytest.mark.parametrize("rec", [pytest.param(r, id=NF.label(r)) for r in SMALL])
def test_c_oracle_reproduces_the_nonfinite_records(oracle, rec):
    m = NF.initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    exp = G.expected(rec)
    status, result, npiv, trace = oracle.simplex(m, rec["width"], rec["height"], pos, var, trace_cap=exp["n_pivots"] + 8,
                                                 **G.options(rec))
    assert np.array_equal(trace, exp["pivots"])
    _check((status, result, npiv, pos, var), rec, m)


@pytest.mark.parametrize("rec", [pytest.param(r, id=NF.label(r)) for r in SMALL])
def test_numpy_restatement_reproduces_the_nonfinite_records(oracle, rec):
    m = NF.initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    o = G.options(rec)
    status, result, npiv = NP.simplex(m, rec["width"], rec["height"], pos, var, o["precision"], o["max_pivots"])
    _check((status, result, npiv, pos, var), rec, m)


def _disagrees(oracle, rec, mutant):
    m = NF.initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    o = G.options(rec)
    exp = G.expected(rec)
    status, result, npiv = NP.simplex(m, rec["width"], rec["height"], pos, var, o["precision"], o["max_pivots"], rules={mutant})
    return not ((status, npiv) == (exp["status"], exp["n_pivots"]) and G.same_number(result, exp["result"])
                and np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
                and G.sha256_canon(m) == exp["final_canon_sha256"])


@pytest.mark.parametrize("mutant,family", [(m, f) for m, fams in TARGETS.items() for f in fams])
def test_each_family_rejects_its_mutants(oracle, mutant, family):
    """A restatement that is wrong only for a NaN or an infinity (tests/_np_simplex.py MUTANTS) must disagree with every
    record of the family it targets, up to 2M entries."""
    recs = [r for r in SMALL if r["family"] == family]
    assert recs
    missed = [NF.label(r) for r in recs if not _disagrees(oracle, r, mutant)]
    assert not missed, (mutant, missed)


def test_every_nonfinite_mutant_has_a_target():
    from tests import test_edge_records as T
    assert set(TARGETS) | set(T.TARGETS) | {"keep_col"} == set(NP.MUTANTS)
    assert not set(TARGETS) & set(T.TARGETS)


def test_canonical_digest_ignores_only_the_nan_words():
    a = np.array([1.0, -0.0, math.inf, NF.bits(NF.FLUSHED), NF.bits(NF.PATTERNS[1]), NF.bits(NF.PATTERNS[3])])
    b = np.array([1.0, -0.0, math.inf, math.nan, math.nan, math.nan])
    assert G.sha256(a) != G.sha256(b) and G.sha256_canon(a) == G.sha256_canon(b)
    for i, x in ((0, 1.0000000000000002), (1, 0.0), (2, -math.inf), (3, 0.0)):
        c = b.copy()
        c[i] = x
        assert G.sha256_canon(c) != G.sha256_canon(b)

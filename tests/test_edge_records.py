"""The edge records (tests/golden/simplex_edges.json.gz: the reference's src/simplex.ts run on the tableaux of
tests/_edges.py) pin the CPU checkers, and every family of them tells a right restatement from a wrong one."""
import numpy as np
import pytest

from tests import _edges as E
from tests import _golden as G
from tests import _np_simplex as NP

RECORDS = G.records("edges")
ALL = [pytest.param(r, id=E.label(r)) for r in RECORDS]
SMALL = [r for r in RECORDS if r["width"] * r["height"] <= 2_000_000]

# mutant -> the families (tests/_edges.py) whose records must each include one that the mutant gets wrong
TARGETS = {
    "obj_ge": ("E6b",),
    "tie_col2": ("E1", "E9"),
    "value_ge": ("E6a",),
    "tie_row2": ("E2",),
    "inf_row2": ("E3u",),
    "break_lt": ("E6a",),
    "no_early_break": ("E2b", "E6a"),
    "rhs_le": ("E6b",),
    "tie_row1": ("E1",),
    "coef_le": ("E6c",),
    "tie_col1": ("E1", "E4"),
    "ninf_col1": ("E3i",),
    "flush_ge_row": ("E5",),
    "flush_ge_coef": ("E5",),
    "keep_neg_zero": ("E4",),
    "patch_kept_only": ("E7",),
    "ftz": ("E8",),
}


def test_records_cover_every_family_and_path_shape():
    assert {r["family"] for r in RECORDS} == set(E.FAMILIES)
    assert {(r["M"], r["N"]) for r in RECORDS} == set(E.SHAPES)
    assert sorted((r["family"], r["M"], r["N"], r["seed"]) for r in RECORDS) == sorted(E.specs())


@pytest.mark.parametrize("rec", ALL)
def test_generator_reproduces_the_initial_tableau(oracle, rec):
    m = E.initial(rec, oracle.dense_lp)  # (asserts init_sha256)
    if "init_coo" in rec:
        ref = np.zeros(m.size)
        ref[G._dec(rec["init_coo"]["idx"], np.int32)] = G._dec(rec["init_coo"]["val"], np.float64)
        assert np.array_equal(m.view(np.int64), ref.view(np.int64))
    assert E.options(rec["family"], rec["M"], rec["N"], rec["seed"]) == G.options(rec)
    assert rec["layout"] == [list(x) for x in E.default_layout(rec["M"], rec["N"])]


def _check(run, rec, m):
    exp = G.expected(rec)
    status, result, npiv, pos, var = run
    assert (status, npiv) == (exp["status"], exp["n_pivots"]) and G.same_number(result, exp["result"])
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
    assert G.sha256(m) == exp["final_sha256"]
    assert np.isfinite(m).all(), "the family must keep the run finite"


@pytest.mark.parametrize("omp", [False, True], ids=["oracle", "oracle-omp"])
@pytest.mark.parametrize("rec", ALL)
def test_c_oracles_reproduce_the_edge_records(oracle, rec, omp):
    from tests import _oracle
    orc = _oracle.load(omp=True) if omp else oracle
    if omp:
        assert orc.set_threads(4) == 4
    m = E.initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    exp = G.expected(rec)
    status, result, npiv, trace = orc.simplex(m, rec["width"], rec["height"], pos, var, trace_cap=exp["n_pivots"] + 8,
                                              **G.options(rec))
    assert np.array_equal(trace, exp["pivots"])
    assert E.col0_matches(m, rec, exp)
    _check((status, result, npiv, pos, var), rec, m)


@pytest.mark.parametrize("rec", [p for p in ALL if not p.values[0]["options"]["checkCycles"]])
def test_numpy_restatement_reproduces_the_edge_records(oracle, rec):
    m = E.initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    o = G.options(rec)
    status, result, npiv = NP.simplex(m, rec["width"], rec["height"], pos, var, o["precision"], o["max_pivots"])
    _check((status, result, npiv, pos, var), rec, m)


def _disagrees(oracle, rec, mutant):
    m = E.initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    o = G.options(rec)
    exp = G.expected(rec)
    try:
        status, result, npiv = NP.simplex(m, rec["width"], rec["height"], pos, var, o["precision"], o["max_pivots"],
                                          rules={mutant})
    except (ValueError, IndexError):  # (a mutant that meets a NaN key: no answer is a wrong answer)
        return True
    return not ((status, npiv) == (exp["status"], exp["n_pivots"]) and G.same_number(result, exp["result"])
                and np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"]) and G.sha256(m) == exp["final_sha256"])


@pytest.mark.parametrize("mutant,family", [(m, f) for m, fams in TARGETS.items() for f in fams])
def test_each_family_rejects_its_mutants(oracle, mutant, family):
    """A deliberately wrong restatement (tests/_np_simplex.py MUTANTS) must disagree with at least one record of each
    family it targets; records without checkCycles and of up to 2M entries (the numpy restatement has no hasCycle)."""
    recs = [r for r in SMALL if r["family"] == family and not r["options"]["checkCycles"]]
    assert recs
    assert any(_disagrees(oracle, r, mutant) for r in recs), (mutant, family)


def test_every_family_is_rejected_by_some_mutant():
    """Every family but E3 (finite ratios beat the +inf / -inf ones whatever a kernel does with them: a path test only),
    E9c (hasCycle: the numpy restatement has none; the C oracles pin it) and every comparison site of the reference has a
    mutant of its own."""
    hit = {f for fams in TARGETS.values() for f in fams}
    assert set(E.FAMILIES) - hit == {"E3", "E9c"}, set(E.FAMILIES) - hit
    from tests import test_nonfinite_records as T  # (the mutants that only a NaN or an infinity shows have their targets there)
    assert set(TARGETS) | {"keep_col"} == set(NP.MUTANTS) - set(T.TARGETS)


def test_chvatal_family_stops_by_has_cycle():
    """E9c stops by hasCycle, not by the pivot budget: status "cycled" after 11 pivots, within every budget."""
    recs = [r for r in RECORDS if r["family"] == "E9c"]
    assert recs and all(r["status"] == "cycled" and r["n_pivots"] == 11 < G.options(r)["max_pivots"] for r in recs)


def test_column_col_in_the_non_zero_list_is_not_observable(oracle):
    """The one mutant no record can reject, and why: keeping column `col` in the non-zero list (src/simplex.ts:17-23)
    only changes what the loops write to column col before :25 and :36 overwrite it (1 / q in the pivot row, -coef / q in
    every updated row).  The records of E7, whose pivot elements lie inside the flush band, show it: the mutant agrees."""
    recs = [r for r in SMALL if r["family"] == "E7"]
    assert recs and not any(_disagrees(oracle, r, "keep_col") for r in recs)
    assert any(_disagrees(oracle, r, "patch_kept_only") for r in recs)

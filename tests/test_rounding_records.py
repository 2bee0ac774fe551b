"""The final rounding against the reference, word for word (tests/golden/simplex_rounding.json.gz and
simplex_rounding_edges.json.gz, inputs in tests/_rounding.py): roundToPrecision (src/util.ts:1-4) through every copy this
repository has, solution() (src/YALPS.ts:8-50) through both of its restatements, and simplex() on the family R, whose runs
end "optimal" with the result -0 or NaN.  The older golden files hold `result` as a JSON number and cannot show the sign of
a zero (tests/_golden.same_number); these hold 64-bit words in hex."""
import math

import numpy as np
import pytest

from tests import _edges as E
from tests import _golden as G
from tests import _np_dense as ND
from tests import _np_simplex as NP
from tests import _rounding as RD

RECORDS = G.records("rounding")
ROUND = [r for r in RECORDS if r["kind"] == "round"]
SOLUTION = [r for r in RECORDS if r["kind"] == "solution"]
R_RECORDS = G.records("rounding_edges")


def _pid(p):
    return "p=%r" % RD.unhex(p)


def test_records_are_the_table_and_the_states_of_the_generator():
    assert [(RD.hexd(p), [RD.hexd(x) for x in nums]) for p, nums in RD.table()] == [(r["precision"], r["nums"]) for r in ROUND]
    keys = ("label", "precision", "sign", "status", "result", "col0", "pos", "var")
    assert [RD.state_spec(s) for s in RD.states()] == [{k: r[k] for k in keys} for r in SOLUTION]
    assert len(ROUND) == len(RD.PRECISIONS) == 15 and len({r["precision"] for r in ROUND}) == 15
    words = sum(1 + 2 * len(r["nums"]) for r in ROUND) + sum(3 + len(r["col0"]) + len(r["out"]["variables"]) for r in SOLUTION)
    assert words < 10000, words  # (the file stays small)


def test_records_hold_the_rows_the_old_rounding_got_wrong():
    """The three rows of the issue, and a tie: the reference's answers, by word."""
    got = {(RD.unhex(r["precision"]), RD.unhex(n)): o for r in ROUND if r["precision"] != RD.hexd(math.nan)
           for n, o in zip(r["nums"], r["outs"]) if n != RD.hexd(math.nan)}
    neg0, pos0 = RD.hexd(-0.0), RD.hexd(0.0)
    assert got[(1e-8, math.nextafter(-RD.EPS, -1.0))] == neg0  # (just inside the window: num + 2^-52 < 0)
    assert got[(1e-8, -RD.EPS)] == pos0  # (num + 2^-52 is +0)
    assert got[(1e-8, -0.5 / 1e8 - RD.EPS)] == neg0  # (the far end)
    assert got[(0.25, -0.125 - RD.EPS)] == neg0  # (Math.round(-0.5) is -0)
    assert got[(-1e-8, 0.0)] == pos0 and got[(-1.0, 0.0)] == pos0  # (a negative rounding: Math.round(-2^-52 * 1e8) is -0, and -0 / -1e8 is +0)
    assert got[(3.0, 1.0)] == got[(2.5, 1.0)] == RD.hexd(math.nan)  # (the rounding is 0)
    assert got[(2.0, 1.0)] == RD.hexd(1.0)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_hip()
    return _native


def _wrong_rows(fn, rec):
    p = RD.unhex(rec["precision"])
    return [(n, o, RD.hexd(got)) for n, o, got in ((n, o, fn(RD.unhex(n), p)) for n, o in zip(rec["nums"], rec["outs"])) if RD.hexd(got) != o]


@pytest.mark.parametrize("rec", [pytest.param(r, id=_pid(r["precision"])) for r in ROUND])
def test_oracle_round_to_precision(oracle, rec):
    assert not _wrong_rows(oracle.round_to_precision, rec)


@pytest.mark.parametrize("rec", [pytest.param(r, id=_pid(r["precision"])) for r in ROUND])
def test_solve_round_to_precision(rec):
    from yalps_amd import solve
    assert not _wrong_rows(solve.round_to_precision, rec)


@pytest.mark.parametrize("rec", [pytest.param(r, id=_pid(r["precision"])) for r in ROUND])
def test_numpy_round_to_precision(rec):
    assert not _wrong_rows(NP.round_to_precision, rec)


@pytest.mark.parametrize("rec", [pytest.param(r, id=_pid(r["precision"])) for r in ROUND])
def test_native_round_to_precision(nat, rec):
    """yalps_round_to_precision: the host side of common.cuh's round_to_precision, the text every kernel compiles."""
    assert not _wrong_rows(nat.round_to_precision, rec)


@pytest.mark.parametrize("rec", [pytest.param(r, id=_pid(r["precision"])) for r in ROUND])
def test_restatement_of_this_module_matches(rec):
    assert not _wrong_rows(RD.round_to_precision, rec)


@pytest.mark.parametrize("mutant", sorted(RD.MUTANTS))
def test_records_reject_each_wrong_rounding(mutant):
    """Each of RD.MUTANTS gets a row wrong at the default precision, and at 0.25 (where the products are exact)."""
    for p in (1e-8, 0.25):
        rec = next(r for r in ROUND if r["precision"] == RD.hexd(p))
        assert _wrong_rows(lambda x, q: RD.round_to_precision(x, q, mutant), rec), (mutant, p)


def _expected_solution(rec):
    out = rec["out"]
    x = RD.dense_x(out["status"], [(j, RD.unhex(v)) for j, v in out["variables"]])
    return out["status"], G.canon(x).tobytes(), RD.unhex(out["result"])


def _state(rec):
    return (np.array([RD.unhex(x) for x in rec["col0"]]), np.array(rec["pos"], np.int32), np.array(rec["var"], np.int32),
            rec["status"], RD.unhex(rec["result"]), float(rec["sign"]), RD.unhex(rec["precision"]))


def _sid(r):
    return "%s-%s-sign%+d-result=%r" % (r["label"], _pid(r["precision"]), r["sign"], RD.unhex(r["result"]))


@pytest.mark.parametrize("rec", [pytest.param(r, id=_sid(r)) for r in SOLUTION])
def test_dense_solution_matches_the_reference(rec):
    """tests/_np_dense.dense_solution: what lp_dense_kernel's `after` is compared with."""
    col0, pos, var, status, result, sign, precision = _state(rec)
    est, ex, eres = _expected_solution(rec)
    x, objective = ND.dense_solution(col0, pos, var, status, result, sign, precision, RD.N)
    assert status == est and G.canon(x).tobytes() == ex, (x, np.frombuffer(ex))
    assert G.same_bits(objective, eres), (objective, eres)


@pytest.mark.parametrize("rec", [pytest.param(r, id=_sid(r)) for r in SOLUTION])
def test_solution_builder_matches_the_reference(rec):
    """yalps_amd.solve.solution with includeZeroVariables, as a dense x."""
    from yalps_amd.model import Tableau, TableauModel
    from yalps_amd.solve import solution
    col0, pos, var, status, result, sign, precision = _state(rec)
    est, ex, eres = _expected_solution(rec)
    tm = TableauModel(Tableau(None, RD.W, RD.H, pos, var, col0), sign, [(j, {}) for j in range(RD.N)], [])
    sol = solution(tm, status, result, {"precision": precision, "includeZeroVariables": True})
    assert sol["status"] == est
    assert G.canon(RD.dense_x(sol["status"], sol["variables"])).tobytes() == ex, sol
    assert [j for j, _ in sol["variables"]] == [j for j, _ in rec["out"]["variables"]]
    assert G.same_bits(sol["result"], eres), (sol["result"], eres)


def test_solution_states_cover_what_they_are_there_for():
    labels = {r["label"] for r in SOLUTION}
    assert labels == {"optimal-A", "optimal-B", "optimal-C", "unbounded-structural", "unbounded-slack", "unbounded-position0",
                      "infeasible", "cycled"}
    assert {r["precision"] for r in SOLUTION} == {RD.hexd(p) for p in RD.PRECISIONS} and {r["sign"] for r in SOLUTION} == {1, -1}
    inf = RD.hexd(math.inf)
    for r in SOLUTION:
        values = [v for _, v in r["out"]["variables"]]
        if r["label"] == "unbounded-structural":
            assert r["out"]["variables"] == [[5, inf]]
        elif r["label"].startswith("unbounded"):
            assert values == []  # (no +inf anywhere)
    # a negative precision lets zeros through to the rounding, and the reference rounds +0 and -0 to +0 there
    neg = [r for r in SOLUTION if r["label"] == "optimal-C" and r["precision"] == RD.hexd(-1e-8)]
    assert neg and all(r["out"]["variables"][0][1] == RD.hexd(0.0) and r["out"]["variables"][1][1] == RD.hexd(0.0) for r in neg)
    # both zeros come back as results
    assert {r["out"]["result"] for r in SOLUTION if r["label"] == "optimal-A"} == {RD.hexd(0.0), RD.hexd(-0.0)}


# ---- the family R -----------------------------------------------------------------------------------------------------------

R_ALL = [pytest.param(r, id=E.label(r)) for r in R_RECORDS]
WINDOW = (-0.5 / 1e8 - RD.EPS, -RD.EPS)


def test_r_records_end_optimal_at_minus_zero_or_nan():
    assert sorted((r["family"], r["M"], r["N"], r["seed"]) for r in R_RECORDS) == sorted(RD.r_specs())
    assert {(r["M"], r["N"]) for r in R_RECORDS} == set(E.SHAPES)
    for r in R_RECORDS:
        assert r["status"] == "optimal" and r["n_pivots"] >= RD.R_MIN_PIVOTS[r["family"]], E.label(r)
        assert r["result_hex"] == (RD.hexd(math.nan) if r["family"] == "R1n" else RD.hexd(-0.0)), E.label(r)
        assert r["n_pivots"] == {"R0": 0, "Rn": r["n_pivots"]}.get(r["family"], 1)


@pytest.mark.parametrize("omp", [False, True], ids=["oracle", "oracle-omp"])
@pytest.mark.parametrize("rec", R_ALL)
def test_c_oracles_reproduce_the_r_records(oracle, rec, omp):
    from tests import _oracle
    orc = _oracle.load(omp=True) if omp else oracle
    if omp:
        assert orc.set_threads(4) == 4
    m = RD.r_initial(rec, oracle.dense_lp)
    assert RD.r_options(rec["family"], rec["M"], rec["N"], rec["seed"]) == G.options(rec)
    pos, var = G.identity_perms(rec)
    exp = G.expected(rec)
    status, result, npiv, trace = orc.simplex(m, rec["width"], rec["height"], pos, var, trace_cap=exp["n_pivots"] + 8, **G.options(rec))
    assert (status, npiv) == (exp["status"], exp["n_pivots"]) and np.array_equal(trace, exp["pivots"])
    assert RD.hexd(result) == rec["result_hex"], (result, rec["result_hex"])
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
    assert E.col0_matches(m, rec, exp) and G.sha256(m) == exp["final_sha256"]
    if rec["family"] in ("R0", "R1"):
        assert m[0] == -2.0 ** -40
    elif rec["family"] == "R1q":
        assert m[0] == -0.125
    elif rec["family"] == "Rn":
        assert WINDOW[0] <= m[0] < WINDOW[1], m[0]


@pytest.mark.parametrize("rec", [p for p in R_ALL if p.values[0]["width"] * p.values[0]["height"] <= 2_000_000])
def test_numpy_restatement_reproduces_the_r_records(oracle, rec):
    """Records of up to 2M entries (the C oracles run them all): the restatement's rounding is a copy of its own."""
    m = RD.r_initial(rec, oracle.dense_lp)
    pos, var = G.identity_perms(rec)
    o = G.options(rec)
    exp = G.expected(rec)
    status, result, npiv = NP.simplex(m, rec["width"], rec["height"], pos, var, o["precision"], o["max_pivots"])
    assert (status, npiv) == (exp["status"], exp["n_pivots"]) and RD.hexd(result) == rec["result_hex"]
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"]) and G.sha256(m) == exp["final_sha256"]

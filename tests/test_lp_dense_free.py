"""yalps_lpdense_solve_free, linprog_batch(free=) and linprog_objective_bounds(free=) on the GPU.  The work runs in three child
processes that import torch first (tests/_lp_dense.py says why); every test compares what a child wrote with the C oracle on the
numpy restatement of the split tableau and of its read-out (tests/_np_dense_free.py), bit for bit, all NaNs counted as one value:
status, pivots, the final matrix, both permutations, column 0, x, the objective and the four marginals."""
import math

import numpy as np
import pytest

from tests import _golden as G
from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _lp_dense_bounds as LBD
from tests import _lp_dense_free as LF
from tests import _np_dense_free as FD
from tests.test_lp_dense import check_answers, of, same
from tests.test_lp_dense_bounds import check_marginals
from tests.test_lp_dense_bounds_model import OBJECTIVE_RESIDUAL, REDUCED_RESIDUAL

pytestmark = pytest.mark.gpu


def run_child(tmp_path_factory, which, env=None):
    import os
    import subprocess
    import sys
    from yalps_amd import build
    build.build_lpdense()
    build.build_hip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("lp_dense_free") / (which + ".npz"))
    child = subprocess.run([sys.executable, "-m", "tests._lp_dense_free", which, path], cwd=root, capture_output=True, text=True, timeout=600,
                           env=dict({k: v for k, v in os.environ.items() if k not in LD.GRID_HOOKS}, **(env or {})))
    assert child.returncode == 0, child.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def ran(tmp_path_factory):
    return run_child(tmp_path_factory, "table")


@pytest.fixture(scope="module")
def hist(tmp_path_factory):
    return run_child(tmp_path_factory, "hist", {"YALPS_LPDENSE_HIST": str(LD.HIST)})


@pytest.fixture(scope="module")
def hard_ran(tmp_path_factory):
    return run_child(tmp_path_factory, "hard")


@pytest.fixture(scope="module")
def calls(oracle):
    return {c.name: c for c in LF.table(oracle)}


@pytest.fixture(scope="module")
def hard_calls():
    return {c.name: c for c in LF.hard_table()}


def check_identities(got, call, tag):
    """On every optimal row of a call of small integers, within the tolerances of the bounds model test (the same generator)."""
    rows = 0
    for i in np.flatnonzero(got["status"] == 0):
        r_obj, r_red = FD.identity_residuals(call.lps[i], call.lbs[i], call.ubs[i], call.idx, call.fidx, float(got["objective"][i]),
                                             *(got[k][i] for k in LF.OUTPUTS))
        assert r_obj <= OBJECTIVE_RESIDUAL and r_red <= REDUCED_RESIDUAL, (tag, int(i), r_obj, r_red)
        rows += 1
    return rows


@pytest.mark.parametrize("name", LF.names())
def test_call_against_the_oracle(ran, calls, oracle, name):
    call, got = calls[name], of(ran, name)
    refs = check_answers(got, call, oracle, name)
    check_marginals(got, call, refs, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    cls, kernel = LF.kernel_of(call)
    assert str(got["kernels"]) == kernel and int(got["launches"]) == 1 and int(got["reruns"]) == 0, (name, got["kernels"])
    assert got["classes"].tolist() == [cls] and got["aux"].tolist() == [1 if name == "aux" else 0]
    assert got["tableau"].shape[1] == (1 + call.n + call.f) * call.h and got["pos"].shape[1] == 1 + call.n + call.f + call.h
    if "bound" in name or name in ("HBM 301x280", "aux"):
        ref = refs[0]
        assert ref["status"] == "optimal" and (ref["x"][list(call.fidx)] < 0).any() and call.fidx[-1] == call.n - 1
        if name.startswith("class"):
            assert LB.size_class(call.w, call.h) == int(name.split()[1]) + (name.split()[3] == "over")
    if name == "statuses":  # all four endings in a call of more LPs than workgroups, the -inf of an unbounded twin, NaN rows
        assert len(call.lps) > int(got["grids"][0]) >= 2048
        assert {r["status"] for r in refs} == set(LD.STATUS)
        bad = np.array([r["status"] != "optimal" for r in refs])
        assert np.array_equal(np.isnan(got["upper"]).all(axis=1), bad) and np.array_equal(np.isnan(got["reduced"]).any(axis=1), bad)
        assert (got["x"] == -math.inf).any() and (got["x"] == math.inf).any()
        twins = [i for i, r in enumerate(refs) if r["status"] == "unbounded" and call.n < int(r["var"][int(r["result"])]) < call.w]
        assert twins and all((got["x"][i] == -math.inf).sum() == 1 for i in twins)
        assert check_identities(got, call, name) >= 20
    if name == "nan lb at free":  # lb is not read there: no NaN reaches the answer, and the bits are those of 0.0 in its place
        zero = of(ran, "zero lb at free")
        assert all(np.isnan(lb[list(call.fidx)]).all() for lb in call.lbs)
        for key in ("x", "objective", "status", "pivots", "tableau", "col0", "pos", "var") + LF.OUTPUTS:
            assert np.array_equal(got[key].view(np.uint8), zero[key].view(np.uint8)), key
        assert not np.isnan(got["tableau"]).any() and not np.isnan(got["x"][got["status"] == 0]).any()
        assert check_identities(zero, calls["zero lb at free"], name) >= 3
    if name == "nonfinite":
        assert np.isnan(refs[0]["start"].reshape(call.h, call.w)[1, 0]) and np.isinf(refs[2]["start"]).any()


@pytest.mark.parametrize("want", LF.PARTIAL, ids=lambda w: "+".join(w) or "none")
def test_only_the_requested_outputs_are_written(ran, oracle, want):
    call = LF.partial_call()
    tag = "partial %s" % ("+".join(want) or "none")
    got = of(ran, tag)
    refs = check_answers(got, call, oracle, tag)
    check_marginals(got, call, refs, tag, want)
    assert str(got["kernels"]) == LF.kernel_of(call)[1]


def test_history_rerun_writes_the_row(hist, oracle):
    call = LF.hist_call(oracle)
    refs = [call.oracle_answer(oracle, i) for i in range(len(call.lps))]
    assert all(r["n_pivots"] > LD.HIST for r in refs)
    assert int(hist["reruns"]) == len(call.lps) and int(hist["passes"]) >= 2
    assert set(str(hist["kernels"]).split()) == {LF.kernel_of(call)[1]} == {"lp_dense_free_kernel<256,check,lds>"}
    for i, ref in enumerate(refs):
        assert LD.STATUS[int(hist["status"][i])] == ref["status"] == "optimal" and int(hist["pivots"][i]) == ref["n_pivots"]
        assert (ref["x"][list(call.fidx)] != 0).any()
        for key in ("x", "objective", "ineqlin", "reduced", "upper"):
            assert same(np.atleast_1d(hist[key][i]), np.atleast_1d(ref[key])), (i, key)


def test_a_call_without_free_variables_is_the_call_it_was(ran):
    """free=(), False and None, with and without bounds: the kernels, by name, and the bits of the call without the argument."""
    call = LBD.partial_call()
    cls = LB.size_class(call.w, call.h - call.k)
    form = "<%d%s>" % (1024 if cls >= 3 else 256, ",lds" if cls < 4 else "")
    for tag, kernel in (("today plain", "lp_dense_kernel"), ("today bounds", "lp_dense_bounds_kernel")):
        a = of(ran, tag)
        assert str(a["kernels"]) == kernel + form
        for name in ("()", "False", "None"):
            b = of(ran, "%s free=%s" % (tag, name))
            assert str(b["kernels"]) == kernel + form and set(a) == set(b)
            for key in a:
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (tag, name, key)


def test_free_alone_runs_the_free_kernel(hard_ran, hard_calls):
    for d in ("min", "max"):
        call = hard_calls["start n=3 f=1 none %s" % d]
        assert not call.has_lb and not call.has_ub and call.f == 1
        for tag in (call.name, call.name + " @0", call.name + " public"):
            assert str(hard_ran[tag + "/kernels"]) == "lp_dense_free_kernel<256,lds>", tag


def test_host_pointers_are_refused_by_name(ran, oracle):
    messages = [str(m) for m in ran["refusal/messages"]]
    for name, m in zip(("lb", "ub", "upper_out"), messages):
        assert ("yalps_lpdense_solve_free: %s is" % name) in m and m.endswith("launches=0"), m
    assert bool(ran["refusal/untouched"])
    call = LF.random_call("refusal", 3, 2, 2, 1, free=(1,))
    got = of(ran, "refusal/after")
    check_marginals(got, call, check_answers(got, call, oracle, "refusal/after"), "refusal/after")


def check_public(got, call, oracle, tag):
    if not call.has_ub:  # (LinprogDuals: the result has no `upper` field)
        assert "upper" not in got and call.k == 0, tag
        got = dict(got, upper=np.empty((len(call.lps), 0)))
    refs = check_answers(got, call, oracle, tag, kept=False)
    check_marginals(got, call, refs, tag)
    return refs


def test_shared_operands_and_views(ran, oracle):
    call, shared = LF.views_inputs()
    names = str(ran["shared/names"]).split()
    refs = check_public({k: v for k, v in of(ran, "shared").items() if k != "names"}, shared, oracle, "shared")
    assert names == [r["status"] for r in refs] and "optimal" in names
    check_public(of(ran, "views"), call, oracle, "views")
    for a, b in (("shared", "shared copies"), ("views", "views copies")):
        x, y = of(ran, a), of(ran, b)
        assert all(same(x[k], y[k]) if x[k].dtype == np.float64 else np.array_equal(x[k], y[k]) for k in y), a
    assert bool(ran["views/unchanged"])
    assert check_identities(of(ran, "views"), call, "views") + check_identities(of(ran, "shared copies"), shared, "shared") >= 3


def test_producer_on_a_side_stream(ran, oracle):
    call, _ = LF.views_inputs()
    assert np.array_equal(ran["stream/c"], call.stacked()[0])
    check_public({k: v for k, v in of(ran, "stream").items() if k != "c"}, call, oracle, "stream")


def test_empty_batch(ran):
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0, 0, 2, 0, 0, 0, 3, 0, 2] and str(ran["empty/type"]) == "LinprogBoundDuals"
    assert int(ran["empty/launches"]) == 0


def test_objective_gradients_with_a_free_variable(ran, oracle):
    """dc = g x with a negative x, dlb exactly zero at the free index, exact zeros from the infeasible row, the batch sum for a
    shared c and a shared lb."""
    call = LF.gradient_call()
    got = of(ran, "gradient rows")
    refs = check_public({k: v for k, v in got.items() if not k.startswith("grad_")}, call, oracle, "gradient rows")
    assert [r["status"] for r in refs] == ["optimal", "optimal", "infeasible"] and got["x"][0, 1] < 0
    g = np.array(LF.GRADIENT_WEIGHTS)[:, None]
    ok = np.array([True, True, False])[:, None]
    z = lambda a: np.where(ok, a, 0.0)
    want_lb = g * z(got["reduced"])
    want_lb[:, list(call.fidx)] = 0.0
    assert np.array_equal(got["grad_lb"], want_lb) and not got["grad_lb"][:, 1].any() and np.count_nonzero(got["grad_lb"][:2])
    assert (got["grad_lb"][:, 1].view(np.int64) == 0).all()  # +0.0, exactly
    assert np.array_equal(got["grad_c"], g * z(got["x"])) and got["grad_c"][0, 1] == g[0, 0] * got["x"][0, 1] < 0
    assert np.array_equal(got["grad_ub"], g * z(got["upper"])) and np.array_equal(got["grad_b_ub"], g * z(got["ineqlin"]))
    assert np.array_equal(got["grad_A_ub"], -(g * z(got["ineqlin"]))[:, :, None] * z(got["x"])[:, None, :])
    assert not got["grad_lb"][2].any() and not got["grad_ub"][2].any() and not got["grad_A_ub"][2].any() and not got["grad_c"][2].any()
    sh = of(ran, "gradient shared")
    assert sh["status"].tolist() == [0, 0, 1]
    shok = (sh["status"] == 0)[:, None]
    assert sh["grad_c"].shape == (3,) and np.array_equal(sh["grad_c"], (g * np.where(shok, sh["x"], 0.0)).sum(axis=0))
    want = (g * np.where(shok, sh["reduced"], 0.0)).sum(axis=0)
    want[list(call.fidx)] = 0.0
    assert sh["grad_lb"].shape == (3,) and np.array_equal(sh["grad_lb"], want) and np.count_nonzero(want)


# ------------------------------------------------------------------------------------------------------- the hard calls

@pytest.mark.parametrize("name", LF.hard_names())
def test_hard_start_tableau(hard_ran, hard_calls, oracle, name):
    """max_pivots = 0: simplex stops in front of the first pivot, and the kept tableau is what fill wrote, every word of it."""
    call = LF.at_budget_0(hard_calls[name])
    got = of(hard_ran, call.name)
    assert (got["status"] == LD.STATUS.index("cycled")).all() and (got["pivots"] == 0).all(), (name, got["status"], got["pivots"])
    for i, (lp, lb, ub) in enumerate(zip(call.lps, call.lbs, call.ubs)):
        want = FD.free_tableau(*lp, lb=lb, ub=ub, upper=call.idx, free=call.fidx, maximize=call.maximize)
        bad = np.flatnonzero(G.canon(got["tableau"][i]).view(np.int64) != G.canon(want).view(np.int64))
        assert not bad.size, ("%s LP %d" % (name, i), "(row, column) of the first words that differ", [divmod(int(p), call.w) for p in bad[:8]],
                              got["tableau"][i][bad[:8]], want[bad[:8]])
        assert same(got["col0"][i], want.reshape(call.h, call.w)[:, 0])
        assert np.array_equal(got["pos"][i], np.arange(call.w + call.h)) and np.array_equal(got["var"][i], np.arange(call.w + call.h))
    assert all(np.isnan(got[key]).all() for key in ("x", "objective") + LF.OUTPUTS), name
    refs = check_answers(got, call, oracle, call.name)
    check_marginals(got, call, refs, call.name)
    assert str(got["kernels"]) == LF.kernel_of(call)[1] and int(got["launches"]) == 1 and int(got["reruns"]) == 0 and bool(got["unchanged"])


@pytest.mark.parametrize("name", LF.hard_names())
def test_hard_call_against_the_oracle(hard_ran, hard_calls, oracle, name):
    call, got = hard_calls[name], of(hard_ran, name)
    refs = check_answers(got, call, oracle, name)
    check_marginals(got, call, refs, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    assert str(got["kernels"]) == LF.kernel_of(call)[1] == "lp_dense_free_kernel<256,lds>" and int(got["launches"]) == 1
    public = of(hard_ran, name + " public")
    assert str(public.pop("kernels")) == LF.kernel_of(call)[1]
    check_public(public, call, oracle, name + " public")
    if name != "rounding":  # (under a precision of 0.25 "optimal" is declared with reduced costs of up to a quarter still open)
        check_identities(got, call, name)
    if name == "rounding":
        assert got["x"][0].tolist() == [-0.75, 0.0]
    if name == "free=True n=5":
        assert call.f == call.n == 5 and call.w == 11


def device_words(got, at0, call):
    return np.concatenate([np.concatenate([at0["tableau"][i], got["x"][i], got["objective"][i:i + 1], got["reduced"][i]]) for i in range(len(call.lps))])


def test_the_device_has_none_of_the_flaws(hard_ran, hard_calls, oracle):
    """For every mutant that any input can tell from the canonical statement, at least one hard call's device words -- the start
    tableau, x, the objective, the reduced costs -- differ from the mutant's and equal the canonical ones.  The two runs of a call
    are compared with the two oracle runs they belong to: the start tableau at max_pivots = 0, the answer with its own options."""
    told = set()
    for name, call in hard_calls.items():
        got, at0 = of(hard_ran, name), of(hard_ran, LF.at_budget_0(call).name)
        device = device_words(got, at0, call)
        full, start = LF.answers(oracle, call), LF.answers(oracle, LF.at_budget_0(call))
        words = lambda a, b: np.concatenate([np.concatenate([s["start"], r["x"], [r["objective"]], r["reduced"]]) for r, s in zip(a, b)])
        canonical = words(full, start)
        assert not LF.differing(device, canonical), name
        for flaw in FD.FLAWS:
            wrong = words(LF.answers(oracle, call, flaw), LF.answers(oracle, LF.at_budget_0(call), flaw))
            if LF.differing(wrong, canonical):
                assert LF.differing(device, wrong), "%s: the device computes what the flaw %r computes" % (name, flaw)
                told.add(flaw)
    assert told == set(FD.FLAWS) - set(FD.UNTELLABLE), sorted(told)

"""yalps_lpdense_solve_bounds, linprog_batch(lb=, ub=, upper=) and linprog_objective_bounds on the GPU.  The work runs in three child
processes that import torch first (tests/_lp_dense.py says why); every test compares what a child wrote with the C oracle on the
numpy restatement of the bounded tableau and of its read-out (tests/_np_dense_bounds.py), bit for bit, all NaNs counted as one
value.

The upper-bound marginals cannot go round the 1024 lanes of the HBM form: k <= n, and a full box on n variables is a tableau of
(n + 1) x (1 + n) doubles, which the 4 MiB limit stops at n = 723 (k = n = 1025 would be 8.4 MB).  "box n=k=723" is the largest
there is: the marginal rows reach lane 722 of 1024."""
import numpy as np
import pytest

from tests import _golden as G
from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _lp_dense_bounds as LBD
from tests import _np_dense_bounds as BD
from tests.test_lp_dense import check_answers, of, same

pytestmark = pytest.mark.gpu


def run_child(tmp_path_factory, which, env=None):
    import os
    import subprocess
    import sys
    from yalps_amd import build
    build.build_lpdense()
    build.build_hip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("lp_dense_bounds") / (which + ".npz"))
    child = subprocess.run([sys.executable, "-m", "tests._lp_dense_bounds", which, path], cwd=root, capture_output=True, text=True, timeout=600,
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
def calls(oracle):
    return {c.name: c for c in LBD.table(oracle)}


def kernel_of(call):
    cls = LB.size_class(call.w, call.h)
    return cls, "lp_dense_bounds_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")


def check_marginals(got, call, refs, tag, want=LBD.OUTPUTS):
    B = len(call.lps)
    for key, width in zip(LBD.OUTPUTS, (call.m_ub, call.m_eq, call.n, call.k)):
        assert got[key].shape == (B, width) and got[key].dtype == np.float64, (tag, key, got[key].shape)
        if key not in want:
            assert (got[key] == LBD.SENTINEL).all(), (tag, key, "written without being asked for")
            continue
        for i, ref in enumerate(refs):
            assert same(got[key][i], ref[key]), ("%s LP %d" % (tag, i), key, ref["status"], got[key][i], ref[key])


@pytest.mark.parametrize("name", LBD.names())
def test_call_against_the_oracle(ran, calls, oracle, name):
    call, got = calls[name], of(ran, name)
    refs = check_answers(got, call, oracle, name)
    check_marginals(got, call, refs, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    cls, kernel = kernel_of(call)
    assert str(got["kernels"]) == kernel and int(got["launches"]) == 1 and int(got["reruns"]) == 0, (name, got["kernels"])
    assert got["classes"].tolist() == [cls] and got["aux"].tolist() == [1 if name.startswith("aux") else 0]
    statuses = {r["status"] for r in refs}
    if name not in ("statuses",):
        assert "optimal" in statuses, (name, statuses)
    if name.startswith("class"):  # the bound rows decide the class: without them both shapes are under the bound
        assert LB.size_class(call.w, call.h - call.k) == int(name.split()[1])
    if name.startswith("box"):
        ref = refs[0]
        c, lb, ub = call.lps[0][0], call.lbs[0], call.ubs[0]
        assert ref["status"] == "optimal" and np.array_equal(ref["x"], np.where(c > 0, ub, lb))
        assert np.array_equal(ref["upper"], np.maximum(c, 0.0)) and ref["upper"][-1] == 3.0 and call.k == LBD.BOX_N > 512
        assert np.array_equal(ref["reduced"], np.minimum(c, 0.0) + 0.0)
    if name == "statuses":  # NaN rows exactly at the LPs that did not end optimal, in a call of more LPs than workgroups
        assert len(call.lps) > int(got["grids"][0]) >= 2048
        assert statuses == set(LD.STATUS)
        bad = np.array([r["status"] != "optimal" for r in refs])
        assert np.array_equal(np.isnan(got["upper"]).all(axis=1), bad) and np.array_equal(np.isnan(got["reduced"]).any(axis=1), bad)
        crossed = [i for i in range(len(refs)) if any(call.ubs[i][j] < call.lbs[i][j] for j in call.idx)]
        assert crossed and all(refs[i]["status"] in ("infeasible", "cycled") for i in crossed)
        unbounded = [r for r in refs if r["status"] == "unbounded"]
        assert any(np.isinf(r["x"]).any() for r in unbounded)
    if name == "nonfinite bounds":
        assert any(not np.isfinite(r["start"]).all() for r in refs)
    if name in ("lb only", "both, check", "n=65"):  # negative lower bounds, and optima at negative x
        assert any(r["status"] == "optimal" and (r["x"] < 0).any() for r in refs)


@pytest.mark.parametrize("want", LBD.PARTIAL, ids=lambda w: "+".join(w) or "none")
def test_only_the_requested_outputs_are_written(ran, oracle, want):
    call = LBD.partial_call()
    tag = "partial %s" % ("+".join(want) or "none")
    got = of(ran, tag)
    refs = check_answers(got, call, oracle, tag)
    check_marginals(got, call, refs, tag, want)
    assert str(got["kernels"]) == kernel_of(call)[1]


def test_history_rerun_writes_the_row(hist, oracle):
    call = LBD.hist_call(oracle)
    refs = [call.oracle_answer(oracle, i) for i in range(len(call.lps))]
    assert all(r["n_pivots"] > LD.HIST for r in refs)
    assert int(hist["reruns"]) == len(call.lps) and int(hist["passes"]) >= 2
    assert set(str(hist["kernels"]).split()) == {kernel_of(call)[1]}
    for i, ref in enumerate(refs):
        assert LD.STATUS[int(hist["status"][i])] == ref["status"] == "optimal" and int(hist["pivots"][i]) == ref["n_pivots"]
        for key in ("x", "objective", "ineqlin", "reduced", "upper"):
            assert same(np.atleast_1d(hist[key][i]), np.atleast_1d(ref[key])), (i, key)


def test_a_call_without_bounds_is_the_call_it_was(ran):
    """linprog_batch(duals=True) without lb / ub: LinprogDuals, the bits of yalps_lpdense_solve_duals, the boundless kernels."""
    a, b = of(ran, "plain"), of(ran, "plain abi")
    assert str(a["type"]) == "LinprogDuals"
    for key in ("x", "objective", "status", "pivots", "ineqlin", "eqlin", "reduced"):
        assert np.array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8)), key
    call = LBD.partial_call()
    cls = LB.size_class(call.w, call.h - call.k)
    assert str(a["kernels"]) == str(b["kernels"]) == "lp_dense_kernel<%d%s>" % (1024 if cls >= 3 else 256, ",lds" if cls < 4 else "")


def test_host_pointers_are_refused_by_name(ran, oracle):
    messages = [str(m) for m in ran["refusal/messages"]]
    for name, m in zip(("lb", "ub", "upper_out"), messages):
        assert ("yalps_lpdense_solve_bounds: %s is" % name) in m and m.endswith("launches=0"), m
    assert bool(ran["refusal/untouched"])
    call = LBD.random_call("refusal", 3, 2, 2, 1)
    got = of(ran, "refusal/after")
    check_marginals(got, call, check_answers(got, call, oracle, "refusal/after"), "refusal/after")


def check_public(got, call, oracle, tag):
    refs = check_answers(got, call, oracle, tag, kept=False)
    check_marginals(got, call, refs, tag)
    return refs


def test_shared_bounds_and_views(ran, oracle):
    call, shared = LBD.views_inputs()
    check_public(of(ran, "shared"), shared, oracle, "shared")
    check_public(of(ran, "views"), call, oracle, "views")
    for a, b in (("shared", "shared copies"), ("views", "views copies")):
        x, y = of(ran, a), of(ran, b)
        assert all(same(x[k], y[k]) if x[k].dtype == np.float64 else np.array_equal(x[k], y[k]) for k in x if k != "unchanged"), a
    assert bool(ran["views/unchanged"])


def test_producer_on_a_side_stream(ran, oracle):
    call, _ = LBD.views_inputs()
    assert np.array_equal(ran["stream/lb"], call.bounds_stacked()[0])
    check_public({k: v for k, v in of(ran, "stream").items() if k != "lb"}, call, oracle, "stream")


def test_empty_batch(ran):
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0, 0, 2, 0, 0, 0, 3, 0, 2] and str(ran["empty/type"]) == "LinprogBoundDuals"
    assert int(ran["empty/launches"]) == 0


def test_objective_gradients_for_the_bounds(ran, oracle):
    """d lb = g reduced_costs, d ub = g upper scattered, from the returned tensors; the batch sum for a shared ub; exact zeros from
    the infeasible row; and the formulas against central differences of the GPU's own objectives."""
    call = LBD.gradient_call()
    got = of(ran, "gradient rows")
    refs = check_public({k: v for k, v in got.items() if not k.startswith("grad_")}, call, oracle, "gradient rows")
    assert [r["status"] for r in refs] == ["optimal", "optimal", "infeasible"]
    g = np.array(LBD.GRADIENT_WEIGHTS)[:, None]
    ok = np.array([True, True, False])[:, None]
    z = lambda a: np.where(ok, a, 0.0)
    assert np.array_equal(got["grad_lb"], g * z(got["reduced"]) * ok) and np.array_equal(got["grad_ub"], g * z(got["upper"]) * ok)
    assert np.array_equal(got["grad_c"], g * z(got["x"]) * ok) and np.array_equal(got["grad_b_ub"], g * z(got["ineqlin"]) * ok)
    assert not got["grad_lb"][2].any() and not got["grad_ub"][2].any() and not got["grad_A_ub"][2].any()
    assert np.count_nonzero(got["grad_lb"][:2]) and np.count_nonzero(got["grad_ub"][:2])
    sh = of(ran, "gradient shared")
    assert sh["status"].tolist() == [0, 0, 0]  # (the shared ub is the first LP's: the third row's box is whole again)
    want = np.zeros(3)
    want[[0, 2]] = (g * sh["upper"]).sum(axis=0)
    assert sh["grad_ub"].shape == (3,) and np.array_equal(sh["grad_ub"], want) and sh["upper"].shape == (3, 2)
    assert np.array_equal(sh["grad_lb"], g * sh["reduced"]) and np.count_nonzero(want)
    diff = LBD.difference_call()
    d = of(ran, "differences")
    check_answers(d, diff, oracle, "differences", kept=False)
    numeric = np.array([(d["objective"][1 + 2 * e] - d["objective"][2 + 2 * e]) / (2.0 * LBD.GRAD_H) for e in range(6)])
    formulas = np.concatenate([got["reduced"][0], got["upper"][0]])
    assert (np.abs(numeric - formulas) <= LBD.GRAD_PRECISION / LBD.GRAD_H).all(), (numeric, formulas)


# ------------------------------------------------------------------------------------------------------- the hard calls
# Data whose rounding shows (tests/_lp_dense_bounds.py, HARD and the pins): the order of shift_sum is in the bits of the start
# tableau's column 0 and of the objective, the read-out in the bits of x and of the objective, and nowhere else.

@pytest.fixture(scope="module")
def hard_ran(tmp_path_factory):
    return run_child(tmp_path_factory, "hard")


@pytest.fixture(scope="module")
def hard_calls(oracle):
    return {c.name: c for c in LBD.hard_table(oracle)}


@pytest.mark.parametrize("name", LBD.hard_names())
def test_hard_start_tableau(hard_ran, hard_calls, oracle, name):
    """max_pivots = 0: simplex stops in front of the first pivot, and the kept tableau is what fill wrote, every word of it."""
    call = LBD.at_budget_0(hard_calls[name])
    got = of(hard_ran, call.name)
    assert (got["status"] == LD.STATUS.index("cycled")).all() and (got["pivots"] == 0).all(), (name, got["status"], got["pivots"])
    for i, (lp, lb, ub) in enumerate(zip(call.lps, call.lbs, call.ubs)):
        want = BD.bounded_tableau(*lp, lb=lb, ub=ub, upper=call.idx, maximize=call.maximize)
        bad = np.flatnonzero(G.canon(got["tableau"][i]).view(np.int64) != G.canon(want).view(np.int64))
        assert not bad.size, ("%s LP %d" % (name, i), "(row, column) of the first words that differ", [divmod(int(p), call.w) for p in bad[:8]],
                              got["tableau"][i][bad[:8]], want[bad[:8]])
        assert same(got["col0"][i], want.reshape(call.h, call.w)[:, 0])
    assert all(np.isnan(got[key]).all() for key in ("x", "objective") + LBD.OUTPUTS), name
    refs = check_answers(got, call, oracle, call.name)
    check_marginals(got, call, refs, call.name)
    assert str(got["kernels"]) == kernel_of(call)[1] and int(got["launches"]) == 1 and int(got["reruns"]) == 0 and bool(got["unchanged"])


@pytest.mark.parametrize("name", LBD.hard_names())
def test_hard_call_against_the_oracle(hard_ran, hard_calls, oracle, name):
    call, got = hard_calls[name], of(hard_ran, name)
    refs = check_answers(got, call, oracle, name)
    check_marginals(got, call, refs, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    cls, kernel = kernel_of(call)
    assert str(got["kernels"]) == kernel and int(got["launches"]) == 1 and int(got["reruns"]) == 0, (name, got["kernels"])
    if name in LBD.HARD:
        assert (cls, int(got["aux"][0])) == LBD.HARD_FORMS[name] and got["classes"].tolist() == [cls]
        form = name[5:name.index(">") + 1] if "<" in name else "<1024>" if LBD.HARD_FORMS[name][1] else "<256,lds>"
        assert kernel == "lp_dense_bounds_kernel" + form, (name, kernel)
        assert 2 * [r["status"] for r in refs].count("optimal") >= len(refs) and max(r["n_pivots"] for r in refs) >= 8
    if name == LBD.PIN_NAMES[2]:
        assert got["objective"].view(np.int64).tolist() == [0]  # +0.0: -0.0 + shift_sum(c, 0)
    if name == LBD.PIN_NAMES[3]:
        assert got["objective"].view(np.int64).tolist() == [-2 ** 63]  # -0.0: nothing is added without lb


def flawed_words(oracle, call, flaw):
    """(start column 0, x, objective) of every LP as one array, under a flaw (None: the canonical ones)."""
    full, at0 = LBD.hard_answers(oracle, call, flaw), LBD.hard_answers(oracle, LBD.at_budget_0(call), flaw)
    return np.concatenate([np.concatenate([a["start"].reshape(call.h, call.w)[:, 0], r["x"], [r["objective"]]]) for r, a in zip(full, at0)])


# the flaws a pins call is made for (the last pin has no lb: nothing is summed, nothing added)
PIN_TELLS = {LBD.PIN_NAMES[0]: {"left to right", "fused", "lanes of 32"}, LBD.PIN_NAMES[1]: {"fold upward"}, LBD.PIN_NAMES[2]: set()}


@pytest.mark.parametrize("name", list(LBD.HARD) + list(PIN_TELLS))
def test_the_device_has_none_of_the_flaws(hard_ran, hard_calls, oracle, name):
    """The words that carry the order and the read-out -- column 0 of the start tableau, x, the objective -- are the canonical
    ones and differ from those of every flawed restatement (tests/test_lp_dense_bounds_model.py: which flaws a call can tell)."""
    call = hard_calls[name]
    got, at0 = of(hard_ran, name), of(hard_ran, LBD.at_budget_0(call).name)
    device = np.concatenate([np.concatenate([at0["tableau"][i].reshape(call.h, call.w)[:, 0], got["x"][i], got["objective"][i:i + 1]])
                             for i in range(len(call.lps))])
    told = []
    for flaw in BD.FLAWS:
        wrong = flawed_words(oracle, call, flaw)
        if LBD.differing(wrong, flawed_words(oracle, call, None)):
            told.append(flaw)
            assert LBD.differing(device, wrong), "%s: the device computes what the flaw %r computes" % (name, flaw)
    assert not LBD.differing(device, flawed_words(oracle, call, None)), (name, "the device differs from the canonical words; it equals",
                                                                           [f for f in BD.FLAWS if not LBD.differing(device, flawed_words(oracle, call, f))])
    must = PIN_TELLS[name] if name in PIN_TELLS else set(BD.FLAWS) - ({"fused", "lanes of 32"} if call.n <= 64 else set())
    assert set(told) >= must, (name, told)


@pytest.mark.parametrize("name", LBD.PUBLIC_HARD)
def test_hard_calls_through_linprog_batch(hard_ran, hard_calls, oracle, name):
    """The public route keeps no tableau: the objective alone carries shift_sum(c, lb).  Its words, and the flaws it tells."""
    call, got = hard_calls[name], of(hard_ran, name + " public")
    kernels = str(got.pop("kernels"))
    refs = check_public(got, call, oracle, name + " public")
    assert kernels == kernel_of(call)[1]
    objective = np.array([r["objective"] for r in refs])
    told = []
    for flaw in BD.SUM_FLAWS + BD.READ_FLAWS[1:]:
        wrong = np.array([r["objective"] for r in LBD.hard_answers(oracle, call, flaw)])
        if LBD.differing(wrong, objective):  # (one addition to a larger number rounds many a one-ulp change of the shift away)
            told.append(flaw)
            assert LBD.differing(got["objective"], wrong), "%s: the objective is what the flaw %r computes" % (name, flaw)
    assert set(told) >= set(BD.READ_FLAWS[1:]) and len(told) > 2, (name, told)
    inner = of(hard_ran, name)
    assert all(same(got[k], inner[k]) for k in ("x", "objective") + LBD.OUTPUTS)


def test_hard_views_give_the_words_of_copies_and_of_the_oracle(hard_ran, hard_calls, oracle):
    """A_ub and A_eq as transposed views (a column stride that is not 1), lb every other element of a wider tensor."""
    call = hard_calls[LBD.VIEWS_HARD]
    assert call.n == 129
    views, copies = of(hard_ran, "hard views"), of(hard_ran, "hard views copies")
    check_public(views, call, oracle, "hard views")
    assert set(views) == set(copies) and all(same(views[k], copies[k]) if views[k].dtype == np.float64 else np.array_equal(views[k], copies[k]) for k in views)

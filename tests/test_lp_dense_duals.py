"""yalps_lpdense_solve_duals, linprog_batch(duals=True) and linprog_objective on the GPU.  The work runs in two child processes
that import torch first (tests/_lp_dense.py says why); every test compares what a child wrote with the numpy restatement of the
marginals (tests/_np_dense_duals.py) on the C oracle's final tableau, bit for bit, all NaNs counted as one value."""
import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _lp_dense as LD
from tests import _lp_dense_duals as LDD
from tests import _np_dense_duals as DD
from tests.test_lp_dense import check_answers, of, same

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


def run_child(tmp_path_factory, which, env=None):
    import os
    import subprocess
    import sys
    from yalps_amd import build
    build.build_lpdense()
    build.build_lpsens()
    build.build_hip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("lp_dense_duals") / (which + ".npz"))
    child = subprocess.run([sys.executable, "-m", "tests._lp_dense_duals", which, path], cwd=root, capture_output=True, text=True, timeout=600,
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
    return {c.name: c for c in LDD.table(oracle)}


def check_marginals(got, call, refs, tag, want=LDD.MARGINALS):
    """The three rows of every LP against dense_marginals of the oracle's answer -- NaN unless it ended optimal --; a row that was
    not asked for still holds the sentinel."""
    B = len(call.lps)
    sign = 1.0 if call.maximize else -1.0
    for key, width in zip(LDD.MARGINALS, (call.m_ub, call.m_eq, call.n)):
        assert got[key].shape == (B, width) and got[key].dtype == np.float64, (tag, key, got[key].shape)
        if key not in want:
            assert (got[key] == LDD.SENTINEL).all(), (tag, key, "written without being asked for")
    for i, ref in enumerate(refs):
        for key, e in zip(LDD.MARGINALS, DD.marginals_of(ref, call.n, call.m_ub, call.m_eq, sign)):
            if key in want:
                assert same(got[key][i], e), ("%s LP %d" % (tag, i), key, ref["status"], got[key][i], e)


@pytest.mark.parametrize("name", LDD.names())
def test_call_against_the_oracle(ran, calls, oracle, name):
    call, got = calls[name], of(ran, name)
    refs = check_answers(got, call, oracle, name)
    check_marginals(got, call, refs, name)
    cls = LB.size_class(call.w, call.h)
    kernel = "lp_dense_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")
    assert str(got["kernels"]) == kernel and int(got["launches"]) == 1, (name, got["kernels"])
    optimal = [r for r in refs if r["status"] == "optimal"]
    sign = 1.0 if call.maximize else -1.0
    if name not in ("n=0", "statuses") and not name.startswith("n=1"):
        assert optimal, name
    if name.startswith("precision"):  # the variables out of the basis have reduced costs, up to the last lane's
        reduced = DD.marginals_of(refs[0], call.n, call.m_ub, call.m_eq, sign)[2]
        assert np.count_nonzero(reduced) >= call.n - call.m_ub - 1 and (call.n - 1) % 64 == 0
    if name == "ineqlin strides":
        ineqlin = DD.marginals_of(refs[0], call.n, call.m_ub, call.m_eq, sign)[0]
        assert np.flatnonzero(ineqlin).tolist() == [511, 1024] and ineqlin[[511, 1024]].tolist() == [2.0, 1.0]
    if name == "eqlin strides":
        eqlin = DD.marginals_of(refs[0], call.n, call.m_ub, call.m_eq, sign)[1]
        assert refs[0]["x"].tolist() == [3.0, 2.0] and np.count_nonzero(eqlin) and eqlin.size == 513
    if name == "both slacks":
        assert DD.slacks_out(refs[0]["pos"], call.n, call.m_ub, call.m_eq)
    if name.startswith("nonfinite"):  # ends optimal with a NaN in row 0: NaN marginals next to finite ones
        m = DD.marginals_of(refs[0], call.n, call.m_ub, call.m_eq, sign)
        assert refs[0]["status"] == "optimal" and np.isnan(refs[0]["matrix"][:call.w]).any()
        assert np.isnan(np.concatenate(m)).any() and not np.isnan(np.concatenate(m)).all(), name
    if name.startswith("aux"):
        assert refs[0]["status"] == "optimal"
    if name == "statuses":  # NaN rows exactly at the LPs that did not end optimal, in a call of more LPs than workgroups
        assert len(call.lps) > int(got["grids"][0]) >= 2048
        assert {r["status"] for r in refs} == set(LD.STATUS)
        bad = np.array([r["status"] != "optimal" for r in refs])
        assert np.array_equal(np.isnan(got["ineqlin"]).all(axis=1), bad) and np.array_equal(np.isnan(got["reduced"]).any(axis=1), bad)


def test_both_directions_of_one_lp(calls, oracle):
    """The calls "both kinds, minimize" and "both kinds, maximize" hold the same LPs."""
    a, b = calls["both kinds, minimize"], calls["both kinds, maximize"]
    assert all(x is None and y is None or np.array_equal(x, y) for p, q in zip(a.lps, b.lps) for x, y in zip(p, q))
    assert a.maximize != b.maximize


@pytest.mark.parametrize("want", LDD.PARTIAL, ids=lambda w: "+".join(w) or "none")
def test_only_the_requested_outputs_are_written(ran, oracle, want):
    """The same LPs with none, one, two and all of the new pointers: what was not asked for keeps its sentinel, what was is the
    oracle's, and x / objective / status / pivots, column 0, permutations and matrix are the same bits whatever was asked."""
    call = LDD.partial_call()
    got = of(ran, "partial %s" % ("+".join(want) or "none"))
    refs = check_answers(got, call, oracle, str(want))
    check_marginals(got, call, refs, str(want), want)
    full = of(ran, "partial %s" % "+".join(LDD.MARGINALS))
    for key in ("x", "objective", "status", "pivots", "col0", "pos", "var", "tableau"):
        assert got[key].tobytes() == full[key].tobytes(), (want, key)
    assert any(r["status"] == "optimal" for r in refs) and any(r["status"] != "optimal" for r in refs)


def test_the_flag_changes_none_of_the_four_old_outputs(ran, oracle):
    off, on = of(ran, "flag off"), of(ran, "flag on")
    assert sorted(off) == ["objective", "pivots", "status", "x"]
    for key in off:
        assert off[key].tobytes() == on[key].tobytes(), key
    refs = check_answers(on, LDD.partial_call(), oracle, "flag on", kept=False)
    check_marginals(on, LDD.partial_call(), refs, "flag on")


def test_history_rerun_writes_the_marginals(ran, hist, oracle):
    call = LD.hist_call(oracle)
    refs = check_answers(hist, call, oracle, "hist", kept=False)
    check_marginals(hist, call, refs, "hist")
    assert int(hist["reruns"]) >= len(call.lps) and int(hist["passes"]) >= 2
    clean = of(ran, "hist clean")
    for key in LDD.MARGINALS:
        assert hist[key].tobytes() == clean[key].tobytes(), key
    assert all(r["status"] == "optimal" for r in refs)


@pytest.mark.parametrize("views,contiguous,make", [("views", "contiguous", lambda: LD.strided_call(LD.strided_inputs())),
                                                  ("offset views", "offset contiguous", lambda: LD.offset_call(LD.offset_inputs()))])
def test_views_give_the_bits_of_contiguous_operands(ran, oracle, views, contiguous, make):
    call = make()
    a, b = of(ran, views), of(ran, contiguous)
    refs = check_answers(a, call, oracle, views, kept=False)
    check_marginals(a, call, refs, views)
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert any(r["status"] == "optimal" for r in refs)


def test_producer_on_a_side_stream(ran, oracle):
    inp = LD.stream_inputs()
    A = ran["stream/A"]
    assert np.array_equal(A, inp["A_half"] * 2.0)
    call = LD.Call("stream", [(inp["c"][i], A[i], inp["b_ub"][i], None, None) for i in range(5)], maximize=True)
    got = of(ran, "stream")
    check_marginals(got, call, check_answers(got, call, oracle, "stream", kept=False), "stream")


def test_empty_batch_and_sides_without_rows(ran):
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0, 0, 2, 0, 1, 0, 3]
    assert ran["no rows/shapes"].tolist() == [2, 0, 2, 0, 2, 3]
    assert str(ran["no rows/types"]) == " ".join(["Tensor torch.float64 cuda"] * 3)
    assert ran["no rows/status"].tolist() == [0, 0] and ran["no rows/reduced"].tolist() == [[1.0] * 3] * 2


def test_host_pointers_for_the_new_outputs_are_refused_by_name(ran, oracle):
    messages = [str(m) for m in ran["refusal/messages"]]
    assert len(messages) == 3
    for m, name in zip(messages, ("ineqlin_out", "eqlin_out", "reduced_out")):
        assert m.startswith("yalps_lpdense error -1: yalps_lpdense_solve_duals: %s is " % name) and "host memory" in m, m
        assert m.endswith("|| launches=0"), m
    assert bool(ran["refusal/untouched"])
    call = LD.random_call("refusal", 3, 2, 2, 1)
    got = of(ran, "refusal/after")
    check_marginals(got, call, check_answers(got, call, oracle, "after the refusals"), "after the refusals")


@pytest.mark.parametrize("k", (0, 2))
def test_marginals_are_sensitivity_many_of_the_equivalent_models(ran, k):
    call = LD.public_calls()[k]
    got = of(ran, "public " + call.name)
    assert np.array_equal(got["status"], got["sens_status"]) and (got["status"] == 0).any()
    for key in LDD.MARGINALS:
        assert same(got[key], got["sens_" + key]), (key, got[key], got["sens_" + key])


def close(a, b, ulps, scale=None):
    """|a - b| within `ulps` roundings of the magnitudes involved: the same real-number formula evaluated in another order."""
    scale = np.maximum(np.abs(a), np.abs(b)) if scale is None else scale
    return a.shape == b.shape and bool((np.abs(a - b) <= ulps * EPS * scale).all())


def formulas(got, i, g):
    return DD.objective_gradients(g, got["x"][i], got["ineqlin"][i], got["eqlin"][i])


GRADS = ("grad_c", "grad_A_ub", "grad_b_ub", "grad_A_eq", "grad_b_eq")


def test_objective_gradients_are_the_formulas_and_an_infeasible_row_is_zero(ran, oracle):
    """All five operands batched and requiring grad: row by row g x, -g y (x) x, g y from the returned tensors (two products in
    another order: 2 ulps); the infeasible row's gradient is exactly zero and nothing is NaN."""
    call = LDD.gradient_call()
    got = of(ran, "gradient rows")
    refs = check_answers(got, call, oracle, "gradient rows", kept=False)
    check_marginals(got, call, refs, "gradient rows")
    assert [r["status"] for r in refs] == ["optimal", "optimal", "infeasible"]
    for i, g in enumerate(LDD.GRADIENT_WEIGHTS):
        for key, want in zip(GRADS, formulas(got, i, g)):
            if refs[i]["status"] == "optimal":
                assert close(got[key][i], want, 2), (i, key, got[key][i], want)
                assert np.count_nonzero(want) or key == "grad_A_ub" and not np.count_nonzero(got["ineqlin"][i])
            else:
                assert not got[key][i].any() and not np.isnan(got[key][i]).any(), (i, key, got[key][i])


def test_a_shared_operand_receives_the_sum_over_the_batch(ran, oracle):
    call = LDD.shared_call()
    got = of(ran, "shared")
    refs = check_answers(got, call, oracle, "shared", kept=False)
    assert all(r["status"] == "optimal" for r in refs)
    rows = [formulas(got, i, g) for i, g in enumerate((1.0, 2.0, -3.0))]
    for k, key in enumerate(GRADS):
        if key == "grad_b_ub":
            assert close(got[key], np.stack([r[k] for r in rows]), 2), key
        else:  # (three terms of two products each, summed in some order)
            assert got[key].shape == rows[0][k].shape
            assert close(got[key], sum(r[k] for r in rows), 8, sum(np.abs(r[k]) for r in rows)), (key, got[key])
    assert np.count_nonzero(got["grad_A_ub"]) and np.count_nonzero(got["grad_c"])


@pytest.mark.parametrize("k", range(len(DD.GRAD_SEEDS)))
def test_objective_gradients_against_central_differences(ran, oracle, k):
    """The central-difference check of tests/test_lp_dense_duals_model.py with the device's objectives and autograd's gradients."""
    lp, maximize = DD.gradient_lps()[k]
    base = of(ran, "base %d" % k)
    auto = {op: base[key] for op, key in enumerate(GRADS)}
    numeric, ref = {}, None
    for call, step, operands in zip(LDD.difference_calls(k), (DD.GRAD_H, DD.GRAD_H_A), ((0, 2, 4), (1, 3))):
        got = of(ran, call.name)
        refs = check_answers(got, call, oracle, call.name, kept=False)
        assert all(r["status"] == "optimal" for r in refs)
        numeric.update(DD.central_differences(got["objective"], lp, step, operands))
        ref = refs[0]
    tol = DD.gradient_tolerances(ref, lp, auto)
    for op in range(5):
        assert auto[op].shape == np.shape(lp[op])
        assert (np.abs(numeric[op] - auto[op]) <= tol[op]).all(), (op, numeric[op], auto[op], tol[op])
    assert not bool(ran["no grad/grad_fn"])

"""libyalps_lpdense.so and linprog_batch on the GPU.  The work runs in three child processes that import torch first
(tests/_lp_dense.py says why); every test here compares what a child wrote with the C oracle on the numpy restatement of the
tableau (tests/_np_dense.py), bit for bit, all NaNs counted as one value."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _lp_batch as LB
from tests import _lp_dense as LD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(tmp_path_factory, which, env=None):
    from yalps_amd import build
    build.build_lpdense()
    build.build_hip()
    path = str(tmp_path_factory.mktemp("lp_dense") / (which + ".npz"))
    child = subprocess.run([sys.executable, "-m", "tests._lp_dense", which, path], cwd=ROOT, capture_output=True, text=True, timeout=600,
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
def public(tmp_path_factory):
    return run_child(tmp_path_factory, "public")


@pytest.fixture(scope="module")
def calls(oracle):
    return {c.name: c for c in LD.table(oracle)}


def same(a, b):
    """Bit for bit, all NaNs one value."""
    return LB.same_words(np.asarray(a, np.float64), np.asarray(b, np.float64), canonical_nan=True)


def check_answers(got, call, oracle, tag, kept=True):
    """x / objective / status / pivots of every LP of a call against the oracle; kept: also column 0, both permutations and the
    final matrix.  Returns the oracle's answers."""
    B = len(call.lps)
    assert got["x"].shape == (B, call.n) and got["objective"].shape == got["status"].shape == got["pivots"].shape == (B,), tag
    assert got["x"].dtype == got["objective"].dtype == np.float64 and got["status"].dtype == np.int32 and got["pivots"].dtype == np.int64
    refs = []
    for i in range(B):
        ref = call.oracle_answer(oracle, i)
        who = "%s LP %d" % (tag, i)
        assert LD.STATUS[int(got["status"][i])] == ref["status"], (who, got["status"][i], ref["status"])
        assert int(got["pivots"][i]) == ref["n_pivots"], (who, got["pivots"][i], ref["n_pivots"])
        assert same(got["objective"][i:i + 1], [ref["objective"]]), (who, got["objective"][i], ref["objective"], ref["result"])
        assert same(got["x"][i], ref["x"]), (who, got["x"][i], ref["x"])
        if kept:
            assert np.array_equal(got["pos"][i], ref["pos"]) and np.array_equal(got["var"][i], ref["var"]), who
            assert same(got["col0"][i], ref["col0"]), who
            assert same(got["tableau"][i], ref["matrix"]), who
        refs.append(ref)
    return refs


def of(ran, name):
    return {k[len(name) + 1:]: v for k, v in ran.items() if k.startswith(name + "/")}


@pytest.mark.parametrize("name", LD.names())
def test_call_against_the_oracle(ran, calls, oracle, name):
    call, got = calls[name], of(ran, name)
    refs = check_answers(got, call, oracle, name)
    assert bool(got["unchanged"]), "the call wrote into its operands"
    cls = LB.size_class(call.w, call.h)
    kernel = "lp_dense_kernel<%d%s%s>" % (1024 if cls >= 3 else 256, ",check" if call.check else "", ",lds" if cls < 4 else "")
    assert str(got["kernels"]) == kernel and int(got["launches"]) == 1 and int(got["reruns"]) == 0, (name, got["kernels"])
    assert got["classes"].tolist() == [cls]
    if name.startswith("aux"):
        assert got["aux"].tolist() == [1]
        want = {"0": ("cycled", 0), "half": ("cycled", None), "inf": ("optimal", None)}[name.split()[2]]
        assert refs[0]["status"] == want[0] and (want[1] is None or refs[0]["n_pivots"] == want[1])
    else:
        assert got["aux"].tolist() == [0]
    if name == "edge E9c":  # ended by hasCycle, not by the budget
        assert refs[0]["status"] == "cycled" and refs[0]["n_pivots"] < call.max_pivots and call.check
    if name == "cycled by budget":
        assert all(r["status"] == "cycled" and r["n_pivots"] == 3 for r in refs)
    if name.startswith("nonfinite N7"):  # finite operands, an option that is not finite or is negative
        assert np.isfinite(refs[0]["start"]).all() and not (0.0 <= call.precision < np.inf and 0.0 <= call.max_pivots), name
    elif name.startswith("nonfinite"):  # planted in the operands, or (N5) made by overflow from finite input
        planted, made = not np.isfinite(refs[0]["start"]).all(), not np.isfinite(refs[0]["matrix"]).all()
        assert (made and not planted) if name == "nonfinite N5" else planted, (name, planted, made)
    if name == "unbounded at the last variable":
        assert refs[0]["status"] == "unbounded" and np.flatnonzero(refs[0]["x"] == np.inf).tolist() == [call.n - 1] and call.n - 1 == 1024
    if name == "unbounded at a slack after a pivot":
        assert refs[0]["status"] == "unbounded" and refs[0]["n_pivots"] == 1 and not np.isinf(refs[0]["x"]).any()
        assert int(refs[0]["var"][int(refs[0]["result"])]) - 1 >= call.n
    if name.startswith("negative precision"):  # the reference rounds zeros there, to +0.0: no -0.0 in x
        assert refs[0]["status"] == "optimal" and (refs[0]["x"] == 0.0).any() and not np.signbit(refs[0]["x"]).any(), refs[0]["x"]
    if name == "queue":
        assert len(call.lps) > int(got["grids"][0]) >= 2048, "every workgroup is to take several LPs"
        assert {r["status"] for r in refs} == {"optimal", "infeasible", "unbounded"}


def test_endings_are_all_reached(calls, oracle):
    """What the table is there for, by the oracle: every status, an unbounded LP whose entering column holds a slack and one whose
    entering column holds a variable, NaN / +inf / -inf among the planted values."""
    seen, slack, planted = set(), set(), set()
    for name, call in calls.items():
        for i in range(min(len(call.lps), 64)):
            ref = call.oracle_answer(oracle, i)
            seen.add(ref["status"])
            if ref["status"] == "unbounded":
                slack.add(not 0 <= int(ref["var"][int(ref["result"])]) - 1 < call.n)
            if name.startswith("nonfinite"):
                s = ref["start"]
                planted |= {k for k, f in (("nan", np.isnan(s)), ("+inf", s == np.inf), ("-inf", s == -np.inf)) if f.any()}
    assert seen == set(LD.STATUS) and slack == {False, True} and planted == {"nan", "+inf", "-inf"}, (seen, slack, planted)


def test_history_rerun_gives_the_clean_answer(ran, hist, oracle):
    """YALPS_LPDENSE_HIST=4: every LP of the call overflows its history, runs again from the untouched operands, and the rerun's
    answer is the clean run's."""
    call = LD.hist_call(oracle)
    refs = check_answers(hist, call, oracle, "hist", kept=False)
    assert all(r["n_pivots"] > 2 * LD.HIST for r in refs)
    assert int(hist["reruns"]) >= len(call.lps) and int(hist["passes"]) >= 2
    clean = of(ran, "hist clean")
    assert int(clean["reruns"]) == 0
    for key in ("x", "objective", "status", "pivots"):
        assert hist[key].tobytes() == clean[key].tobytes(), key


def test_views_give_the_bits_of_contiguous_operands(ran, oracle):
    """A shared A_ub passed as a transposed view, a batched A_eq as a transposed view, c and b_ub as every-other-element slices,
    a shared b_eq: the same LPs passed contiguous give the same bits, both are the oracle's, and no input changed."""
    call = LD.strided_call(LD.strided_inputs())
    views, contiguous = of(ran, "views"), of(ran, "contiguous")
    refs = check_answers(views, call, oracle, "views", kept=False)
    check_answers(contiguous, call, oracle, "contiguous", kept=False)
    for key in ("x", "objective", "status", "pivots"):
        assert views[key].tobytes() == contiguous[key].tobytes(), key
    assert bool(views["unchanged"])
    assert any(r["status"] == "optimal" for r in refs)


def test_expanded_and_offset_views_give_the_bits_of_contiguous_operands(ran, oracle):
    """c and b_ub as one row expanded over the batch (a batch stride of 0), A_ub as the slice [:, 1:, 2:] of a wider tensor (a
    storage offset, padded rows): the oracle's bits, the bits of contiguous copies, and no input changed."""
    call = LD.offset_call(LD.offset_inputs())
    views, contiguous = of(ran, "offset views"), of(ran, "offset contiguous")
    refs = check_answers(views, call, oracle, "offset views", kept=False)
    check_answers(contiguous, call, oracle, "offset contiguous", kept=False)
    for key in ("x", "objective", "status", "pivots"):
        assert views[key].tobytes() == contiguous[key].tobytes(), key
    assert bool(views["unchanged"])
    assert any(r["status"] == "optimal" for r in refs)


def test_precision_calls_put_basic_values_on_the_edges(calls, oracle):
    """What the precision calls are there for, by the oracle: at every precision from 1e-8 up the run ends optimal with every
    bounded variable basic at b / 4, values at the precision itself (not above it: 0), one ulp above it, on ties; the free variable
    stays out of the basis; a rounded x differs from the value somewhere; the last variable is among the basic ones."""
    for (n, m) in LD.PRECISION_SHAPES:
        for p in (1e-8, 0.25, 0.75, 2.0, 2.5, 3.0):  # (at 1e-17 and 5e-324 the pivot flushes such right-hand sides to +0.0: |x| <= 1e-16)
            call = calls["precision %r n=%d" % (p, n)]
            ref = call.oracle_answer(oracle, 0)
            c, A, b = call.lps[0][:3]
            bound = {int(np.flatnonzero(row)[0]): b[i] / 4.0 for i, row in enumerate(A) if row.any()}
            cols = sorted(bound)
            assert ref["status"] == "optimal" and ref["n_pivots"] == len(cols), (p, n, ref["status"], ref["n_pivots"])
            basic = {j: float(ref["col0"][int(ref["pos"][j + 1]) - call.w]) for j in range(n) if ref["pos"][j + 1] >= call.w}
            assert basic == bound and cols[0] == 0 and cols[-1] == n - 1 and len(cols) < n, (p, n)
            assert p in basic.values() and np.nextafter(p, np.inf) in basic.values()
            assert ref["x"][[j for j in cols if basic[j] == p]].tolist() == [0.0] * sum(1 for j in cols if basic[j] == p)


def test_producer_on_a_side_stream_and_one_handle_for_two_shapes(ran, oracle):
    """A_ub comes out of torch ops enqueued on a non-default stream directly before the call inside torch.cuda.stream(s): the
    call reads what they wrote.  A second call of another shape on that stream reuses the cached handle."""
    inp = LD.stream_inputs()
    A = ran["stream/A"]
    assert np.array_equal(A, inp["A_half"] * 2.0)
    first = LD.Call("stream", [(inp["c"][i], A[i], inp["b_ub"][i], None, None) for i in range(5)], maximize=True)
    second = LD.Call("stream2", [(inp["c"][0, :3], A[i, :2, :3], inp["b_ub"][i, :2], None, None) for i in range(5)], maximize=True)
    check_answers(of(ran, "stream"), first, oracle, "stream", kept=False)
    check_answers(of(ran, "stream2"), second, oracle, "stream2", kept=False)
    default_handles, mid, end = ran["stream/handles"].tolist()
    assert (default_handles, mid, end) == (1, 2, 2), "one handle per (device, stream), kept between calls"
    assert str(ran["stream/kernels"]) == "lp_dense_kernel<256,lds>"


def test_empty_batch(ran):
    assert ran["empty/shapes"].tolist() == [0, 3, 0, 0, 0]
    assert str(ran["empty/dtypes"]) == "torch.float64 torch.float64 torch.int32 torch.int64"
    assert int(ran["empty/launches"]) == 0


def test_host_pointers_are_refused_not_read(ran, oracle):
    """LpDense.solve given host memory -- pageable or pinned -- for an operand or an output returns YALPS_E_ARG with a text that
    names the argument; nothing is launched, nothing is written, and the handle solves the next call."""
    messages = [str(m) for m in ran["refusal/messages"]]
    assert len(messages) == 3
    for m, name in zip(messages, ("c", "b_ub", "x_out")):
        assert m.startswith("yalps_lpdense error -1: yalps_lpdense_solve: %s is " % name) and "host memory" in m, m
        assert m.endswith("|| launches=0"), m
    assert bool(ran["refusal/x_untouched"])
    check_answers(of(ran, "refusal/after"), LD.random_call("refusal", 3, 2, 2, 0), oracle, "after the refusals")


@pytest.mark.parametrize("k", range(3))
def test_linprog_batch_is_solve_of_the_equivalent_model(public, oracle, k):
    """For finite data row i is solve(equivalent_model(i), includeZeroVariables=True): status, result bits, variable values."""
    call = LD.public_calls()[k]
    got = of(public, call.name)
    check_answers(got, call, oracle, call.name, kept=False)
    assert np.array_equal(got["status"], got["solve_status"])
    assert same(got["objective"], got["solve_result"]), (got["objective"], got["solve_result"])
    assert same(got["x"], got["solve_x"])
    assert (got["status"] == 0).any()

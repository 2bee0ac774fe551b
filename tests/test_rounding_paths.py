"""The family R (tests/_rounding.py: runs that end "optimal" with the result -0, or NaN at precision 3.0) through the batch
libraries, at one shape per size class: lp_batch, lp_sens, lp_variants, lp_warm, and as root LPs of MILPs through
milp_node_kernel's lockstep driver and milp_tree_kernel.  Everything is compared with the C oracle as the libraries' own tests
compare it, and the result word for word (the oracle's rounding is pinned by tests/test_rounding_records.py).  The paths of
libyalps_hip.so and the row shards run the same family from the reference's records in tests/test_edge_paths.py."""
import math

import numpy as np
import pytest

from tests import _bnc
from tests import _lp_batch as LB
from tests import _milp_batch as MB
from tests import _np_sensitivity as NS
from tests import _np_warm as NW
from tests import _rounding as RD

WINDOW = (-0.5 / 1e8 - RD.EPS, -RD.EPS)
SPECS = [(cls, f, M, N, RD.R_SEEDS.get((f, M, N), RD.R_SEED)) for cls, (M, N) in sorted(RD.R_CLASS_SHAPES.items()) for f in RD.R_FAMILIES]


def r_lp(oracle, family, M, N, seed):
    o = RD.r_options(family, M, N, seed)
    return LB.from_dense(RD.r_make(family, M, N, seed, dense_lp=oracle.dense_lp), N + 1, M + 1, **o)


@pytest.fixture(scope="module")
def lps(oracle):
    """[(spec, lp, the oracle's answer)], made once; every answer is "optimal" at -0 (R1n: NaN), Rn after at least 8 pivots."""
    out = []
    for spec in SPECS:
        cls, family, M, N, seed = spec
        lp = r_lp(oracle, family, M, N, seed)
        ref = LB.oracle_answer(oracle, lp)
        assert LB.size_class(lp[0], lp[1]) == cls, spec
        assert ref["status"] == "optimal" and ref["n_pivots"] >= RD.R_MIN_PIVOTS[family], (spec, ref["status"], ref["n_pivots"])
        assert RD.hexd(ref["result"]) == RD.hexd(math.nan if family == "R1n" else -0.0), (spec, ref["result"])
        if family == "Rn":
            assert WINDOW[0] <= ref["matrix"][0] < WINDOW[1], (spec, ref["matrix"][0])
        out.append((spec, lp, ref))
    return out


def test_the_family_does_what_it_is_there_for_at_every_class_shape(lps):
    assert {s[0] for s, _, _ in lps} == {0, 1, 2, 3, 4} and {s[1] for s, _, _ in lps} == set(RD.R_FAMILIES)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    assert _native.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return _native


def _bits(results, i, ref, spec):
    assert RD.hexd(float(results[i])) == RD.hexd(ref["result"]), (spec, float(results[i]), ref["result"])


@pytest.mark.gpu
def test_lp_batch_rounds_to_the_reference_zero(nat, lps):
    batch = nat.LpBatch(0)
    try:
        out = batch.solve([lp for _, lp, _ in lps], keep_tableaux=True)
        for i, (spec, lp, ref) in enumerate(lps):
            LB.check_lp(batch, i, out, ref, lp, label=str(spec))
            _bits(out[1], i, ref, spec)
        assert sorted({k["class"] for k in batch.info()["kernels"]}) == [0, 1, 2, 3, 4], batch.info()["text"]
    finally:
        batch.close()


@pytest.mark.gpu
def test_lp_sens_rounds_to_the_reference_zero(nat, lps):
    sens = nat.LpSens(0)
    try:
        out = sens.solve([lp for _, lp, _ in lps], keep_tableaux=True)
        for i, (spec, lp, ref) in enumerate(lps):
            NS.check_lp(sens, i, out, ref, lp, tag=str(spec))
            _bits(out[1], i, ref, spec)
        assert sorted({k["class"] for k in sens.info()["kernels"]}) == [0, 1, 2, 3, 4], sens.info()["text"]
    finally:
        sens.close()


def _no_patch():
    return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", sorted(RD.R_CLASS_SHAPES))
def test_lp_variants_round_to_the_reference_zero(nat, oracle, lps, cls):
    """Every tableau of the class as a base with two variants: the empty patch, and R0's m[0, 0] = -2^-40 written by a patch
    (over R0 itself it changes nothing; over the others it moves the final m[0, 0] by -2^-40: still inside the window, but for
    R1q, which leaves the tie and rounds to -0.25)."""
    lv = nat.LpVariants(0)
    try:
        for spec, lp, ref in (x for x in lps if x[0][0] == cls):
            w, h, row, col, val, precision, max_pivots, check = lp
            plant = (np.zeros(1, np.int32), np.zeros(1, np.int32), np.array([-2.0 ** -40]))
            out = lv.solve(nat.PackedVariants(w, h, row, col, val, [_no_patch(), plant], [(precision, max_pivots, check)] * 2),
                           keep_tableaux=True)
            LB.check_lp(lv, 0, out, ref, lp, label=str(spec))
            _bits(out[1], 0, ref, spec)
            m = LB.scatter(lp)
            m[0] = -2.0 ** -40
            planted = LB.from_dense(m, w, h, precision, max_pivots, check)
            pref = LB.oracle_answer(oracle, planted)
            want = -0.25 if spec[1] == "R1q" else ref["result"]  # (R1q sits on the tie: 4 * (-0.125 - 2^-40) rounds to -1)
            assert pref["status"] == "optimal" and RD.hexd(pref["result"]) == RD.hexd(want), spec
            LB.check_lp(lv, 1, out, pref, planted, label=str(spec) + " planted")
            _bits(out[1], 1, pref, spec)
    finally:
        lv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", sorted(RD.R_CLASS_SHAPES))
def test_lp_warm_rounds_to_the_reference_zero(nat, oracle, lps, cls):
    """Every tableau of the class as a base (the base's own result by bits) with two variants reoptimised from its final
    tableau: the empty patch (0 pivots: the final m[0, 0] is rounded again) and one right-hand side written with its own
    value."""
    lw = nat.LpWarm(0)
    try:
        for spec, lp, ref in (x for x in lps if x[0][0] == cls):
            w, h, row, col, val, precision, max_pivots, check = lp
            cells = (row, col, val)
            base = NW.solve_base(oracle, cells, w, h, precision, max_pivots, check)
            b0 = NW.edge_cells(cells, w)
            patches = [[], [(w, float(LB.scatter(lp)[w]))]]
            out = lw.solve(NW.packed_cells(nat, lp, patches, [(precision, max_pivots, check)] * 2, base_options=(precision, max_pivots, check)),
                           keep_tableaux=True)
            assert out is not None and lw.base[0] == "optimal" and lw.base[2] == ref["n_pivots"], (spec, lw.base)
            assert RD.hexd(lw.base[1]) == RD.hexd(ref["result"]), (spec, lw.base)
            for i, patch in enumerate(patches):
                want = NW.warm_answer(oracle, base, w, h, b0, patch, precision, max_pivots, check)
                LB.check_lp(lw, i, out, want, lp, label=str(spec) + " warm %d" % i)
                _bits(out[1], i, want, spec)
                assert RD.hexd(want["result"]) == RD.hexd(ref["result"]), (spec, i, want["result"])
    finally:
        lw.close()


# ---- MILPs whose root LP is a tableau of the family ----------------------------------------------------------------------------

def _milp_cases(oracle):
    """[(label, milp tuple, root, the scalar run over the oracle | None)]: R0 with integer variables that stay out of the basis
    (the root is integral: the answer is the root's -0), R1 with its one basic variable integer (basic at 2^-20: a tree under a
    root whose result is -0), Rn with one integer variable."""
    from yalps_amd.model import Tableau, TableauModel
    from tests import _edges as E
    out = []
    for family, (M, N), pick in (("R0", (60, 50), lambda w, h, c: [1, 2, w - 1]), ("R1", (60, 50), lambda w, h, c: [c]),
                                 ("R1", (130, 120), lambda w, h, c: [c]), ("Rn", (30, 30), lambda w, h, c: [1]),
                                 ("R1", (300, 280), lambda w, h, c: [c])):
        seed = RD.R_SEEDS.get((family, M, N), RD.R_SEED)
        w, h = N + 1, M + 1
        m = RD.r_make(family, M, N, seed, dense_lp=oracle.dense_lp)
        integers = pick(w, h, E._cols(E.default_layout(M, N), w, 1)[0])
        pos = np.arange(w + h, dtype=np.int32)
        tm = TableauModel(Tableau(m.copy(), w, h, pos, pos.copy()), 1.0, [("x%d" % j, {}) for j in range(1, w)], integers)
        root, run = MB.oracle_tree(oracle, None, None, tabmod=tm)
        milp = (w, h, *LB.cells_of(m, w, h), integers, 1.0, MB.options(None))
        out.append(("%s-%dx%d" % (family, M, N), milp, root, run))
    return out


@pytest.fixture(scope="module")
def milps(oracle):
    cases = _milp_cases(oracle)
    for label, _, root, run in cases:
        assert root.status == "optimal" and RD.hexd(root.result) == RD.hexd(-0.0) and run is not None, (label, root.status, root.result)
        assert run["iterations"] <= 64, (label, run["iterations"])  # (small trees)
    assert cases[0][3]["iterations"] == 0 and RD.hexd(cases[0][3]["result"]) == RD.hexd(-0.0)  # (the integral root: its -0 is the answer)
    assert any(run["iterations"] > 0 for _, _, _, run in cases)
    return cases


def _check_milps(handle, milps, statuses, results, used):
    for i, (label, _, root, run) in enumerate(milps):
        height, col0, pos, var = handle.solution(i)
        assert (statuses[i], _bnc.hexd(results[i]), int(used[i])) == (run["status"], _bnc.hexd(run["result"]), run["iterations"]), \
            (label, statuses[i], results[i], used[i], run["status"], run["result"], run["iterations"])
        assert (height, _bnc.sha(col0), _bnc.sha(pos, var)) == (run["best_height"], run["best_col0"], run["best_perm"]), label


@pytest.mark.gpu
def test_milp_node_roots_at_minus_zero(nat, milps):
    mb = nat.MilpBatch(0)
    try:
        statuses, results, used, _, _ = mb.solve([m for _, m, _, _ in milps])
        _check_milps(mb, milps, statuses, results, used)
    finally:
        mb.close()


@pytest.mark.gpu
def test_milp_tree_equals_the_lockstep_driver_by_bits(nat, milps):
    """milptree_solve against the scalar run over the oracle, and its status and result against the lockstep driver's, word
    for word."""
    mt, mb = nat.MilpTree(0), nat.MilpBatch(0)
    try:
        statuses, results, used, _, _ = mt.solve([m for _, m, _, _ in milps])
        _check_milps(mt, milps, statuses, results, used)
        lstatuses, lresults, lused, _, _ = mb.solve([m for _, m, _, _ in milps])
        assert list(statuses) == list(lstatuses) and [int(x) for x in used] == [int(x) for x in lused]
        assert [_bnc.hexd(x) for x in results] == [_bnc.hexd(x) for x in lresults]
    finally:
        mt.close()
        mb.close()

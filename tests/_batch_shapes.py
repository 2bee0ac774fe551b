"""Helpers of tests/test_batch_shapes.py (TEST INFRASTRUCTURE): the shapes and endings of lp_batch_kernel and milp_node_kernel
that the record-driven tests do not reach, as three tables with one row per purpose.

  shape_table   LPs for the root pass: both sides of the aux bound (colbuf / prow in LDS or behind the tableau in HBM), the far
                sides of the aux form, an odd column count in the HBM form, the degenerate shapes the validator admits, the
                batch limit
  node_table    (root, synthetic cut list, budget) for milp_node_kernel: zero cuts, cuts on basic and non-basic variables,
                signed-zero cut values, both sides of every class bound from one root, budgets that end a node inside phase 1
                and inside phase 2, a node hasCycle ends
  tree_table    whole models: finite maxPivots that makes nodes "cycled", trees that grow across a class bound or (a tall one
                and a wide one) across the aux bound, roots that are not optimal

Every expectation is computed at test time by the C oracle (oracle/simplex_oracle.c) and tests/_bnc.py; every comparison is
bit for bit.  Each row says which ending it was built for, and the builders assert that the oracle produces it."""
import math

import numpy as np

from tests import _bnc as BN
from tests import _edges as E
from tests import _lp_batch as LB
from tests import _milp_batch as MB
from tests import _milps as ML

AUX_LDS_MAX = 64 * 1024  # wg_queue_host.inc: colbuf + prow of the HBM form stay in LDS up to this many bytes
INF = math.inf


def pcols(w):
    """small_pcols(w - 1) (yalps_amd/csrc/wg_simplex.cuh): the columns 1 .. w - 1 padded to an even count."""
    return w & ~1


def aux_hbm(w, h):
    """The aux form of the HBM class (wg_queue_host.inc::lp_aux_hbm), restated: pcols + h > 8192."""
    return 8 * (pcols(w) + h) > AUX_LDS_MAX


def bits(x):
    """A result's value bits; every NaN is one value (the reference returns NaN for "cycled" and "infeasible")."""
    return "nan" if math.isnan(x) else BN.hexd(x)


def with_options(lp, max_pivots, check_cycles):
    return (*lp[:6], float(max_pivots), bool(check_cycles))


def hand(rows, **opts):
    """A small hand-made tableau: rows[0] the objective row, column 0 the right-hand sides."""
    a = np.array(rows, np.float64)
    return LB.from_dense(a.ravel().copy(), a.shape[1], a.shape[0], **opts)


def column(values, **opts):
    """A tableau without variables (w = 1): column 0 only."""
    return hand([[v] for v in values], **opts)


def edge_lp(oracle, family, M, N, seed):
    o = E.options(family, M, N, seed)
    return LB.from_dense(E.make(family, M, N, seed, dense_lp=oracle.dense_lp), N + 1, M + 1, o["precision"], o["max_pivots"],
                         o["check_cycles"])


# ------------------------------------------------------------------------------------------------ the root pass

def shape_table(oracle):
    """[(name, lp)]: one row per purpose.  A row whose name starts with "aux" is in the aux form and stands in the table six
    times: budgets 0, half the oracle's pivot count (strictly between 0 and it) and inf, checkCycles off and on."""
    D = lambda M, N, seed=3, **o: LB.dense_lp(oracle, M, N, seed, **o)
    rows = [
        # both sides of the aux bound, pcols + h = 8192 | 8193
        ("bound wide 8152+40, in LDS", D(39, 8151)),
        ("aux bound wide 8152+41", D(40, 8151)),
        ("bound tall 30+8162, in LDS", D(8161, 30)),
        ("aux bound tall 30+8163", D(8162, 30)),
        ("aux bound wide 8152+41, even n (w 8153)", D(40, 8152)),
        # the far sides of the aux form
        ("aux far wide 2 x 262144", D(1, 262143)),
        ("aux far tall 8191 x 64", D(8190, 63)),
        ("aux w = 2, 20000 rows", D(19999, 1)),
        # odd n in the HBM class: the last column of every row is padding
        ("odd n HBM 301 x 280", D(300, 279)),
        ("odd n HBM 301 x 280, checkCycles", D(300, 279, 4, check_cycles=True)),
        ("odd n HBM 161 x 152", D(160, 151)),
        ("odd n HBM 301 x 280 E4 signed zeros", edge_lp(oracle, "E4", 300, 279, 1)),
        ("odd n HBM 301 x 280 E5 flush band", edge_lp(oracle, "E5", 300, 279, 1)),
        ("odd n HBM 301 x 280 E1 entering ties, last column", edge_lp(oracle, "E1", 300, 279, 1)),
        ("odd n HBM 301 x 280 E3i infeasible", edge_lp(oracle, "E3i", 300, 279, 1)),
        ("aux odd n 41 x 8152 E4 signed zeros", edge_lp(oracle, "E4", 40, 8151, 1)),
        ("aux odd n 41 x 8152 E1 entering ties, last column", edge_lp(oracle, "E1", 40, 8151, 1)),
        # degenerate shapes
        ("w = 1, LDS, optimal", column([0.0, 1.0, 2.0, 0.0, 5.0])),
        ("w = 1, LDS, infeasible", column([0.0, 1.0, -2.0, 3.0])),
        ("w = 1, h = 1", column([7.0])),
        ("w = 1, HBM, infeasible in the last row", column([0.0] * 3999 + [-1.0])),
        ("w = 1, HBM, optimal", column([3.0] + [1.0] * 3999)),
        ("w = 2, LDS, one pivot", hand([[0.0, 2.0], [4.0, 2.0], [3.0, 1.0]])),
        ("w = 2, LDS, unbounded", hand([[0.0, 1.0], [4.0, -1.0], [3.0, 0.0]])),
        ("w = 2, h = 1", hand([[0.0, -1.0]])),
        ("w = 2, HBM, 6000 rows", D(5999, 1)),
        ("h = 1, LDS, optimal", hand([[1.5] + [-1.0, 0.0] * 24 + [-0.0]])),
        ("h = 1, LDS, unbounded in the last column", hand([[0.0] + [-1.0] * 48 + [2.0]])),
        ("h = 1, LDS class 3, 5001 columns", hand([[0.0] + [-1.0] * 5000])),
        ("h = 2, LDS class 3", D(1, 2999)),
        ("h = 2, HBM, in LDS", D(1, 6999)),
        ("h = 2, odd n, LDS class 0", D(1, 8)),
        # the batch limit: 4 MiB exactly
        ("batch limit 1024 x 512", D(1023, 511)),
    ]
    out = []
    for name, lp in rows:
        w, h = lp[0], lp[1]
        assert name.startswith("aux") == (LB.size_class(w, h) == 4 and aux_hbm(w, h)), (name, w, h)
        if not name.startswith("aux"):
            out.append((name, lp))
            continue
        n = LB.oracle_answer(oracle, with_options(lp, INF, False))["n_pivots"]
        assert n >= 1, name  # (a budget strictly between 0 and n exists: n / 2, whole or not)
        for budget in (0.0, n / 2.0, INF):
            for check in (False, True):
                out.append(("%s budget %g%s" % (name, budget, " check" if check else ""), with_options(lp, budget, check)))
    return out


# ------------------------------------------------------------------------------------------------ nodes

def packing(m, n, n_int, seed, density):
    return ML._packing(np.random.RandomState(seed), m, n, n_int, density=density)


def rows_under(bound, w):
    """The largest h with lds_bytes(w, h) <= bound."""
    h = 1
    while LB.lds_bytes(w, h + 1) <= bound:
        h += 1
    return h


def apply_cuts_basic_as_nonbasic(matrix, width, height, pos, var, cuts):
    """_bnc._apply_cuts WRONG on purpose: a cut on a variable that is basic at the root gets the row of a non-basic one."""
    fake = np.array(pos).copy()
    for _, v, _ in cuts:
        if fake[v] >= width:
            fake[v] = 1 + (fake[v] - width) % (width - 1)
    out, h, _, _ = BN._apply_cuts(matrix, width, height, fake, var, cuts)
    _, _, p, v = BN._apply_cuts(matrix, width, height, pos, var, cuts)
    return out, h, p, v


def node_reference(oracle, root, cuts, budget=None, apply=BN._apply_cuts, trace_cap=0):
    """What a MILP record holds of a node, by _apply_cuts and the oracle: the initial tableau's digest, then status, result
    bits, pivots, permutations and the final tableau as the budget leaves them (None: the root's maxPivots)."""
    m, h, p, v = apply(root.matrix, root.w, root.h, root.pos, root.var, cuts)
    node = dict(height=h, init_sha256=BN.sha(m))
    st, res, npiv, trace = oracle.simplex(m, root.w, h, p, v, precision=root.opt["precision"],
                                          max_pivots=root.opt["maxPivots"] if budget is None else budget,
                                          check_cycles=root.opt["checkCycles"], trace_cap=trace_cap)
    node.update(status=st, result=bits(res), n_pivots=npiv, final_sha256=BN.sha(m), perm_sha256=BN.sha(p, v),
                col0_sha256=BN.sha(m[::root.w][:h]))
    return node, trace


def phases(oracle, root, cuts):
    """(pivots of phase 1, pivots of phase 2, status) of a node under the default budget of 8192 pivots a phase: the oracle's pivot
    trace replayed with the oracle's pivot(); phase 1 lasts while a right-hand side below -precision is left
    (src/simplex.ts:111-120)."""
    node, trace = node_reference(oracle, root, cuts, 8192.0, trace_cap=1 << 14)
    assert node["n_pivots"] == len(trace)
    m, h, p, v = BN._apply_cuts(root.matrix, root.w, root.h, root.pos, root.var, cuts)
    w, prec, p1 = root.w, root.opt["precision"], len(trace)
    for k, (r, c) in enumerate(trace):
        if p1 == len(trace) and not (m[w:w * h:w] < -prec).any():
            p1 = k
        oracle.pivot(m, w, h, p, v, int(r), int(c))
    assert BN.sha(m) == node["final_sha256"], "the replay of the trace does not end where the oracle did"
    return p1, len(trace) - p1, node["status"]


def basic_at(root, v):
    return int(root.pos[v]) >= root.w


def value_of(root, v):
    p = int(root.pos[v])
    return float(root.matrix[(p - root.w) * root.w]) if p >= root.w else 0.0


def bound_cuts(root, k):
    """k synthetic cuts over the root's integer variables in turn: x <= floor(value), then x >= ceil(value) + 1 and so on."""
    ints, cuts = list(root.tm.integers), []
    for j in range(k):
        v = ints[j % len(ints)]
        x = value_of(root, v)
        cuts.append((1, v, float(math.floor(x))) if j < len(ints) else (-1, v, float(math.ceil(x)) - 1.0))
    return cuts


# (name, model, options that differ from the defaults) of every root of the node table
BOUND_WIDTHS = {0: 47, 1: 67, 2: 99, 3: 137}  # class k: a root of this width and rows_under(BOUNDS[k]) rows is just under the bound


def bound_model(k):
    w = BOUND_WIDTHS[k]
    return packing(rows_under(LB.BOUNDS[k], w) - 1, w - 1, 8, 2, 0.6)


def node_roots():
    odd = packing(150, 151, 8, 7, 0.3)
    return [
        ("ties", ML.make("ties", 0)[0], {}),
        ("cycles check", ML.make("cycles", 0)[0], {"checkCycles": True}),
        ("under bound 0", bound_model(0), {}),
        ("under bound 1", bound_model(1), {}),
        ("under bound 2", bound_model(2), {}),
        ("under bound 3", bound_model(3), {}),
        ("odd n HBM", odd, {}),
        ("odd n HBM check", odd, {"checkCycles": True}),
        ("tall under the aux bound", packing(8160, 30, 6, 1, 0.3), {}),
        ("odd n HBM, root stopped in phase 2", odd, {"maxPivots": 200}),
        ("class 1 check, root stopped in phase 2", bound_model(1), {"maxPivots": 50, "checkCycles": True}),
        ("batch limit, root stopped in phase 2", packing(1021, 511, 4, 1, 0.05), {"maxPivots": 20}),
        ("wide under the aux bound", packing(40, 8150, 6, 1, 0.3), {}),
        ("E9c, hasCycle", edge_model("E9c", 20, 24, 1, 6), {"checkCycles": True}),
        ("E9c odd n HBM, hasCycle", edge_model("E9c", 300, 279, 1, 6), {"checkCycles": True}),
    ]


def node_table(roots):
    """[(name, root index, cuts, budget, wanted ending)] over node_roots() solved (MB.Root).  budget None is the root's own
    maxPivots.  The wanted ending is a status, or "phase 1" / "phase 2": the budget ends the node inside that phase."""
    R = {name: i for i, (name, _, _) in enumerate(node_roots())}
    T = []
    add = lambda name, root, cuts, budget=None, want="optimal": T.append((name, R[root], list(cuts), budget, want))
    for r in ("ties", "cycles check", "odd n HBM", "tall under the aux bound", "under bound 3"):
        add("zero cuts", r, [])
    # one cut on a variable that is basic at the root and on one that is not, both signs (src/branchAndCut.ts:32-42)
    for r in ("ties", "odd n HBM", "under bound 2"):
        root = roots[R[r]]
        for basic in (True, False):
            v = next(x for x in root.tm.integers if basic_at(root, x) == basic)
            x = value_of(root, v)
            add("basic" if basic else "non-basic", r, [(1, v, float(math.floor(x)))], want=None)
            add("basic" if basic else "non-basic", r, [(-1, v, float(math.ceil(x)) + (0.0 if basic else 1.0))], want=None)
            # signed-zero cut values: the zeros applyCuts writes, seen at budget 0 and after the solve
            for sign in (1, -1):
                for zero in (-0.0, 0.0):
                    add("signed zero", r, [(sign, v, zero)], 0.0, "cycled")
                    add("signed zero", r, [(sign, v, zero)], None, None)
    # both sides of every class bound and of the aux bound among the nodes of one root
    for k in range(4):
        for ncuts in range(0, 7):
            add("class bound %d" % k, "under bound %d" % k, bound_cuts(roots[R["under bound %d" % k]], ncuts))
    tall, wide = roots[R["tall under the aux bound"]], roots[R["wide under the aux bound"]]
    for ncuts in range(1, 5):
        add("aux bound tall", "tall under the aux bound", bound_cuts(tall, ncuts))
        add("aux bound wide", "wide under the aux bound", [(-1, v, 1.0) for v in list(wide.tm.integers)[:ncuts]], want=None)
    for ncuts in range(1, 6):
        add("odd n", "odd n HBM", bound_cuts(roots[R["odd n HBM"]], ncuts))
        add("odd n check", "odd n HBM check", bound_cuts(roots[R["odd n HBM check"]], ncuts))
    limit = roots[R["batch limit, root stopped in phase 2"]]
    add("4 MiB node", "batch limit, root stopped in phase 2", bound_cuts(limit, 2), 10.0, "cycled")
    # budgets that end a node inside phase 1: nodes of optimal roots (a cut list on an optimal root leaves phase 2 nothing to do)
    add("budget", "under bound 1", bound_cuts(roots[R["under bound 1"]], 2), 9.0, "phase 1")
    add("budget", "under bound 2", bound_cuts(roots[R["under bound 2"]], 8), 15.0, "phase 1")
    add("budget", "under bound 3", bound_cuts(roots[R["under bound 3"]], 6), 8.0, "phase 1")
    add("budget", "odd n HBM", bound_cuts(roots[R["odd n HBM"]], 1), 8.0, "phase 1")
    add("budget", "odd n HBM check", bound_cuts(roots[R["odd n HBM check"]], 4), 12.5, "phase 1")
    add("budget", "tall under the aux bound", bound_cuts(tall, 2), 40.0, "phase 1")
    add("budget", "tall under the aux bound", bound_cuts(tall, 1), 1.0, "phase 1")
    # ... and inside phase 2: nodes of roots that their own budget stopped before the optimum
    for r in ("odd n HBM, root stopped in phase 2", "class 1 check, root stopped in phase 2"):
        add("budget", r, [], 7.0, "phase 2")
        add("budget", r, [], 1.0, "phase 2")
        add("budget", r, [], None, "phase 2")  # (the root's own budget: it is short for the node as well)
        add("budget", r, bound_cuts(roots[R[r]], 1), 30.0, "phase 1" if r.startswith("odd") else "phase 2")
        add("budget", r, bound_cuts(roots[R[r]], 3), 8192.0, None)
    # nodes that hasCycle ends (see has_cycle_search below): under the root's budget and under an infinite one
    for r in ("E9c, hasCycle", "E9c odd n HBM, hasCycle"):
        for cuts in ([], [(1, 1, 0.0)], [(-1, 2, 1.0)], [(1, 3, 5.0), (1, 4, 2.0)]):
            add("hasCycle", r, cuts, None, "hasCycle")
        add("hasCycle", r, [(-1, 2, 1.0)], INF, "hasCycle")
    return T


def ending(oracle, root, cuts, budget):
    """Where a node ends: its status, or "phase 1" / "phase 2" where the budget runs out inside that phase, or "hasCycle" where
    checkCycles ends it before either phase has used its budget."""
    b = root.opt["maxPivots"] if budget is None else budget
    if b <= 0:
        return "cycled"
    p1, p2, status = phases(oracle, root, cuts)
    if b < p1:
        return "phase 1"
    if p1 < 8192 and b < p2:
        return "phase 2"

    if status == "cycled" and root.opt["checkCycles"] and p1 < b and p2 < b:
        return "hasCycle"  # (neither phase used its budget up: hasCycle ended the node, src/simplex.ts:98)
    return status


def has_cycle_search(oracle, families=("cycles", "negzero", "ties", "eqmm"), seeds=range(40)):
    """(nodes tried, [(family, seed, cuts)] that hasCycle ends) over the seeded MILP families with checkCycles on and the
    default budget: every list of one cut and every list of two cuts on different integer variables with sign +1 | -1 and
    value 0 | 1 | 2.  Seconds on one core; test_what_the_tables_cover asserts what the comment below says of it."""
    tried, found = 0, []
    for family in families:
        for seed in seeds:
            root = MB.Root(oracle, ML.make(family, seed)[0], {"checkCycles": True})
            one = [(s, v, x) for v in root.tm.integers for s in (1, -1) for x in (0.0, 1.0, 2.0)]
            for cuts in [[c] for c in one] + [[a, b] for a in one for b in one if a[1] < b[1]]:
                node = node_reference(oracle, root, cuts)[0]
                tried += 1
                if node["status"] == "cycled" and node["n_pivots"] < root.opt["maxPivots"]:
                    found.append((family, seed, cuts))
    return tried, found


# has_cycle_search(oracle) tries 106920 nodes of the MILP families and the oracle ends none of them as "cycled".  The degenerate
# edge families have one that cycles, E9c (Chvatal's cycling LP, tests/_edges.py): with checkCycles its root LP is ended by
# hasCycle after 11 pivots, and a node cut from the tableau that leaves (zero cuts, one cut, two cuts) starts with an empty
# history, cycles again and is ended by hasCycle after 11 or 12 pivots of a budget of 8192.  Those are the "hasCycle" rows
# of node_table, in the LDS form and, with an odd column count, in the HBM form; the budget-cycled nodes of checkCycles roots
# (the "check" rows) stay next to them.


def edge_model(family, M, N, seed, n_int):
    """An edge-family tableau (tests/_edges.py) as the root of a tree: its first n_int variables are integer."""
    from yalps_amd.model import Tableau, TableauModel
    w, h = N + 1, M + 1
    perm = np.arange(w + h, dtype=np.int32)
    return TableauModel(Tableau(E.make(family, M, N, seed), w, h, perm, perm.copy()), 1.0,
                        [("x%d" % j, {}) for j in range(1, w)], list(range(1, n_int + 1)))


def solve_root(oracle, model, extra):
    """MB.Root of a node_roots() row: a model, or the TableauModel of an edge family."""
    return MB.Root(oracle, None, extra, tabmod=model) if hasattr(model, "tableau") else MB.Root(oracle, model, extra)


def root_lp(model, extra):
    """A node_roots() row as LpBatch / MilpBatch.roots take it."""
    if not hasattr(model, "tableau"):
        return MB.lp_of(MB.milp_of(model, extra))
    t, opt = model.tableau, MB.options(extra)
    return LB.from_dense(t.matrix, t.width, t.height, opt["precision"], opt["maxPivots"], opt["checkCycles"])


def takes_basic_branch(root, cuts):
    """Per cut, whether applyCuts takes the branch of a variable that is basic at the root (milp_node_kernel.cuh: p >= w)."""
    return [basic_at(root, v) for _, v, _ in cuts]


# ------------------------------------------------------------------------------------------------ trees

def infeasible_model():
    return ML._model("maximize", [1.0, 2.0], [[1, 1], [1, 1]], [{"max": 1.0}, {"min": 2.0}], range(2))


def unbounded_model():
    return ML._model("maximize", [1.0, 1.0], [[1, -1]], [{"max": 2.0}], range(2))


def wide_model():
    """A wide tree across the aux bound, made by hand: a 40 x 8150 packing model is almost always integral at the root (of its
    8150 columns at most 40 are basic, and the few integer ones are rarely among them), so the 8 integer columns of
    packing(40, 8150, seed 2, density 0.3) get an objective coefficient of 60, three times the largest of the others.  They
    enter the basis at fractional values: the root is 41 x 8151 (pcols + h = 8191), its two children have 8192 and stay in
    LDS, everything below them is in the aux form.  18 nodes, ending "optimal"."""
    m = packing(40, 8150, 8, 2, 0.3)
    for name in m["integers"]:
        m["variables"][name]["obj"] = 60.0
    return m


def tree_table():
    """[(name, model, options)]: the whole-solve cases.  The endings each was built for are asserted in the tests."""
    cyc = ML.make("cycles", 0)[0]
    return [
        ("cycles-0, default budget", cyc, {"checkCycles": True}),
        ("cycles-0, maxPivots 5", cyc, {"checkCycles": True, "maxPivots": 5}),
        ("cycles-0, default budget again", cyc, {"checkCycles": True}),
        ("ties-0, maxPivots 3", ML.make("ties", 0)[0], {"maxPivots": 3}),
        ("cycles-0, maxPivots 5 again", cyc, {"checkCycles": True, "maxPivots": 5}),
        ("break-0, maxPivots 4", ML.make("break", 0)[0], {"maxPivots": 4}),
        ("eqmm-0, maxPivots 5", ML.make("eqmm", 0)[0], {"maxPivots": 5}),
        ("eqmm-0, default budget", ML.make("eqmm", 0)[0], {}),
        ("eqmm-3, maxPivots 5", ML.make("eqmm", 3)[0], {"maxPivots": 5}),
        ("class 2 -> 3", packing(97, 98, 8, 2, 0.6), {}),
        ("class 3 -> HBM", bound_model(3), {"maxIterations": 24}),
        ("odd n HBM", packing(150, 151, 8, 7, 0.3), {"maxIterations": 24}),
        ("tall across the aux bound", packing(8160, 30, 6, 1, 0.3), {"maxIterations": 24}),
        ("wide across the aux bound", wide_model(), {"maxIterations": 24}),
        ("root infeasible", infeasible_model(), {}),
        ("root unbounded", unbounded_model(), {}),
        ("root cycled by budget", packing(60, 60, 6, 1, 0.6), {"maxPivots": 3}),
        ("root cycled by budget, ties-1", ML.make("ties", 1)[0], {"maxPivots": 2}),
        ("cycles-0, default budget, last", cyc, {"checkCycles": True}),
    ]


def tree_disagreement(out, root, run):
    """None where a lockstep run of one model (nat.milp_search's tuple) equals the scalar branch and cut (MB.oracle_tree), else
    the first difference.  A root that is not optimal: the root's status and result, no node used, the root's tableau."""
    status, result, height, col0, pos, var, used, evaluated = out
    if run is None:
        want = (root.status, bits(root.result), 0, root.h, BN.sha(root.matrix[::root.w][:root.h]), BN.sha(root.pos, root.var))
    else:
        want = (run["status"], bits(run["result"]), run["iterations"], run["best_height"], run["best_col0"], run["best_perm"])
    got = (status, bits(result), used, height, BN.sha(col0), BN.sha(pos, var))
    return None if got == want and used <= evaluated else "%r != %r" % (got, want)


def hbm_launches(nat, oracle, roots, node_batch):
    """What the lockstep driver (the one MilpBatch.solve runs) puts into the HBM-class launch of every round, by the oracle as
    evaluator: {(round, checkCycles): (nodes, aux members, the launch's dynamic LDS)}.  The LDS is that of the non-aux members
    alone, rounded up to 16 bytes (milp_batch.hip)."""
    rounds = []

    class Logged(MB.OracleEvaluator):
        def __call__(self, nodes):
            rounds.append([(m, len(cuts)) for m, cuts in nodes])
            return super().__call__(nodes)

    nat.milp_search([r.packed() for r in roots], Logged(oracle, roots), node_batch=node_batch)
    out = {}
    for k, members in enumerate(rounds):
        for check in (False, True):
            shape = [(roots[m].w, roots[m].h + n) for m, n in members if bool(roots[m].opt["checkCycles"]) == check]
            shape = [(w, h) for w, h in shape if LB.size_class(w, h) == 4]
            if shape:
                lds = max([8 * (pcols(w) + h) for w, h in shape if not aux_hbm(w, h)], default=0)
                out[(k, check)] = (len(shape), sum(aux_hbm(w, h) for w, h in shape), max((lds + 15) & ~15, 16))
    return out

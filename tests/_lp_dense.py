"""Helpers of tests/test_lp_dense.py (TEST INFRASTRUCTURE): the calls the GPU tests of libyalps_lpdense.so / linprog_batch make,
and the three child processes that make them.

torch brings a HIP runtime along, and a pointer or a stream is only good in the runtime that made it, so torch has to be
loaded before any of the package's libraries -- which the test process, long past its first library call, cannot arrange.
Each child imports torch first, runs its calls, and writes everything they left behind to one .npz; the tests compare those
files with the C oracle (tests/_oracle.py) on tests/_np_dense.py's restatement of the tableau.

  table(oracle)   [Call]: every call of the child "table" -- through _native.LpDense with kept tableaux, so that column 0, both
                  permutations and the final matrix of every LP can be compared besides x / objective / status / pivots
  child "table"   the table, then the plumbing calls through linprog_batch: strided views, a producer on a side stream, one
                  handle for two shapes, B = 0, the refusal of host pointers
  child "hist"    under YALPS_LPDENSE_HIST=4: the rerun of LPs whose checkCycles history overflows
  child "public"  linprog_batch next to solve() of the equivalent models
"""
import math
import sys

import numpy as np

from tests import _batch_shapes as BS
from tests import _edges as E
from tests import _lp_batch as LB
from tests import _nonfinite as NF
from tests import _np_dense as ND
from tests import _rounding as RD

INF = math.inf
STATUS = ("optimal", "infeasible", "unbounded", "cycled")
EDGE_SHAPE = (30, 29)         # (M, N) of the edge families: class 0, odd n
EDGE_SEED = 1
NONFINITE_SHAPE = (60, 64)    # (M, N) of the non-finite families
AUX_SHAPE = (8162, 30)        # (m_ub, n): pcols + h = 30 + 8163 = 8193, colbuf / prow behind the tableau in HBM
QUEUE_LPS = 2100              # more than class 0's grid of 8 x 256 workgroups
HIST = 4                      # YALPS_LPDENSE_HIST of the child "hist"
GRID_HOOKS = ("YALPS_LPDENSE_CUS", "YALPS_LPDENSE_PER_CU")  # (test hooks that shrink the grid: kept out of the children's environments)


class Call:
    """One call: B LPs of one shape, each (c, A_ub, b_ub, A_eq, b_eq) in numpy (None: no rows of that kind), one set of options."""

    def __init__(self, name, lps, maximize=False, precision=1e-8, max_pivots=8192.0, check=False):
        self.name, self.lps, self.maximize = name, list(lps), bool(maximize)
        self.precision, self.max_pivots, self.check = precision, float(max_pivots), bool(check)
        self.n, self.m_ub, self.m_eq = ND.shape_of(*self.lps[0])
        assert all(ND.shape_of(*lp) == (self.n, self.m_ub, self.m_eq) for lp in self.lps), name
        self.w, self.h = self.n + 1, 1 + self.m_ub + 2 * self.m_eq

    def stacked(self):
        """(c [B, n], A_ub [B, m_ub, n], b_ub [B, m_ub], A_eq, b_eq), None where there are no such rows."""
        out = []
        for k, shape in enumerate(((self.n,), (self.m_ub, self.n), (self.m_ub,), (self.m_eq, self.n), (self.m_eq,))):
            rows = self.m_ub if k in (1, 2) else self.m_eq
            out.append(None if k and not rows else np.stack([np.asarray(lp[k], np.float64).reshape(shape) for lp in self.lps]))
        return out

    def oracle_answer(self, oracle, i):
        m = ND.dense_tableau(*self.lps[i], maximize=self.maximize)
        start = m.copy()
        pos, var = np.arange(self.w + self.h, dtype=np.int32), np.arange(self.w + self.h, dtype=np.int32)
        status, result, npiv, _ = oracle.simplex(m, self.w, self.h, pos, var, precision=self.precision, max_pivots=self.max_pivots,
                                                 check_cycles=self.check)
        col0 = m.reshape(self.h, self.w)[:, 0].copy()
        x, objective = ND.dense_solution(col0, pos, var, status, result, 1.0 if self.maximize else -1.0, self.precision, self.n)
        return dict(status=status, result=result, n_pivots=npiv, matrix=m, start=start, col0=col0, pos=pos, var=var, x=x, objective=objective)


def random_lp(rng, n, m_ub, m_eq):
    """Small integers, zeros and negative right-hand sides among them: optimal, infeasible and unbounded LPs all occur."""
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    return (ints(-2, 5, n), ints(-2, 4, m_ub, n) if m_ub else None, ints(-1, 7, m_ub) if m_ub else None,
            ints(-2, 4, m_eq, n) if m_eq else None, ints(0, 5, m_eq) if m_eq else None)


def random_call(name, B, n, m_ub, m_eq, **options):
    rng = np.random.default_rng([20261019, B, n, m_ub, m_eq])
    return Call(name, [random_lp(rng, n, m_ub, m_eq) for _ in range(B)], **options)


def tableau_call(name, tableaux, w, h, **options):
    """Dense tableaux whose cell (0, 0) is +0.0 as maximising LPs without equalities (tests/_np_dense.py::from_tableau)."""
    return Call(name, [(*ND.from_tableau(m, w, h), None, None) for m in tableaux], maximize=True, **options)


def bound_shapes():
    """(k, w, h) just under and just over every LDS class bound."""
    out = []
    for k, w in sorted(BS.BOUND_WIDTHS.items()):
        h0 = BS.rows_under(LB.BOUNDS[k], w)
        out += [(k, w, h0), (k, w, h0 + 1)]
    return out


def edge_families(oracle):
    """The edge families whose tableau at EDGE_SHAPE has +0.0 in cell (0, 0)."""
    M, N = EDGE_SHAPE
    out = []
    for f in E.FAMILIES:
        if E.shapes_for(f, M, N):
            m = E.make(f, M, N, EDGE_SEED, dense_lp=oracle.dense_lp)
            if m[:1].view(np.int64)[0] == 0:
                out.append((f, m))
    return out


def nonfinite_families(oracle):
    M, N = NONFINITE_SHAPE
    out = []
    for f in NF.FAMILIES[:6]:
        seed = NF.SEEDS.get((f, M, N), NF.SEED)
        m = NF.make(f, M, N, seed, dense_lp=oracle.dense_lp)
        if m[:1].view(np.int64)[0] == 0:
            out.append((f, seed, m))
    return out


N7_SEEDS = tuple(range(NF.SEED, NF.SEED + 10))  # the ten variants of N7: options that are not finite, on finite tableaux
PRECISION_SHAPES = ((65, 65), (257, 16), (1025, 64))  # (n, m_ub) of the precision calls: 256 lanes in LDS twice, 1024 lanes in HBM


def precision_names():
    return ["precision %r n=%d" % (p, n) for n, _ in PRECISION_SHAPES for p in RD.PRECISIONS]


def precision_lp(n, m, p):
    """maximize 5 (x_k1 + .. + x_km) + 0 x_free - (the others), 4 x_ki <= b_i: every bounded variable ends basic at b_i / 4
    (exact: a power of two), x_free and the others stay out of the basis.  b / 4 holds `precision`, its two neighbours, the
    ties (j + 0.5) * precision, the ends of the -0 window of its rounding and 1e300, in turn; where the precision is not
    positive and finite they are built around 1e-8.  The bounded variables are spread over 0 .. n - 1, both ends among them."""
    q = p if 0.0 < p < math.inf else 1e-8
    edges = [q, math.nextafter(q, math.inf), math.nextafter(q, 0.0)] + [(j + 0.5) * q for j in range(6)]
    edges += [max(1.5 * q - RD.EPS, 0.0), math.nextafter(1.5 * q, math.inf), 1e300, 0.375, 3.0, 2.0 ** 53 * q, 0.49999999999999994 * q + q]
    cols = sorted({(i * (n - 1)) // (m - 1) for i in range(m)}) if m < n else list(range(n))
    free = next(j for j in range(n - 2, -1, -1) if j not in cols) if m < n else None
    c = np.full(n, -1.0)
    c[cols] = 5.0
    A = np.zeros((len(cols), n))
    b = np.zeros(len(cols))
    for i, j in enumerate(cols):
        A[i, j] = 4.0
        b[i] = 4.0 * edges[i % len(edges)]
    if free is not None:
        c[free] = 0.0
    else:  # (m = n: one variable is given up as the free one; its row bounds nothing)
        free = n - 2
        c[free], A[free, free] = 0.0, 0.0
    return c, A, b, None, None


def precision_call(n, m, p):
    return Call("precision %r n=%d" % (p, n), [precision_lp(n, m, p)], maximize=True, precision=p)


def ending_calls():
    """Endings of `after` no other call reaches by design: a negative precision on an LP that ends optimal (reduced costs of -2
    and right-hand sides of 1 and more, so that neither `> precision` nor `< -precision` starts anything) with variables out of
    the basis: their 0.0 passes `value > precision` and is rounded, by the reference to +0.0; "unbounded" at the last of n
    variables (n - 1 = 1024: the lane that writes +inf is lane 0 of the second round); "unbounded" where the entering column
    holds a slack after a phase-1 pivot (no +inf anywhere)."""
    n = 9
    c = np.array([5.0, 5.0, 5.0, -2.0, -2.0, 5.0, -2.0, -2.0, 5.0])
    A = np.zeros((5, n))
    A[np.arange(5), [0, 1, 2, 5, 8]] = 4.0
    b = np.array([4.0, 8.0, 12.0, 6.0, 4.0 * (1.0 + 2.5e-8)])
    neg = [Call("negative precision %r, zeros" % p, [(c, A, b, None, None)], maximize=True, precision=p) for p in (-1e-8, -1.0)]
    n = 1025
    c = np.zeros(n)
    c[-1] = 1.0
    c[:8] = 0.5
    A = np.zeros((3, n))
    A[0, :8], A[1, 8:16], A[2, -1] = 1.0, 1.0, -1.0
    last = Call("unbounded at the last variable", [(c, A, np.array([2.0, 3.0, 1.0]), None, None)], maximize=True)
    slack = Call("unbounded at a slack after a pivot", [(np.array([1.0, -1.0, 0.0]), np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 1.0]]),
                                                        np.array([-1.0, 2.0]), None, None)], maximize=True)
    return neg + [last, slack]


ENDING_NAMES = ["negative precision -1e-08, zeros", "negative precision -1.0, zeros", "unbounded at the last variable",
                "unbounded at a slack after a pivot"]


def names():
    """The names of table()'s calls, without building one (the tests are parametrised by them)."""
    out = ["n=1 m=1", "n=2 m=1", "odd n, both kinds of rows", "even n, both kinds of rows, maximize", "equalities only", "n=0",
           "n=0 m=0", "n=0, HBM form", "inequalities only, precision 0.25"]
    out += ["class %d bound %s, %dx%d" % (k, "under" if j % 2 == 0 else "over", h, w) for j, (k, w, h) in enumerate(bound_shapes())]
    out += ["HBM odd n 301x280"]
    out += ["aux budget %s%s" % (b, " check" if c else "") for b in ("0", "half", "inf") for c in (False, True)]
    out += ["limit 1024x512"]
    out += ["edge %s" % f for f in E.FAMILIES if E.shapes_for(f, *EDGE_SHAPE)]
    out += ["nonfinite %s" % f for f in NF.FAMILIES[:6]]
    out += ["cycled by budget", "hist clean", "queue"]
    out += ["nonfinite N7 s%d" % seed for seed in N7_SEEDS] + precision_names() + ENDING_NAMES
    return out


def hist_call(oracle):
    """Four dense LPs with checkCycles on, each of more than 2 * HIST pivots: a history of HIST pivots overflows for all."""
    return tableau_call("hist clean", [oracle.dense_lp(30, 29, s) for s in (3, 4, 5, 6)], 30, 31, check=True)


def table(oracle):
    D = oracle.dense_lp
    T = [random_call("n=1 m=1", 6, 1, 1, 0), random_call("n=2 m=1", 6, 2, 1, 0),
         random_call("odd n, both kinds of rows", 8, 5, 4, 3), random_call("even n, both kinds of rows, maximize", 8, 6, 3, 2, maximize=True),
         random_call("equalities only", 6, 9, 0, 4), random_call("n=0", 4, 0, 3, 0), random_call("n=0 m=0", 2, 0, 0, 0),
         random_call("n=0, HBM form", 2, 0, 4000, 0),
         random_call("inequalities only, precision 0.25", 6, 8, 3, 0, maximize=True, precision=0.25)]
    for j, (k, w, h) in enumerate(bound_shapes()):
        assert LB.size_class(w, h) == k + j % 2, (k, w, h)
        T.append(tableau_call("class %d bound %s, %dx%d" % (k, "under" if j % 2 == 0 else "over", h, w), [D(h - 1, w - 1, 3), D(h - 1, w - 1, 4)], w, h))
    assert LB.size_class(280, 301) == 4 and not BS.aux_hbm(280, 301)
    T.append(tableau_call("HBM odd n 301x280", [D(300, 279, 3), E.make("E4", 300, 279, 1, dense_lp=D)], 280, 301))
    m_ub, n = AUX_SHAPE
    assert LB.size_class(n + 1, m_ub + 1) == 4 and BS.aux_hbm(n + 1, m_ub + 1) and not BS.aux_hbm(n + 1, m_ub)
    aux = D(m_ub, n, 3)
    full = tableau_call("aux", [aux], n + 1, m_ub + 1, max_pivots=INF).oracle_answer(oracle, 0)["n_pivots"]
    assert full >= 1
    for label, budget in (("0", 0.0), ("half", full / 2.0), ("inf", INF)):
        for check in (False, True):
            T.append(tableau_call("aux budget %s%s" % (label, " check" if check else ""), [aux], n + 1, m_ub + 1, max_pivots=budget, check=check))
    T.append(tableau_call("limit 1024x512", [D(1023, 511, 3)], 512, 1024))
    M, N = EDGE_SHAPE
    made = dict(edge_families(oracle))
    for f in E.FAMILIES:
        if E.shapes_for(f, M, N):
            assert f in made, "edge family %s does not decompose: cell (0, 0) is not +0.0" % f
            o = E.options(f, M, N, EDGE_SEED)
            T.append(tableau_call("edge %s" % f, [made[f]], N + 1, M + 1, precision=o["precision"], max_pivots=o["max_pivots"], check=o["check_cycles"]))
    M, N = NONFINITE_SHAPE
    nf = {f: (seed, m) for f, seed, m in nonfinite_families(oracle)}
    for f in NF.FAMILIES[:6]:
        assert f in nf, "non-finite family %s does not decompose: cell (0, 0) is not +0.0" % f
        o = NF.options(f, M, N, nf[f][0])
        T.append(tableau_call("nonfinite %s" % f, [nf[f][1]], N + 1, M + 1, precision=o["precision"], max_pivots=o["max_pivots"], check=o["check_cycles"]))
    T.append(tableau_call("cycled by budget", [D(30, 29, 3), D(30, 29, 4)], 30, 31, max_pivots=3.0))
    T.append(hist_call(oracle))
    T.append(random_call("queue", QUEUE_LPS, 4, 4, 0, maximize=True))
    for seed in N7_SEEDS:
        m = NF.make("N7", M, N, seed, dense_lp=D)
        o = NF.options("N7", M, N, seed)
        T.append(tableau_call("nonfinite N7 s%d" % seed, [m], N + 1, M + 1, precision=o["precision"], max_pivots=o["max_pivots"], check=o["check_cycles"]))
    T += [precision_call(n, m, p) for n, m in PRECISION_SHAPES for p in RD.PRECISIONS]
    T += ending_calls()
    assert [c.name for c in T] == names()
    return T


def public_calls():
    """Finite data in three shapes for linprog_batch next to solve(): both kinds of rows, inequalities only (class 2),
    equalities only."""
    rng = np.random.default_rng(20261020)
    dense = [(rng.random(80), rng.random((96, 80)), 5.0 + rng.random(96), None, None) for _ in range(3)]
    return [random_call("both kinds of rows", 8, 5, 4, 3), Call("inequalities only 96x80", dense, maximize=True),
            random_call("equalities only", 6, 9, 0, 4, maximize=True)]


# ------------------------------------------------------------------------------------------------ the children

def _device_operands(torch, call):
    from yalps_amd import tensors
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    return ops, tuple(tensors._strides(t, True, k in (1, 3)) for k, t in enumerate(ops))


def run_call(torch, handle, call):
    """One Call through LpDense.solve with kept tableaux: everything it left behind, as numpy arrays."""
    B, n = len(call.lps), call.n
    ops, operands = _device_operands(torch, call)
    x = torch.full((B, n), -7.0, dtype=torch.float64, device="cuda")
    objective = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    pivots = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    ptr = lambda t: t.data_ptr() if t.numel() else None
    handle.solve(B, n, call.m_ub, call.m_eq, operands, maximize=call.maximize, precision=call.precision, max_pivots=call.max_pivots,
                 check_cycles=call.check, keep_tableaux=True, x=ptr(x), objective=ptr(objective), status=ptr(status), pivots=ptr(pivots))
    sols = [handle.solution(i) for i in range(B)]
    info = handle.info()
    after = [None if t is None else t.cpu().numpy() for t in ops]
    unchanged = all(a is None or a.tobytes() == b.tobytes() for a, b in zip(after, call.stacked()))
    return dict(x=x.cpu().numpy(), objective=objective.cpu().numpy(), status=status.cpu().numpy(), pivots=pivots.cpu().numpy(),
                col0=np.stack([s[0] for s in sols]), pos=np.stack([s[1] for s in sols]), var=np.stack([s[2] for s in sols]),
                tableau=np.stack([handle.tableau(i) for i in range(B)]), launches=np.int64(info["launches"]),
                reruns=np.int64(info["reruns"]), kernels=np.array(" ".join(k["kernel"] for k in info["kernels"])),
                classes=np.array([k["class"] for k in info["kernels"]], np.int64), aux=np.array([k["aux"] for k in info["kernels"]], np.int64),
                grids=np.array([k["grid"] for k in info["kernels"]], np.int64), unchanged=np.bool_(unchanged))


def answer(out):
    """A LinprogBatch as numpy arrays."""
    return dict(x=out.x.cpu().numpy(), objective=out.objective.cpu().numpy(), status=out.status.cpu().numpy(), pivots=out.pivots.cpu().numpy())


def strided_inputs():
    """The LPs of the strides test: B = 6, n = 5, m_ub = 4, m_eq = 2; A_ub and b_eq shared by the batch."""
    rng = np.random.default_rng(20261021)
    B, n, m_ub, m_eq = 6, 5, 4, 2
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    return dict(c=ints(-2, 5, B, n), A_ub=ints(0, 4, m_ub, n), b_ub=ints(1, 9, B, m_ub), A_eq=ints(0, 3, B, m_eq, n), b_eq=ints(1, 4, m_eq))


def offset_inputs():
    """The LPs of the second views test: B = 5, n = 6, m_ub = 3; c and b_ub are one row each, expanded over the batch (a batch
    stride of 0 in a batched tensor), A_ub lies inside a wider tensor behind a storage offset."""
    rng = np.random.default_rng(20261023)
    ints = lambda lo, hi, *shape: rng.integers(lo, hi, shape).astype(np.float64)
    return dict(c=ints(1, 6, 6), A_ub=ints(0, 4, 5, 3, 6), b_ub=ints(1, 9, 3))


def offset_call(inputs):
    return Call("offset views", [(inputs["c"], inputs["A_ub"][i], inputs["b_ub"], None, None) for i in range(inputs["A_ub"].shape[0])], maximize=True)


def strided_call(inputs):
    """strided_inputs() as the Call the oracle answers: every LP with its own copy of the shared operands."""
    B = inputs["c"].shape[0]
    return Call("strides", [(inputs["c"][i], inputs["A_ub"], inputs["b_ub"][i], inputs["A_eq"][i], inputs["b_eq"]) for i in range(B)])


def stream_inputs():
    rng = np.random.default_rng(20261022)
    return dict(c=rng.integers(1, 5, (5, 7)).astype(np.float64), A_half=rng.integers(0, 4, (5, 6, 7)).astype(np.float64),
                b_ub=rng.integers(2, 9, (5, 6)).astype(np.float64))


def plumbing(torch, out):
    """The calls through linprog_batch; what each left behind goes into `out` under "<test>/<key>"."""
    from yalps_amd import _native as nat
    from yalps_amd import tensors
    dev = lambda a: torch.from_numpy(a).cuda()

    def put(tag, d):
        out.update({"%s/%s" % (tag, k): v for k, v in d.items()})

    # views: A_ub shared and transposed, A_eq batched and transposed, c and b_ub every other element of wider tensors
    inp = strided_inputs()
    B, n = inp["c"].shape
    c_wide, b_wide = torch.full((B, 2 * n), -9.0, dtype=torch.float64, device="cuda"), torch.full((B, 8), -9.0, dtype=torch.float64, device="cuda")
    c_wide[:, ::2], b_wide[:, ::2] = dev(inp["c"]), dev(inp["b_ub"])
    A_ub_t = dev(np.ascontiguousarray(inp["A_ub"].T))            # [n, m]: .t() is A_ub with strides (1, m)
    A_eq_t = dev(np.ascontiguousarray(inp["A_eq"].transpose(0, 2, 1)))
    b_eq = dev(inp["b_eq"])
    held = [c_wide, b_wide, A_ub_t, A_eq_t, b_eq]
    before = [t.cpu().numpy().copy() for t in held]
    views = (c_wide[:, ::2], A_ub_t.t(), b_wide[:, ::2], A_eq_t.transpose(1, 2), b_eq)
    assert not views[0].is_contiguous() and not views[1].is_contiguous() and not views[3].is_contiguous() and views[1].stride() == (1, 4)
    put("views", answer(tensors.linprog_batch(*views)))
    out["views/unchanged"] = np.bool_(all(a.tobytes() == t.cpu().numpy().tobytes() for a, t in zip(before, held)))
    call = strided_call(inp)
    put("contiguous", answer(tensors.linprog_batch(*[dev(a) for a in call.stacked()])))

    # views again: c and b_ub expanded over the batch (stride 0), A_ub behind a storage offset inside a wider tensor
    inp = offset_inputs()
    B, m, n = inp["A_ub"].shape
    A_wide = torch.full((B, m + 1, n + 2), -9.0, dtype=torch.float64, device="cuda")
    A_wide[:, 1:, 2:] = dev(inp["A_ub"])
    c_row, b_row = dev(inp["c"]), dev(inp["b_ub"])
    held = [A_wide, c_row, b_row]
    before = [t.cpu().numpy().copy() for t in held]
    views = (c_row.expand(B, n), A_wide[:, 1:, 2:], b_row.expand(B, m))
    assert views[0].stride() == (0, 1) and views[2].stride() == (0, 1) and views[1].storage_offset() == (n + 2) + 2 and not views[1].is_contiguous()
    put("offset views", answer(tensors.linprog_batch(*views, maximize=True)))
    out["offset views/unchanged"] = np.bool_(all(a.tobytes() == t.cpu().numpy().tobytes() for a, t in zip(before, held)))
    put("offset contiguous", answer(tensors.linprog_batch(*[dev(a) for a in offset_call(inp).stacked()[:3]], maximize=True)))
    default_handles = len(tensors._handles)

    # the producer of A_ub on a side stream, directly before the call on that stream; then another shape on the same handle
    inp = stream_inputs()
    side = torch.cuda.Stream()
    half, c, b = dev(inp["A_half"]), dev(inp["c"]), dev(inp["b_ub"])
    torch.cuda.synchronize()
    stats = {}
    with torch.cuda.stream(side):
        big = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        for _ in range(4):
            big = big @ big * 2.0 ** -11  # (work in front of the producer: every entry stays 1.0)
        A = half * 2.0 + big[:6, :7] - 1.0
        first = tensors.linprog_batch(c, A, b, maximize=True, stats=stats)
        handles_mid = len(tensors._handles)
        second = tensors.linprog_batch(c[0, :3], A[:, :2, :3], b[:, :2], maximize=True)
        handles_end = len(tensors._handles)
    put("stream", answer(first))
    put("stream2", answer(second))
    out["stream/A"] = A.cpu().numpy()
    out["stream/handles"] = np.array([default_handles, handles_mid, handles_end], np.int64)
    out["stream/kernels"] = np.array(" ".join(k["kernel"] for k in stats["kernels"]))
    del side

    # B = 0
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    stats = {}
    empty = tensors.linprog_batch(z(0, 3), z(0, 2, 3), z(0, 2), stats=stats)
    out["empty/shapes"] = np.array([*empty.x.shape, *empty.objective.shape, *empty.status.shape, *empty.pivots.shape], np.int64)
    out["empty/dtypes"] = np.array(" ".join(str(t.dtype) for t in empty))
    out["empty/launches"] = np.int64(stats["launches"])

    # refusals: a host pointer for one operand, pageable and pinned; nothing is launched, and the handle still works afterwards
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    call = random_call("refusal", 3, 2, 2, 0)
    ops, operands = _device_operands(torch, call)
    x = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    host = np.zeros((3, 2))
    pinned = torch.zeros((3, 2), dtype=torch.float64).pin_memory()
    messages = []
    for k, (name, p) in enumerate((("c", host.ctypes.data), ("b_ub", pinned.data_ptr()), ("x_out", host.ctypes.data))):
        bad = list(operands)
        if name == "c":
            bad[0] = (p, 2, 1, 0)
        elif name == "b_ub":
            bad[2] = (p, 2, 1, 0)
        try:
            handle.solve(3, 2, 2, 0, bad, x=p if name == "x_out" else x.data_ptr())
            messages.append("no error")
        except nat.NativeError as e:
            messages.append(str(e))
        messages[-1] += " || launches=%d" % handle.info()["launches"]
    out["refusal/messages"] = np.array(messages)
    out["refusal/x_untouched"] = np.bool_(bool((x == -7.0).all().item()))
    put("refusal/after", run_call(torch, handle, call))
    handle.close()


def child_table(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import _native as nat
    out = {}
    handle = nat.LpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    try:
        for call in table(_oracle.load()):
            out.update({"%s/%s" % (call.name, k): v for k, v in run_call(torch, handle, call).items()})
    finally:
        handle.close()
    plumbing(torch, out)
    np.savez(path, **out)


def child_hist(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import os
    assert os.environ.get("YALPS_LPDENSE_HIST") == str(HIST)
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import tensors
    call = hist_call(_oracle.load())
    stats = {}
    ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
    got = tensors.linprog_batch(*ops, maximize=call.maximize, check_cycles=True, stats=stats)
    out = answer(got)
    out.update(reruns=np.int64(stats["reruns"]), launches=np.int64(stats["launches"]),
               passes=np.int64(1 + max(k["pass"] for k in stats["kernels"])))
    np.savez(path, **out)


def child_public(path):
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from yalps_amd import tensors
    from yalps_amd.solve import solve
    out = {}
    for call in public_calls():
        ops = [None if a is None else torch.from_numpy(a).cuda() for a in call.stacked()]
        got = tensors.linprog_batch(*ops, maximize=call.maximize)
        out.update({"%s/%s" % (call.name, k): v for k, v in answer(got).items()})
        sols = [ND.model_solution(solve(ND.equivalent_model(*lp, maximize=call.maximize), {"includeZeroVariables": True}), call.n)
                for lp in call.lps]
        out["%s/solve_status" % call.name] = np.array([STATUS.index(s[0]) for s in sols], np.int32)
        out["%s/solve_x" % call.name] = np.stack([s[1] for s in sols])
        out["%s/solve_result" % call.name] = np.array([s[2] for s in sols], np.float64)
    np.savez(path, **out)


if __name__ == "__main__":
    {"table": child_table, "hist": child_hist, "public": child_public}[sys.argv[1]](sys.argv[2])

"""Helpers of tests/test_sensitivity_exact.py (TEST INFRASTRUCTURE): what sensitivity_many returns, from the textbook definitions
in exact rational arithmetic (fractions.Fraction, every float taken exactly).  Shares no code with yalps_amd/sensitivity.py or
tests/_np_sensitivity.py, and never looks at a tableau's rows: it works from the model's own terms.

  sides      every finite side of every merged constraint [l, u] is one equation of the standard form,
               a.x + s = u  (an upper side)        a.x - t = l  (a lower side)        x, s, t >= 0
             maximise c'.x with c' = c for "maximize" and -c for "minimize" (the maximise sense)
  basis      the one the C oracle's solve ended on, read from its final permutations: tableau variable j is column j of the
             model, tableau variable width + r the s or t of the side that tableau row r stands for
  solve      B^-1 by Gauss-Jordan over Fractions; x_B = B^-1 b, y = c'_B B^-1, for non-basic q: T_q = B^-1 A_q, d_q = y.A_q - c'_q
  dual       of a constraint: sign * y_i of whichever of its sides is non-basic (0 if neither): d(optimal c.x) / d(bound)
  ranges     of a side: bound + delta over the delta with x_B + delta * B^-1 e_i >= 0, the other side held fixed
  variables  non-basic j: reduced cost -sign * d_j, c'_j may rise by d_j and fall without limit; basic in position k: c'_j + delta
             over the delta with d_q + delta * T_q[k] >= 0 for every non-basic q; both as intervals of the MODEL's coefficient

self_check() then asks of every end of every range, in exact arithmetic and without a solver, whether the basis is primal
and dual feasible there -- and that it is not a little beyond."""
import math
from fractions import Fraction

from tests import _np_sensitivity as NS

INF = math.inf
ZERO, ONE = Fraction(0), Fraction(1)


def frac(x):
    return Fraction(float(x))


def invert(B):
    """B^-1 of a square matrix of Fractions (lists of rows) by Gauss-Jordan elimination; a singular B is an AssertionError."""
    m = len(B)
    rows = [list(r) + [ONE if i == j else ZERO for j in range(m)] for i, r in enumerate(B)]
    for c in range(m):
        piv = next((r for r in range(c, m) if rows[r][c] != 0), None)
        assert piv is not None, "the basis matrix is singular"
        rows[c], rows[piv] = rows[piv], rows[c]
        prow = rows[c]
        inv = ONE / prow[c]
        if inv != 1:
            prow[:] = [v * inv if v else v for v in prow]
        nz = [k for k, v in enumerate(prow) if v]
        for r in range(m):
            f = rows[r][c]
            if r != c and f:
                row = rows[r]
                for k in nz:
                    row[k] -= f * prow[k]
    return [r[m:] for r in rows]


class Exact:
    """The exact analysis of one model at the oracle's final basis.  status is the oracle's; everything else is present only
    where it is "optimal"."""

    def __init__(self, oracle, model, options=None):
        from yalps_amd.model import entries, tableau_model_with_bounds
        from yalps_amd.solve import _DEFAULTS
        tabmod, info = tableau_model_with_bounds(model, sparse=True)
        opt = dict(_DEFAULTS)
        if options:
            opt.update({k: v for k, v in options.items() if v is not None})
        t = tabmod.tableau
        self.status, self.result, _ = NS.oracle_one(oracle, t, opt)
        if self.status != "optimal":
            return
        w, h = t.width, t.height
        pos = [int(p) for p in t.position_of_variable]
        self.sign = sign = -1 if model.get("direction") == "minimize" else 1
        objective = model.get("objective")
        # ---- the model's own terms
        self.sides = []  # (constraint key, "upper" | "lower", bound, tableau row)
        self.keys = list(info["bounds"])
        for key, b in info["bounds"].items():
            row = b["row"]
            if math.isfinite(b["upper"]):
                self.sides.append((key, "upper", frac(b["upper"]), row))
                row += 1
            if math.isfinite(b["lower"]):
                self.sides.append((key, "lower", frac(b["lower"]), row))
        m = self.m = len(self.sides)
        assert m == h - 1, (m, h)
        rows_of = {}
        for i, (key, _, _, _) in enumerate(self.sides):
            rows_of.setdefault(key, []).append(i)
        self.columns = []  # (variable key, {side: coefficient}, c' in the maximise sense)
        for key, coefs in entries(model.get("variables", {})):
            last = {}
            for ckey, coef in entries(coefs):
                last[ckey] = frac(coef)  # (a later duplicate overwrites an earlier one)
            col = {i: v for ckey, v in last.items() for i in rows_of.get(ckey, ()) if v != 0}
            cost = sign * last[objective] if objective is not None and objective in last else ZERO
            self.columns.append((key, col, cost))
        n = self.n = len(self.columns)
        assert n == w - 1
        self.b = [bound for _, _, bound, _ in self.sides]
        # ---- the basis: standard-form variable v < n is column v + 1 of the model, n + i the slack of side i
        tab_var = [j + 1 for j in range(n)] + [w + row for _, _, _, row in self.sides]
        assert sorted(tab_var) == list(range(1, w)) + list(range(w + 1, w + h))
        self.basic_at = {}  # position k (tableau row k + 1) -> standard-form variable
        self.position = {}  # standard-form variable -> position, for the basic ones
        for v, tv in enumerate(tab_var):
            if pos[tv] >= w:
                k = pos[tv] - w - 1
                assert 0 <= k < m and k not in self.basic_at
                self.basic_at[k], self.position[v] = v, k
        assert len(self.basic_at) == m, "the final permutations do not name a basis"
        self.nonbasic = [v for v in range(n + m) if v not in self.position]
        B = [[ZERO] * m for _ in range(m)]
        for k, v in self.basic_at.items():
            for i, a in self.column(v).items():
                B[i][k] = a
        self.Binv = Binv = invert(B)
        self.xB = [sum((Binv[k][i] * self.b[i] for i in range(m) if Binv[k][i]), ZERO) for k in range(m)]
        cB = [self.cost(self.basic_at[k]) for k in range(m)]
        self.y = [sum((cB[k] * Binv[k][i] for k in range(m) if cB[k] and Binv[k][i]), ZERO) for i in range(m)]
        self.T, self.d = {}, {}
        for q in self.nonbasic:
            col = self.column(q)
            self.T[q] = [sum((Binv[k][i] * a for i, a in col.items() if Binv[k][i]), ZERO) for k in range(m)]
            self.d[q] = sum((self.y[i] * a for i, a in col.items()), ZERO) - self.cost(q)
        self.ignore_below = ZERO
        self.sensitivity = self._sensitivity()

    def column(self, v):
        if v < self.n:
            return self.columns[v][1]
        i = v - self.n
        return {i: ONE if self.sides[i][1] == "upper" else -ONE}

    def cost(self, v):
        return self.columns[v][2] if v < self.n else ZERO

    def smallest_entry(self):
        """The smallest magnitude among the nonzero entries of B^-1 and B^-1 N (the kernel ignores |entry| <= precision)."""
        values = [abs(v) for row in self.Binv for v in row if v] + [abs(v) for col in self.T.values() for v in col if v]
        return min(values) if values else None

    def sensitivity_ignoring(self, threshold):
        """The sensitivity with every entry of B^-1 and B^-1 N below `threshold` in magnitude taken as 0 in the ratio tests."""
        self.ignore_below = Fraction(threshold)
        try:
            return self._sensitivity()
        finally:
            self.ignore_below = ZERO

    # ---- the definitions

    def side_interval(self, i):
        """(low, high) of side i's bound over which x_B + delta * B^-1 e_i >= 0; None for an infinite end."""
        lo = hi = None
        for k in range(self.m):
            t = self.Binv[k][i]
            if abs(t) < self.ignore_below:
                continue
            if t > 0:
                lo = -self.xB[k] / t if lo is None else max(lo, -self.xB[k] / t)
            elif t < 0:
                hi = self.xB[k] / -t if hi is None else min(hi, self.xB[k] / -t)
        bound = self.b[i]
        return (None if lo is None else bound + lo, None if hi is None else bound + hi)

    def cost_interval(self, j):
        """(low, high) of c'_j, the maximise-sense coefficient of column j, over which every reduced cost keeps its sign."""
        cost = self.cost(j)
        if j not in self.position:
            return None, cost + self.d[j]
        k, lo, hi = self.position[j], None, None
        for q in self.nonbasic:
            t = self.T[q][k]
            if abs(t) < self.ignore_below:
                continue
            if t > 0:
                lo = -self.d[q] / t if lo is None else max(lo, -self.d[q] / t)
            elif t < 0:
                hi = self.d[q] / -t if hi is None else min(hi, self.d[q] / -t)
        return (None if lo is None else cost + lo, None if hi is None else cost + hi)

    def _sensitivity(self):
        s, n = self.sign, self.n
        by_key = {}
        for i, (key, kind, _, _) in enumerate(self.sides):
            by_key.setdefault(key, {})[kind] = i
        constraints = []
        for key in self.keys:
            mine = by_key.get(key, {})
            loose = [i for i in mine.values() if n + i not in self.position]
            assert len(loose) <= 1, (key, "both sides non-basic")
            entry = {"dual": s * self.y[loose[0]] if loose else ZERO}
            for kind, name in (("upper", "upper_range"), ("lower", "lower_range")):
                if kind in mine:
                    lo, hi = self.side_interval(mine[kind])
                    entry[name] = (-INF if lo is None else lo, INF if hi is None else hi)
            constraints.append((key, entry))
        variables = []
        for j, (key, _, _) in enumerate(self.columns):
            lo, hi = self.cost_interval(j)
            if s < 0:
                lo, hi = (None if hi is None else -hi), (None if lo is None else -lo)
            reduced = ZERO if j in self.position else -s * self.d[j]
            variables.append((key, {"reduced_cost": reduced, "objective_range": (-INF if lo is None else lo, INF if hi is None else hi)}))
        return {"constraints": constraints, "variables": variables}

    # ---- the reference checks itself

    def feasible(self, side=None, bound=None, column=None, coefficient=None):
        """Whether the basis is primal and dual feasible with side `side` at `bound`, or with the MODEL's objective coefficient
        of column `column` at `coefficient`; everything else as the model has it."""
        xB, d = self.xB, self.d
        if side is not None:
            delta = bound - self.b[side]
            xB = [x + delta * self.Binv[k][side] for k, x in enumerate(xB)]
        if column is not None:
            delta = self.sign * coefficient - self.cost(column)
            if column in self.position:
                k = self.position[column]
                d = {q: v + delta * self.T[q][k] for q, v in d.items()}
            else:
                d = dict(d)
                d[column] -= delta
        return all(x >= 0 for x in xB) and all(v >= 0 for v in d.values())

    def self_check(self):
        """Both ends and the midpoint of every finite range are feasible, (1 + |end|) / 1024 beyond a finite end is not, an
        infinite end stays feasible 1, 2^10 and 2^20 away.  Returns the number of points looked at."""
        assert self.feasible(), "the oracle's final basis is not primal and dual feasible in exact arithmetic"
        points = 0

        def walk(lo, hi, at, ask, what):
            nonlocal points
            assert (lo == -INF or lo <= at) and (hi == INF or at <= hi), (what, lo, at, hi)
            for end, away in ((lo, -1), (hi, 1)):
                if end in (-INF, INF):
                    for dist in (1, 2 ** 10, 2 ** 20):
                        assert ask(at + away * dist), (what, "infinite end", away * dist)
                        points += 1
                else:
                    assert ask(end), (what, "end", float(end))
                    assert not ask(end + away * (1 + abs(end)) / 1024), (what, "beyond", float(end))
                    points += 2
            if lo != -INF and hi != INF:
                assert ask((lo + hi) / 2), (what, "midpoint")
                points += 1

        by_side = {(key, kind): i for i, (key, kind, _, _) in enumerate(self.sides)}
        for key, entry in self.sensitivity["constraints"]:
            for kind, name in (("upper", "upper_range"), ("lower", "lower_range")):
                assert (name in entry) == ((key, kind) in by_side), (key, name)
                if name in entry:
                    i = by_side[(key, kind)]
                    walk(*entry[name], self.b[i], lambda v, i=i: self.feasible(side=i, bound=v), (key, name))
        for j, (key, entry) in enumerate(self.sensitivity["variables"]):
            walk(*entry["objective_range"], self.sign * self.cost(j), lambda v, j=j: self.feasible(column=j, coefficient=v),
                 (key, "objective_range"))
        return points


# ---------------------------------------------------------------------------------------------- the comparison

def disagreement(got, exact):
    """|got - exact| / max(1, |got|, |exact|) of one number; infinite values must be equal as infinities (else inf)."""
    got = float(got)
    if exact in (INF, -INF) or got in (INF, -INF):
        return 0.0 if got == exact else INF
    assert not math.isnan(got)
    return float(abs(Fraction(got) - exact) / max(ONE, abs(Fraction(got)), abs(exact)))


def compare(got, exact):
    """[(disagreement, constraint or variable key, field)] of every number of a "sensitivity" value against the exact one; the
    keys, their order and the presence of upper_range / lower_range must match exactly (AssertionError)."""
    out = []
    for part, kinds in (("constraints", ("dual", "upper_range", "lower_range")), ("variables", ("reduced_cost", "objective_range"))):
        assert [k for k, _ in got[part]] == [k for k, _ in exact[part]], part
        for (key, g), (_, e) in zip(got[part], exact[part]):
            assert list(g) == list(e) and set(g) <= set(kinds), (part, key, list(g), list(e))
            for field in g:
                if field.endswith("_range"):
                    assert len(g[field]) == 2
                    out.append((disagreement(g[field][0], e[field][0]), key, field + " low"))
                    out.append((disagreement(g[field][1], e[field][1]), key, field + " high"))
                else:
                    out.append((disagreement(g[field], e[field]), key, field))
    return out

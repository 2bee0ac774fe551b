"""Model -> tableau (host side).  Restates the reference's `tableauModel`
(/root/reference/src/tableau.ts:47-137) and the Tableau layout (:9-21): it feeds the HIP core,
it is not part of the accelerated path.  Pinned by tests/test_host_model.py against the initial
tableaux the reference itself built for its 46 test models (tests/golden/simplex_cases.json.gz).

A model is a dict shaped like the reference's `Model` (src/types.ts:48-148):
  {"direction": "maximize"|"minimize", "objective": key,
   "constraints": {key: {"equal"|"min"|"max": number}} or iterable of (key, constraint),
   "variables":   {key: {constraint_key: coef}}        or iterable of (key, coefficients),
   "integers": bool | iterable of variable keys, "binaries": bool | iterable of variable keys}
"""
import math
from dataclasses import dataclass

import numpy as np


@dataclass
class Tableau:
    """src/tableau.ts:9-15.  matrix is row-major width*height float64; row 0 = objective row,
    column 0 = RHS column; the two permutations have width+height int32 entries."""
    matrix: np.ndarray
    width: int
    height: int
    position_of_variable: np.ndarray
    variable_at_position: np.ndarray
    col0: np.ndarray = None  # RHS column alone, when only that was copied back from the GPU (matrix may be None)
    cells: tuple = None  # (row, col, val) of the cells tableauModel wrote, sorted by (row, col), when the
    #                      tableau was built sparse (matrix is None until dense() or the GPU fills col0)

    def dense(self):
        """The row-major matrix of a tableau built with sparse=True."""
        if self.matrix is None:
            row, col, val = self.cells
            self.matrix = np.zeros(self.width * self.height, np.float64)
            self.matrix[row.astype(np.int64) * self.width + col] = val
        return self.matrix

    def rhs(self, row):
        """index(tableau, row, 0)"""
        return float(self.col0[row]) if self.col0 is not None else float(self.matrix[row * self.width])


@dataclass
class TableauModel:
    """src/tableau.ts:26-31"""
    tableau: Tableau
    sign: float
    variables: list  # [(key, coefficients)]
    integers: list   # 1-based column indices of integer (incl. binary) variables


def _is_array_index(key):
    """JS 'integer index' property names: canonical decimal strings 0 .. 2^32-2."""
    return isinstance(key, str) and key.isdigit() and (key == "0" or key[0] != "0") and int(key) < 4294967295


def entries(seq):
    """convertToIterable (src/tableau.ts:33-38).  A dict plays the role of a JS plain object, so
    its entries come in JS property order (Object.entries): integer-like keys ascending first, then
    the others in insertion order.  Anything else is taken as an iterable of (key, value) pairs."""
    if isinstance(seq, dict):
        idx = sorted((k for k in seq if _is_array_index(k)), key=int)
        if idx:
            rest = [k for k in seq if not _is_array_index(k)]
            return [(k, seq[k]) for k in idx + rest]
        return list(seq.items())
    return list(seq)


def _to_set(s):
    """convertToSet (src/tableau.ts:41-45): True | set"""
    if s is True:
        return True
    if s is False or s is None:
        return set()
    return s if isinstance(s, (set, frozenset)) else set(s)


def _get(constraint, name):
    v = constraint.get(name) if isinstance(constraint, dict) else getattr(constraint, name, None)
    return None if v is None else float(v)


class _Cells(dict):
    """Stand-in for the zeroed Float64Array while the model is walked: flat index -> last value written."""

    def arrays(self, width):
        idx = np.fromiter(self.keys(), np.int64, len(self))
        val = np.fromiter(self.values(), np.float64, len(self))
        order = np.argsort(idx, kind="stable")
        idx, val = idx[order], val[order]
        return (idx // width).astype(np.int32), (idx % width).astype(np.int32), val


def tableau_model(model, sparse=False):
    """src/tableau.ts:47-137, line for line in behaviour.  sparse=True keeps only the cells the
    reference writes into its zeroed matrix (Tableau.cells; for yalps_tableau_assemble)."""
    return tableau_model_with_bounds(model, sparse)[0]


def tableau_model_with_bounds(model, sparse=False):
    """(tableau_model(model, sparse), bounds_info): what tableau_model builds, and next to it what variant_patch needs to
    patch that tableau without walking the model again -- {"bounds": {constraint key: {"row", "lower", "upper"}} (the merged
    bounds with their rows), "objective": the objective key, "columns": {variable key: [its columns]}}."""
    sign = -1.0 if model.get("direction") == "minimize" else 1.0  # :51
    objective = model.get("objective")
    integers, binaries = model.get("integers"), model.get("binaries")
    constraints_iter = entries(model.get("constraints", {}))
    variables = entries(model.get("variables", {}))

    binary_constraint_col, ints = [], []  # :57-71
    if integers is not None or binaries is not None:
        binary_vars = _to_set(binaries)
        integer_vars = True if binary_vars is True else _to_set(integers)
        for i in range(1, len(variables) + 1):
            key = variables[i - 1][0]
            if binary_vars is True or key in binary_vars:
                binary_constraint_col.append(i)
                ints.append(i)
            elif integer_vars is True or key in integer_vars:
                ints.append(i)

    # :73-80 merge same-key constraints to the tightest [lower, upper]; `equal` beats min/max
    bounds = {}
    for key, constraint in constraints_iter:
        b = bounds.get(key)
        fresh = b is None
        if fresh:
            b = {"row": -1, "lower": -math.inf, "upper": math.inf}
        eq, mn, mx = _get(constraint, "equal"), _get(constraint, "min"), _get(constraint, "max")
        b["lower"] = max(b["lower"], eq if eq is not None else (mn if mn is not None else -math.inf))
        b["upper"] = min(b["upper"], eq if eq is not None else (mx if mx is not None else math.inf))
        if fresh:
            bounds[key] = b

    num_constraints = 1  # :82-86 rows in first-seen key order, upper row first then lower row
    for b in bounds.values():
        b["row"] = num_constraints
        num_constraints += (1 if math.isfinite(b["lower"]) else 0) + (1 if math.isfinite(b["upper"]) else 0)
    width = len(variables) + 1
    height = num_constraints + len(binary_constraint_col)
    num_vars = width + height
    m = _Cells() if sparse else np.zeros(width * height, np.float64)
    pos = np.arange(num_vars, dtype=np.int32)  # :95-98 identity
    var = np.arange(num_vars, dtype=np.int32)

    for c in range(1, width):  # :100-118 (a later duplicate coefficient overwrites an earlier one)
        for constraint, coef in entries(variables[c - 1][1]):
            coef = float(coef)
            if constraint == objective and objective is not None:
                m[c] = sign * coef
            b = bounds.get(constraint)
            if b is not None:
                if math.isfinite(b["upper"]):
                    m[b["row"] * width + c] = coef
                    if math.isfinite(b["lower"]):
                        m[(b["row"] + 1) * width + c] = -coef
                elif math.isfinite(b["lower"]):
                    m[b["row"] * width + c] = -coef

    for b in bounds.values():  # :120-128 RHS column
        if math.isfinite(b["upper"]):
            m[b["row"] * width] = b["upper"]
            if math.isfinite(b["lower"]):
                m[(b["row"] + 1) * width] = -b["lower"]
        elif math.isfinite(b["lower"]):
            m[b["row"] * width] = -b["lower"]

    for i, col in enumerate(binary_constraint_col):  # :130-134 x <= 1 rows for binaries
        row = num_constraints + i
        m[row * width] = 1.0
        m[row * width + col] = 1.0

    columns = {}
    for c in range(1, width):
        columns.setdefault(variables[c - 1][0], []).append(c)
    info = {"bounds": bounds, "objective": objective, "columns": columns}
    if sparse:
        return TableauModel(Tableau(None, width, height, pos, var, cells=m.arrays(width)), sign, variables, ints), info
    return TableauModel(Tableau(m, width, height, pos, var), sign, variables, ints), info


# ---- variants of one model: the same model under other bounds and coefficients (solve.solve_variants) ----
# A variant is {"constraints": {key: constraint}, "variables": {variable key: {constraint key: coef}}}, both optional.

def _merged(constraint):
    """The [lower, upper] of one constraint alone (src/tableau.ts:73-80 on a fresh entry)."""
    eq, mn, mx = _get(constraint, "equal"), _get(constraint, "min"), _get(constraint, "max")
    return (max(-math.inf, eq if eq is not None else (mn if mn is not None else -math.inf)),
            min(math.inf, eq if eq is not None else (mx if mx is not None else math.inf)))


def apply_variant(model, variant):
    """The full model a variant stands for: `model` with
      variant["constraints"][key]  in place of EVERY entry of constraint `key`, at the position of the first one;
      variant["variables"][key]    coefficients written over (or added to) those of every variable entry `key`, the
                                   objective key included -- a later coefficient overwrites an earlier one, as in tableau_model.
    A constraint key or a variable key the model does not have is a ValueError (a new variable would change the width).
    Nothing the variant leaves alone is copied: unchanged constraints and coefficient sets are the model's own objects."""
    out = dict(model)
    new_constraints = variant.get("constraints") or {}
    if new_constraints:
        cons = model.get("constraints", {})
        if isinstance(cons, dict):
            missing = [k for k in new_constraints if k not in cons]
            replaced = dict(cons)
            replaced.update(new_constraints)  # (an existing key keeps its place)
        else:
            replaced, seen = [], set()
            for key, constraint in cons:
                if key in new_constraints:
                    if key not in seen:
                        replaced.append((key, new_constraints[key]))
                    seen.add(key)
                else:
                    replaced.append((key, constraint))
            missing = [k for k in new_constraints if k not in seen]
        if missing:
            raise ValueError("apply_variant: the model has no constraint %r" % (missing[0],))
        out["constraints"] = replaced
    new_coefs = variant.get("variables") or {}
    if new_coefs:
        vars_ = model.get("variables", {})

        def patched(coefs, over):
            if isinstance(coefs, dict):
                merged = dict(coefs)
                merged.update(over)
                return merged
            return list(coefs) + entries(over)

        if isinstance(vars_, dict):
            missing = [k for k in new_coefs if k not in vars_]
            replaced = dict(vars_)
            for key in new_coefs:
                if key in vars_:
                    replaced[key] = patched(vars_[key], new_coefs[key])
        else:
            replaced, seen = [], set()
            for key, coefs in vars_:
                if key in new_coefs:
                    seen.add(key)
                    coefs = patched(coefs, new_coefs[key])
                replaced.append((key, coefs))
            missing = [k for k in new_coefs if k not in seen]
        if missing:
            raise ValueError("apply_variant: the model has no variable %r" % (missing[0],))
        out["variables"] = replaced
    return out


def variant_patch_cells(tabmod, bounds_info, variant):
    """variant_patch as one list [(flat index, value)] sorted by index (what solve_variants concatenates), or None."""
    width, sign = tabmod.tableau.width, tabmod.sign
    bounds, objective, columns = bounds_info["bounds"], bounds_info["objective"], bounds_info["columns"]
    m = {}
    replaced = {}
    for key, constraint in (variant.get("constraints") or {}).items():
        b = bounds.get(key)
        if b is None:
            raise ValueError("variant_patch: the model has no constraint %r" % (key,))
        lower, upper = _merged(constraint)
        if math.isfinite(lower) != math.isfinite(b["lower"]) or math.isfinite(upper) != math.isfinite(b["upper"]):
            return None  # other rows: the height or the row order changes
        replaced[key] = {"row": b["row"], "lower": lower, "upper": upper}
    for key, over in (variant.get("variables") or {}).items():
        cols = columns.get(key)
        if cols is None:
            raise ValueError("variant_patch: the model has no variable %r" % (key,))
        for constraint, coef in entries(over):  # src/tableau.ts:100-118 for these coefficients alone
            coef = float(coef)
            b = replaced.get(constraint) or bounds.get(constraint)
            for c in cols:
                if constraint == objective and objective is not None:
                    m[c] = sign * coef
                if b is not None:
                    if math.isfinite(b["upper"]):
                        m[b["row"] * width + c] = coef
                        if math.isfinite(b["lower"]):
                            m[(b["row"] + 1) * width + c] = -coef
                    elif math.isfinite(b["lower"]):
                        m[b["row"] * width + c] = -coef
    for b in replaced.values():  # src/tableau.ts:120-128 for the replaced bounds alone
        if math.isfinite(b["upper"]):
            m[b["row"] * width] = b["upper"]
            if math.isfinite(b["lower"]):
                m[(b["row"] + 1) * width] = -b["lower"]
        elif math.isfinite(b["lower"]):
            m[b["row"] * width] = -b["lower"]
    return sorted(m.items())


def variant_patch(tabmod, bounds_info, variant):
    """The cells in which the tableau of apply_variant(model, variant) differs from tabmod's (built from `model`, with
    bounds_info from tableau_model_with_bounds): (row, col, val) sorted strictly by (row, col), every value computed by the
    expression tableau_model uses for that cell (sign * coef, coef, -coef, upper, -lower: a lower bound of 0 is -0.0 here as
    there).  Cells the variant names are in the patch whether or not their value changes.
    None where the variant changes the tableau's STRUCTURE: a replaced constraint whose finite sides (upper finite? lower
    finite?) differ from the base's merged bound, so that rows would appear, vanish or move.  Unknown keys: ValueError."""
    cells = variant_patch_cells(tabmod, bounds_info, variant)
    if cells is None:
        return None
    width = tabmod.tableau.width
    idx = np.fromiter((k for k, _ in cells), np.int64, len(cells))
    val = np.fromiter((v for _, v in cells), np.float64, len(cells))
    return (idx // width).astype(np.int32), (idx % width).astype(np.int32), val


# src/constraint.ts:7-25
def less_eq(value):
    return {"max": value}


def greater_eq(value):
    return {"min": value}


def equal_to(value):
    return {"equal": value}


def in_range(lower, upper):
    return {"min": lower, "max": upper}

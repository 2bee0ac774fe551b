"""Helpers of tests/test_variant_shapes.py (TEST INFRASTRUCTURE): any LP of tests/_lp_batch.py's kind as a variant of a base of
its shape, so that the tables written for lp_batch_kernel (tests/_batch_shapes.py::shape_table, tests/_edges.py) run through
lp_variants_kernel as they are.

  diff_patch    the cells whose 64-bit words differ between the dense base and the dense target, with the target's words
  near_base     a target with k cells disturbed (removed, changed, added, a signed zero flipped; row 0, column 0, the last
                column and the last row among them)
  empty_base    no cells: the patch is the target's whole cell list
  packed_group  PackedVariants through flat=, optionally with junk entries in front of the patch arrays (offsets[0] > 0)
  Group         a base, its targets (each with its own precision / maxPivots / checkCycles) and the lead
  *_groups      the groups of the GPU tests: both sides of every class bound, the shape table by shape, the edge families of
                one base, the queue groups (4 x the grid's variants, heavy and empty patches in turn)
  mutant_start  the dense start tableau one of five mistakes of the kernel or its host side would produce

The expected answer of a variant is LB.oracle_answer(oracle, target): the patch takes no part in it."""
import numpy as np

from tests import _batch_shapes as BS
from tests import _edges as E
from tests import _golden as G
from tests import _lp_batch as LB
from tests import _lp_variants as V

PLUS_ZERO = 0  # the word of +0.0
MUTANTS = ("a", "b", "c", "d", "e")


# ------------------------------------------------------------------------------------------------ restatements for info()

def even(h):
    return (h + 1) & ~1


def pitch(w, h):
    """The row pitch of the image and of the tableau a variant starts from: small_lds_pitch(n) in the LDS classes,
    small_pcols(n) in the HBM form (lp_variants.hip::solve_impl)."""
    return BS.pcols(w) | 2 if LB.size_class(w, h) < 4 else BS.pcols(w)


def image_bytes(w, h):
    return 8 * (h * pitch(w, h) + even(h))


def is_aux(w, h):
    return LB.size_class(w, h) == 4 and BS.aux_hbm(w, h)


def launch_lds(w, h):
    """The dynamic LDS of a solving launch: the whole tableau block in the LDS classes, colbuf + prow in the HBM form unless
    they lie behind the tableau (aux)."""
    if LB.size_class(w, h) < 4:
        b = LB.lds_bytes(w, h)
    else:
        b = 0 if is_aux(w, h) else 8 * (BS.pcols(w) + h)
    return max((b + 15) & ~15, 16)


def lanes(w, h):
    return V.KERNEL_LANES[LB.size_class(w, h)]


# ------------------------------------------------------------------------------------------------ base + patch

def options_of(lp):
    return lp[5], lp[6], lp[7]


def with_options(lp, precision=None, max_pivots=None, check_cycles=None):
    p, m, c = options_of(lp)
    return (*lp[:5], p if precision is None else precision, float(m if max_pivots is None else max_pivots),
            bool(c if check_cycles is None else check_cycles))


def words(a):
    return np.ascontiguousarray(a).view(np.int64)


def diff_patch(base_lp, target_lp):
    """(row, col, val), int32 / int32 / float64, strictly increasing by (row, col): every cell whose word differs between the
    dense base and the dense target, with the target's word (an explicit +0.0 where the base has something else)."""
    w, h = target_lp[:2]
    assert (w, h) == tuple(base_lp[:2])
    b, t = LB.scatter(base_lp), LB.scatter(target_lp)
    idx = np.flatnonzero(words(b) != words(t))
    return (idx // w).astype(np.int32), (idx % w).astype(np.int32), np.ascontiguousarray(t[idx])


def overwrite(m, w, patch):
    row, col, val = patch
    m[row.astype(np.int64) * w + col] = val
    return m


KINDS = ("removed", "changed", "added", "zero flipped", "row 0", "column 0", "last column", "last row")


def kinds_between(base_lp, target_lp):
    """Which of KINDS the cells that differ between a base and a target are (as near_base names them)."""
    w, h = target_lp[:2]
    b, t = LB.scatter(base_lp), LB.scatter(target_lp)
    idx = np.flatnonzero(words(b) != words(t))
    bv, tv, r, c = b[idx], t[idx], idx // w, idx % w
    tz, bz = words(tv) == PLUS_ZERO, words(bv) == PLUS_ZERO
    flags = {"removed": (tv != 0) & bz, "changed": (tv != 0) & (bv != 0), "added": tz & (bv != 0), "zero flipped": (tv == 0) & (bv == 0),
             "row 0": r == 0, "column 0": c == 0, "last column": c == w - 1, "last row": r == h - 1}
    return {k for k, f in flags.items() if f.any()}


def near_base(target_lp, rng, k=48):
    """The target with min(k, w * h) cells disturbed: at least one of every kind of KINDS the shape and the target's values
    admit (a removed cell needs a non-zero cell, an added one a +0.0, a flip a zero of either sign).  The bytes depend on the
    target and on the generator's state alone."""
    w, h = target_lp[:2]
    t = LB.scatter(target_lp)
    b = t.copy()
    size = w * h
    k = min(k, size)
    chosen = set()

    def pick(cands):
        cands = np.setdiff1d(cands, np.fromiter(chosen, np.int64, len(chosen)))
        return None if cands.size == 0 or len(chosen) >= k else int(cands[int(rng.integers(cands.size))])

    def disturb(i, how=None):
        v = t[i]
        if how is None:
            how = ("removed", "changed")[int(rng.integers(2))] if v != 0 else ("added", "zero flipped")[int(rng.integers(2))]
        if how == "removed":
            b[i] = 0.0
        elif how == "changed":
            b[i] = v * 1.5 + 0.25 if v != -0.5 else 0.75
        elif how == "added":
            b[i] = 0.25 + rng.random()
        else:
            b[i] = -0.0 if words(t[i:i + 1])[0] == PLUS_ZERO else 0.0
        assert words(b[i:i + 1])[0] != words(t[i:i + 1])[0]
        chosen.add(i)

    everywhere = np.arange(size, dtype=np.int64)
    nonzero, zero = np.flatnonzero(t != 0), np.flatnonzero(t == 0)
    plus_zero = np.flatnonzero(words(t) == PLUS_ZERO)
    minus_zero = np.setdiff1d(zero, plus_zero)
    for how, cands in (("removed", nonzero), ("changed", nonzero), ("added", plus_zero), ("zero flipped", minus_zero),
                       ("zero flipped", plus_zero)):
        i = pick(cands)
        if i is not None:
            disturb(i, how)
    for cands in (everywhere[:w], everywhere[::w], everywhere[w - 1::w], everywhere[size - w:]):
        i = pick(cands)
        if i is not None:
            disturb(i)
    while len(chosen) < k:
        disturb(pick(everywhere))
    return LB.from_dense(b, w, h, *options_of(target_lp))


def empty_base(w, h):
    z = lambda dt: np.zeros(0, dt)
    return (w, h, z(np.int32), z(np.int32), z(np.float64), 1e-8, 8192.0, False)


def junk(w, h, lead):
    """`lead` entries nothing may read: rows / cols outside the tableau and, among the cells inside it, an unsorted run
    (the last cell, the middle one, cell (0, 0)); values that no tableau here holds."""
    cells = [(h, 0), (0, w), (-1, -1), (h - 1, w - 1), (h // 2, w // 2), (0, 0), (h + 5, w + 5)]
    cells = [cells[j % len(cells)] for j in range(lead)]
    return (np.array([r for r, _ in cells], np.int32), np.array([c for _, c in cells], np.int32),
            np.array([-7.5e5 - j for j in range(lead)], np.float64))


def packed_group(nat, base_lp, targets, lead=0, patches=None):
    """PackedVariants of a base and the LPs it is to become, patches by diff_patch, options the targets' own.  lead > 0:
    junk(w, h, lead) in front of the patch arrays and offsets[0] = lead."""
    w, h = base_lp[:2]
    patches = [diff_patch(base_lp, t) for t in targets] if patches is None else patches
    off = np.full(len(targets) + 1, lead, np.int64)
    off[1:] += np.cumsum([p[0].size for p in patches], dtype=np.int64)
    front = junk(w, h, lead)
    flat = (off, *(np.concatenate([front[j]] + [p[j] for p in patches]) for j in range(3)))
    return nat.PackedVariants(w, h, *base_lp[2:5], targets, [options_of(t) for t in targets], flat=flat)


class Group:
    """One call: a base, the targets its variants stand for (labels alongside), the lead of its patch arrays."""

    def __init__(self, name, base, targets, labels=None, lead=0):
        self.name, self.base, self.targets, self.lead = name, base, list(targets), lead
        self.labels = list(labels) if labels is not None else ["%d" % i for i in range(len(self.targets))]
        self.w, self.h = base[:2]
        assert all(tuple(t[:2]) == (self.w, self.h) for t in self.targets) and len(self.labels) == len(self.targets), name
        self.cls, self.aux = LB.size_class(self.w, self.h), is_aux(self.w, self.h)
        self._patches = None

    @property
    def patches(self):
        if self._patches is None:
            self._patches = [diff_patch(self.base, t) for t in self.targets]
        return self._patches

    def packed(self, nat):
        return packed_group(nat, self.base, self.targets, self.lead, self.patches)

    def checks(self):
        return [bool(t[7]) for t in self.targets]

    def kernels(self):
        """{kernel spelling: the longest patch a launch of it receives}."""
        out = {}
        for t, p in zip(self.targets, self.patches):
            name = V.kernel_of(self.cls, bool(t[7]))
            out[name] = max(out.get(name, 0), p[0].size)
        return out


# ------------------------------------------------------------------------------------------------ the groups

def rng_of(*key):
    return np.random.default_rng([20261018, *[int(x) for x in key]])


def bound_shapes():
    """(k, w, h): both widths and both heights at every class bound (class k | k + 1); then an odd height in class 1, which the
    bounds reach with even heights only, and the bound of class 3 at a width whose last LDS height is odd (123 rows: the one-run
    image copy of the largest LDS shapes ends at colbuf[0] with h = 134 and in it with h = 123)."""
    out = []
    for k, w in sorted(BS.BOUND_WIDTHS.items()):
        h0 = BS.rows_under(LB.BOUNDS[k], w)
        out += [(k, ww, hh) for ww in (w, w - 1) for hh in (h0, h0 + 1)]
    return out + [(1, 67, 69), (1, 66, 69)] + [(3, ww, hh) for ww in (149, 148) for hh in (123, 124)]


def bound_targets(oracle, w, h, seed):
    """(the dense LP of the shape, the same with a right-hand side below zero: phase 1 runs, the same with another one and
    checkCycles on)."""
    dense = LB.dense_lp(oracle, h - 1, w - 1, seed)
    A = LB.scatter(dense).reshape(h, w)
    B = A.copy()
    B[1, 0], B[1, 1] = -0.5, -1.0
    C = A.copy()
    C[h - 1, 0], C[h - 1, w - 1], C[0, w - 1] = -0.25, -2.0, 0.5
    return dense, LB.from_dense(B.ravel(), w, h), LB.from_dense(C.ravel(), w, h, check_cycles=True)


def bound_group(oracle, w, h, seed=5):
    """The variants of test_class_bounds_from_both_sides: the empty patch (the base itself), the restoring patch, a right-hand
    side below zero, one with checkCycles on."""
    dense, neg, check = bound_targets(oracle, w, h, seed)
    base = near_base(dense, rng_of(1, w, h))
    return Group("bound %dx%d" % (h, w), base, [base, dense, neg, check], ["empty patch", "restoring", "rhs below zero", "checkCycles"])


def bound_groups(oracle):
    return [bound_group(oracle, w, h) for _, w, h in bound_shapes()]


def table_by_shape(shapes):
    """{(w, h): [(name, lp)]} of a shape table, in the table's order."""
    out = {}
    for name, lp in shapes:
        out.setdefault((lp[0], lp[1]), []).append((name, lp))
    return out


LEAD = 7
LEAD_GROUPS = ("table 301x280", "empty base 47x47")  # (Group.name of the two groups with offsets[0] = LEAD)


def table_groups(shapes):
    """One group per shape of the shape table: near_base of the first target, every target of the shape as a variant."""
    out = []
    for (w, h), rows in table_by_shape(shapes).items():
        name = "table %dx%d" % (h, w)
        out.append(Group(name, near_base(rows[0][1], rng_of(2, w, h)), [lp for _, lp in rows], [n for n, _ in rows],
                         lead=LEAD if name in LEAD_GROUPS else 0))
    return out


def empty_base_groups(oracle, shapes):
    """A base without cells under at most three targets: the class-0 and class-3 shapes at their bounds, 280 x 301 (HBM form)
    and 41 x 8152 (aux form, E4 and E1 among the targets).  Every kernel spelling gets a patch of the whole tableau."""
    out = []
    for k in (0, 3):
        w = BS.BOUND_WIDTHS[k]
        h = BS.rows_under(LB.BOUNDS[k], w)
        out.append((w, h, list(zip(("dense", "rhs below zero", "checkCycles"), bound_targets(oracle, w, h, 5)))))
    by_shape = table_by_shape(shapes)
    rows = by_shape[(280, 301)]
    out.append((280, 301, [next(r for r in rows if r[0] == "odd n HBM 301 x 280"), next(r for r in rows if r[1][7]),
                           next(r for r in rows if "E4" in r[0])]))
    rows = by_shape[(8152, 41)]
    out.append((8152, 41, [next(r for r in rows if "E4" in r[0]), next(r for r in rows if "E1" in r[0]),
                           next(r for r in rows if r[1][7] and r[1][6] == BS.INF)]))
    groups = []
    for w, h, rows in out:
        name = "empty base %dx%d" % (h, w)
        groups.append(Group(name, empty_base(w, h), [lp for _, lp in rows], [n for n, _ in rows], lead=LEAD if name in LEAD_GROUPS else 0))
    return groups


EDGE_SHAPES = ((30, 29), (300, 279))  # (M, N): LDS class 0 | the HBM form with an odd column count
EDGE_SEED = 1


def edge_groups(oracle):
    """Per shape every edge family as a variant of the dense LP it is planted into: the patch is the planted edge."""
    out = []
    for M, N in EDGE_SHAPES:
        families = [f for f in E.FAMILIES if E.shapes_for(f, M, N)]
        out.append(Group("edges %dx%d" % (M + 1, N + 1), LB.dense_lp(oracle, M, N, EDGE_SEED),
                         [BS.edge_lp(oracle, f, M, N, EDGE_SEED) for f in families], families))
    return out


def klee_minty_base(oracle, w, h, seed):
    """A base whose solve is long although it has w - 1 variables: the Klee-Minty cube of dimension w - 1 in the rows 1 .. w - 1
    (Dantzig's rule visits every vertex: 2^(w-1) - 1 pivots), under rows of dense-LP(h - 1, w - 1, seed) whose right-hand sides
    are 1e9: never binding, so the pivots are the cube's, and every one of them rewrites every row."""
    n = w - 1
    A = LB.scatter(LB.dense_lp(oracle, h - 1, n, seed)).reshape(h, w)
    A[1:, 0] = 1e9 + np.arange(1, h)
    A[0, 0] = 0.0
    for i in range(1, n + 1):
        A[i, 1:] = 0.0
        A[i, 1:i] = [2.0 ** (i - j + 1) for j in range(1, i)]
        A[i, i] = 1.0
        A[i, 0] = 5.0 ** i
        A[0, i] = 2.0 ** (n - i)
    return LB.from_dense(A.ravel(), w, h)


QUEUE_GRID = 256  # one workgroup per CU under YALPS_LPVAR_PER_CU=1 (the GPU test asserts the launch's grid)
QUEUE_HIST = 2    # YALPS_LPVAR_HIST of the queue test
QUEUE_SHAPES = ((9, BS.rows_under(LB.BOUNDS[3], 9) + 1), (2, 8191))  # the smallest class-4 shape of width 9 | the aux bound


def heavy_target(base_lp, rng, check, free):
    """The base with at least 1025 cells changed, rows, row 0 and column 0 among them.  free: anything may change, and a few rows
    turn into >= rows (phase 1 runs).  Otherwise the cells that decide the pivots stay: row 0 but its constant, the rows
    1 .. w - 1, and the sign and size of everything else."""
    w, h = base_lp[:2]
    A = LB.scatter(base_lp).reshape(h, w).copy()
    flat = A.reshape(-1)
    lo = 0 if free else w * w
    idx = lo + rng.choice(w * h - lo, 1100, replace=False)
    flat[idx] *= 1.0 + 0.25 * (rng.random(idx.size) - 0.5)
    A[0, 0] = 1.0 + rng.random()
    A[w + rng.choice(h - w, 40, replace=False), 0] *= 1.0 + rng.random(40)
    if free:
        A[0, 1:] *= 0.5 + rng.random(w - 1)
        r = w + rng.choice(h - w, 6, replace=False)
        A[r, 1:] *= -1.0
        A[r, 0] = -rng.random(r.size)
    return LB.from_dense(flat, w, h, check_cycles=check)


def queue_group(oracle, w, h, grid=QUEUE_GRID):
    """4 x grid variants: a heavy patch and the empty patch in turn, checkCycles alternating between the pairs.  Every second
    heavy patch is free (see heavy_target).  With more than one variable the base's solve is long (klee_minty_base), so that a
    short checkCycles history overflows pass after pass."""
    base = klee_minty_base(oracle, w, h, 3) if w > 2 else LB.dense_lp(oracle, h - 1, w - 1, 3)
    rng = rng_of(3, w, h)
    targets, labels = [], []
    for pair in range(2 * grid):
        check = bool(pair % 2)
        free = bool((pair // 2) % 2)
        targets += [heavy_target(base, rng, check, free), with_options(base, check_cycles=check)]
        labels += ["heavy%s" % (" free" if free else ""), "empty patch"]
    return Group("queue %dx%d" % (h, w), base, targets, labels)


def must_rerun(targets, refs, hist=QUEUE_HIST):
    """Per pass the variants a history of hist * 4^pass pivots per phase cannot hold: checkCycles on and more than twice that many
    pivots in all (test_history_rerun_only_for_the_variants_that_overflowed's rule).  Stops at the first empty pass."""
    out, cap = [], hist
    while True:
        ids = [i for i, (t, r) in enumerate(zip(targets, refs)) if t[7] and r["n_pivots"] > 2 * cap]
        if not ids:
            return out
        out.append(ids)
        cap *= 4


# ------------------------------------------------------------------------------------------------ wrong starts

def launch_order(group):
    """[variants] per launch of pass 0: checkCycles off, then on, each in the call's order (wg_queue_host.inc::plan_launches)."""
    return [[i for i, c in enumerate(group.checks()) if c == check] for check in (False, True)]


def mutant_start(group, i, mutant=None, grid=QUEUE_GRID):
    """The dense tableau variant i of a group starts from -- mutant None: the base with its patch over it -- or would start
    from under one of the mistakes the GPU comparison is there to catch:
      a  only the first T patch cells applied (T the lanes of the group's kernel: the patch loop takes one trip)
      b  the patch of the variant the same workgroup solved before left in place (hand-out order k, k + grid, ...)
      c  the patch read from offset 0 of the patch arrays instead of offsets[0] (cells outside the tableau are skipped)
      d  explicit +0.0 patch cells skipped: the base's value survives
      e  column-0 patch cells written as matrix cells, at r * pitch - 1: column 0 keeps the base's value, and where the pitch
         is the column count (HBM form, even n) the last column of the row above takes the patch's"""
    w, h = group.w, group.h
    m = LB.scatter(group.base)
    row, col, val = group.patches[i]
    if mutant is None:
        return overwrite(m, w, (row, col, val))
    if mutant == "a":
        T = lanes(w, h)
        return overwrite(m, w, (row[:T], col[:T], val[:T]))
    if mutant == "b":
        launch = next(L for L in launch_order(group) if i in L)
        p = launch.index(i)
        if p >= grid:
            overwrite(m, w, group.patches[launch[p - grid]])
        return overwrite(m, w, (row, col, val))
    if mutant == "c":
        lead = group.lead
        front = junk(w, h, lead)
        flat = [np.concatenate([front[j]] + [p[j] for p in group.patches]) for j in range(3)]
        lo = sum(p[0].size for p in group.patches[:i])  # (offsets[i] - offsets[0])
        r, c, v = (a[lo:lo + row.size] for a in flat)
        for rr, cc, vv in zip(r, c, v):
            if 0 <= rr < h and 0 <= cc < w:
                m[int(rr) * w + int(cc)] = vv
        return m
    if mutant == "d":
        keep = words(val) != PLUS_ZERO
        return overwrite(m, w, (row[keep], col[keep], val[keep]))
    if mutant == "e":
        body = col != 0
        overwrite(m, w, (row[body], col[body], val[body]))
        if pitch(w, h) == w - 1:
            for rr, vv in zip(row[~body], val[~body]):
                if rr >= 1:
                    m[(int(rr) - 1) * w + w - 1] = vv
        return m
    raise ValueError(mutant)


def signature(oracle, m, lp):
    """(status, pivots, result bits, digest of the final matrix) of the oracle's run from a start tableau under lp's options."""
    w, h = lp[:2]
    ref = LB.oracle_answer(oracle, LB.from_dense(m, w, h, *options_of(lp)))
    return ref["status"], ref["n_pivots"], BS.bits(ref["result"]), G.sha256(ref["matrix"])


# ------------------------------------------------------------------------------------------------ a handle on a caller's stream

STREAM_SHAPE = (47, 47)  # (w, h) of the group test_caller_stream solves


def outputs(lv, out, count):
    """Everything a solve left behind, as arrays: statuses, results, pivots, and per variant column 0, both permutations, the
    final matrix."""
    sols = [lv.solution(i) for i in range(count)]
    return dict(status=np.array(out[0]), result=np.asarray(out[1]), pivots=np.asarray(out[2]),
                col0=np.stack([s[0] for s in sols]), pos=np.stack([s[1] for s in sols]), var=np.stack([s[2] for s in sols]),
                tableau=np.stack([lv.tableau(i) for i in range(count)]))


def caller_stream_child(path):
    """The group of STREAM_SHAPE through an LpVariants on a stream torch made, its outputs to `path` (.npz).  A process of its
    own: torch brings a HIP runtime along, and a stream is only good in the runtime that made it, so torch has to be loaded
    before the library -- which the test process, long past its first library call, cannot arrange."""
    assert "libamdhip64" not in open("/proc/self/maps").read(), "a HIP runtime was loaded before torch"
    import torch
    torch.cuda.init()
    from tests import _oracle
    from yalps_amd import _native as nat
    group = bound_group(_oracle.load(), *STREAM_SHAPE)
    stream = torch.cuda.Stream()
    lv = nat.LpVariants(0, stream=stream.cuda_stream)
    try:
        out = lv.solve(group.packed(nat), keep_tableaux=True)
        np.savez(path, launches=lv.info()["launches"], **outputs(lv, out, len(group.targets)))
    finally:
        lv.close()  # (before the stream is dropped)
    del stream


if __name__ == "__main__":
    import sys
    caller_stream_child(sys.argv[1])

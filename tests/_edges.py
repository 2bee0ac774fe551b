"""Edge-case tableaux for the kernels' restatements of the reference's selection and pivot rules (TEST INFRASTRUCTURE).

Every tableau starts as dense-LP(M, N, seed) (tests/_oracle.py) and has one edge planted by fixed formulas, so that
(family, M, N, seed, layout) always gives the same bytes.  `layout` is a pair of lists: row numbers and column numbers at
which the kernels split their work (rows per workgroup, XCD interleave, shard bounds; units per lane, panels, the tail
unit of 2^k + 1 columns).  The planted candidates sit on both sides of those splits.  The rules pinned (src/simplex.ts):

  E1  entering-column ties: equal phase-2 reduced costs and equal phase-1 ratios; the first column wins (:75, :127)
  E2  leaving-row ties: three or more equal minimal ratios, the first of them past the first block (:89)
  E2b the early break: the first ratio <= precision is taken although later ratios are smaller (:92)
  E3  +inf phase-2 ratios are skipped, -inf phase-1 ratios are skipped (:89, :127)
  E3u every eligible phase-2 ratio is +inf: "unbounded" (:96)
  E3i every phase-1 ratio is -inf: "infeasible" (:133)
  E4  signed zeros: -0.0 in the right-hand sides, the objective and the pivot row (flushed to +0.0, :20); a phase-1 tie
      between the ratios -0.0 and +0.0 (equal numbers: the first column wins)
  E5  the flush band: 1e-16, one ulp either side, and their negatives, in pivot rows and the pivot column (:17, :31)
  E6a pivot entry == precision (not eligible, :86), ratio == precision (the early break, :92)
  E6b reduced cost == precision (not eligible, :74), rhs == -precision (no phase 1, :115)
  E6c phase-1 coefficient == -precision (not eligible, :126)
  E7  precision 0 / 1e-17: a pivot element inside the flush band (its row entry flushed, then 1 / q at :25)
  E8  a pivot element of 2^980 over a row scaled by 2^-40, rows scaled by 2^-50: subnormal quotients and products
      (rows scaled by 2^-1000 would fall into the flush band and never be touched), nothing overflows
  E9  small integers scaled by powers of two: ties that recur over many pivots, to the pivot budget
  E9c Chvatal's cycling LP spread across the splits, with checkCycles: hasCycle stops it (:98)

Every family keeps the run finite (tests/test_edge_records.py checks the final tableau)."""
import math

import numpy as np

FAMILIES = ("E1", "E2", "E2b", "E3", "E3u", "E3i", "E4", "E5", "E6a", "E6b", "E6c", "E7", "E8", "E9", "E9c")
# the families of the largest shapes: the ones whose edges depend on how the work is split
PARTITION_FAMILIES = ("E1", "E2", "E2b", "E3", "E4", "E5", "E8", "E9")

BAND = (1e-16, math.nextafter(1e-16, 0.0), math.nextafter(1e-16, 1.0), -1e-16, -math.nextafter(1e-16, 0.0),
        -math.nextafter(1e-16, 1.0))


def partition(height, nranks):
    """Row bounds of the row shards (yalps_amd/sharded.py)."""
    from yalps_amd import sharded
    return sharded.partition(height, nranks)


def default_layout(M, N):
    """Rows: multiples of 64 .. 8192 and the shard bounds of two and three ranks; columns: 2^k and 2^k + 1 (the tail unit),
    64 .. 16384, and the last column."""
    h, w = M + 1, N + 1
    rows = {b for k in range(6, 14) for b in (1 << k,) if b < h - 1}
    for world in (2, 3):
        rows |= {b for b in partition(h, world)[1:-1] if 1 < b < h - 1}
    cols = {c for k in range(6, 15) for c in ((1 << k), (1 << k) + 1) if c < w - 1}
    return sorted(rows), sorted(cols | {w - 1})


def _pick(seq, lo, hi, count):
    """`count` members of seq inside [lo, hi), spread from the front to the back."""
    seq = [x for x in seq if lo <= x < hi]
    if len(seq) <= count:
        return seq
    return [seq[round(i * (len(seq) - 1) / (count - 1))] for i in range(count)] if count > 1 else [seq[-1]]


def _rows(layout, h, count):
    """Tie rows: one on each side of some split, the first of them past the first split (fallback: spread rows)."""
    rows = []
    for b in _pick(layout[0][1:], 2, h - 1, count):  # (past the first split: the first of them is not in block 0)
        rows += [b, b + 1] if len(rows) < 2 * count - 1 else [b]
    rows = sorted({r for r in rows if 1 <= r < h})
    if len(rows) < count:
        rows = sorted(set(rows) | {max(1, (k * (h - 1)) // (count + 1)) for k in range(1, count + 1)})
    return rows


def _cols(layout, w, count, skip=()):
    cols = [c for c in layout[1] if c not in skip]
    cols = _pick(cols, 2, w, count)
    if len(cols) < count:
        cols = sorted(set(cols) | {c for c in range(2, w) if c not in skip} if w <= 3 * count else
                      set(cols) | {max(2, (k * (w - 1)) // (count + 1)) for k in range(1, count + 1)} - set(skip))
    return sorted(cols)[:max(count, 1)]


def options(family, M, N, seed):
    """Options of a record: the precision of the family (E7: 0 for even seeds, 1e-17 for odd ones), a pivot budget by size
    (the integer LPs may cycle), checkCycles."""
    size = (M + 1) * (N + 1)
    budget = 12.0 if size > 8_000_000 else 24.0 if size > 1_000_000 else 60.0
    precision = {"E7": 0.0 if seed % 2 == 0 else 1e-17}.get(family, 1e-8)
    return dict(precision=precision, max_pivots=budget, check_cycles=family == "E9c")


def make(family, M, N, seed, layout=None, dense_lp=None):
    """The (M+1) x (N+1) tableau of the family, flat, row-major, float64."""
    if dense_lp is None:
        from tests import _oracle
        dense_lp = _oracle.load().dense_lp
    if layout is None:
        layout = default_layout(M, N)
    h, w = M + 1, N + 1
    m = dense_lp(M, N, seed)
    A = m.reshape(h, w)
    prec = options(family, M, N, seed)["precision"]
    mid = h // 2
    if family == "E1":
        # phase 1 first: the rows P (rhs -1, copies of each other, the first of them `mid`) are negative only in the
        # columns T1 (none in the first unit), whose ratios -(-2) / -0.5 are all equal; then phase 2: the columns T2, column 1
        # and the last column among them, have the largest reduced cost 1.5; the columns of each set are copies
        t2 = sorted({1, w - 1} | set(_cols(layout, w, 3)))
        t1 = _cols(layout, w, 3, skip=t2) or [c for c in range(2, w) if c not in t2][:2]
        P = sorted({mid} | {r for r in _rows(layout, h, 3) if r > mid} | {h - 1})
        A[P] = 0.0
        A[P, 0] = -1.0
        for group, obj in ((t1, -2.0), (t2, 1.5)):
            A[:, group] = A[:, [group[0]]]
            A[0, group] = obj
        A[np.ix_(P, t1)] = -0.5
    elif family == "E2":
        # column c enters (reduced cost 2); the rows T are copies of each other with the smallest ratio 0.25 / 0.5: the first
        # just past the shard bound of two ranks, the second past the second bound of three ranks, the last row
        c = _cols(layout, w, 1)[0]
        b2, b3 = partition(h, 2)[1], partition(h, 3)[2]
        t = sorted({min(b2 + 1, h - 3), min(b3 + 1, h - 2), h - 1})
        A[0, c] = 2.0
        A[t] = A[t[0]]
        A[t, 0] = 0.25
        A[t, c] = 0.5
    elif family == "E2b":
        # column c enters; row a has ratio 4 precision (> precision), row b ratio -precision / 2 (<= precision: taken at
        # once), the later row d the smaller ratio -precision / 2 / 1e-3
        c = _cols(layout, w, 1)[0]
        r = _rows(layout, h, 3)
        while len(r) < 3:
            r.append(r[-1] + 1 if r[-1] + 1 < h else 1)
        a, b, d = sorted(set(r))[:3] if len(set(r)) >= 3 else (1, max(2, h // 2), h - 1)
        A[0, c] = 2.0
        A[a, 0], A[a, c] = 4 * prec, 1.0
        A[b, 0], A[b, c] = -prec / 2, 1.0
        A[d, 0], A[d, c] = -prec / 2, 1e-3
    elif family in ("E3", "E3u", "E3i"):
        c = _cols(layout, w, 1)[0]
        inf_rows = _rows(layout, h, 3)
        tiny = prec * (1.0 + 2.0 ** -20) if prec > 0 else 1e-8
        A[0, c] = 2.0
        if family == "E3u":
            A[1:, c] = -A[1:, c]  # no positive entry but those of the +inf rows
        for r in inf_rows:  # rhs 1e301 over an entry just above precision: the ratio overflows to +inf
            A[r] = 0.0
            A[r, 0], A[r, c] = 1e301, tiny
        if family in ("E3", "E3i"):
            # phase 1: row p (rhs -1); its candidates have ratio -(-1e301) / -tiny = -inf, except (E3) one finite column
            p = mid if mid not in inf_rows else 1
            cand = _cols(layout, w, 3, skip=[c])
            A[p] = 0.0
            A[p, 0] = -1.0
            A[p, cand] = -tiny
            A[0, cand] = -1e301
            if family == "E3":
                f = max(cand) + 1 if max(cand) + 1 < w and max(cand) + 1 != c else min(set(range(2, w)) - set(cand) - {c})
                A[p, f], A[0, f] = -0.5, 0.25
                A[inf_rows, f] = 0.0
    elif family == "E4":
        # -0.0 on a lattice (right-hand sides included), in the objective, and in the phase-1 row p, whose two candidates
        # have the ratios -(-0.0) / -0.5 = -0.0 and -(+0.0) / -0.5 = +0.0: equal, so the first column enters
        r, c = np.ogrid[:h, :w]
        A[((r + 3 * c) % 7 == 0) & (r > 0)] = -0.0
        A[0, 5::5] = -0.0
        c1, c2 = (_cols(layout, w, 2) + [w - 1, w - 1])[:2]
        if c1 == c2:
            c1 = 1
        A[mid] = np.where((np.arange(w) % 3) == 0, -0.0, 0.0)
        A[mid, 0] = -1.0
        A[mid, [c1, c2]] = -0.5
        A[0, c1], A[0, c2] = -0.0, 0.0
    elif family == "E5":
        # band values on a lattice; column c enters, pivot row q (ratio 0.25 / 0.5), band values in column c
        r, c = np.ogrid[:h, :w]
        lat = ((5 * r + 3 * c) % 13 == 0) & (r > 0) & (c > 0)
        A[lat] = np.asarray(BAND)[((r + c) % 6) * np.ones_like(lat, dtype=np.int64)][lat]
        col = _cols(layout, w, 1)[0]
        A[0, col] = 2.0
        A[1::2, col] = np.asarray(BAND)[np.arange(1, h, 2) % 6]
        q = _rows(layout, h, 2)[-1]
        A[q, 0], A[q, col] = 0.25, 0.5
        A[q, 1::4] = np.asarray(BAND)[np.arange(1, w, 4) % 6]
    elif family == "E6a":
        # column c enters; row a: entry == precision (not eligible), rhs 0 (its ratio 0 would be taken at once); row b:
        # ratio == precision (taken: ratio <= precision); row d > b: the smaller ratio precision / 2
        c = _cols(layout, w, 1)[0]
        rr = sorted(set(_rows(layout, h, 3)) | {1, h - 1})
        a, b, d = rr[0], rr[len(rr) // 2], rr[-1]
        A[0, c] = 2.0
        A[a, 0], A[a, c] = 0.0, prec
        A[b, 0], A[b, c] = prec, 1.0
        A[d, 0], A[d, c] = prec / 2, 1.0
    elif family == "E6b":
        # no reduced cost above precision, one equal to it: optimal at once; a row with rhs == -precision (no phase 1)
        A[0, 1:] = -A[0, 1:]
        A[0, _cols(layout, w, 1)[0]] = prec
        A[mid, 0] = -prec
        A[mid, 1::2] = -A[mid, 1::2]
    elif family == "E6c":
        # phase 1 on row p: column a has coefficient == -precision and the largest ratio (not eligible), column b -0.5
        a, b = (_cols(layout, w, 2) + [1, 2])[:2]
        if a == b:
            a, b = 1, 2 if w > 2 else 1
        A[mid] = np.abs(A[mid])
        A[mid, 0] = -1.0
        A[mid, a], A[0, a] = -prec, 1.0
        A[mid, b], A[0, b] = -0.5, 0.5
        A[h - 1 if mid != h - 1 else 1, 0] = -prec  # rhs == -precision: never a phase-1 row
    elif family == "E7":
        # column c enters; its only positive entry is 5e-17 (inside the flush band, above both precisions) in row q; that row's other entries
        # are 1e-17-sized (flushed) or 1e-15-sized (kept)
        c = _cols(layout, w, 1)[0]
        q = _rows(layout, h, 2)[-1]
        A[0, c] = 2.0
        A[1:, c] = -A[1:, c]
        A[q] *= np.where(np.arange(w) % 2 == 0, 1e-17, 1e-15)
        A[q, c] = 5e-17
    elif family == "E8":
        # column c enters with reduced cost 2^980; its entry in row p is 2^980 too, so p's ratio is ~0 (the early break);
        # p's other entries are scaled by 2^-40, so the pivot row p / q is 2^-1020-sized: partly subnormal; the rows S are
        # scaled by 2^-50 (coefficients still above 1e-16) and have exact zeros, which become -coef * p: subnormal products
        c = _cols(layout, w, 1)[0]
        rows = _rows(layout, h, 4)
        p, srows = rows[len(rows) // 2], [r for r in rows if r != rows[len(rows) // 2]]
        A[p, 1:] *= 2.0 ** -40
        A[p, c] = 2.0 ** 980
        A[0, c] = 2.0 ** 980
        A[srows] *= 2.0 ** -50
        A[srows, 1::3] = 0.0
        A[srows, c] = 0.75 * 2.0 ** -50
        A[1:p, c] = np.minimum(A[1:p, c], 0.5)
    elif family == "E9c":
        # Chvatal's cycling LP (the reference's test case "Chvatal Cycling") on rows and columns across the splits, in the
        # same order; the other rows are 0 in its columns, its rows 0 elsewhere, the other reduced costs <= 0: Dantzig's rule
        # with the lowest-index tie-breaks cycles with period 6, and hasCycle stops it after 11 pivots
        rows = (_rows(layout, h, 3) + [1, 2, 3])[:3] if h > 4 else [1, 2, 3]
        rows = sorted(set(rows)) if len(set(rows)) == 3 else [1, 2, 3]
        cols = _cols(layout, w, 4) if len(_cols(layout, w, 4)) == 4 else [1, 2, 3, 4]
        A[0] = -np.abs(A[0])
        A[0, 0] = 0.0
        A[:, cols] = 0.0
        A[rows] = 0.0
        A[0, cols] = (10.0, -57.0, -9.0, -24.0)
        A[np.ix_(rows, cols)] = ((0.5, -5.5, -2.5, 9.0), (0.5, -1.5, -0.5, 1.0), (1.0, 0.0, 0.0, 0.0))
        A[rows, 0] = (0.0, 0.0, 1.0)
    elif family == "E9":
        B = A.copy()
        A[:, 1:] = np.floor(B[:, 1:] * 5.0) - 1.0                       # -1 .. 3
        A[1:, 0] = np.floor(B[1:, 1] * 4.0) if w > 1 else 0.0           # 0 .. 3: many zero right-hand sides
        A[0, 0] = 0.0
        A[0, 1:] = np.floor(B[0, 1:] * 4.0) - 1.0
        A[1:] *= np.exp2((np.arange(1, h) % 3) - 1.0)[:, None]          # rows scaled by 1/2, 1, 2
    else:
        raise ValueError(family)
    return m


def shapes_for(family, M, N):
    return family in FAMILIES if (M + 1) * (N + 1) <= 8_000_000 else family in PARTITION_FAMILIES


# (M, N) of every GPU path in tests/test_edge_paths.py (each taken from the parity test that names the kernel)
# (60, 64), (1400, 8192) and (4300, 4096): rows of 2^k + 1 columns, one tail unit
SHAPES = [(60, 64), (300, 200), (600, 2500), (2800, 3300), (900, 7000), (1400, 8192), (2500, 5000), (4300, 4096), (2100, 12345),
          (300, 9000), (600, 16000), (4000, 500), (2000, 1000), (4000, 2000), (200, 20000), (200, 150), (120, 3000),
          (2300, 4200), (3300, 4200), (13000, 2100)]
SEED = 3


def specs():
    """(family, M, N, seed) of every record of tests/golden/simplex_edges.json.gz."""
    return [(f, M, N, seed) for M, N in SHAPES for i, f in enumerate(FAMILIES) if shapes_for(f, M, N)
            for seed in ((SEED, SEED + 1) if f == "E7" else (SEED + (i % 2),))]  # (E7 at precision 1e-17 and 0)


def label(rec):
    return "%s-%dx%d-s%d" % (rec["family"], rec["M"], rec["N"], rec["seed"])


def initial(rec, dense_lp=None):
    """The initial tableau of an edge record, regenerated; its bytes must be the ones the reference ran on."""
    m = make(rec["family"], rec["M"], rec["N"], rec["seed"], tuple(rec["layout"]), dense_lp)
    from tests import _golden as G
    assert G.sha256(m) == rec["init_sha256"], "initial tableau differs from the reference's"
    return m


def col0_matches(matrix, rec, exp):
    """Column 0 of a final tableau against the record: the doubles, or (large records) their SHA-256."""
    from tests import _golden as G
    col0 = np.ascontiguousarray(matrix.reshape(rec["height"], rec["width"])[:, 0])
    if exp["col0"] is None:
        return G.sha256(col0) == exp["col0_sha256"]
    return np.array_equal(col0.view(np.int64), exp["col0"].view(np.int64))

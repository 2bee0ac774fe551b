"""resident2_kernel<T, J, R> with its rows held as slot vectors (resident2_kernel.cuh): what a run-time
slot index now selects -- the candidate row, the pivot row, the published row, the entering column's vector -- on tiny
tableaux forced onto every instantiation (YALPS_HIP_RVARIANT, a few workgroups via YALPS_HIP_BLOCKS), against the CPU
oracle bit for bit: status, result, pivot count, both permutations, the whole matrix.

The seeds below were found on the CPU with the oracle; each test recomputes from the oracle's pivot sequence what its
seed is there for and asserts it, so a changed generator cannot hide a case that no longer does its job."""
import numpy as np
import pytest

from tests import _golden as G

pytestmark = pytest.mark.gpu

RESIDENT2 = [(256, 1, 4), (256, 1, 9), (256, 2, 4), (512, 2, 4), (512, 2, 6), (512, 2, 9), (512, 3, 4)]
NB = 4  # workgroups: row r lives in slot r // NB of workgroup r % NB


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    assert _native.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return _native


def dense(oracle, M, N, seed):
    return oracle.dense_lp(M, N, seed)


def sparse(oracle, M, N, seed):
    """~2 % of the constraint entries kept -- one per column on a diagonal band (every column stays bounded), the rest at
    random: every pivot row has flushed entries in every wave's slice, few rows change per pivot."""
    m = oracle.dense_lp(M, N, seed)
    A = m.reshape(M + 1, N + 1)
    keep = np.random.default_rng(seed).random((M, N)) < 0.02 - 1.0 / M
    keep[np.arange(N) % M, np.arange(N)] = True
    A[1:, 1:] *= keep
    assert 0.015 < keep.mean() < 0.025
    return m


def negative_rhs(oracle, M, N, seed):
    """Every third row "-a x <= -b": the start is infeasible, phase 1 runs first."""
    m = oracle.dense_lp(M, N, seed)
    A = m.reshape(M + 1, N + 1)
    A[1::3, 0] *= -0.05
    A[1::3, 1:] *= -1.0
    return m


def reference(oracle, m, w, h, **opts):
    ref = m.copy()
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    st, res, piv, trace = oracle.simplex(ref, w, h, pos, var, trace_cap=4096, **opts)
    return dict(status=st, result=res, pivots=piv, trace=trace, matrix=ref, pos=pos, var=var)


def solve_on(nat, monkeypatch, variant, m, w, h, chunk=None, blocks=NB, **opts):
    """The tableau through resident2_kernel<variant> on `blocks` workgroups (the switches are read when the context and
    the tableau are created)."""
    monkeypatch.setenv("YALPS_HIP_SMALL", "0")
    monkeypatch.setenv("YALPS_HIP_TAG", "0")
    monkeypatch.setenv("YALPS_HIP_RESIDENT_GEN", "2")
    monkeypatch.setenv("YALPS_HIP_RVARIANT", "%d,%d,%d" % variant)
    monkeypatch.setenv("YALPS_HIP_BLOCKS", str(blocks))
    if chunk is not None:
        monkeypatch.setenv("YALPS_HIP_RESIDENT_CHUNK", str(chunk))
    c = nat.Context(0)
    try:
        t = nat.DeviceTableau(c, w, h)
        try:
            pos = np.arange(w + h, dtype=np.int32)
            t.upload(m, h, pos, pos.copy())
            st, res, piv, _ = t.solve(**opts)
            info = t.info()
            gm, gp, gv = t.download()
        finally:
            t.close()
    finally:
        c.close()
    assert info["last_path"] == "resident" and info["resident"] == "resident2_kernel<%d,%d,%d>" % variant, info
    return dict(status=st, result=res, pivots=piv, matrix=gm, pos=gp, var=gv, info=info)


def same(got, exp):
    assert (got["status"], got["pivots"]) == (exp["status"], exp["pivots"]) and G.same_number(got["result"], exp["result"])
    assert np.array_equal(got["pos"], exp["pos"]) and np.array_equal(got["var"], exp["var"])
    assert np.array_equal(got["matrix"].view(np.int64), exp["matrix"].view(np.int64))


def general_path_pivots(oracle, m, w, h, trace):
    """Pivots of the oracle's sequence that cannot take the kernel's dense path: the pivot row has a flushed entry
    (|x| <= 1e-16, src/simplex.ts:17-24) among the real columns, or a row has one in the pivot column (:31)."""
    a = m.copy()
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    count = 0
    for row, col in trace.tolist():
        A = a.reshape(h, w)
        if (np.abs(A[row, 1:]) <= 1e-16).any() or (np.abs(A[1:, col]) <= 1e-16).any():
            count += 1
        oracle.pivot(a, w, h, pos, var, row, col)
    return count


def rows_for(R, blocks=NB):
    return blocks * R - 1  # constraint rows: h = blocks * R, every slot of every workgroup holds a row


_REF = {}


def cached_reference(oracle, kind, M, N, seed, **opts):
    """One oracle run per input, shared by the instantiations that solve it."""
    key = (kind.__name__, M, N, seed, tuple(sorted(opts.items())))
    if key not in _REF:
        m = kind(oracle, M, N, seed)
        _REF[key] = (m, reference(oracle, m, N + 1, M + 1, **opts))
    return _REF[key]


# ---- every instantiation: the dense path, the general path, phase 1 then 2 ---------------------------------------
@pytest.mark.parametrize("kind,N,seed,blocks,min_pivots", [(dense, 37, 10, NB, 10), (sparse, 301, 1, 16, 100), (negative_rhs, 37, 12, NB, 10)],
                         ids=["dense", "sparse", "negative-rhs"])
@pytest.mark.parametrize("variant", RESIDENT2, ids=lambda v: "%d-%d-%d" % v)
def test_every_instantiation_matches_oracle(nat, oracle, monkeypatch, variant, kind, N, seed, blocks, min_pivots):
    """(sparse: 16 workgroups, so that one entry per column is ~2 % at every R)"""
    M = rows_for(variant[2], blocks)
    m, exp = cached_reference(oracle, kind, M, N, seed, max_pivots=np.inf)
    assert exp["status"] == "optimal" and exp["pivots"] >= min_pivots, exp["pivots"]  # (the input does some work at this height)
    if kind is negative_rhs:
        assert (m.reshape(M + 1, N + 1)[1:, 0] < 0).any()
    if kind is sparse:
        assert general_path_pivots(oracle, m, N + 1, M + 1, exp["trace"]) >= exp["pivots"] // 2
    same(solve_on(nat, monkeypatch, variant, m, N + 1, M + 1, blocks=blocks, max_pivots=np.inf), exp)


# ---- the pivot row in every slot: slot 8 beside the 8-wide vector (R = 9), the last used slot of it (R = 6) -------
@pytest.mark.parametrize("variant,N,seed", [((512, 2, 9), 37, 10), ((512, 2, 6), 37, 10), ((256, 1, 4), 37, 10)],
                         ids=lambda v: "%d-%d-%d" % v if isinstance(v, tuple) else None)
def test_pivot_rows_cover_every_slot(nat, oracle, monkeypatch, variant, N, seed):
    R = variant[2]
    M = rows_for(R)
    m, exp = cached_reference(oracle, dense, M, N, seed, max_pivots=np.inf)
    slots = set((exp["trace"][:, 0] // NB).tolist())
    assert slots == set(range(R)), sorted(slots)  # (row index of the tableau, objective row = 0)
    same(solve_on(nat, monkeypatch, variant, m, N + 1, M + 1, max_pivots=np.inf), exp)


# ---- the entering column: last real column beside a padding column, both elements of a unit, dead slots -----------
@pytest.mark.parametrize("M", [rows_for(9), rows_for(9) - 2], ids=["full-slots", "dead-slots"])
def test_entering_column_positions(nat, oracle, monkeypatch, M):
    N = 37  # odd: column N (element 0 of the last unit) sits beside a padding column
    h = M + 1
    assert (h % NB == 0) == (M == rows_for(9))
    key = ("entering", M)
    if key not in _REF:
        m = oracle.dense_lp(M, N, 5)
        m.reshape(h, N + 1)[0, N] *= 60.0  # Dantzig pricing (src/simplex.ts:71-79) takes the last column first
        _REF[key] = (m, reference(oracle, m, N + 1, h, max_pivots=np.inf))
    m, exp = _REF[key]
    cols = exp["trace"][:, 1]
    assert N in cols.tolist() and {0, 1} <= set(((cols - 1) & 1).tolist()), cols
    same(solve_on(nat, monkeypatch, (512, 2, 9), m, N + 1, h, max_pivots=np.inf), exp)


# ---- units j >= 1 and waves above 0: the other arms of the ladders over a lane's elements ---------------------------
@pytest.mark.parametrize("variant,kind", [((256, 2, 4), dense), ((256, 2, 4), sparse), ((512, 3, 4), dense), ((512, 2, 9), dense)],
                         ids=["256-2-4-dense", "256-2-4-sparse", "512-3-4-dense", "512-2-9-dense"])
def test_entering_columns_in_every_unit_of_a_lane(nat, oracle, monkeypatch, variant, kind):
    """Rows wider than 2 T columns, so that units j >= 1 of a lane hold real columns; the objective makes columns of
    every j, of lanes in waves above 0 and of both elements enter within the budget (Dantzig pricing takes the largest
    coefficient first).  Dense: the deposit, the dense column patch; sparse: the general path's column patch."""
    T, J, R = variant
    blocks = 16 if kind is sparse else NB  # (sparse: one entry per column is ~2 % at 16 R rows)
    M, N = rows_for(R, blocks), 2 * T * (J - 1) + 2 * 70 + 1  # the last unit is j = J - 1 of lane 70 (wave 1), element 0 only
    h, w = M + 1, N + 1
    key = ("units", variant, kind.__name__)
    if key not in _REF:
        m = kind(oracle, M, N, 7)
        A = m.reshape(h, w)
        want = [N, N - 1, N - 2] + [2 * T * j + 2 * 65 + e + 1 for j in range(J) for e in (0, 1)]  # tableau columns
        A[0, want] = np.abs(A[0, 1:]).max() * (2.0 + 0.01 * np.arange(len(want)))
        _REF[key] = (m, reference(oracle, m, w, h, max_pivots=12.0))
    m, exp = _REF[key]
    cols = exp["trace"][:, 1] - 1  # zero-based variable columns: unit (c >> 1), lane unit % T, j = unit // T, e = c & 1
    units = cols >> 1
    assert exp["pivots"] >= 8
    assert set((units // T).tolist()) == set(range(J)), cols       # every j
    assert ((units % T) >= 64).any() and {0, 1} <= set((cols[units // T >= 1] & 1).tolist()), cols  # a wave above 0; both e at j >= 1
    if kind is sparse:
        assert general_path_pivots(oracle, m, w, h, exp["trace"]) >= 6
    same(solve_on(nat, monkeypatch, variant, m, w, h, blocks=blocks, max_pivots=12.0), exp)


# ---- launch boundaries: leave and re-enter every 7 pivots, with different slots holding the pivot row ---------------
@pytest.mark.parametrize("variant,seed", [((512, 2, 9), 6), ((512, 2, 6), 12), ((256, 1, 4), 12)],
                         ids=lambda v: "%d-%d-%d" % v if isinstance(v, tuple) else None)
def test_launch_boundaries(nat, oracle, monkeypatch, variant, seed):
    M, N = rows_for(variant[2]), 37
    m, exp = cached_reference(oracle, negative_rhs, M, N, seed, max_pivots=np.inf)
    last = exp["trace"][6::7, 0] // NB  # the slot of the last pivot row of each launch
    assert exp["pivots"] >= 15 and len(set(last.tolist())) >= 2, (exp["pivots"], last)
    got = solve_on(nat, monkeypatch, variant, m, N + 1, M + 1, chunk=7, max_pivots=np.inf)
    assert int(got["info"]["last_resident_launches"]) >= (exp["pivots"] + 6) // 7, got["info"]
    same(got, exp)


# ---- checkCycles: the verdict exchange in every pivot, and a cycle that closes -------------------------------------
@pytest.mark.parametrize("variant", [(512, 2, 9), (256, 1, 4)], ids=lambda v: "%d-%d-%d" % v)
def test_check_cycles(nat, oracle, monkeypatch, variant):
    M, N = rows_for(variant[2]), 37
    m, exp = cached_reference(oracle, dense, M, N, 10, max_pivots=np.inf, check_cycles=True)
    assert exp["status"] == "optimal"
    same(solve_on(nat, monkeypatch, variant, m, N + 1, M + 1, max_pivots=np.inf, check_cycles=True), exp)
    # Chvatal's cycling LP on top of rows of zeros: "cycled" at the oracle's pivot
    rec = next(r for r in G.records("cases") if r["name"] == "Chvatal Cycling")
    small = G.initial_matrix(rec, oracle).reshape(rec["height"], rec["width"])
    h = NB * variant[2] - 1
    big = np.zeros((h, rec["width"]))
    big[:rec["height"]] = small
    opts = dict(G.options(rec))
    assert opts["check_cycles"]
    exp = reference(oracle, big.reshape(-1), rec["width"], h, **opts)
    assert exp["status"] == "cycled" and exp["pivots"] >= 2
    same(solve_on(nat, monkeypatch, variant, big.reshape(-1), rec["width"], h, **opts), exp)


# ---- max_pivots: a budget that ends in the middle of a phase --------------------------------------------------------
@pytest.mark.parametrize("kind,seed,budget", [(negative_rhs, 12, 3), (dense, 10, 11)], ids=["phase-1", "phase-2"])
@pytest.mark.parametrize("variant", [(512, 2, 9), (512, 2, 6), (256, 1, 4)], ids=lambda v: "%d-%d-%d" % v)
def test_pivot_budget_ends_mid_phase(nat, oracle, monkeypatch, variant, kind, seed, budget):
    M, N = rows_for(variant[2]), 37
    _, whole = cached_reference(oracle, kind, M, N, seed, max_pivots=np.inf)
    m, exp = cached_reference(oracle, kind, M, N, seed, max_pivots=float(budget))
    assert whole["pivots"] > budget and (exp["status"], exp["pivots"]) == ("cycled", budget)
    col0 = exp["matrix"].reshape(M + 1, N + 1)[1:, 0]
    assert (col0 < -1e-8).any() == (kind is negative_rhs)  # phase 1 still has an infeasible row / phase 2 is under way
    same(solve_on(nat, monkeypatch, variant, m, N + 1, M + 1, max_pivots=float(budget)), exp)

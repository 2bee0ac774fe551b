"""Every compiled kernel instantiation by name.  CENSUS holds one row per kernel that does pivot arithmetic: a shape, the
YALPS_HIP_* switches that select the kernel, checkCycles, a pivot budget and the `launched=` value yalps_tableau_info must
report.  The CPU test checks that the built library's kernels are exactly CENSUS and EXEMPT; the GPU tests run every row
and compare status, pivot count, result, both permutations and every word of the final tableau with the C oracle.

Shape rule (where the dispatcher allows it): the row spans the variant's full width -- T * J 16-byte units, N odd so that
the last unit is half padding -- and a workgroup holds exactly R rows while the last ones hold fewer (M + 1 = 256 R - 1 rows
over 256 workgroups).  The persistent kernels cross launch boundaries (YALPS_HIP_RESIDENT_CHUNK = CHUNK pivots per launch);
the delayed kernels run more than twice their delay depth, and not a multiple of it.  Row-shard rows run at world size 1
in one child process (tests/_census_shards.py); their multi-rank behaviour is tests/test_sharded.py's."""
import ast
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _census
from tests import _golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 7   # pivots per persistent launch
DEPTH = 4   # pending pivots of the delayed kernels
PERSISTENT_BUDGET = 3 * CHUNK - 4          # 17: three launches, the last one cut short
DELAYED_BUDGET = 2 * DEPTH + 1             # 9: two launches, twice the depth and one pivot pending at the end

BASE = {"YALPS_HIP_SMALL": "0", "YALPS_HIP_RESIDENT_CHUNK": str(CHUNK)}
FALLBACK = dict(BASE, YALPS_HIP_RESIDENT="0", YALPS_HIP_INPLACE="0")
IN_PLACE = dict(BASE, YALPS_HIP_RESIDENT="0")


def tall(R):
    """M for R rows per workgroup over 256 workgroups, the last one a row short."""
    return 256 * R - 2


def wide(units):
    """N for rows of exactly `units` 16-byte units, the last one half padding."""
    return 2 * units - 1


def _create_tj(N):
    """The launch-per-pivot variant's lanes and units per lane (tableau_create_impl)."""
    units = (N + 1) // 2
    T, J = (256 if units <= 512 else 1024), 1
    while T * J < units:
        J *= 2
    return T, J


def row(shape, env, launched, check=False, budget=PERSISTENT_BUDGET, shard=False):
    return {"shape": shape, "env": env, "check": check, "budget": budget, "launched": launched, "shard": shard}


CENSUS = {}

# ---- single-workgroup and any-shape paths
CENSUS["small_kernel<256>"] = row((30, 31), {"YALPS_HIP_RESIDENT_CHUNK": str(CHUNK)}, "small_kernel<256>", budget=float("inf"))
CENSUS["small_kernel<256,check>"] = row((30, 31), {}, "small_kernel<256,check>", check=True, budget=float("inf"))
CENSUS["small_kernel<1024>"] = row((96, 79), {}, "small_kernel<1024>", budget=float("inf"))
CENSUS["small_kernel<1024,check>"] = row((96, 79), {}, "small_kernel<1024,check>", check=True, budget=float("inf"))
for _k in ("generic_decide_kernel", "generic_apply_kernel"):
    CENSUS[_k] = row((60, 63), dict(BASE, YALPS_HIP_GENERIC="1"), "generic_decide_kernel+generic_apply_kernel", budget=40)

# ---- register-resident kernels: YALPS_HIP_RVARIANT picks the shape, _RESIDENT_GEN and _TAG the form
RESIDENT = [(256, 1, 4), (256, 1, 9), (256, 1, 16), (256, 2, 4), (256, 2, 9), (512, 1, 24), (512, 1, 32), (512, 1, 40),
            (512, 2, 4), (512, 2, 6), (512, 2, 9), (512, 2, 12), (512, 2, 16), (512, 3, 4), (512, 3, 6), (512, 3, 9),
            (512, 3, 12), (512, 4, 4), (512, 4, 6), (512, 4, 8), (512, 5, 4), (512, 5, 6), (512, 6, 4)]
RESIDENT2 = [(256, 1, 4), (256, 1, 9), (256, 2, 4), (512, 2, 4), (512, 2, 6), (512, 2, 9), (512, 3, 4)]
RESIDENT_LDS = [(512, 1, 38), (512, 2, 16), (512, 3, 11), (512, 4, 7), (512, 5, 5), (512, 6, 3)]
for T, J, R in RESIDENT:
    k = "resident_kernel<%d,%d,%d>" % (T, J, R)
    CENSUS[k] = row((tall(R), wide(T * J)), dict(BASE, YALPS_HIP_RVARIANT="%d,%d,%d" % (T, J, R), YALPS_HIP_RESIDENT_GEN="1",
                                                 YALPS_HIP_TAG="0"), k)
for T, J, R in RESIDENT2:
    k = "resident2_kernel<%d,%d,%d>" % (T, J, R)
    CENSUS[k] = row((tall(R), wide(T * J)), dict(BASE, YALPS_HIP_RVARIANT="%d,%d,%d" % (T, J, R), YALPS_HIP_RESIDENT_GEN="2",
                                                 YALPS_HIP_TAG="0"), k)
CENSUS["resident_kernel<256,1,4,tag>"] = row((tall(4), wide(256)), dict(BASE, YALPS_HIP_RVARIANT="256,1,4", YALPS_HIP_TAG="1"),
                                             "resident_kernel<256,1,4,tag>", check=True)
for T, J, R in RESIDENT_LDS:  # one row per workgroup beyond the registers: in LDS
    k = "resident_kernel<%d,%d,%d,lds>" % (T, J, R)
    CENSUS[k] = row((tall(R + 1), wide(T * J)), dict(BASE, YALPS_HIP_RVARIANT="%d,%d,%d" % (T, J, R), YALPS_HIP_RESIDENT_GEN="1"), k)

# ---- persistent in place, one pivot per sweep (stream_kernel: checkCycles selects the CHECK form)
for T, J in ((256, 1), (256, 2), (1024, 1), (1024, 2), (1024, 4)):
    env = dict(IN_PLACE, YALPS_HIP_DELAY="0", YALPS_HIP_SWEEP="0")
    k = "stream_kernel<%d,%d>" % (T, J)
    CENSUS[k] = row((tall(2), wide(T * J)), env, k)
    if J < 4:
        CENSUS[k[:-1] + ",check>"] = row((tall(2), wide(T * J)), env, k[:-1] + ",check>", check=True)
# sweep_kernel<512, 2 J>: tableaux of create-J 4 (YALPS_HIP_SWEEP=2) and 8
for J in (8, 16):
    for nt in (0, 1):
        env = dict(IN_PLACE, YALPS_HIP_DELAY="0", YALPS_HIP_SWEEP="2", YALPS_HIP_SWEEP_NT=str(nt))
        k = "sweep_kernel<512,%d%s>" % (J, ",nt" if nt else "")
        CENSUS[k] = row((tall(2), wide(512 * J)), env, k)
        if J == 8:
            k = "sweep_kernel<512,8,check%s>" % (",nt" if nt else "")
            CENSUS[k] = row((tall(2), wide(512 * J)), env, k, check=True)

# ---- persistent in place with delayed row updates
for T, J, nt in ((256, 1, 0), (256, 2, 0), (1024, 1, 0), (1024, 2, 0), (512, 8, 0), (1024, 2, 1), (512, 8, 1)):
    env = dict(IN_PLACE, YALPS_HIP_DELAY_KERNEL="2", YALPS_HIP_DELAY_NT=str(nt), YALPS_HIP_DELAY_DEPTH=str(DEPTH))
    k = "stream2_kernel<%d,%d%s>" % (T, J, ",nt" if nt else "")
    CENSUS[k] = row((tall(DEPTH), wide(T * J)), env, k, budget=DELAYED_BUDGET)
for J in (1, 2, 4, 6, 8, 16):
    for nt in (0, 1):
        for panel in (1, 0):
            env = dict(IN_PLACE, YALPS_HIP_DELAY_NT=str(nt), YALPS_HIP_STREAM3_PANEL=str(panel), YALPS_HIP_DELAY_DEPTH=str(DEPTH))
            form = "panel" if panel else "direct"
            k = "stream3_kernel<512,%d%s,%s>" % (J, ",nt" if nt else "", form)
            CENSUS[k] = row((tall(DEPTH), wide(512 * J)), env, k, budget=DELAYED_BUDGET)
            if J != 16 or not panel:  # (checkCycles on rows of 16 units per lane: no panel form -- the direct one runs)
                kc = "stream3_kernel<512,%d%s,check,%s>" % (J, ",nt" if nt else "", form)
                CENSUS[kc] = row((tall(DEPTH), wide(512 * J)), env, kc, check=True, budget=DELAYED_BUDGET)

# ---- one launch per pivot: pivot_kernel where no wide_kernel takes the row updates, else as the DECIDE launch of checkCycles
for T, J, R in ((256, 1, 4), (256, 1, 9), (256, 1, 16), (256, 2, 4), (256, 2, 8), (1024, 1, 4), (1024, 1, 9), (1024, 1, 16)):
    k = "pivot_kernel<%d,%d,%d>" % (T, J, R)
    CENSUS[k] = row((tall(R), wide(T * J)), FALLBACK, k)
for T, J, R in ((1024, 2, 4), (1024, 2, 8), (1024, 4, 4), (1024, 8, 2)):
    k = "pivot_kernel<%d,%d,%d>" % (T, J, R)
    CENSUS[k] = row((tall(R), wide(T * J)), dict(FALLBACK, YALPS_HIP_WIDE8="1"), "wide_kernel<%d,%d>+%s" % (T, J, k), check=True)
for T, J in ((256, 1), (256, 2), (1024, 1), (1024, 2), (1024, 4), (1024, 8)):
    k = "wide_kernel<%d,%d>" % (T, J)
    CENSUS[k] = row((tall(2), wide(T * J)), dict(FALLBACK, YALPS_HIP_WIDE="1", YALPS_HIP_WIDE8="1"), k)


# ---- row shards at world size 1 (the bootstrap scan is the ping-pong wide_kernel: YALPS_HIP_WIDE=1 makes every width have one)
def _shard_launched(N, select, step, check=False, sweep=None):
    T, J = _create_tj(N)
    return "+".join(["wide_kernel<%d,%d>" % (T, J), select] + (["shard_cycle_kernel"] if check else []) + [step] + ([sweep] if sweep else []))


SHARD = {"YALPS_HIP_WIDE": "1", "YALPS_HIP_SHARD_INPLACE": "1"}
for T, J, lT, lJ in ((256, 1, 256, 1), (256, 2, 256, 2), (1024, 1, 1024, 1), (1024, 2, 1024, 2), (1024, 4, 1024, 4), (1024, 8, 512, 16)):
    for nt in (0, 1):
        k = "wide_kernel<%d,%d,inplace%s>" % (lT, lJ, ",nt" if nt else "")
        N = wide(T * J)
        CENSUS[k] = row((tall(2), N), dict(SHARD, YALPS_HIP_SHARD_DELAY="0", YALPS_HIP_SHARD_NT=str(nt)),
                        _shard_launched(N, "shard_select_kernel", k), shard=True)
CENSUS["shard_select_kernel"] = dict(CENSUS["wide_kernel<1024,1,inplace>"])
CENSUS["shard_cycle_kernel"] = row((tall(2), wide(1024)), dict(SHARD, YALPS_HIP_SHARD_DELAY="0", YALPS_HIP_SHARD_NT="0"),
                                   _shard_launched(wide(1024), "shard_select_kernel", "wide_kernel<1024,1,inplace>", check=True),
                                   check=True, shard=True)
for J in (1, 2, 4, 6, 8, 16):
    for nt in (0, 1):
        for panel in (0, 1):
            k = "dshard_kernel<512,%d%s%s>" % (J, ",nt" if nt else "", ",panel" if panel else "")
            N = wide(512 * J)
            env = dict(SHARD, YALPS_HIP_SHARD_NT=str(nt), YALPS_HIP_SHARD_PANEL=str(panel), YALPS_HIP_DELAY_DEPTH=str(DEPTH),
                       YALPS_HIP_SHARD_XSWEEP="0")
            CENSUS[k] = row((tall(DEPTH), N), env, _shard_launched(N, "dshard_select_kernel<256>", k), budget=DELAYED_BUDGET, shard=True)
CENSUS["dshard_select_kernel<256>"] = dict(CENSUS["dshard_kernel<512,2>"])
# more than 256 workgroups (YALPS_HIP_BLOCKS, read when the context is created): the 1024-lane select
CENSUS["dshard_select_kernel<1024>"] = row((512 * DEPTH - 2, wide(512)), dict(SHARD, YALPS_HIP_BLOCKS="512", YALPS_HIP_SHARD_NT="0",
                                                                            YALPS_HIP_SHARD_PANEL="0", YALPS_HIP_DELAY_DEPTH=str(DEPTH),
                                                                            YALPS_HIP_SHARD_XSWEEP="0"),
                                           _shard_launched(wide(512), "dshard_select_kernel<1024>", "dshard_kernel<512,1>"),
                                           budget=DELAYED_BUDGET, shard=True)
# the shard's sweep as a launch of its own: once DEPTH pivots are pending (yalps_shard_run's batches are a multiple of DEPTH)
for nt in (0, 1):
    k = "dshard_sweep_kernel%s" % ("<nt>" if nt else "")
    step = "dshard_kernel<512,4%s>" % (",nt" if nt else "")
    CENSUS[k] = row((tall(DEPTH), wide(2048)), dict(SHARD, YALPS_HIP_SHARD_NT=str(nt), YALPS_HIP_SHARD_PANEL="0",
                                                   YALPS_HIP_DELAY_DEPTH=str(DEPTH), YALPS_HIP_SHARD_XSWEEP="1"),
                    _shard_launched(wide(2048), "dshard_select_kernel<256>", step, sweep=k), budget=DELAYED_BUDGET, shard=True)

# Kernels without a census row: no pivot arithmetic, or run by name by the test named ("file::function")
EXEMPT = {
    "assemble_clear_kernel": "test_hip_parity.py::test_assemble_then_solve_matches_reference_golden",
    "assemble_scatter_kernel": "test_hip_parity.py::test_assemble_then_solve_matches_reference_golden",
    "apply_cuts_kernel": "test_milp_paths.py::test_node_solve_replays_every_node",
    "node_prepare_kernel": "test_milp_paths.py::test_node_solve_replays_every_node",
    "node_finish_kernel": "test_milp_paths.py::test_node_solve_replays_every_node",
    "flush_swap_kernel": "test_hip_parity.py::test_single_pivot_matches_oracle",
    "exchange_floor_kernel<256,1>": "test_bench_contract.py::test_default_workload_line",
    "exchange_floor_kernel<256,2>": "test_bench_contract.py::test_default_workload_line",
    "exchange_floor_kernel<512,2>": "test_bench_contract.py::test_default_workload_line",
    "exchange_floor_kernel<512,3>": "test_bench_contract.py::test_default_workload_line",
    # (batch_kernel<256, true> in LDS, <1024, false> in HBM: chosen by YALPS_HIP_NO_LDS, every node against the oracle)
    "batch_kernel<256,lds>": "test_batch.py::test_batch_nodes_match_oracle",
    "batch_kernel<1024>": "test_batch.py::test_batch_nodes_match_oracle",
}


def _depth(env):
    return int(env["YALPS_HIP_DELAY_DEPTH"]) if "YALPS_HIP_DELAY_DEPTH" in env else None


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_census_names_every_compiled_kernel():
    """A kernel added to a table without a census row, or a row whose kernel is no longer built, fails here."""
    from yalps_amd import build
    built = _census.census(build.kernel_metadata())
    assert not set(CENSUS) & set(EXEMPT), set(CENSUS) & set(EXEMPT)
    assert set(built) - set(CENSUS) - set(EXEMPT) == set(), "compiled without a census row: %s" % sorted(set(built) - set(CENSUS) - set(EXEMPT))
    assert set(CENSUS) | set(EXEMPT) == set(built), "census rows for kernels that are not built: %s" % sorted(set(CENSUS) | set(EXEMPT) - set(built))
    for key, r in CENSUS.items():  # (what a row expects to run is built)
        assert set(r["launched"].split("+")) <= set(built), (key, r["launched"])


def test_census_rows_follow_the_shape_and_budget_rules():
    for key, r in CENSUS.items():
        names = r["launched"].split("+")
        assert key in names, (key, r["launched"])
        M, N = r["shape"]
        assert N % 2 == 1, key
        d = _depth(r["env"])
        if d is not None:
            assert r["budget"] > 2 * d and r["budget"] % d != 0, key
        if any(n.startswith(("resident", "stream", "sweep_kernel")) for n in names):
            assert r["budget"] > int(r["env"]["YALPS_HIP_RESIDENT_CHUNK"]), key
        if key.startswith("resident") and ",lds" not in key:
            T, J, R = (int(x) for x in key[key.index("<") + 1:].rstrip(">").split(",")[:3])
            assert (N + 1) // 2 == T * J and -(-(M + 1) // 256) == R and (M + 1) % R != 0, key


def test_exempt_kernels_name_a_test_that_exists():
    for key, where in EXEMPT.items():
        path, func = where.split("::")
        tree = ast.parse(open(os.path.join(ROOT, "tests", path)).read())
        assert any(isinstance(n, ast.FunctionDef) and n.name == func for n in tree.body), (key, where)


# ---------------------------------------------------------------------------------------------------------------- GPU
_ORACLE_RUNS = {}


def _oracle_run(M, N, check, budget):
    """(status, result, pivots, tableau, pos, var) of the C oracle on the census input; rows that share it share the run."""
    key = (M, N, check, budget)
    if key not in _ORACLE_RUNS:
        from tests import _oracle
        from tests._census_shards import census_input
        big = (M + 1) * (N + 1) > 4_000_000
        orc = _oracle.load(omp=big)
        if big:
            orc.set_threads(8)
        w, h = N + 1, M + 1
        m = census_input(orc, M, N)
        pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
        st, res, piv, _ = orc.simplex(m, w, h, pos, var, max_pivots=budget, check_cycles=check)
        _ORACLE_RUNS[key] = (st, res, piv, m, pos, var)
    return _ORACLE_RUNS[key]


def _compare(key, r, status, result, npiv, got, gpos, gvar):
    M, N = r["shape"]
    est, eres, epiv, ref, rpos, rvar = _oracle_run(M, N, r["check"], r["budget"])
    assert (status, npiv) == (est, epiv), (key, status, npiv, est, epiv)
    assert G.same_number(result, eres), (key, result, eres)
    assert np.array_equal(gpos, rpos) and np.array_equal(gvar, rvar), key
    assert np.array_equal(np.asarray(got).view(np.int64), ref.view(np.int64)), key


SINGLE = [k for k, r in CENSUS.items() if not r["shard"]]
SHARDED = [k for k, r in CENSUS.items() if r["shard"]]


@pytest.mark.gpu
@pytest.mark.parametrize("key", SINGLE)
def test_census_row(monkeypatch, key):
    from yalps_amd import _native
    r = CENSUS[key]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    M, N = r["shape"]
    w, h = N + 1, M + 1
    from tests import _oracle
    from tests._census_shards import census_input
    m = census_input(_oracle.load(), M, N)
    pos, var = np.arange(w + h, dtype=np.int32), np.arange(w + h, dtype=np.int32)
    ctx = _native.Context(0)
    try:
        t = _native.DeviceTableau(ctx, w, h)
        try:
            t.upload(m, h, pos, var)
            status, result, npiv, _ = t.solve(max_pivots=r["budget"], check_cycles=r["check"], timing=False)
            info = t.info()
            got, gpos, gvar = t.download()
        finally:
            t.close()
    finally:
        ctx.close()
    assert info["launched"] == r["launched"], (key, info)
    _compare(key, r, status, result, npiv, got, gpos, gvar)


@pytest.fixture(scope="module")
def shard_results(tmp_path_factory):
    """Every row-shard row in one child process (tests/_census_shards.py), switches set between the set_shard calls."""
    tmp = tmp_path_factory.mktemp("census_shards")
    rows = [{"key": k, "M": CENSUS[k]["shape"][0], "N": CENSUS[k]["shape"][1], "env": CENSUS[k]["env"], "check": CENSUS[k]["check"],
             "budget": CENSUS[k]["budget"]} for k in SHARDED]
    spec, out_npz = str(tmp / "rows.json"), str(tmp / "out.npz")
    with open(spec, "w") as f:
        json.dump(rows, f)
    out = subprocess.run([sys.executable, "-m", "tests._census_shards", spec, out_npz], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
    res = np.load(out_npz)
    return {k: {f: res["r%d_%s" % (i, f)] for f in ("status", "result", "pivots", "launched", "matrix", "pos", "var")}
            for i, k in enumerate(SHARDED)}


@pytest.mark.gpu
@pytest.mark.parametrize("key", SHARDED)
def test_census_shard_row(shard_results, key):
    r, got = CENSUS[key], shard_results[key]
    assert str(got["launched"]) == r["launched"], (key, str(got["launched"]))
    _compare(key, r, str(got["status"]), float(got["result"]), int(got["pivots"]), got["matrix"], got["pos"], got["var"])

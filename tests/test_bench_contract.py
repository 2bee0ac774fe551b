"""bench.py as the driver runs it (small sizes): one JSON line with the contract's keys, `roofline` and `cpu_baseline`
at N=1; the sharded workload's line.  A crash in either path is a lost round-end measurement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline")


def _bench(args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_default_workload_line():
    rec = _bench(["--size", "300", "--steps", "2", "--warmup", "1", "--cpu-pivots", "200", "--sweep-launches", "4"])
    for k in KEYS + ("cpu_baseline",):
        assert k in rec, k
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["vs_baseline"] is None and rec["dtype"] == "f64"
    assert rec["value"] > 0 and rec["roofline"]["bound"] in ("hbm", "mfma", "onchip") and rec["cpu_baseline"]["value"] > 0
    assert "workload" in rec["config"]
    rf = rec["roofline"]
    if rf["bound"] == "onchip":  # the register-resident kernel: one bound stated consistently, the HBM figure beside it
        assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and rf["unit"] == "pivots/s" and rf["frac_hbm"] > 0
        floor = rf["onchip_floor"]
        assert 0 < floor["measured_exchange"]["flags_only_us"] <= floor["measured_exchange"]["publish_flags_fetch_us"] < floor["us"] < 50


@pytest.mark.gpu
@pytest.mark.parametrize("extra,kernel", [([], "dshard_kernel"), (["--shard-rows", "300"], "wide_kernel")])
def test_sharded_workload_line(extra, kernel, tmp_path, oracle):
    """--workload sharded at one rank (RCCL transport, world 1): 5 000 columns; 1 200 rows take the delayed shard kernel,
    300 rows (two per workgroup) one sweep per pivot.  --dump-outputs: the whole tableau after the timed pivots, bit for
    bit the oracle's."""
    rec = _bench(["--workload", "sharded", "--size", "5000", "--steps", "1", "--warmup", "1", "--pivots-per-step", "24",
                  "--dump-outputs", str(tmp_path)] + (extra if extra else ["--shard-rows", "1200"]))
    assert sorted(os.listdir(tmp_path)) == DUMPED
    _check_sharded_dump(oracle, [_load_dump(tmp_path)], 300 if extra else 1200, 5000, 24)
    for k in KEYS:
        assert k in rec, k
    assert rec["scaling"] == "strong" and rec["value"] > 0
    assert rec["roofline"]["kernel"].startswith(kernel), rec["roofline"]
    assert rec["parity"]["ok"] is True and rec["parity"]["pivots"] == 48 and rec["cpu_baseline"]["value"] > 0, rec["parity"]
    if kernel == "dshard_kernel":
        assert rec["roofline"]["delay_depth"] == 8 and "algorithmic_equiv" in rec["roofline"]


def _bench_ranks(n, args):
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
                          "127.0.0.1", "--master-port", str(port), "bench.py", "--gpus", str(n)] + args, cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_two_ranks_line_carries_the_row_sharded_measurement():
    """The driver's multi-GPU command, rehearsed with two ranks sharing the test GPU: the replicas headline, and beside it
    `sharded_c5` -- ONE tableau row-sharded over the ranks, measured by child processes in a group of their own (here a
    4097 x 4097 stand-in for config 5 over the host transport; on a node: 16385 x 16385 over RCCL)."""
    rec = _bench_ranks(2, ["--size", "300", "--steps", "2", "--warmup", "1", "--sharded-c5-size", "4096", "--pivots-per-step", "40"])
    for k in KEYS[:-1]:
        assert k in rec, k
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and rec["value"] > 0
    c5 = rec["sharded_c5"]
    assert "error" not in c5, c5
    assert c5["n_gpus"] == 2 and c5["scaling"] == "strong" and c5["value"] > 0 and c5["us_per_pivot"] > 0
    assert c5["roofline"]["kernel"].startswith("dshard_kernel") and c5["exchange"]["transport"] == "host"
    assert "4097x4097" in c5["workload"] and c5["parity"]["ok"] is True, c5.get("parity")


@pytest.mark.gpu
def test_a_failing_row_sharded_measurement_leaves_the_headline_alone():
    """Children that do not finish in time are killed and reported; the line, its headline and the return code stay."""
    rec = _bench_ranks(2, ["--size", "300", "--steps", "2", "--warmup", "1", "--sharded-c5-size", "4096", "--sharded-c5-timeout", "0.05"])
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and "timed out" in rec["sharded_c5"]["error"]


DUMPED = ["position_of_variable.npy", "summary.npy", "tableau.npy", "tableau_rows.npy", "variable_at_position.npy"]


def _load_dump(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_stay_within_the_budget(tmp_path):
    """--dump-outputs: float64 files only, at most 64 MB in all; a tableau above that is written as a fixed, seeded sample
    of its rows (the objective row among them), the same sample from run to run; a small one whole."""
    import bench
    h, w = 3000, 4097  # 98 MB of rows
    tab = np.arange(h * w, dtype=np.float64).reshape(h, w)
    pos = np.arange(w + h, dtype=np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, 1, tab, np.arange(h), "cycled", -1.5, 7, pos, pos[::-1].copy())
    assert sorted(os.listdir(tmp_path / "a")) == DUMPED
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in DUMPED) <= 64 * 10**6
    a, b = _load_dump(tmp_path / "a"), _load_dump(tmp_path / "b")
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["tableau_rows"].astype(np.int64)
    assert rows[0] == 0 and np.all(np.diff(rows) > 0) and rows[-1] < h and len(rows) > h // 2
    assert np.array_equal(a["tableau"], tab[rows])
    assert a["summary"].tolist() == [3.0, -1.5, 7.0] and np.array_equal(a["variable_at_position"], pos[::-1])
    bench.dump_outputs(str(tmp_path / "c"), 1, 2, tab[:50, :40], np.arange(50), "optimal", 2.0, 3, pos[:90], pos[:90])
    c = _load_dump(tmp_path / "c")
    assert sorted(c) == ["rank1_" + f[:-4] for f in DUMPED]
    assert np.array_equal(c["rank1_tableau"], tab[:50, :40]) and np.array_equal(c["rank1_tableau_rows"], np.arange(50))


@pytest.mark.parametrize("world", [1, 2])
def test_dump_outputs_headers_inside_the_budget(tmp_path, world):
    """The shapes of `bench.py --size 4096` (a 4097 x 4097 tableau): files and their .npy headers together stay within
    64 * 10**6 bytes (64 MB in either reading of MB), this rank's share of it when the ranks share the budget."""
    import bench
    n = 4097
    tab = np.zeros((n, n))
    pos = np.arange(2 * n, dtype=np.int32)
    bench.dump_outputs(str(tmp_path), 0, world, tab, np.arange(n), "optimal", 1.0, 9, pos, pos)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert len(os.listdir(tmp_path)) == len(DUMPED) and 0.99 * 64e6 / world < total <= 64 * 10**6 // world, total


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step(tmp_path, oracle):
    """bench.py --dump-outputs: the tableau, permutations, status, objective cell and pivot count of the last timed solve,
    bit for bit those of the CPU oracle on the same LP."""
    rec = _bench(["--size", "300", "--steps", "3", "--warmup", "1", "--cpu-pivots", "0", "--sweep-launches", "4",
                  "--dump-outputs", str(tmp_path)])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == DUMPED
    got = _load_dump(tmp_path)
    from yalps_amd import _native
    w = h = 301
    m = _native.dense_lp(300, 300, 42)  # (bench.py's input)
    pos = np.arange(w + h, dtype=np.int32)
    var = pos.copy()
    status, result, npiv, _ = oracle.simplex(m, w, h, pos, var, max_pivots=float("inf"))
    assert got["summary"].tolist() == [_native.STATUS.index(status), result, npiv] and npiv == rec["config"]["pivots_per_step"]
    assert np.array_equal(got["tableau_rows"], np.arange(h))
    assert np.array_equal(got["tableau"].reshape(-1).view(np.int64), m.view(np.int64))
    assert np.array_equal(got["position_of_variable"], pos) and np.array_equal(got["variable_at_position"], var)


def _check_sharded_dump(oracle, dumps, M, N, pivots):
    """Every rank's dump of a row-sharded dense-LP(M,N,42) after `pivots` pivots: the objective row and the rank's own block
    of rows, which together cover the tableau, each row and both permutations bit for bit the oracle's."""
    from yalps_amd import _native
    w, h = N + 1, M + 1
    m = oracle.dense_lp(M, N, 42)
    pos = np.arange(w + h, dtype=np.int32)
    var = pos.copy()
    status, result, npiv, _ = oracle.simplex(m, w, h, pos, var, max_pivots=float(pivots))
    m = m.reshape(h, w)
    seen = []
    for d in dumps:
        rows = d["tableau_rows"].astype(np.int64)
        assert rows[0] == 0 and np.array_equal(rows[1:], np.arange(rows[1], rows[-1] + 1)), rows
        assert d["tableau"].shape == (len(rows), w)
        assert np.array_equal(d["tableau"].view(np.int64), m[rows].view(np.int64))
        assert np.array_equal(d["position_of_variable"], pos) and np.array_equal(d["variable_at_position"], var)
        assert np.array_equal(d["summary"], [_native.STATUS.index(status), result, npiv], equal_nan=True), (d["summary"], status)
        seen.extend(rows[1:].tolist())
    assert sorted(seen) == list(range(1, h))


@pytest.mark.gpu
def test_two_ranks_sharded_dump(tmp_path, oracle):
    """--workload sharded --dump-outputs over two ranks (sharing the test GPU, host transport): rank0_ and rank1_ files, the
    objective row and each rank's own rows, together the oracle's whole tableau after the timed pivots."""
    rec = _bench_ranks(2, ["--workload", "sharded", "--size", "1000", "--steps", "1", "--warmup", "1", "--pivots-per-step", "24",
                           "--dump-outputs", str(tmp_path)])
    assert rec["n_gpus"] == 2 and rec["steps"] == 1 and rec["parity"]["ok"] is True
    assert sorted(os.listdir(tmp_path)) == sorted("rank%d_%s" % (r, f) for r in (0, 1) for f in DUMPED)
    got = _load_dump(tmp_path)
    dumps = [{k[len("rank%d_" % r):]: v for k, v in got.items() if k.startswith("rank%d_" % r)} for r in (0, 1)]
    _check_sharded_dump(oracle, dumps, 1000, 1000, 24)

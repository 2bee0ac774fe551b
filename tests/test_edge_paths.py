"""Every device path on the edge records (tests/_edges.py, tests/golden/simplex_edges.json.gz): exact ties across the
kernels' splits, infinite ratios, signed zeros, the flush band, exact thresholds, subnormals.  Each path asserts the kernel
it expects (shape and switches taken from the parity test that names that kernel) before status, pivot count, result,
basis and the SHA-256 of the whole final tableau are compared with the reference's record."""
import os

import numpy as np
import pytest

from tests import _edges as E
from tests import _golden as G
from tests import _rounding as RD

pytestmark = pytest.mark.gpu

NO_DELAY = {"YALPS_HIP_DELAY": "0"}
FALLBACK = {"YALPS_HIP_RESIDENT": "0", "YALPS_HIP_INPLACE": "0"}

# name -> (kernel family, shape, switches, the info() entries expected (a tuple: any of them; `launched`: by checkCycles), checkCycles
# supported).  (stream3-j16-panels: checkCycles has no panel form for rows of 16 units per lane -- those records run the direct one.)
PATHS = {
    "small": ("small", (60, 64), {}, {"last_path": "small", "launched": {False: "small_kernel<1024>", True: "small_kernel<1024,check>"}}, True),
    "resident-gen1": ("resident", (600, 2500), {"YALPS_HIP_RESIDENT_GEN": "1"},
                      {"last_path": "resident", "resident": "resident_kernel<512,3,4>",
                       "launched": {False: "resident_kernel<512,3,4>", True: "resident_kernel<512,3,4>"}}, True),
    "resident-gen2": ("resident2", (600, 2500), {"YALPS_HIP_RESIDENT_GEN": "2"},
                      {"last_path": "resident", "resident": ("resident2_kernel<512,3,4>", "resident_kernel<512,3,4>"),
                       "launched": {False: "resident2_kernel<512,3,4>", True: "resident2_kernel<512,3,4>"}}, True),
    "resident-tag": ("resident-tag", (300, 200), {"YALPS_HIP_SMALL": "0", "YALPS_HIP_TAG": "1", "YALPS_HIP_RESIDENT_GEN": "2"},
                     {"last_path": "resident", "resident": "resident_kernel<256,1,4,tag>",
                      "launched": {False: "resident_kernel<256,1,4,tag>", True: "resident_kernel<256,1,4,tag>"}}, True),
    "resident2-flags": ("resident2", (300, 200), {"YALPS_HIP_SMALL": "0", "YALPS_HIP_TAG": "0", "YALPS_HIP_RESIDENT_GEN": "2"},
                        {"last_path": "resident", "resident": "resident2_kernel<256,1,4>",
                         "launched": {False: "resident2_kernel<256,1,4>", True: "resident2_kernel<256,1,4>"}}, True),
    "resident-lds": ("resident-lds", (2800, 3300), {}, {"last_path": "resident", "resident": "resident_kernel<512,4,7,lds>",
                                                      "lds_rows": "4", "launched": {False: "resident_kernel<512,4,7,lds>", True: "resident_kernel<512,4,7,lds>"}}, True),
    "stream": ("stream_kernel", (2800, 3300), {"YALPS_HIP_DELAY": "0", "YALPS_HIP_SWEEP": "0", "YALPS_HIP_LDS_ROWS": "0"},
               {"last_path": "inplace", "inplace": "stream_kernel",
                "launched": {False: "stream_kernel<1024,2>", True: "stream_kernel<1024,2,check>"}}, True),
    "stream2": ("stream2_kernel", (900, 7000), {"YALPS_HIP_DELAY_KERNEL": "2"},
                {"last_path": "inplace", "inplace": "stream2_kernel<512,8>"}, False),
    "stream2-nt": ("stream2_kernel", (1400, 8192), {"YALPS_HIP_DELAY_NT": "1", "YALPS_HIP_DELAY_KERNEL": "2"},
                   {"last_path": "inplace", "inplace": "stream2_kernel<512,8,nt>"}, False),
    "stream3-j4": ("stream3_kernel", (4300, 4096), {}, {"last_path": "inplace", "inplace": "stream3_kernel<512,4>"}, False),
    "stream3-j8-panels": ("stream3_kernel", (900, 7000), {"YALPS_HIP_STREAM3_PANEL": "1"},
                          {"last_path": "inplace", "inplace": "stream3_kernel<512,8>", "sweep": "panels",
                           "launched": {False: "stream3_kernel<512,8,panel>", True: "stream3_kernel<512,8,check,panel>"}}, True),
    "stream3-j8-direct": ("stream3_kernel", (900, 7000), {"YALPS_HIP_STREAM3_PANEL": "0"},
                          {"last_path": "inplace", "inplace": "stream3_kernel<512,8>", "sweep": "direct",
                           "launched": {False: "stream3_kernel<512,8,direct>", True: "stream3_kernel<512,8,check,direct>"}}, True),
    "stream3-j16-panels": ("stream3_kernel", (2100, 12345), {"YALPS_HIP_STREAM3_PANEL": "1"},
                           {"last_path": "inplace", "inplace": "stream3_kernel<512,16>",
                           "launched": {False: "stream3_kernel<512,16,panel>", True: "stream3_kernel<512,16,check,direct>"}}, True),
    "stream3-j16-direct": ("stream3_kernel", (2100, 12345), {"YALPS_HIP_STREAM3_PANEL": "0"},
                           {"last_path": "inplace", "inplace": "stream3_kernel<512,16>", "sweep": "direct",
                           "launched": {False: "stream3_kernel<512,16,direct>", True: "stream3_kernel<512,16,check,direct>"}}, True),
    "sweep-j8": ("sweep_kernel", (1400, 8192), dict(NO_DELAY, YALPS_HIP_SWEEP="2"),
                 {"last_path": "inplace", "inplace": "sweep_kernel<512,8>"}, False),
    "sweep-j8-nt": ("sweep_kernel", (2500, 5000), dict(NO_DELAY, YALPS_HIP_SWEEP="2", YALPS_HIP_SWEEP_NT="1"),
                    {"last_path": "inplace", "inplace": "sweep_kernel<512,8,nt>"}, False),
    "sweep-j16": ("sweep_kernel", (600, 16000), NO_DELAY, {"last_path": "inplace", "inplace": "sweep_kernel<512,16>"}, False),
    "sweep-j16-nt": ("sweep_kernel", (300, 9000), dict(NO_DELAY, YALPS_HIP_SWEEP_NT="1"),
                     {"last_path": "inplace", "inplace": "sweep_kernel<512,16,nt>"}, False),
    "pivot-1024-1-16": ("pivot_kernel", (4000, 2000), FALLBACK, {"last_path": "streaming", "streaming": "pivot_kernel<1024,1,16>"}, False),
    "pivot-256-1-16": ("pivot_kernel", (4000, 500), FALLBACK, {"last_path": "streaming", "streaming": "pivot_kernel<256,1,16>"}, False),
    "pivot-256-2-8": ("pivot_kernel", (2000, 1000), FALLBACK, {"last_path": "streaming", "streaming": "pivot_kernel<256,2,8>"}, False),
    "generic-forced": ("generic", (60, 64), {"YALPS_HIP_SMALL": "0", "YALPS_HIP_GENERIC": "1"}, {"last_path": "generic", "launched": {False: "generic_decide_kernel+generic_apply_kernel", True: "generic_decide_kernel+generic_apply_kernel"}}, True),
    "generic-wide": ("generic", (200, 20000), {}, {"last_path": "generic", "launched": {False: "generic_decide_kernel+generic_apply_kernel", True: "generic_decide_kernel+generic_apply_kernel"}}, True),
    # batch_kernel through NodeBatch with an empty cut list (the node is the root tableau): in LDS, and in HBM -- chosen by
    # YALPS_HIP_NO_LDS as in tests/test_batch.py; NodeBatch reports no kernel, so these two are the only unasserted rows
    "batch-lds": ("batch_kernel", (60, 64), {}, None, False),
    "batch-hbm": ("batch_kernel", (60, 64), {"YALPS_HIP_NO_LDS": "1"}, None, False),
}

# name -> (kernel family, worker kind, world, shape, switches, kernel the worker reports (a prefix), its shard_sweep, the
# fewest pivots a record must have: the sweep launch (dsweep_kernel.cuh) runs once `delay_depth` pivots are pending)
SHARDS = {
    "shard-hip-w1": ("shard-hip", "hip", 1, (200, 150), {}, "pivot_kernel", "none", 0),
    "shard-rccl-w1": ("shard-rccl", "hip-rccl", 1, (200, 150), {}, "pivot_kernel", "none", 0),
    "shard-native-w2": ("shard-native", "hip-native", 2, (200, 150), {}, "pivot_kernel", "none", 0),
    "shard-wide-w2": ("wide_kernel", "hip", 2, (2300, 4200), {"YALPS_HIP_SHARD_DELAY": "0"}, "wide_kernel<1024,4>", "none", 0),
    "dshard-w2": ("dshard_kernel", "hip", 2, (120, 3000), {"YALPS_HIP_DELAY_MIN_ROWS": "1", "YALPS_HIP_DELAY_DEPTH": "4"},
                  "dshard_kernel<512,4>,delay_depth:4", "inline", 0),
    "dshard-launch-w3": ("dsweep_kernel", "hip-native", 3, (3300, 4200), {}, "dshard_kernel<512,6>,delay_depth:8", "launch", 8),
    "dshard-inline-w3": ("dshard_kernel", "hip-native", 3, (3300, 4200), {"YALPS_HIP_SHARD_XSWEEP": "0"},
                         "dshard_kernel<512,6>,delay_depth:8", "inline", 0),
    "dshard-panel-w2": ("dshard_kernel", "hip-native", 2, (13000, 2100), {}, "dshard_kernel<512,4,panel>,delay_depth:16", "inline", 0),
    "dshard-panel-launch-w2": ("dsweep_kernel", "hip-native", 2, (13000, 2100), {"YALPS_HIP_SHARD_XSWEEP": "1", "YALPS_HIP_DELAY_DEPTH": "8"},
                               "dshard_kernel<512,4,panel>,delay_depth:8", "launch", 8),
}
# the families the row shards run (a launch of `world` processes per record): ties across ranks, the early break, +inf
# ratios, signed zeros, the flush band, subnormals
SHARD_FAMILIES = ("E1", "E2", "E2b", "E3u", "E4", "E5", "E8", "E9c")

KERNEL_FAMILIES = {"small", "resident", "resident2", "resident-tag", "resident-lds", "stream_kernel", "stream2_kernel",
                   "stream3_kernel", "sweep_kernel", "pivot_kernel", "generic", "batch_kernel", "shard-hip", "shard-native",
                   "shard-rccl", "wide_kernel", "dshard_kernel", "dsweep_kernel"}


def _records(shape, check_ok, families=None, min_pivots=0):
    return [r for r in G.records("edges") if (r["M"], r["N"]) == shape and (check_ok or not r["options"]["checkCycles"])
            and (families is None or r["family"] in families) and r["n_pivots"] >= min_pivots]


CASES = [pytest.param(name, rec, id="%s-%s" % (name, E.label(rec))) for name, (_, shape, _, _, ck) in PATHS.items()
         for rec in _records(shape, ck)]
SHARD_CASES = [pytest.param(name, rec, id="%s-%s" % (name, E.label(rec))) for name, (_, _, _, shape, _, _, _, least) in SHARDS.items()
               for rec in _records(shape, True, SHARD_FAMILIES, least)]


# the family R (tests/_rounding.py, tests/golden/simplex_rounding_edges.json.gz): runs that end "optimal" with the result -0 (or
# NaN: precision 3.0) after 0, 1 and many pivots, through the same two tables; the row shards run R0, R1 and Rn
R_SHARD_FAMILIES = ("R0", "R1", "Rn")


def _r_records(shape, families=None, min_pivots=0):
    return [r for r in G.records("rounding_edges") if (r["M"], r["N"]) == shape and (families is None or r["family"] in families)
            and r["n_pivots"] >= min_pivots]


R_CASES = [pytest.param(name, rec, id="%s-%s" % (name, E.label(rec))) for name, (_, shape, _, _, _) in PATHS.items()
           for rec in _r_records(shape)]
R_SHARD_CASES = [pytest.param(name, rec, id="%s-%s" % (name, E.label(rec))) for name, (_, _, _, shape, _, _, _, least) in SHARDS.items()
                 for rec in _r_records(shape, R_SHARD_FAMILIES, least)]


def test_path_table_runs_the_rounding_family_on_every_row():
    """Every path and every shard row has R records with at least as many pivots as the row needs, each of them "optimal"
    with the reference's result -0 (NaN at precision 3.0): the sign of a rounded zero is compared on every kernel path."""
    for name, (_, shape, _, _, _) in PATHS.items():
        recs = _r_records(shape)
        assert {r["family"] for r in recs} == set(RD.R_FAMILIES), name
        assert any(r["n_pivots"] >= 8 for r in recs), name
    for name, (_, _, _, shape, _, _, _, least) in SHARDS.items():
        recs = _r_records(shape, R_SHARD_FAMILIES, least)
        assert recs and any(r["n_pivots"] >= max(least, 8) for r in recs), name
        assert least > 0 or {r["family"] for r in recs} == set(R_SHARD_FAMILIES), name
    for p in R_CASES + R_SHARD_CASES:
        rec = p.values[1]
        assert rec["status"] == "optimal" and rec["result_hex"] in (RD.hexd(-0.0), RD.hexd(float("nan"))), p.id
        assert (rec["result_hex"] == RD.hexd(float("nan"))) == (rec["family"] == "R1n"), p.id


def test_path_table_names_every_kernel_family():
    """Dropping a path from the tables (or its every record) fails here, whatever else runs."""
    assert {v[0] for v in PATHS.values()} | {v[0] for v in SHARDS.values()} == KERNEL_FAMILIES
    for name, (_, shape, _, _, ck) in PATHS.items():
        assert _records(shape, ck), name
    for name, (_, _, _, shape, _, _, _, least) in SHARDS.items():
        assert _records(shape, True, SHARD_FAMILIES, least), name
    assert {v[2] for v in SHARDS.values()} == {1, 2, 3}
    assert {v[1] for v in SHARDS.values()} == {"hip", "hip-native", "hip-rccl"}
    assert all((v[0] == "dsweep_kernel") == (v[6] == "launch") for v in SHARDS.values())


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    assert _native.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return _native


def _matches(key, got, want):
    """A full kernel name must be met exactly, except the resident kernel's (info adds its loop's details); a name without
    template arguments (stream_kernel) is a prefix; a tuple lists the alternatives."""
    if isinstance(want, tuple):
        return any(_matches(key, got, w) for w in want)
    if key == "launched":
        return got == want
    if key == "resident" or not want.endswith(">"):
        return got.startswith(want)
    return got == want


def _compare(rec, status, result, npiv, matrix, pos, var):
    exp = G.expected(rec)
    assert (status, npiv) == (exp["status"], exp["n_pivots"]), (status, npiv, exp["status"], exp["n_pivots"])
    assert G.same_number(result, exp["result"]), (result, exp["result"])
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
    assert E.col0_matches(matrix, rec, exp)
    assert G.sha256(matrix) == exp["final_sha256"]


def _run_on_path(nat, monkeypatch, name, rec, initial):
    """The record's tableau (initial(rec, dense_lp)) through the path `name`: asserts the kernel, returns what _compare takes."""
    _, _, env, want, _ = PATHS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from tests import _oracle
    m = initial(rec, _oracle.load().dense_lp)
    w, h = rec["width"], rec["height"]
    pos, var = G.identity_perms(rec)
    o = G.options(rec)
    ctx = nat.Context(0)
    try:
        if want is None:  # NodeBatch: the root tableau with no cut is the node
            batch = nat.NodeBatch(ctx, w, h, 2, 1)
            try:
                batch.set_root(m, pos, var)
                st, res, piv, heights, _ = batch.solve([()], o["precision"], o["max_pivots"])
                assert int(heights[0]) == h
                got, col0, gpos, gvar = batch.download(0, h, matrix=True)
            finally:
                batch.close()
            status, result, npiv = st[0], float(res[0]), int(piv[0])
            assert np.array_equal(col0.view(np.int64), got.reshape(h, w)[:, 0].view(np.int64))
        else:
            t = nat.DeviceTableau(ctx, w, h)
            try:
                t.upload(m, h, pos, var)
                status, result, npiv, _ = t.solve(**o)
                info = t.info()
                got, gpos, gvar = t.download()
            finally:
                t.close()
            for k, v in want.items():
                v = v[o["check_cycles"]] if k == "launched" else v
                assert _matches(k, info.get(k, ""), v), (k, v, info)
    finally:
        ctx.close()
    return status, result, npiv, got, gpos, gvar


@pytest.mark.parametrize("name,rec", CASES)
def test_edge_record_on_path(nat, monkeypatch, name, rec):
    _compare(rec, *_run_on_path(nat, monkeypatch, name, rec, E.initial))


@pytest.mark.parametrize("name,rec", R_CASES)
def test_rounding_record_on_path(nat, monkeypatch, name, rec):
    """test_edge_record_on_path on the family R, and the result word for word: -0 is not +0."""
    out = _run_on_path(nat, monkeypatch, name, rec, RD.r_initial)
    _compare(rec, *out)
    assert RD.hexd(out[1]) == rec["result_hex"], (out[1], rec["result_hex"])


def _run_on_row_shards(tmp_path, monkeypatch, name, rec, initial):
    from tests import _oracle
    from tests.test_sharded import run_world
    _, kind, world, _, env, kernel, sweep, _ = SHARDS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = initial(rec, _oracle.load().dense_lp)
    path = str(tmp_path / "edge.npy")
    np.save(path, m)
    o = G.options(rec)
    spec = "npy:" + path + (":check" if o["check_cycles"] else "") + ":precision=%r" % o["precision"]
    res = run_world(kind, world, rec["M"], rec["N"], 0, tmp_path, [o["max_pivots"], spec])
    assert str(res["kernel"]).startswith(kernel), (str(res["kernel"]), kernel)
    assert str(res["shard_sweep"]) == sweep, (str(res["shard_sweep"]), sweep)
    _compare(rec, str(res["status"]), float(res["result"]), int(res["pivots"]), res["matrix"], res["pos"], res["var"])
    os.remove(path)
    return float(res["result"])


@pytest.mark.parametrize("name,rec", SHARD_CASES)
def test_edge_record_on_row_shards(tmp_path, monkeypatch, name, rec):
    """tests/_shard_worker.py with the record's tableau (`npy:`), precision, checkCycles and pivot budget."""
    _run_on_row_shards(tmp_path, monkeypatch, name, rec, E.initial)


@pytest.mark.parametrize("name,rec", R_SHARD_CASES)
def test_rounding_record_on_row_shards(tmp_path, monkeypatch, name, rec):
    """test_edge_record_on_row_shards on the family R, and the result word for word."""
    result = _run_on_row_shards(tmp_path, monkeypatch, name, rec, RD.r_initial)
    assert RD.hexd(result) == rec["result_hex"], (result, rec["result_hex"])

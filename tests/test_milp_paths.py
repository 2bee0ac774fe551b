"""Every branch-and-cut node path on the MILP records (tests/golden/simplex_milp.json.gz, tests/_milps.py).  Every recorded
node goes through DeviceTableau.node_solve: LDS-sized roots on small_kernel, roots of 128 KB .. 4 MB fused and call by
call, checkCycles call by call, the root over 4 MB next to its resident root.  Every node without checkCycles goes through
NodeBatch (LDS and HBM switch settings).  Then every model runs through yalps_milp_f64 with node_batch 0 and 32, through
solve()'s native and Python drivers, and a subset through napi/yalps.js under node.  Every node must match the
reference's node bit for bit; every flow must consume the recorded number of nodes and return the recorded best tableau
and Solution."""
import numpy as np
import pytest

from tests import _bnc as B
from tests import _golden as G
from tests import _milps as ML
from tests.test_milp_records import marshal, options
from yalps_amd import model as M
from yalps_amd import solve as S

pytestmark = pytest.mark.gpu

RECORDS = G.records("milp")
WITH_NODES = [r for r in RECORDS if r["nodes"]]


def _id(rec):
    return ML.label(rec["family"], rec["seed"], rec["variant"])


def _lds(rec):
    return 8 * rec["width"] * rec["height"] < 128 << 10


# name -> (records, switches, what info() must show after each node: last_path, and whether node_fused_runs grows)
NODE_PATHS = {
    "small": ([r for r in WITH_NODES if _lds(r) and not r["options"].get("checkCycles")], {}, ("small", False)),
    "small-checkcycles": ([r for r in WITH_NODES if _lds(r) and r["options"].get("checkCycles")], {}, ("small", False)),
    "fused": ([r for r in WITH_NODES if r["family"] == "mid" and not r["options"].get("checkCycles")], {}, ("resident", True)),
    # the root over 4 MB: whichever kernel the node's shape takes, the node is solved next to the resident root
    "resident-root-4mb": ([r for r in WITH_NODES if r["family"] == "big"], {}, (None, None)),
    "call-by-call": ([r for r in WITH_NODES if not _lds(r) and r["family"] == "mid" and not r["options"].get("checkCycles")],
                     {"YALPS_HIP_NODE_FUSED": "0"}, (None, False)),
    "call-by-call-checkcycles": ([r for r in WITH_NODES if not _lds(r) and r["options"].get("checkCycles")], {}, (None, False)),
}
NODE_CASES = [pytest.param(name, rec, id="%s-%s" % (name, _id(rec))) for name, (recs, _, _) in NODE_PATHS.items() for rec in recs]
# (record, in LDS): the nodes of LDS-sized roots both ways, the others in HBM only (they take it either way)
BATCH_CASES = [pytest.param(rec, lds, id="%s-%s" % (_id(rec), "lds" if lds else "hbm")) for rec in WITH_NODES
               if not rec["options"].get("checkCycles") and 8 * rec["width"] * rec["height"] <= S.NODE_BATCH_MAX_BYTES
               for lds in ((True, False) if _lds(rec) else (False,))]


def test_node_path_table():
    """Every record with nodes goes through node_solve on some path."""
    assert all(recs for recs, _, _ in NODE_PATHS.values())
    assert {id(r) for recs, _, _ in NODE_PATHS.values() for r in recs} == {id(r) for r in WITH_NODES}
    assert {p.values[1] for p in BATCH_CASES} == {True, False} and any(not _lds(p.values[0]) for p in BATCH_CASES)


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    assert _native.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return _native


def _model(rec):
    tm = M.tableau_model(ML.make(rec["family"], rec["seed"], rec["variant"])[0])
    assert G.sha256(tm.tableau.matrix) == rec["init_sha256"]
    return tm


def _check_node(i, node, status, result, matrix, pos, var):
    assert (status, B.hexd(result)) == (node["status"], node["result"]), i
    assert B.sha(pos, var) == node["perm_sha256"], i
    assert G.sha256(matrix) == node["final_sha256"], i


@pytest.mark.parametrize("name,rec", NODE_CASES)
def test_node_solve_replays_every_node(nat, monkeypatch, name, rec):
    """The root solved and kept in HBM, then every recorded node through yalps_tableau_node_solve; the node's whole final
    tableau is downloaded for its SHA-256."""
    _, env, (path, fused) = NODE_PATHS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = _model(rec).tableau
    opt = options(rec)
    ctx = nat.Context(0)
    root = nat.DeviceTableau(ctx, t.width, t.height)
    node = nat.DeviceTableau(ctx, t.width, t.height + 2 * len(rec["integers"]))
    try:
        root.upload(t.matrix, t.height, t.position_of_variable, t.variable_at_position)
        st, res, npiv, _ = root.solve(opt["precision"], opt["maxPivots"], opt["checkCycles"])
        assert (st, B.hexd(res), npiv) == (rec["root"]["status"], rec["root"]["result"], rec["root"]["n_pivots"])
        assert G.sha256(root.download(perms=False)[0]) == rec["root"]["final_sha256"]
        for i, n in enumerate(rec["nodes"]):
            cuts = [(s, v, float(np.frombuffer(bytes.fromhex(x), ">f8")[0])) for s, v, x in n["cuts"]]
            runs = int(node.info().get("node_fused_runs", 0))
            status, result, h, col0, pos, var = node.node_solve(root, cuts, opt["precision"], opt["maxPivots"], opt["checkCycles"])
            info = node.info()
            if fused is not None:
                assert (int(info["node_fused_runs"]) > runs) == fused, (i, info)
            if path is not None:
                assert info["last_path"] == path, (i, info)
            else:
                assert info["last_path"] not in ("small", "none"), (i, info)
            matrix, dpos, dvar = node.download()
            assert h == t.height + len(cuts) and matrix.size == h * t.width
            _check_node(i, n, status, result, matrix, dpos, dvar)
            if status == "optimal":
                assert np.array_equal(pos, dpos) and np.array_equal(var, dvar), i
                assert np.array_equal(col0.view(np.int64), matrix[::t.width].view(np.int64)), i
    finally:
        node.close()
        root.close()
        ctx.close()


@pytest.mark.parametrize("rec,lds", BATCH_CASES)
def test_node_batch_replays_every_node(nat, oracle, monkeypatch, rec, lds):
    """Every recorded node through NodeBatch (batch_kernel), 32 nodes per batch.  lds: as the batch chooses (LDS when a node
    fits); hbm: YALPS_HIP_NO_LDS=1, the HBM workspace.  Pivot counts are compared as well.  Which workspace ran is NOT
    asserted: NodeBatch reports no path (no info() in the C ABI), so the ids name the switch set, as in
    tests/test_edge_paths.py's batch rows."""
    if not lds:
        monkeypatch.setenv("YALPS_HIP_NO_LDS", "1")
    t = _model(rec).tableau
    opt = options(rec)
    st, res, npiv, _ = oracle.simplex(t.matrix, t.width, t.height, t.position_of_variable, t.variable_at_position,
                                      precision=opt["precision"], max_pivots=opt["maxPivots"])
    assert G.sha256(t.matrix) == rec["root"]["final_sha256"]
    nodes = rec["nodes"]
    ctx = nat.Context(0)
    batch = nat.NodeBatch(ctx, t.width, t.height, 2 * len(rec["integers"]), 32)
    try:
        batch.set_root(t.matrix, t.position_of_variable, t.variable_at_position)
        for lo in range(0, len(nodes), 32):
            chunk = nodes[lo:lo + 32]
            cut_lists = [tuple((s, v, float(np.frombuffer(bytes.fromhex(x), ">f8")[0])) for s, v, x in n["cuts"]) for n in chunk]
            st, res, piv, heights, _ = batch.solve(cut_lists, opt["precision"], opt["maxPivots"])
            for k, n in enumerate(chunk):
                assert int(piv[k]) == n["n_pivots"], (lo + k, int(piv[k]), n["n_pivots"])
                matrix, col0, pos, var = batch.download(k, int(heights[k]), matrix=True)
                _check_node(lo + k, n, st[k], float(res[k]), matrix, pos, var)
    finally:
        batch.close()
        ctx.close()


@pytest.mark.parametrize("node_batch", [0, 32])
@pytest.mark.parametrize("rec", [pytest.param(r, id=_id(r)) for r in RECORDS])
def test_native_driver_reproduces_the_record(nat, rec, node_batch):
    """yalps_milp_f64: status, result bits, the best tableau's column 0 and basis, and the nodes it consumed."""
    t = _model(rec).tableau
    o = options(rec)
    status, result, height, col0, pos, var, stats = nat.milp(
        t.matrix, t.width, t.height, t.position_of_variable, t.variable_at_position, rec["integers"], rec["sign"],
        precision=o["precision"], max_pivots=o["maxPivots"], check_cycles=o["checkCycles"], tolerance=o["tolerance"],
        timeout=o["timeout"], max_iterations=o["maxIterations"], node_batch=node_batch)
    best = rec["best"]
    assert (status, B.hexd(result), height) == (best["status"], best["result"], best["height"])
    assert (B.sha(col0), B.sha(pos, var)) == (best["col0_sha256"], best["perm_sha256"])
    assert stats["nodes_used"] == rec["iterations"]


@pytest.mark.parametrize("flow", ["native", "python-device", "python-batched"])
@pytest.mark.parametrize("rec", [pytest.param(r, id=_id(r)) for r in RECORDS])
def test_solve_reproduces_the_solution(nat, rec, flow):
    """solve() through yalps_milp_f64 (node_batch 32), the Python one-node-at-a-time driver (the device driver for roots
    over 128 KB) and the batched Python driver: the recorded Solution exactly (names, order, value bits)."""
    model = ML.make(rec["family"], rec["seed"], rec["variant"])[0]
    kw = {"native": dict(), "python-device": dict(native=False, node_batch=0), "python-batched": dict(native=False, node_batch=32)}[flow]
    assert marshal(S.solve(model, rec["options"], **kw)) == rec["solution"]
    if "solution_flip" in rec:
        flipped = dict(rec["options"], includeZeroVariables=not rec["options"].get("includeZeroVariables", False))
        assert marshal(S.solve(model, flipped, **kw)) == rec["solution_flip"]


# napi/yalps.js under node: every family's Solution marshalling in JS (precision 0, timedout with and without a result,
# includeZeroVariables both ways, a root of 128 KB .. 4 MB), with the addon's yalps_milp_f64 underneath
JS_SUBSET = ("ties-s0", "integral-s2", "iters-s0-i5", "iters-s2-i7", "eqmm-s0", "timeout0-s0", "intinf-s1", "negzero-s3",
             "mid-s0", "full-s437")
JS_DRIVER = r"""
"use strict"
const { solve } = require(process.argv[2])
const hexd = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x, 0); return b.toString("hex") }
const job = JSON.parse(require("fs").readFileSync(0, "utf-8"))
const s = solve(job.model, job.options, job.nodeBatch)
console.log(JSON.stringify({ status: s.status, result: hexd(s.result), variables: s.variables.map(([k, v]) => [k, hexd(v)]) }))
"""


def test_js_subset_is_recorded():
    assert set(JS_SUBSET) <= {_id(r) for r in RECORDS}


@pytest.mark.parametrize("node_batch", [0, 32])
@pytest.mark.parametrize("rec", [pytest.param(r, id=_id(r)) for r in RECORDS if _id(r) in JS_SUBSET])
def test_yalps_js_reproduces_the_solution(nat, tmp_path, rec, node_batch):
    """yalps.js `solve(model, options, nodeBatch)` (model -> tableau in JS, solveInteger = yalps_milp_f64 in the addon,
    solution() in JS): the recorded Solution exactly, value bits printed by the driver."""
    import json
    import os
    import shutil
    import subprocess
    from yalps_amd import build
    assert shutil.which("node") is not None, "node is needed for the napi tests on the GPU machine"
    build.build_hip()
    assert build.build_napi() is not None
    driver = tmp_path / "solve_hex.js"
    driver.write_text(JS_DRIVER)
    yalps_js = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yalps_amd", "napi", "yalps.js")
    model = ML.make(rec["family"], rec["seed"], rec["variant"])[0]
    for key, opts in (("solution", rec["options"]),
                      ("solution_flip", dict(rec["options"], includeZeroVariables=not rec["options"].get("includeZeroVariables", False)))):
        if key not in rec:
            continue
        out = subprocess.run(["node", str(driver), yalps_js], input=json.dumps({"model": model, "options": opts, "nodeBatch": node_batch}),
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert json.loads(out.stdout.strip().splitlines()[-1]) == rec[key], key

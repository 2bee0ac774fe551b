"""Every device path on the non-finite records (tests/_nonfinite.py, tests/golden/simplex_nonfinite.json.gz): NaN and
infinite tableau entries, overflow from finite input, NaN bit patterns (the kernels' own FLUSHED marker among them) and
options that are not finite.  The path tables are those of tests/test_edge_paths.py: each path asserts the kernel it
expects before status, pivot count, result, basis, column 0 and the SHA-256 of the whole final tableau are compared with
the reference's record -- bit for bit once all NaNs are made one value (arithmetic NaNs get the sign and payload of the
unit that made them)."""
import os

import numpy as np
import pytest

from tests import _golden as G
from tests import _nonfinite as NF
from tests.test_edge_paths import PATHS, SHARDS, _matches

pytestmark = pytest.mark.gpu

SHARD_FAMILIES = ("N1", "N2", "N3", "N6")
# the paths on which the host splits the pivot budget into launches: the options of N7 reach the host's loop as well
N7_PATHS = ("small", "resident-gen1", "resident-gen2", "stream", "stream3-j4", "pivot-256-2-8", "generic-forced")


def _records(shape, families, min_pivots=0):
    return [r for r in G.records("nonfinite") if (r["M"], r["N"]) == shape and r["family"] in families
            and r["n_pivots"] >= min_pivots]


def _families(name):
    return tuple(f for f in NF.FAMILIES if f != "N7" or name in N7_PATHS)


CASES = [pytest.param(name, rec, id="%s-%s" % (name, NF.label(rec))) for name, (_, shape, _, _, _) in PATHS.items()
         for rec in _records(shape, _families(name))]
SHARD_CASES = [pytest.param(name, rec, id="%s-%s" % (name, NF.label(rec))) for name, (_, _, _, shape, _, _, _, least) in SHARDS.items()
               for rec in _records(shape, SHARD_FAMILIES, least)]


def test_every_path_has_records_of_the_partition_families():
    """tests/test_edge_paths.py's rule: a path without records fails here.  Every row runs N1, N2 and N6 at least."""
    for name, (_, shape, _, _, _) in PATHS.items():
        assert set(NF.PARTITION_FAMILIES) <= {r["family"] for r in _records(shape, _families(name))}, name
    for name, (_, _, _, shape, _, _, _, least) in SHARDS.items():
        assert set(NF.PARTITION_FAMILIES) <= {r["family"] for r in _records(shape, SHARD_FAMILIES, least)}, name
    for name in N7_PATHS:
        assert len(_records(PATHS[name][1], ("N7",))) == 10, name


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import _native
    assert _native.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return _native


def _compare(rec, status, result, npiv, matrix, pos, var):
    exp = G.expected(rec)
    assert (status, npiv) == (exp["status"], exp["n_pivots"]), (status, npiv, exp["status"], exp["n_pivots"])
    assert G.same_number(result, exp["result"]), (result, exp["result"])
    assert np.array_equal(pos, exp["pos"]) and np.array_equal(var, exp["var"])
    assert NF.col0_matches(matrix, rec, exp)
    assert G.sha256_canon(matrix) == exp["final_canon_sha256"]


@pytest.mark.parametrize("name,rec", CASES)
def test_nonfinite_record_on_path(nat, monkeypatch, name, rec):
    _, _, env, want, _ = PATHS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from tests import _oracle
    m = NF.initial(rec, _oracle.load().dense_lp)
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
            assert np.array_equal(G.canon(col0).view(np.int64), G.canon(got.reshape(h, w)[:, 0]).view(np.int64))
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
    _compare(rec, status, result, npiv, got, gpos, gvar)


@pytest.mark.parametrize("name,rec", SHARD_CASES)
def test_nonfinite_record_on_row_shards(tmp_path, monkeypatch, name, rec):
    """tests/_shard_worker.py with the record's tableau (`npy:`), precision and pivot budget."""
    from tests import _oracle
    from tests.test_sharded import run_world
    _, kind, world, _, env, kernel, sweep, _ = SHARDS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = NF.initial(rec, _oracle.load().dense_lp)
    path = str(tmp_path / "nonfinite.npy")
    np.save(path, m)
    o = G.options(rec)
    spec = "npy:" + path + ":precision=%r" % o["precision"]
    res = run_world(kind, world, rec["M"], rec["N"], 0, tmp_path, [o["max_pivots"], spec])
    assert str(res["kernel"]).startswith(kernel), (str(res["kernel"]), kernel)
    assert str(res["shard_sweep"]) == sweep, (str(res["shard_sweep"]), sweep)
    _compare(rec, str(res["status"]), float(res["result"]), int(res["pivots"]), res["matrix"], res["pos"], res["var"])
    os.remove(path)


# ---- resident2_kernel on tiny tableaux: every instantiation (tests/test_resident2_slots.py forces them) -------------------

def _canon_same(got, exp):
    assert (got["status"], got["pivots"]) == (exp["status"], exp["pivots"]) and G.same_number(got["result"], exp["result"])
    assert np.array_equal(got["pos"], exp["pos"]) and np.array_equal(got["var"], exp["var"])
    assert np.array_equal(G.canon(got["matrix"]).view(np.int64), G.canon(exp["matrix"]).view(np.int64))


_TINY = {}


def tiny_reference(oracle, family, M, N):
    """One tableau and one oracle run per (family, shape), shared by the instantiations of that height."""
    from tests.test_resident2_slots import reference
    key = (family, M, N)
    if key not in _TINY:
        m = NF.make(family, M, N, NF.SEED, dense_lp=oracle.dense_lp)
        _TINY[key] = (m, reference(oracle, m, N + 1, M + 1, max_pivots=60.0))
    return _TINY[key]


@pytest.mark.parametrize("family", NF.PARTITION_FAMILIES)
@pytest.mark.parametrize("variant", [(256, 1, 4), (256, 1, 9), (256, 2, 4), (512, 2, 4), (512, 2, 6), (512, 2, 9), (512, 3, 4)],
                         ids=lambda v: "%d-%d-%d" % v)
def test_resident2_instantiations_on_tiny_tableaux(nat, oracle, monkeypatch, variant, family):
    """The dense path, the general path and the slot-vector candidate row carry NaN, the FLUSHED bits and infinities through
    a register-relative move: rows_for(R) x 37, four workgroups, against the oracle."""
    from tests.test_resident2_slots import RESIDENT2, rows_for, solve_on
    assert variant in RESIDENT2
    M, N = rows_for(variant[2]), 37
    m, exp = tiny_reference(oracle, family, M, N)
    assert exp["pivots"] >= 1 and not np.isfinite(m).all()
    _canon_same(solve_on(nat, monkeypatch, variant, m, N + 1, M + 1, max_pivots=60.0), exp)


# ---- the queue kernels (wg_queue): lp_batch_kernel, lp_variants_kernel, milp_node_kernel ---------------------------------

def class_lps(oracle, w, h, families=NF.FAMILIES):
    """[(label, LP)] of the families at one shape, checkCycles off and on (N7: its ten variants)."""
    from tests import _lp_batch as LB
    M, N = h - 1, w - 1
    out = []
    for check in (False, True):
        for f in families:
            for seed in (range(NF.SEED, NF.SEED + 10) if f == "N7" else (NF.SEED,)):
                o = NF.options(f, M, N, seed)
                m = NF.make(f, M, N, seed, dense_lp=oracle.dense_lp)
                out.append(("%s-s%d%s" % (f, seed, "-check" if check else ""),
                            LB.from_dense(m, w, h, o["precision"], o["max_pivots"], check)))
    return out


_ANSWERS = {}


def class_answers(oracle, w, h, families=NF.FAMILIES):
    from tests import _lp_batch as LB
    key = (w, h, families)
    if key not in _ANSWERS:
        lps = class_lps(oracle, w, h, families)
        _ANSWERS[key] = (lps, [LB.oracle_answer(oracle, lp) for _, lp in lps])
    return _ANSWERS[key]


def _planted_something(lps, refs):
    """The LPs of a class meet what they plant: some input and some final tableau are not finite, some pivots were made."""
    from tests import _lp_batch as LB
    assert any(not np.isfinite(lp[4]).all() for _, lp in lps)
    assert any(not np.isfinite(r["matrix"]).all() for r in refs) and sum(r["n_pivots"] for r in refs) >= len(refs)


QUEUE_SHAPES = [(31, 31), (8, 300), (80, 97), (121, 131), (281, 301)]  # tests/test_lp_warm.py CLASS_SHAPES
AUX_SHAPE = (8152, 41)


@pytest.mark.parametrize("w,h", QUEUE_SHAPES + [AUX_SHAPE], ids=lambda x: str(x))
def test_lp_batch_kernel_on_nonfinite_lps(nat, oracle, w, h):
    from tests import _batch_shapes as BS
    from tests import _lp_batch as LB
    from tests.test_lp_warm import CLASS_SHAPES
    assert tuple(QUEUE_SHAPES) == tuple(CLASS_SHAPES)
    aux = (w, h) == AUX_SHAPE
    assert aux == (LB.size_class(w, h) == 4 and BS.aux_hbm(w, h))
    lps, refs = class_answers(oracle, w, h, ("N1", "N6") if aux else NF.FAMILIES)
    _planted_something(lps, refs)
    b = nat.LpBatch(0)
    try:
        out = b.solve([lp for _, lp in lps], keep_tableaux=True)
        info = b.info()
        cls = LB.size_class(w, h)
        assert {(k["class"], "check" in k["kernel"]) for k in info["kernels"]} == {(cls, False), (cls, True)}, info["text"]
        for i, ((label, lp), ref) in enumerate(zip(lps, refs)):
            LB.check_lp(b, i, out, ref, lp, label=label, canonical_nan=True)
    finally:
        b.close()


@pytest.mark.parametrize("w,h", QUEUE_SHAPES + [AUX_SHAPE], ids=lambda x: str(x))
def test_lp_variants_kernel_patches_in_the_nonfinite_cells(nat, oracle, w, h):
    """The same LPs as variants of a finite base: the patch carries the NaN and infinite cells."""
    from tests import _lp_batch as LB
    from tests import _variant_shapes as VS
    aux = (w, h) == AUX_SHAPE
    lps, refs = class_answers(oracle, w, h, ("N1", "N6") if aux else NF.FAMILIES)
    base = LB.dense_lp(oracle, h - 1, w - 1, NF.SEED)
    assert np.isfinite(base[4]).all()
    targets = [lp for _, lp in lps]
    lv = nat.LpVariants(0)
    try:
        out = lv.solve(VS.packed_group(nat, base, targets), keep_tableaux=True)
        assert all(k["kernel"].startswith("lp_variants_kernel<") for k in lv.info()["kernels"]), lv.info()["text"]
        for i, ((label, lp), ref) in enumerate(zip(lps, refs)):
            LB.check_lp(lv, i, out, ref, lp, label=label, canonical_nan=True)
    finally:
        lv.close()


def test_milp_node_kernel_from_a_root_with_nan(nat, oracle):
    """One node without a cut and one with one cut from an N1 root: milp_node_kernel starts from the root tableau the root
    pass left on the device, NaN included.  The reference node: tests/_batch_shapes.py::node_reference."""
    import types
    from tests import _batch_shapes as BS
    from tests import _bnc as BN
    from tests import _lp_batch as LB
    M, N = 30, 30
    w, h = N + 1, M + 1
    m = NF.make("N1", M, N, NF.SEED, dense_lp=oracle.dense_lp)
    lp = LB.from_dense(m, w, h, 1e-8, 60.0, False)
    ref = LB.oracle_answer(oracle, lp)
    assert ref["status"] == "optimal" and ref["n_pivots"] >= 3 and np.isnan(ref["matrix"]).any()
    root = types.SimpleNamespace(w=w, h=h, matrix=ref["matrix"], pos=ref["pos"], var=ref["var"],
                                 opt=dict(precision=1e-8, maxPivots=60.0, checkCycles=False))
    basic = next(v for v in range(1, w) if root.pos[v] >= w and np.isfinite(root.matrix[(root.pos[v] - w) * w]))
    cut_lists = [[], [(1, basic, float(np.floor(root.matrix[(root.pos[basic] - w) * w])))]]
    b = nat.MilpBatch(0)
    try:
        st, res, piv = b.roots([lp])
        assert (st[0], int(piv[0])) == (ref["status"], ref["n_pivots"]) and G.same_number(float(res[0]), ref["result"])
        _, rpos, rvar, rm = b.root(0, matrix=True)
        assert LB.same_words(rm, ref["matrix"], canonical_nan=True) and np.array_equal(rpos, ref["pos"]) and np.array_equal(rvar, ref["var"])
        statuses, results, pivots, heights = b.nodes([0, 0], cut_lists, keep_tableaux=True)
        assert all(k["kernel"].startswith("milp_node_kernel<") for k in b.info()["kernels"]), b.info()["text"]
        worked = 0
        for k, cuts in enumerate(cut_lists):
            node, _ = BS.node_reference(oracle, root, cuts)
            want, hh, wpos, wvar = BN._apply_cuts(root.matrix, w, h, root.pos, root.var, cuts)  # (node_reference keeps digests only)
            oracle.simplex(want, w, hh, wpos, wvar, precision=1e-8, max_pivots=60.0)
            assert BN.sha(want) == node["final_sha256"] and BN.sha(wpos, wvar) == node["perm_sha256"]
            assert (statuses[k], int(pivots[k]), int(heights[k])) == (node["status"], node["n_pivots"], node["height"]), (k, statuses[k], node)
            assert BS.bits(float(results[k])) == node["result"]
            col0, pos, var = b.node(k)
            assert BN.sha(pos, var) == node["perm_sha256"]
            got = b.node_tableau(k)
            assert LB.same_words(got, want, canonical_nan=True) and LB.same_words(col0, want[::w][:hh], canonical_nan=True)
            worked += node["n_pivots"]
        assert worked >= 1  # (the cut makes the node pivot)
    finally:
        b.close()


# ---- lp_warm: non-finite deltas in the fill, at the C ABI ------------------------------------------------------------

def warm_patches(base, b0, w, h):
    """{label: patch} with the values +inf, -inf and NaN on a basic and a non-basic slack, a basic and a non-basic variable,
    and on a column 0 cell and a row 0 cell that meet (tests/test_lp_warm.py::fill_patches picks the same records)."""
    import math
    F, pos = base["matrix"].reshape(h, w), base["pos"]
    slack_nb = [r for r in range(1, h) if pos[w + r] < w]
    slack_b = [r for r in range(1, h) if pos[w + r] >= w]
    var_nb = [c for c in range(1, w) if pos[c] < w]
    var_b = [c for c in range(1, w) if pos[c] >= w]
    meet = next((c, r) for c in var_b for r in slack_nb if F[pos[c] - w, pos[w + r]] != 0.0)
    sites = {"non-basic slack": [slack_nb[-1] * w], "basic slack": [slack_b[0] * w], "non-basic variable": [var_nb[0]],
             "basic variable": [var_b[-1]], "column 0 and row 0 meet": [meet[0], meet[1] * w]}
    return {"%s %r" % (name, v): sorted((k, v) for k in cells) for name, cells in sites.items() for v in (math.inf, -math.inf, math.nan)}


@pytest.mark.parametrize("w,h", [(31, 31), (281, 301)], ids=lambda x: str(x))
def test_lp_warm_fill_with_nonfinite_deltas(oracle, w, h):
    import math
    from yalps_amd import _native
    from tests import _lp_batch as LB
    from tests import _np_warm as NW
    from tests.test_lp_warm import base_of
    lp, base, b0 = base_of(oracle, w, h)
    patches = warm_patches(base, b0, w, h)
    assert len(patches) == 15
    names = list(patches)
    lw = _native.LpWarm(0)
    try:
        for budget in (0.0, 8192.0):
            out = lw.solve(NW.packed_cells(_native, lp, [patches[k] for k in names], [(1e-8, budget, False)] * len(names),
                                           base_options=(1e-8, math.inf, False)), keep_tableaux=True)
            assert out is not None and lw.base[0] == "optimal" and lw.base[2] == base["n_pivots"], lw.base
            cls = LB.size_class(w, h)
            assert {k["kernel"] for k in lw.info()["kernels"]} == {NW.kernel_of(cls, False)}, lw.info()["text"]
            for i, name in enumerate(names):
                ref = NW.warm_answer(oracle, base, w, h, b0, patches[name], max_pivots=budget)
                assert not np.isfinite(ref["start"]).all(), name
                if budget == 0.0:  # the kept matrix is the warm tableau itself
                    assert ref["n_pivots"] == 0 and LB.same_words(ref["matrix"], ref["start"].reshape(-1), canonical_nan=True), name
                LB.check_lp(lw, i, out, ref, lp, label="%s, budget %g" % (name, budget), canonical_nan=True)
    finally:
        lw.close()

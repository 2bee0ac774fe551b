"""lp_variants_kernel (libyalps_lpvar.so) at the shapes, patch lengths and queue states tests/test_lp_variants.py does not reach
(tests/_variant_shapes.py holds the helpers and the groups).  Any LP is base + patch -- the patch being the cells whose words
differ between the dense base and the dense target -- so the tables written for lp_batch_kernel run through this kernel as
they are: both sides of every class bound at both parities of n, the 73 LPs of tests/_batch_shapes.py::shape_table grouped by
shape, the edge families of tests/_edges.py as variants of the dense LP they are planted into; a base without cells (the patch
is the whole tableau: every kernel spelling's patch loop takes more than four trips), patch arrays with junk in front
(patch_offsets[0] > 0), the HBM and the aux form's workgroups taking four variants each with history reruns, info()'s second
call, a handle on a caller's stream.

Every expectation is the C oracle's answer on the dense target; every comparison is bit for bit (tests/_lp_batch.py::check_lp).
What the groups cover is counted and asserted (test_what_the_groups_cover), and the inputs are shown to tell five wrong start
tableaux from the right one (test_the_inputs_tell_a_wrong_start_from_the_right_one)."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from tests import _batch_shapes as BS
from tests import _lp_batch as LB
from tests import _lp_variants as V
from tests import _variant_shapes as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPELLINGS = sorted({V.kernel_of(cls, check) for cls in range(5) for check in (False, True)})
TABLE_PARTS = ("lds", "hbm", "aux")


@pytest.fixture(scope="module")
def nat():
    from yalps_amd import build, _native
    build.build_lpvar()
    return _native


@pytest.fixture(scope="module")
def shapes(oracle):
    return BS.shape_table(oracle)


@pytest.fixture(scope="module")
def groups(oracle, shapes):
    """{test: [Group]}, built once."""
    return {"bounds": VS.bound_groups(oracle), "table": VS.table_groups(shapes), "empty base": VS.empty_base_groups(oracle, shapes),
            "edges": VS.edge_groups(oracle), "queue": [VS.queue_group(oracle, w, h) for w, h in VS.QUEUE_SHAPES]}


@pytest.fixture(scope="module")
def answers(oracle):
    """The oracle's answer per (group, variant), computed once; the empty-patch variants of a queue group share the base's."""
    cache = {}

    def of(group, i):
        lp = group.targets[i]
        key = (group.name, "empty patch", lp[7]) if group.name.startswith("queue") and group.labels[i] == "empty patch" else (group.name, i)
        if key not in cache:
            cache[key] = LB.oracle_answer(oracle, lp)
        return cache[key]
    return of


def every(groups):
    return [g for gs in groups.values() for g in gs]


def table_part(group):
    return "aux" if group.aux else "hbm" if group.cls == 4 else "lds"


# ---------------------------------------------------------------------------------------------------------- CPU

def test_diff_patch_rebuilds_every_target(nat, groups):
    assert len(every(groups)) == len({g.name for g in every(groups)})
    leads = 0
    for g in every(groups):
        base = LB.scatter(g.base)
        for i, (t, (row, col, val)) in enumerate(zip(g.targets, g.patches)):
            assert (row.dtype, col.dtype, val.dtype) == (np.int32, np.int32, np.float64), g.name
            assert np.all(np.diff(row.astype(np.int64) * g.w + col) > 0), (g.name, i)
            assert LB.same_words(VS.overwrite(base.copy(), g.w, (row, col, val)), LB.scatter(t)), (g.name, i)
            assert LB.same_words(VS.mutant_start(g, i), LB.scatter(t)), (g.name, i)
        p = g.packed(nat)
        p.validate()
        assert (p.count, p.offsets[0], p.patch_row.size) == (len(g.targets), g.lead, p.offsets[-1])
        if g.lead:
            leads += 1
            p.offsets = p.offsets.copy()
            p.offsets[0] = 0  # (variant 0 now begins with the junk)
            with pytest.raises(nat.NativeError, match="variant 0: patch cell 0 lies outside"):
                p.validate()
            front = VS.junk(g.w, g.h, g.lead)
            key = front[0].astype(np.int64) * g.w + front[1]
            inside = (front[0] >= 0) & (front[0] < g.h) & (front[1] >= 0) & (front[1] < g.w)
            assert (~inside).sum() >= 3 and np.any(np.diff(key[inside]) < 0), g.name  # out of range, and an unsorted run inside
    assert leads == 2
    # a patch of nothing but an explicit +0.0 | -0.0 | a subnormal, as they are
    base = LB.from_dense(np.array([1.0, 2.0, -0.0, 0.0]), 2, 2)
    target = LB.from_dense(np.array([0.0, 2.0, 5e-324, -0.0]), 2, 2)
    row, col, val = VS.diff_patch(base, target)
    assert (list(row), list(col)) == ([0, 1, 1], [0, 0, 1]) and list(VS.words(val)) == [0, 1, np.int64(-2 ** 63)]
    # near_base: seeded, and the same bytes every run
    t = groups["bounds"][0].targets[1]
    a, b = VS.near_base(t, VS.rng_of(9)), VS.near_base(t, VS.rng_of(9))
    assert LB.same_words(LB.scatter(a), LB.scatter(b)) and VS.diff_patch(a, t)[0].size == 48
    e = VS.empty_base(5, 3)
    assert e[2].size == 0 and LB.same_words(LB.scatter(e), np.zeros(15))


def test_what_the_groups_cover(oracle, groups, answers):
    all_groups = every(groups)
    assert {k: len(v) for k, v in groups.items()} == {"bounds": 22, "table": 23, "empty base": 4, "edges": 2, "queue": 2}
    assert sum(len(g.targets) for g in groups["table"]) == 73
    # the patch loop: every kernel spelling gets a patch longer than its lane count and one longer than 4 x its lane count
    longest = Counter()
    for g in all_groups:
        for name, cells in g.kernels().items():
            longest[name] = max(longest[name], cells)
    assert sorted(longest) == SPELLINGS
    for name in SPELLINGS:
        T = 1024 if "<1024" in name else 256
        assert longest[name] > 4 * T, (name, longest[name])
    # classes, checkCycles, parities
    seen = {(g.cls, c) for g in all_groups for c in g.checks()}
    assert seen == {(cls, c) for cls in range(5) for c in (False, True)}
    for cls in range(5):
        assert {g.h % 2 for g in all_groups if g.cls == cls} == {0, 1}, cls
        assert {(g.w - 1) % 2 for g in all_groups if g.cls == cls} == {0, 1}, cls
    assert {(g.w - 1) % 2 for g in all_groups if g.aux} == {0, 1}
    assert {g.aux for g in all_groups if g.cls == 4} == {False, True}
    # both sides of every class bound, at both widths
    for k, w in BS.BOUND_WIDTHS.items():
        h0 = BS.rows_under(LB.BOUNDS[k], w)
        for ww in (w, w - 1):
            assert (LB.size_class(ww, h0), LB.size_class(ww, h0 + 1)) == (k, k + 1), (k, ww)
    assert [BS.rows_under(LB.BOUNDS[k], w) for k, w in sorted(BS.BOUND_WIDTHS.items())] == [47, 70, 98, 134]
    # the largest LDS shape: the one-run image copy ends in colbuf[0] (h odd: the image's closing zero), or exactly at it
    assert {g.h for g in groups["bounds"] if g.cls == 3 and LB.size_class(g.w, g.h + 1) == 4} == {134, 123}
    # a base without cells, patch arrays with a lead
    assert all(g.base[2].size == 0 for g in groups["empty base"]) and {g.cls for g in groups["empty base"]} == {0, 3, 4}
    assert {g.aux for g in groups["empty base"]} == {False, True}
    assert sorted(g.name for g in all_groups if g.lead) == sorted(VS.LEAD_GROUPS) and VS.LEAD == 7
    assert {g.cls for g in all_groups if g.lead} == {0, 4}
    # near_base: every kind of disturbed cell the targets admit (a dense LP's only zero is its cell (0, 0): it is "added", and
    # no zero is left to flip; the hand-made rows of the shape table have zeros of both signs)
    for g in groups["bounds"]:
        assert VS.kinds_between(g.base, g.targets[1]) >= set(VS.KINDS) - {"zero flipped"}, g.name
    kinds = Counter(k for g in groups["table"] for k in VS.kinds_between(g.base, g.targets[0]))
    assert set(kinds) == set(VS.KINDS) and kinds["zero flipped"] >= 3
    explicit_zero = sum(int((VS.words(p[2]) == VS.PLUS_ZERO).sum()) for g in groups["bounds"] + groups["table"] for p in g.patches)
    assert explicit_zero >= len(groups["bounds"])
    # the edge families of one base: the patch is the planted edge, shorter than the tableau unless the family rewrites it (E9)
    for g, (M, N) in zip(groups["edges"], VS.EDGE_SHAPES):
        assert g.labels == list(VS.E.FAMILIES) and (g.w, g.h) == (N + 1, M + 1)
        sizes = dict(zip(g.labels, (p[0].size for p in g.patches)))
        assert all(0 < sizes[f] < g.w * g.h // 2 for f in g.labels if f != "E9") and sizes["E9"] > g.w * g.h // 2, sizes
    assert [g.cls for g in groups["edges"]] == [0, 4]
    # the queue groups: 4 x the grid, heavy (>= 1025 cells, row 0, column 0 and rows among them) and empty in turn, checkCycles
    # alternating between the pairs; the HBM one's info text must outgrow the first buffer of LpVariants.info()
    for g, (w, h) in zip(groups["queue"], VS.QUEUE_SHAPES):
        assert (g.w, g.h, g.cls, len(g.targets)) == (w, h, 4, 4 * VS.QUEUE_GRID)
        assert LB.size_class(w, h - 1) == 3 or BS.aux_hbm(w, h) and not BS.aux_hbm(w, h - 1)
        for i, (row, col, val) in enumerate(g.patches):
            assert g.targets[i][7] == bool((i // 2) % 2)
            if i % 2:
                assert row.size == 0
            else:
                assert row.size >= 1025 and (row == 0).any() and (col == 0).sum() > 1 and len(set(row.tolist())) > 100, (g.name, i)
    hbm, aux = groups["queue"]
    assert not hbm.aux and aux.aux
    refs = [answers(hbm, i) for i in range(len(hbm.targets))]
    assert answers(hbm, 1)["n_pivots"] == 2 ** (hbm.w - 1) - 1 and answers(hbm, 1)["status"] == "optimal"  # (Klee-Minty)
    assert len({r["n_pivots"] for r in refs}) > 8
    must = VS.must_rerun(hbm.targets, refs)
    ids = sum(len(str(i)) + 1 for ids in must for i in ids)
    assert len(must) >= 3 and ids > 4096, (len(must), ids)  # (the ids alone, without the launches' lines)
    # the aux one has a single variable and at most two pivots: no history of 2 must overflow, its queue reuse is what it adds
    refs = [answers(aux, i) for i in range(len(aux.targets))]
    assert max(r["n_pivots"] for r in refs) <= 2 and {r["status"] for r in refs} == {"optimal", "infeasible"}


MUTANT_GROUPS = {"a": ("empty base", "queue"), "b": ("queue",), "c": None, "d": ("bounds",), "e": ("bounds",)}


@pytest.mark.parametrize("mutant", VS.MUTANTS)
def test_the_inputs_tell_a_wrong_start_from_the_right_one(oracle, groups, mutant):
    """The GPU comparison means something only if the inputs react to the mistakes it is there to catch: per mutant and per group
    named for it, the oracle started from the tableau the mistake would leave must end elsewhere than from the right one for at
    least one variant -- (status, pivots, result bits, digest of the final matrix) -- and the unmutated start must not."""
    named = [g for g in every(groups) if g.lead] if mutant == "c" else [g for k in MUTANT_GROUPS[mutant] for g in groups[k]]
    assert named
    for g in named:
        if g.name.startswith("queue"):  # (the first variants a workgroup takes second; heavy ones are every other one)
            members = [L[p] for L in VS.launch_order(g) for p in range(VS.QUEUE_GRID, VS.QUEUE_GRID + 4)] if mutant == "b" else [0, 2, 4, 6]
        else:
            members = range(len(g.targets))
        seen = False
        for i in members:
            lp = g.targets[i]
            right = VS.signature(oracle, LB.scatter(lp), lp)
            assert VS.signature(oracle, VS.mutant_start(g, i), lp) == right, (g.name, i)
            seen = seen or VS.signature(oracle, VS.mutant_start(g, i, mutant), lp) != right
        assert seen, (mutant, g.name)
    if mutant == "e":  # both readings of r * pitch - 1: into the padding | into the last column of the row above
        assert {VS.pitch(g.w, g.h) == g.w - 1 for g in named} == {False, True}
    if mutant == "a":
        assert {V.kernel_of(g.cls, c) for g in named for c in g.checks()} == set(SPELLINGS)


# ---------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu(nat):
    assert nat.lib().yalps_device_count() >= 1, "no HIP device: the GPU tests need a real MI355X"
    return nat


@pytest.fixture(scope="module")
def lv(gpu):
    v = gpu.LpVariants(0)
    yield v
    v.close()


def check_info(info, group, passes=None):
    """What info() says of a group's call against the restatements of _variant_shapes.py: the pass-0 launches (checkCycles off,
    then on), the form, the dynamic LDS, the image, the cell counts."""
    w, h = group.w, group.h
    checks = Counter(group.checks())
    want = [(V.kernel_of(group.cls, c), group.cls, int(group.aux), checks[c], VS.launch_lds(w, h)) for c in (False, True) if checks[c]]
    got = [(k["kernel"], k["class"], k["aux"], k["lps"], k["lds"]) for k in info["kernels"] if k["pass"] == 0]
    assert got == want, (group.name, got, want)
    assert info["image_bytes"] == VS.image_bytes(w, h), (group.name, info["image_bytes"])
    assert info["base_cells"] == group.base[2].size and info["patch_cells"] == sum(p[0].size for p in group.patches), group.name
    if passes == 1:
        assert info["launches"] == len(want) and info["reruns"] == 0 and info["rerun_lps"] == [], (group.name, info["text"])


def run_group(nat, lv, group, answers, tableau=True, passes=1):
    out = lv.solve(group.packed(nat), keep_tableaux=tableau)
    assert len(out[0]) == len(group.targets)
    for i, lp in enumerate(group.targets):
        LB.check_lp(lv, i, out, answers(group, i), lp, tableau=tableau, label="%s: %s" % (group.name, group.labels[i]))
    info = lv.info()
    check_info(info, group, passes)
    return out, info


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(BS.BOUND_WIDTHS))
def test_class_bounds_from_both_sides(gpu, lv, groups, answers, k):
    mine = [(g, hh) for g, (kk, ww, hh) in zip(groups["bounds"], VS.bound_shapes()) if kk == k]
    assert len(mine) == {0: 4, 1: 6, 2: 4, 3: 8}[k]
    for g, h in mine:
        assert g.cls == (k if h <= BS.rows_under(LB.BOUNDS[k], g.w) else k + 1) and g.labels == ["empty patch", "restoring", "rhs below zero", "checkCycles"]
        out, info = run_group(gpu, lv, g, answers)
        assert info["launches"] == 2 and info["reruns"] == 0
        assert [(x["kernel"], x["lps"]) for x in info["kernels"]] == [(V.kernel_of(g.cls, False), 3), (V.kernel_of(g.cls, True), 1)]
        assert g.patches[0][0].size == 0 and g.patches[1][0].size == 48
        assert len({BS.bits(answers(g, i)["result"]) for i in range(4)}) == 4, g.name  # (the patches matter)


@pytest.mark.gpu
@pytest.mark.parametrize("part", TABLE_PARTS)
def test_shape_table_as_variants(gpu, lv, groups, answers, part):
    mine = [g for g in groups["table"] if table_part(g) == part]
    assert mine
    for g in mine:
        run_group(gpu, lv, g, answers)
    assert part != "hbm" or any(g.lead == VS.LEAD for g in mine)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(4))
def test_shape_table_targets_from_an_empty_base(gpu, lv, groups, answers, which):
    g = groups["empty base"][which]
    assert (g.cls, g.aux) == [(0, False), (3, False), (4, False), (4, True)][which] and len(g.targets) == 3
    out, info = run_group(gpu, lv, g, answers)
    assert info["base_cells"] == 0 and info["patch_cells"] > 4 * VS.lanes(g.w, g.h) * 3
    assert g.lead == (VS.LEAD if which == 0 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(VS.EDGE_SHAPES)))
def test_edge_families_as_variants_of_one_base(gpu, lv, groups, answers, which):
    g = groups["edges"][which]
    out, info = run_group(gpu, lv, g, answers)
    assert len({s for s in out[0]}) >= 3 and info["launches"] == 2  # (E9c alone runs with checkCycles)
    assert {lp[5] for lp in g.targets} == {1e-8, 1e-17}  # (precision is per variant: E7's)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(VS.QUEUE_SHAPES)))
def test_hbm_queue_reuse_with_history_reruns(gpu, groups, answers, monkeypatch, which):
    """Every workgroup of the HBM form (0) and of the aux form (1) takes four variants, heavy and empty patches in turn, with a
    checkCycles history of 2 pivots: the matrix in the reused workspace, column 0 and the permutations in the variants' output
    slots, the workgroup's history and the reruns from the image.  The aux form without tableaux: column 0 and permutations;
    its LP has one variable and two pivots at most, so nothing there must be rerun and its info text stays short."""
    monkeypatch.setenv("YALPS_LPVAR_PER_CU", "1")
    monkeypatch.setenv("YALPS_LPVAR_HIST", str(VS.QUEUE_HIST))
    g = groups["queue"][which]
    refs = [answers(g, i) for i in range(len(g.targets))]
    v = gpu.LpVariants(0)
    try:
        out, info = run_group(gpu, v, g, answers, tableau=which == 0, passes=None)
    finally:
        v.close()
    first = [k for k in info["kernels"] if k["pass"] == 0]
    assert len(first) == 2 and all(k["grid"] == VS.QUEUE_GRID and k["lps"] == 2 * k["grid"] for k in first), info["text"][:400]
    assert sum(k["lps"] for k in first) == len(g.targets) == 4 * VS.QUEUE_GRID
    assert all(refs[i] is answers(g, 1 + 2 * ((i // 2) % 2)) for i in range(1, len(g.targets), 2))  # (compared above: an empty patch is the base)
    rerun = info["rerun_lps"]
    assert info["reruns"] == len(rerun) and not [i for i in rerun if not g.targets[i][7]]
    must = VS.must_rerun(g.targets, refs)
    later = [k for k in info["kernels"] if k["pass"] > 0]
    assert len({k["pass"] for k in later}) >= len(must) and sum(k["lps"] for k in later) == len(rerun)
    assert all(k["kernel"] == V.kernel_of(4, True) and k["hist_cap"] == VS.QUEUE_HIST * 4 ** k["pass"] for k in later)
    counts = Counter(rerun)
    for p, ids in enumerate(must):  # a variant that must overflow pass p's history was rerun after each of the passes 0 .. p
        assert all(counts[i] >= p + 1 for i in ids), (p, [i for i in ids if counts[i] < p + 1][:5])
    if which == 0:
        assert len(info["text"]) > 4096 and info["text"].count("\n") == 1 + len(info["kernels"])  # (the second yalps_lpvar_info call)
        assert len(must) >= 3


@pytest.mark.gpu
def test_caller_stream(gpu, lv, oracle, answers):
    """An LpVariants on a stream the caller made (torch's), in a process that loads torch first (see caller_stream_child):
    the same group must come out word for word as from this module's own-stream handle, and as the oracle has it."""
    import tempfile
    g = VS.bound_group(oracle, *VS.STREAM_SHAPE)
    out, info = run_group(gpu, lv, g, answers)
    mine = VS.outputs(lv, out, len(g.targets))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "stream.npz")
        child = subprocess.run([sys.executable, "-m", "tests._variant_shapes", path], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert child.returncode == 0, child.stderr[-2000:]
        theirs = dict(np.load(path))
    assert int(theirs.pop("launches")) == info["launches"] == 2
    assert sorted(theirs) == sorted(mine)
    for key, a in mine.items():
        b = theirs[key]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), key

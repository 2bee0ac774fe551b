"""MILPs per second of a batch of independent models with integer variables: (a) one MilpBatch.solve (yalps_milpbatch_solve)
of pre-packed arrays, the same with the packing inside the clock, and solve_many from the model dicts; (b) the loop of
solve() calls, which is what solve_many did with these models before the MILP batch; (c) for orientation, the Python driver
over the C oracle on one core.  Same box, same run; per figure the median of `--repeats` timed repeats after one warm-up, with
min and max.  Per workload also the rounds, the launches, the nodes evaluated / used, the share of the wall time spent
outside kernels (HIP-event time of all kernels against the host clock) and what the node launches looked like per size class.
With --sweep the node_batch table on the mixed workload, which solve.MILP_NODE_BATCH rests on.
Writes profiles/milp_batch_throughput.json.

    python tools/milp_batch_throughput.py [--repeats 5] [--loop-sample 128] [--only NAME] [--no-baselines] [--sweep] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _cases as K  # noqa: E402
from tests import _milp_batch as MB  # noqa: E402
from tests import _milps as ML  # noqa: E402
from tests import _oracle  # noqa: E402
from tests.test_lp_batch import oracle_backend  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import solve as S  # noqa: E402

SWEEP = (1, 2, 4, 8, 16, 32)


def workloads(only=None):
    """name -> [(model, options)], seeded, from tests/_milps.py generators and the committed cases."""
    out = {}
    if only in (None, "small", "mix"):
        out["small"] = MB.small_family_models(2048, first_seed=1000)
    if only in (None, "pack60", "mix"):
        out["pack60"] = [(MB.packing_model(60, 60, 6, 3000 + s), {}) for s in range(512)]
    if only in (None, "pack100", "mix"):
        out["pack100"] = [(MB.packing_model(100, 100, 6, 4000 + s), {}) for s in range(256)]
    if only in (None, "cases_hbm", "mix"):
        cases = []
        for name in ("Large Farm MIP", "Sudoku 4x4"):
            c = K.load(name)
            cases.append((c["model"], {k: v for k, v in (c["options"] or {}).items() if k != "timeout" and v is not None}))
        out["cases_hbm"] = [cases[k % 2] for k in range(128)]
    if only in (None, "mix"):
        mix = out["small"] + out["pack60"] + out["pack100"] + out["cases_hbm"]
        out["mix"] = [mix[j] for j in np.random.default_rng(1).permutation(len(mix))]
    return {k: v for k, v in out.items() if only in (None, k)}


def timed(fn, repeats):
    fn()  # warm-up
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def rate(count, ts):
    return {"milps_per_s": count / statistics.median(ts), "milps_per_s_min": count / max(ts), "milps_per_s_max": count / min(ts),
            "seconds": ts, "milps": count}


def node_launch_table(info):
    """Per (kernel, class): launches, nodes, the mean and the largest node count and grid of a launch."""
    table = {}
    for k in info["kernels"]:
        if not k["kernel"].startswith("milp_node_kernel"):
            continue
        row = table.setdefault("%s class %d" % (k["kernel"], k["class"]), {"launches": 0, "nodes": 0, "max_nodes": 0, "max_grid": 0})
        row["launches"] += 1
        row["nodes"] += k["nodes"]
        row["max_nodes"] = max(row["max_nodes"], k["nodes"])
        row["max_grid"] = max(row["max_grid"], k["grid"])
    for row in table.values():
        row["mean_nodes_per_launch"] = row["nodes"] / row["launches"]
    return table


def batch_figure(work, repeats, node_batch, end_to_end=True):
    milps = [MB.milp_of(m, o) for m, o in work]
    b = N.MilpBatch(0)
    try:
        packed = N.PackedMilps(milps)
        calls = []
        ts = timed(lambda: calls.append(b.solve(packed, node_batch)), repeats)
        fig = rate(len(milps), ts)
        _, _, used, evaluated, call = calls[-1]
        info = b.info()
        fig.update(node_batch=node_batch, rounds=call["rounds"], launches=call["launches"], nodes_used=int(used.sum()),
                   nodes_evaluated=int(evaluated.sum()), gpu_ms=[c[4]["gpu_ms"] for c in calls[1:]],
                   share_outside_kernels=[1.0 - c[4]["gpu_ms"] / 1000.0 / t for c, t in zip(calls[1:], ts)],
                   node_launches=node_launch_table(info))
        if end_to_end:
            # the same with the packing of the Python tuples into the cell arrays inside the clock
            fig["with_packing"] = rate(len(milps), timed(lambda: b.solve(N.PackedMilps(milps), node_batch), repeats))
    finally:
        b.close()
    if end_to_end:
        # and from the model dicts, as a caller of solve_many pays it (tableau_model, packing, solution() included)
        models, opts = [m for m, _ in work], [o for _, o in work]
        saved, S.MILP_NODE_BATCH = S.MILP_NODE_BATCH, node_batch
        try:
            fig["solve_many"] = rate(len(work), timed(lambda: S.solve_many(models, opts), repeats))
        finally:
            S.MILP_NODE_BATCH = saved
    return fig


def loop_figure(work, repeats, sample):
    work = work[:sample]
    return rate(len(work), timed(lambda: [S.solve(m, o) for m, o in work], repeats))


def oracle_figure(orc, work, repeats, sample):
    work = work[:sample]
    one = oracle_backend(orc)
    return rate(len(work), timed(lambda: [S._solve_with(one, m, o) for m, o in work], repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-sample", type=int, default=128, help="models of each workload the solve() loop and the oracle are timed on")
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="also the node_batch table on the mixed workload")
    ap.add_argument("--node-batch", type=int, default=S.MILP_NODE_BATCH)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "milp_batch_throughput.json"))
    args = ap.parse_args()
    orc = _oracle.load()
    result = {"repeats": args.repeats, "loop_sample": args.loop_sample, "node_batch": args.node_batch, "workloads": {}}
    all_work = workloads(args.only)
    for name, work in all_work.items():
        row = {"milps": len(work), "batch": batch_figure(work, args.repeats, args.node_batch)}
        if not args.no_baselines:
            row["loop"] = loop_figure(work, args.repeats, args.loop_sample)
            row["oracle_python_driver_1_core"] = oracle_figure(orc, work, args.repeats, args.loop_sample)
            row["batch_with_packing_beats_loop_beyond_spread"] = row["batch"]["with_packing"]["milps_per_s_min"] > row["loop"]["milps_per_s_max"]
            row["solve_many_beats_loop_beyond_spread"] = row["batch"]["solve_many"]["milps_per_s_min"] > row["loop"]["milps_per_s_max"]
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["milps_per_s"]) if isinstance(v, dict) else v) for k, v in row.items()}),
              "with packing", round(row["batch"]["with_packing"]["milps_per_s"]), "solve_many", round(row["batch"]["solve_many"]["milps_per_s"]),
              "rounds", row["batch"]["rounds"], "outside kernels %.2f" % statistics.median(row["batch"]["share_outside_kernels"]), flush=True)
    if args.sweep and "mix" in all_work:
        table = []
        for nb in SWEEP:
            fig = batch_figure(all_work["mix"], args.repeats, nb, end_to_end=False)
            table.append({k: fig[k] for k in ("node_batch", "milps_per_s", "milps_per_s_min", "milps_per_s_max", "rounds", "launches",
                                              "nodes_used", "nodes_evaluated", "gpu_ms", "share_outside_kernels")})
            print("node_batch", nb, round(fig["milps_per_s"]), "rounds", fig["rounds"], "evaluated", fig["nodes_evaluated"], flush=True)
        result["node_batch_sweep"] = {"workload": "mix", "rows": table,
                                      "best": max(table, key=lambda r: r["milps_per_s"])["node_batch"]}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()

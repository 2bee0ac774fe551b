"""MILPs per second of the device-side search (MilpTree.solve, yalps_milptree_solve: one workgroup walks a whole tree) against
the lockstep driver (MilpBatch.solve at node_batch 8) on the five workloads of tools/milp_batch_throughput.py, same seeds:
both on pre-packed arrays, and solve_many both ways from the model dicts.  Same box, same run; per figure the median of
`--repeats` timed repeats after one warm-up, with min and max.  Per workload also the kernels' own time (HIP events), the
launches, the reruns and the longest tree's node count.  The baseline of every ratio is MilpBatch.solve of THIS run.
Writes profiles/milp_tree_throughput.json.

    python tools/milp_tree_throughput.py [--repeats 5] [--only NAME] [--no-solve-many] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _milp_batch as MB  # noqa: E402
from tools.milp_batch_throughput import rate, timed, workloads  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import solve as S  # noqa: E402

NODE_BATCH = 8


def figure(work, repeats, solve_many=True):
    milps = [MB.milp_of(m, o) for m, o in work]
    packed = N.PackedMilps(milps)
    fig = {}
    tree, batch = N.MilpTree(0), N.MilpBatch(0)
    try:
        calls = []
        ts = timed(lambda: calls.append(tree.solve(packed)), repeats)
        info = tree.info()
        _, _, used, _, _ = calls[-1]
        fig["tree"] = dict(rate(len(milps), ts), gpu_ms=[c[4]["gpu_ms"] for c in calls[1:]], launches=calls[-1][4]["launches"],
                           reruns=info["reruns"], overflows=info["overflows"], nodes_used=int(used.sum()), longest_tree=int(used.max()),
                           kernels=[{k: v for k, v in x.items()} for x in info["kernels"]])
        tree_out = calls[-1]
        calls = []
        ts = timed(lambda: calls.append(batch.solve(packed, NODE_BATCH)), repeats)
        _, _, bused, evaluated, call = calls[-1]
        fig["lockstep"] = dict(rate(len(milps), ts), node_batch=NODE_BATCH, gpu_ms=[c[4]["gpu_ms"] for c in calls[1:]],
                               launches=call["launches"], rounds=call["rounds"], nodes_used=int(bused.sum()),
                               nodes_evaluated=int(evaluated.sum()))
        same = all(a == b for a, b in zip(tree_out[0], calls[-1][0])) and int(used.sum()) == int(bused.sum())
        fig["same_statuses_and_nodes"] = bool(same)
    finally:
        tree.close()
        batch.close()
    if solve_many:
        models, opts = [m for m, _ in work], [o for _, o in work]
        fig["solve_many_device"] = rate(len(work), timed(lambda: S.solve_many(models, opts, milp_search="device"), repeats))
        fig["solve_many_host"] = rate(len(work), timed(lambda: S.solve_many(models, opts), repeats))
        fig["solve_many_device_over_host"] = fig["solve_many_device"]["milps_per_s"] / fig["solve_many_host"]["milps_per_s"]
    fig["tree_over_lockstep"] = fig["tree"]["milps_per_s"] / fig["lockstep"]["milps_per_s"]
    fig["tree_gpu_ms_over_lockstep_gpu_ms"] = statistics.median(fig["tree"]["gpu_ms"]) / statistics.median(fig["lockstep"]["gpu_ms"])
    return fig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-solve-many", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "milp_tree_throughput.json"))
    args = ap.parse_args()
    out = {"tool": "tools/milp_tree_throughput.py", "repeats": args.repeats, "baseline": "MilpBatch.solve at node_batch 8, same run",
           "workloads": {}}
    for name, work in workloads(args.only).items():
        fig = figure(work, args.repeats, not args.no_solve_many)
        out["workloads"][name] = fig
        print("%-10s %5d MILPs  tree %9.0f/s  lockstep %9.0f/s  x%.2f   kernels %.1f ms vs %.1f ms   longest tree %d nodes, %d reruns" % (
            name, len(work), fig["tree"]["milps_per_s"], fig["lockstep"]["milps_per_s"], fig["tree_over_lockstep"],
            statistics.median(fig["tree"]["gpu_ms"]), statistics.median(fig["lockstep"]["gpu_ms"]), fig["tree"]["longest_tree"],
            fig["tree"]["reruns"]), flush=True)
        with open(args.out, "w") as f:  # (after every workload: a run that is cut short leaves what it measured)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""MILPs per second of a batch of dense MILPs that already lie on the GPU as tensors: (a) milp_batch from the resident tensors,
outputs as tensors; (b) the bare MilpDense.solve on the same pointers into preallocated outputs; and what a tensor user paid
before libyalps_milpdense.so -- (c) MilpTree.solve on the same MILPs pre-packed on the host (the packing not counted), (d) the
copy of the tensors to the host, the packing (dense_cells + PackedMilps), the upload and MilpTree.solve inside the clock.
The workloads are tools/milp_tree_throughput.py's written densely, one shape and one set of integer variables per call (the
first MILP's): 2048 small trees, 512 x packing(60, 60, 6), 256 x packing(100, 100, 6).  Same box, same run; per figure the
median of `--repeats` timed windows of at least 0.1 s after two warm-up calls, with min and max (tools/lp_dense_throughput.py's
windowing); the kernels' own time per call (HIP events, median) of root pass, tree pass and epilogue apart, next to MilpTree's.
Writes profiles/milp_dense_throughput.json.

    python tools/milp_dense_throughput.py [--repeats 5] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the package's libraries: yalps_amd/tensors.py says why)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

torch.cuda.init()

from tests import _np_milp_dense as NM  # noqa: E402
from tools.lp_dense_throughput import timed  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import milp_dense, tensors  # noqa: E402

WORKLOADS = {"small": (8, 8, 6, 1000, 2048), "pack60": (60, 60, 6, 3000, 512), "pack100": (100, 100, 6, 4000, 256)}
OPTIONS = {"precision": 1e-8, "maxPivots": 8192.0, "checkCycles": False, "tolerance": 0.0, "timeout": float("inf"), "maxIterations": 32768.0}


def rate(count, ts):
    return {"milps_per_s": count / statistics.median(ts), "milps_per_s_min": count / max(ts), "milps_per_s_max": count / min(ts),
            "seconds_per_call": ts, "milps": count}


def figures(m, n, n_int, seed0, count, repeats):
    made = [NM.packing_dense(m, n, n_int, seed0 + s) for s in range(count)]
    ints = made[0][1]
    lps = [lp for lp, _ in made]
    c, A, b = (torch.from_numpy(np.stack([lp[k] for lp in lps])).cuda() for k in range(3))
    pack = lambda rows: N.PackedMilps([milp_dense.packed_milp(lp, ints, [], True, OPTIONS) for lp in rows])
    packed = pack(lps)
    tree = N.MilpTree(0)
    bare = N.MilpDense(0, stream=torch.cuda.current_stream().cuda_stream or 1)
    x = torch.empty((count, n), dtype=torch.float64, device="cuda")
    objective = torch.empty((count,), dtype=torch.float64, device="cuda")
    status = torch.empty((count,), dtype=torch.int32, device="cuda")
    nodes, node_pivots, root_pivots = (torch.empty((count,), dtype=torch.int64, device="cuda") for _ in range(3))
    operands = (tensors._strides(c, True, False), tensors._strides(A, True, True), tensors._strides(b, True, False), None, None)
    torch.cuda.synchronize()
    try:
        ms = {"milp_batch": [], "root": [], "tree": [], "epilogue": [], "milpdense": [], "milptree": [], "milptree_packing": []}
        held = {}

        def fa():
            stats = {}
            held["a"] = tensors.milp_batch(c, A, b, integers=ints, maximize=True, stats=stats)
            ms["milp_batch"].append(stats["gpu_ms"])
            held["stats"] = stats

        def fb():
            call = bare.solve(count, n, m, 0, operands, integers=ints, maximize=True, x=x.data_ptr(), objective=objective.data_ptr(),
                              status=status.data_ptr(), nodes=nodes.data_ptr(), node_pivots=node_pivots.data_ptr(),
                              root_pivots=root_pivots.data_ptr())
            for k in ("root", "tree", "epilogue"):
                ms[k].append(call[k + "_ms"])
            ms["milpdense"].append(call["gpu_ms"])
            held["b"] = call

        def fc():
            held["c"] = tree.solve(packed)
            ms["milptree"].append(held["c"][4]["gpu_ms"])

        def fd():
            host = [t.cpu().numpy() for t in (c, A, b)]
            p = pack([(host[0][i], host[1][i], host[2][i], None, None) for i in range(count)])
            ms["milptree_packing"].append(tree.solve(p)[4]["gpu_ms"])

        row = {"milps": count, "shape": [m, n, n_int], "milp_batch": rate(count, timed(fa, repeats)),
               "milpdense_solve": rate(count, timed(fb, repeats)), "milptree_prepacked": rate(count, timed(fc, repeats)),
               "milptree_with_packing": rate(count, timed(fd, repeats))}
        # the routes solve the same MILPs: same statuses, same node counts, same objective bits
        a, (statuses, results, used, pivots, _), stats = held["a"], held["c"], held["stats"]
        over = stats["overflows"]
        if not over:
            assert tensors.status_names(a.status) == list(statuses) == tensors.status_names(status)
            assert np.array_equal(a.nodes.cpu().numpy(), used) and np.array_equal(a.node_pivots.cpu().numpy(), pivots)
            ok = np.array([s in ("optimal", "timedout") for s in statuses]) & ~np.isnan(results)
            assert np.array_equal(a.objective.cpu().numpy()[ok].view(np.int64), (-results[ok]).view(np.int64))
            assert torch.equal(a.x, x) and torch.equal(a.nodes, nodes)
        tree_info = tree.info()
        med = lambda v: statistics.median(v[2:])
        row.update(statuses={s: int(sum(t == s for t in statuses)) for s in set(statuses)}, nodes_used=int(np.sum(used)),
                   longest_tree=int(np.max(used)), overflows=int(over), reruns=int(stats["reruns"]), milptree_reruns=int(tree_info["reruns"]),
                   gpu_ms={k: med(v) for k, v in ms.items()},
                   gpu_ms_spread={k: [min(v[2:]), max(v[2:])] for k, v in ms.items()},
                   launches=[(k["kernel"], k["class"], k.get("lps", k.get("trees")), k["grid"], k["lds"]) for k in stats["kernels"]],
                   operand_bytes=int(8 * (c.numel() + A.numel() + b.numel())), cell_bytes=int(16 * packed.lps.row.size))
        for k in ("milptree_prepacked", "milptree_with_packing"):
            row["milp_batch_over_" + k] = row["milp_batch"]["milps_per_s"] / row[k]["milps_per_s"]
            row["milp_batch_beats_%s_beyond_spread" % k] = row["milp_batch"]["milps_per_s_min"] > row[k]["milps_per_s_max"]
        # the tree pass runs the same kernel as MilpTree's: its time next to the whole of MilpTree's kernels (root pass included there)
        row["tree_pass_ms_over_milptree_kernels_ms"] = med(ms["tree"]) / med(ms["milptree"])
        return row
    finally:
        bare.close()
        tree.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "milp_dense_throughput.json"))
    args = ap.parse_args()
    result = {"tool": "tools/milp_dense_throughput.py", "repeats": args.repeats, "workloads": {}}
    for name, spec in WORKLOADS.items():
        if args.only is not None and name not in args.only.split(","):
            continue
        row = figures(*spec, args.repeats)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["milps_per_s"]) if isinstance(v, dict) and "milps_per_s" in v else v)
                                for k, v in row.items() if k not in ("gpu_ms_spread", "launches")}), flush=True)
        with open(args.out, "w") as f:  # (after every workload: a run that is cut short leaves what it measured)
            json.dump(result, f, indent=1)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

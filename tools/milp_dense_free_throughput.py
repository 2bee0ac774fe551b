"""What free variables cost in milp_batch_free on the three packing workloads of tools/milp_dense_throughput.py (2048 small trees,
512 x packing(60, 60, 6), 256 x packing(100, 100, 6)), same windowing: per figure the median of `--repeats` timed windows of at
least 0.1 s after two warm-up calls, with min and max, and the kernels' own time per call (HIP events, median) split into root
pass, tree pass and epilogue.  Every second integer variable is free: its objective coefficient is negated, so that the maximum
pushes it below zero, and a guard row -x[j] <= 2 under A_ub holds it (a whole number: a free integer variable that an LP leaves
at a fraction starts a chain of cuts on p and q in turn that only maxIterations ends); every call has a budget of `--nodes` nodes.
The guard rows are part of the workload, for every route.

  (a) milp_batch_free(c, A, b, free=F, integers=I): the twins generated on the device
  (b) the only route the parent commit offers, pre-built outside the clock: [c, -c_F] and [A_ub, -A_ub[:, F]] concatenated by
      torch, the twins of the free integer variables appended to the integer set; inside the clock the call and the subtraction
      of the halves of x
  (c) the same route with the cat inside the clock
      -- (b) and (c) with the bytes they materialise, (a) with the bytes of its index lists
  (d) a call with free=() of this build against the parent commit's libraries (--parent-lib FILE, beside which its
      libyalps_milpdense_bounds.so lies), boundless and with a box on the integer variables, alternating: child processes of
      this tool, this build and the parent's library in turn, `--rounds` each, every child the same windows; the figure is the
      median over a side's windows, the spread its min and max.  Skipped without --parent-lib.

Writes profiles/milp_dense_free_throughput.json.

    python tools/milp_dense_free_throughput.py [--repeats 5] [--rounds 2] [--nodes 4096] [--parent-lib FILE] [--only NAME[,NAME]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch  # (before the package's libraries: yalps_amd/tensors.py says why)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

torch.cuda.init()

from tools.lp_dense_throughput import timed  # noqa: E402
from tools.milp_dense_bounds_throughput import PARTS, box, operands  # noqa: E402
from tools.milp_dense_throughput import WORKLOADS, rate  # noqa: E402
from yalps_amd import _native as N  # noqa: E402
from yalps_amd import tensors  # noqa: E402

GUARD = 2.0


def held_down(c, A, b, ints):
    """(c, A, b, F): every second integer variable free, pushed down by its objective coefficient and held by a guard row."""
    F = list(ints[::2])
    count, _, n = A.shape
    c = c.clone()
    c[:, F] = -c[:, F]
    guards = torch.zeros((len(F), n), dtype=torch.float64, device="cuda")
    guards[torch.arange(len(F)), F] = -1.0
    A = torch.cat([A, guards.expand(count, len(F), n)], dim=1).contiguous()
    b = torch.cat([b, torch.full((count, len(F)), GUARD, dtype=torch.float64, device="cuda")], dim=1).contiguous()
    return c, A, b, F


def figures(m, n, n_int, seed0, count, repeats, nodes):
    c, A, b, ints = operands(m, n, n_int, seed0, count)
    c, A, b, F = held_down(c, A, b, ints)
    wide_ints = list(ints) + [n + t for t in range(len(F))]  # (every free variable here is an integer one)
    torch.cuda.synchronize()
    ms = {key: {p: [] for p in PARTS} for key in ("free", "prebuilt", "built_in_clock")}
    held = {}

    def note(key, stats):
        for p in PARTS:
            ms[key][p].append(stats[p])

    def build():
        return torch.cat([c, -c[:, F]], dim=1), torch.cat([A, -A[:, :, F]], dim=2)

    def route(key, c2, A2):
        stats = {}
        out = tensors.milp_batch(c2, A2, b, integers=wide_ints, maximize=True, max_iterations=nodes, stats=stats)
        x = out.x[:, :n].clone()
        x[:, F] = x[:, F] - out.x[:, n:]
        held[key] = (x, out.objective, out.status, out.nodes)
        note(key, stats)

    def free():
        stats = {}
        held["free"] = tensors.milp_batch_free(c, A, b, free=F, integers=ints, maximize=True, max_iterations=nodes, stats=stats)
        note("free", stats)
        held["launches"] = [(q["kernel"], q["class"], q.get("lps", q.get("trees")), q["grid"], q["lds"]) for q in stats["kernels"]]
        held["overflows"] = stats["overflows"]

    c2, A2 = build()
    row = {"milps": count, "shape": [m, n, n_int], "free": len(F), "guard_rows": len(F), "node_budget": nodes}
    for key, fn in (("free", free), ("prebuilt", lambda: route("prebuilt", c2, A2)), ("built_in_clock", lambda: route("built_in_clock", *build()))):
        row[key] = rate(count, timed(fn, repeats))
        print("  %dx%d %s: %.0f MILPs/s" % (m, n, key, row[key]["milps_per_s"]), file=sys.stderr, flush=True)
    a, p = held["free"], held["prebuilt"]
    # the same tableau cell for cell and the same integer columns: the same answers
    same = a.status == p[2]
    solved = same & ((a.status == 0) | ((a.status == 4) & ~torch.isnan(a.objective)))
    assert bool(same.all()) and bool(torch.equal(a.nodes, p[3])), float(same.double().mean())
    assert bool(torch.equal(a.objective[solved], p[1][solved])) and bool(torch.equal(a.x[solved], p[0][solved]))
    med = lambda v: statistics.median(v[2:])
    row.update(optimal=int((a.status == 0).sum()), timedout=int((a.status == 4).sum()), negative_free_values=int((a.x[solved][:, F] < 0).sum()),
               nodes_used=int(a.nodes.sum()), longest_tree=int(a.nodes.max()), overflows=int(held["overflows"]),
               gpu_ms={key: {q: med(v) for q, v in parts.items()} for key, parts in ms.items()},
               gpu_ms_spread={key: {q: [min(v[2:]), max(v[2:])] for q, v in parts.items()} for key, parts in ms.items()},
               launches=held["launches"], operand_bytes=int(8 * (c.numel() + A.numel() + b.numel())),
               free_bytes=int(4 * (len(F) + n)), materialised_bytes=int(8 * (c2.numel() + A2.numel())))
    for key in ("prebuilt", "built_in_clock"):
        row["free_over_" + key] = row["free"]["milps_per_s"] / row[key]["milps_per_s"]
        row["free_beats_%s_beyond_spread" % key] = row["free"]["milps_per_s_min"] > row[key]["milps_per_s_max"]
        row["free_loses_to_%s_beyond_spread" % key] = row["free"]["milps_per_s_max"] < row[key]["milps_per_s_min"]
    for q in PARTS:
        row["kernel_%s_free_over_prebuilt" % q] = row["gpu_ms"]["free"][q] / row["gpu_ms"]["prebuilt"][q]
    return row


def child(repeats, only):
    """The free=() calls, boundless and bounded, on whatever library YALPS_MILPDENSE_LIB names:
    {workload: {kind: {"seconds_per_call": [...], parts}}}."""
    parent = bool(os.environ.get("YALPS_MILPDENSE_LIB"))
    if parent:  # (the parent's library has no free entries to bind, and its milp_batch no free=)
        for key in ("validate_free", "solve_free"):
            N._BATCH_LIBS["yalps_milpdense"][1].pop(key, None)
    out = {}
    for name, spec in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        c, A, b, ints = operands(*spec)
        lb, ub = box(spec[1], spec[-1], ints)
        for kind, kw in (("boundless", {}), ("bounded", dict(lb=lb, ub=ub, upper=ints))):
            ms = {p: [] for p in PARTS}
            slot = out.setdefault(name, {}).setdefault(kind, {})

            def fn():
                stats = {}
                tensors.milp_batch_free(c, A, b, integers=ints, maximize=True, stats=stats, free=(), **kw)
                for p in PARTS:
                    ms[p].append(stats[p])
                slot["kernels"] = [q["kernel"] for q in stats["kernels"]]

            ts = timed(fn, repeats)
            slot.update(seconds_per_call=ts, milps=spec[-1], **{p: statistics.median(v[2:]) for p, v in ms.items()})
    print("CHILD " + json.dumps(out), flush=True)


def alternate(parent_lib, rounds, repeats, only):
    sides = {"this_build": [], "parent": []}
    for _ in range(rounds):
        for side in ("this_build", "parent"):
            env = dict(os.environ)
            env.pop("YALPS_MILPDENSE_LIB", None)
            if side == "parent":
                env["YALPS_MILPDENSE_LIB"] = os.path.abspath(parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(repeats)] + (["--only", ",".join(only)] if only else [])
            done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if done.returncode != 0:
                raise RuntimeError("%s child failed:\n%s" % (side, done.stderr[-2000:]))
            sides[side].append(json.loads(next(l for l in done.stdout.splitlines() if l.startswith("CHILD "))[6:]))
    result = {}
    for name in sides["this_build"][0]:
        for kind in ("boundless", "bounded"):
            row = {}
            for side, runs in sides.items():
                ts = [t for r in runs for t in r[name][kind]["seconds_per_call"]]
                row[side] = dict(rate(runs[0][name][kind]["milps"], ts), kernels=runs[0][name][kind]["kernels"],
                                 **{p: [r[name][kind][p] for r in runs] for p in PARTS})
            a, p = row["this_build"], row["parent"]
            row["this_build_over_parent"] = a["milps_per_s"] / p["milps_per_s"]
            row["spreads_overlap"] = a["milps_per_s_min"] <= p["milps_per_s_max"] and p["milps_per_s_min"] <= a["milps_per_s_max"]
            row["same_kernels"] = a["kernels"] == p["kernels"]
            result.setdefault(name, {})[kind] = row
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--nodes", type=float, default=4096.0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "milp_dense_free_throughput.json"))
    args = ap.parse_args()
    only = args.only.split(",") if args.only else None
    if args.child:
        return child(args.repeats, only)
    result = {"tool": "tools/milp_dense_free_throughput.py", "repeats": args.repeats, "workloads": {}}

    def write():
        with open(args.out, "w") as f:  # (after every step: a run that is cut short leaves what it measured)
            json.dump(result, f, indent=1)
            f.write("\n")

    for name, spec in WORKLOADS.items():
        if only is not None and name not in only:
            continue
        row = figures(*spec, args.repeats, args.nodes)
        result["workloads"][name] = row
        print(name, json.dumps({k: (round(v["milps_per_s"]) if isinstance(v, dict) and "milps_per_s" in v else v)
                                for k, v in row.items() if k not in ("gpu_ms_spread", "launches")}), flush=True)
        write()
    if args.parent_lib:
        result["free_none_against_parent"] = dict(rounds=args.rounds, workloads=alternate(args.parent_lib, args.rounds, args.repeats, only))
        for name, kinds in result["free_none_against_parent"]["workloads"].items():
            for kind, row in kinds.items():
                print("free=()", kind, name, json.dumps({k: (round(v["milps_per_s"]) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()

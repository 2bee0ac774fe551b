#!/usr/bin/env python3
"""Generate tests/golden/* by RUNNING THE REFERENCE's own hot path.

TEST-FIXTURE TOOLING, build container only (needs /root/reference and node).
  1. erase_types.py strips the type syntax of /root/reference/src/{simplex,
     tableau,util}.ts into /tmp/yalps_erased (outside the repo, never shipped);
  2. a small driver (written below, our code) feeds the reference's
     tableauModel()+simplex() with (a) every tests/cases/*.json model of the
     reference's own test-suite, (b) dense-LP(M,N,seed) tableaux (SURVEY.md
     section 8d), (c) sparse mixed-sign tableaux with near-1e-16 entries and
     (d) the edge tableaux of tests/_edges.py (ties, infinite ratios, signed
     zeros, the flush band, exact thresholds, extreme exponents),
     (f) `--only nonfinite`: the tableaux of tests/_nonfinite.py (NaN and
     infinite entries and options), final state recorded with every NaN word
     replaced by 0x7ff8000000000000 (V8 and a GPU give arithmetic NaNs
     different sign bits),
     (g) `--only rounding`: roundToPrecision (util.ts) on the table of
     tests/_rounding.py and solution() (YALPS.ts) on its hand-built final
     states, every float as its 64-bit word in hex (a JSON number drops the
     sign of a zero), and `--only rounding_edges`: the family R of the same
     module through simplex(), `result_hex` beside `result`,
     (e) `--only milp`: the MILP models of tests/_milps.py through the
     reference's solve() (YALPS.ts, branchAndCut.ts on the heap stand-in
     below), recording every popped node, the exit and the Solution,
     and records for each run: status, result, the pivot sequence, the final
     permutations, the final RHS column and SHA-256 digests of the initial and
     final Float64Array bytes;
  3. the records are written as gzip'd JSON DATA under tests/golden/, and the
     reference's test-case data files are copied to tests/golden/cases/.

Only data travels: no reference source text is stored anywhere in the repo.
Usage:  python oracle/tools/gen_golden.py [--max-dense 2048]
"""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from erase_types import erase  # noqa: E402

DRIVER = r"""
import { simplex } from "./simplex.mjs"
import { tableauModel } from "./tableau.mjs"
import { solve, solution } from "./YALPS.mjs"
import { roundToPrecision } from "./util.mjs"
import * as fs from "fs"
import * as crypto from "crypto"

const b64 = (ta) => Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength).toString("base64")
const sha = (ta) => crypto.createHash("sha256").update(Buffer.from(ta.buffer, ta.byteOffset, ta.byteLength)).digest("hex")
const num = (x) => (Number.isFinite(x) ? x : String(x))
// a double as its 64-bit word in hex, all NaNs one value; and back
const hexw = (x) => { if (x !== x) return "7ff8000000000000"; const b = Buffer.alloc(8); b.writeDoubleBE(x, 0); return b.toString("hex") }
const unhex = (s) => Buffer.from(s, "hex").readDoubleBE(0)

// the reference test-suite's PRNG (tests/helpers/util.ts:20-41), restated
const hash32 = (n) => { let x = n; x ^= x >>> 16; x = Math.imul(x, 0x21f0aaad); x ^= x >>> 15; x = Math.imul(x, 0xd35a2d97); x ^= x >>> 15; return x }
const newRand = (seed) => () => { seed += 0x9e3779b9; return (hash32(seed) >>> 0) / 4294967296 }

const identityPerms = (n) => { const p = new Int32Array(n), v = new Int32Array(n); for (let i = 0; i < n; i++) { p[i] = i; v[i] = i } return [p, v] }

const coo = (matrix) => {
  const idx = [], vals = []
  for (let i = 0; i < matrix.length; i++) if (matrix[i] !== 0 || Object.is(matrix[i], -0)) { idx.push(i); vals.push(matrix[i]) }
  return { idx: b64(Int32Array.from(idx)), val: b64(Float64Array.from(vals)) }
}

// every NaN word becomes 0x7ff8000000000000 (little-endian halves), in place
const canonNaN = (ta) => {
  const u = new Uint32Array(ta.buffer, ta.byteOffset, 2 * ta.length)
  for (let i = 0; i < ta.length; i++) if (ta[i] !== ta[i]) { u[2 * i] = 0; u[2 * i + 1] = 0x7ff80000 }
}

const run = (rec, tableau, options, storeInit, canon) => {
  rec.width = tableau.width; rec.height = tableau.height
  rec.init_sha256 = sha(tableau.matrix)
  if (storeInit) rec.init_coo = coo(tableau.matrix)
  rec.options = { precision: canon ? num(options.precision) : options.precision, maxPivots: num(options.maxPivots), checkCycles: !!options.checkCycles }
  globalThis.__yalps_trace = []
  const t0 = Date.now()
  const [status, result] = simplex(tableau, options)
  rec.wall_ms = Date.now() - t0
  rec.status = status; rec.result = num(result)
  if (rec.kind === "rounding_edges") rec.result_hex = hexw(result)  // (a JSON number cannot hold the sign of a zero)
  rec.n_pivots = globalThis.__yalps_trace.length / 2
  rec.pivots = b64(Int32Array.from(globalThis.__yalps_trace))
  rec.pos = b64(tableau.positionOfVariable); rec.var = b64(tableau.variableAtPosition)
  if (canon) canonNaN(tableau.matrix)
  const col0 = new Float64Array(tableau.height)
  for (let r = 0; r < tableau.height; r++) col0[r] = tableau.matrix[r * tableau.width]
  if (canon) canonNaN(col0)
  rec.col0 = b64(col0)
  rec[canon ? "final_canon_sha256" : "final_sha256"] = sha(tableau.matrix)
  console.log(JSON.stringify(rec))
}

const defaults = { precision: 1e-8, checkCycles: false, maxPivots: 8192 }
const mode = process.argv[2]

if (mode === "cases") {
  const dir = "/root/reference/tests/cases"
  for (const file of fs.readdirSync(dir).sort()) {
    const data = JSON.parse(fs.readFileSync(dir + "/" + file, "utf-8"))
    const tm = tableauModel(data.model)
    const rec = { kind: "case", name: file.replace(/\.json$/, ""), sign: tm.sign, integers: tm.integers }
    run(rec, tm.tableau, Object.assign({}, defaults, data.options || {}), true)
  }
} else if (mode === "dense") {
  const maxDense = Number(process.argv[3])
  const shapes = [[2, 2, 42], [5, 7, 42], [16, 16, 42], [16, 16, 7], [33, 20, 42], [64, 64, 42], [64, 64, 7], [100, 37, 3],
                  [128, 128, 42], [200, 300, 42], [256, 256, 42], [512, 512, 42], [1024, 1024, 42], [2048, 2048, 42]]
  for (const [M, N, seed] of shapes) {
    if (Math.max(M, N) > maxDense) continue
    const w = N + 1, h = M + 1, rand = newRand(seed)
    const matrix = new Float64Array(w * h)
    for (let j = 1; j < w; j++) matrix[j] = rand()
    for (let r = 1; r < h; r++) { matrix[r * w] = N * 0.25 * (1 + rand()); for (let j = 1; j < w; j++) matrix[r * w + j] = rand() }
    const [pos, vr] = identityPerms(w + h)
    run({ kind: "dense", M, N, seed }, { matrix, width: w, height: h, positionOfVariable: pos, variableAtPosition: vr },
        Object.assign({}, defaults, { maxPivots: Infinity }), false)
  }
} else if (mode === "mixed") {
  // sparse mixed-sign tableaux: negative RHS rows (phase 1), exact zeros and
  // entries straddling the 1e-16 flush/skip threshold of pivot()
  const shapes = [[3, 3], [5, 4], [12, 9], [9, 14], [30, 40], [64, 33], [100, 80], [150, 200]]
  const variants = [
    {}, { checkCycles: true }, {}, { maxPivots: 3 }, { precision: 1e-6 }, {}, { precision: 1e-11, checkCycles: true },
    { maxPivots: 2.5 }, {}, { maxPivots: 0 }, { checkCycles: true, maxPivots: 700 }, { precision: 0 }, {},
  ]
  let id = 0
  for (const [M, N] of shapes) for (let s = 0; s < 6; s++) {
    const seed = 1000 * M + 10 * N + s, rand = newRand(seed)
    const density = 0.15 + 0.7 * rand(), negFrac = s % 3 === 0 ? 0 : 0.4 * rand()
    const w = N + 1, h = M + 1
    const init = new Float64Array(w * h)
    const entry = () => { const u = rand(); if (u >= density) return 0; const t = rand(); return t < 0.06 ? (rand() - 0.5) * 4e-16 : rand() * 2 - 1 }
    for (let j = 1; j < w; j++) init[j] = entry()
    for (let r = 1; r < h; r++) {
      init[r * w] = rand() < negFrac ? -rand() * N * 0.1 : (rand() < 0.15 ? 0 : rand() * N * 0.25)
      for (let j = 1; j < w; j++) init[r * w + j] = entry()
    }
    const opts = Object.assign({}, defaults, variants[(id + s) % variants.length])
    const [pos, vr] = identityPerms(w + h)
    run({ kind: "mixed", id: id++, M, N, seed }, { matrix: Float64Array.from(init), width: w, height: h, positionOfVariable: pos, variableAtPosition: vr }, opts, true)
  }
} else if (mode === "milp") {
  // models of tests/_milps.py (argv[3] lists them, JSON) through the reference's solve(): the root, every popped node of
  // branchAndCut, the loop's exit, the tableau solution() reads and the Solution itself
  const hexd = (x) => { const b = Buffer.alloc(8); b.writeDoubleBE(x, 0); return b.toString("hex") }
  const sha2 = (a, b) => crypto.createHash("sha256").update(Buffer.from(a.buffer, a.byteOffset, a.byteLength))
    .update(Buffer.from(b.buffer, b.byteOffset, b.byteLength)).digest("hex")
  const col0Of = (t) => { const c = new Float64Array(t.height); for (let r = 0; r < t.height; r++) c[r] = t.matrix[r * t.width]; return c }
  const marshal = (sol) => ({ status: sol.status, result: hexd(sol.result), variables: sol.variables.map(([k, v]) => [k, hexd(v)]) })
  for (const spec of JSON.parse(fs.readFileSync(process.argv[3], "utf-8"))) {
    const rec = { kind: "milp", family: spec.family, seed: spec.seed, variant: spec.variant, options: spec.options }
    const tm = tableauModel(spec.model)
    rec.width = tm.tableau.width; rec.height = tm.tableau.height; rec.init_sha256 = sha(tm.tableau.matrix)
    rec.sign = tm.sign; rec.integers = tm.integers
    const nodes = []
    let popped = null
    rec.exit = "root"
    globalThis.__yalps_bnc = {
      pop: (ev, cuts) => { popped = { eval: hexd(ev), cuts: cuts.map(([s, v, x]) => [s, v, hexd(x)]) } },
      node: (t, status, result) => {
        if (status === undefined) { popped.init_sha256 = sha(t.matrix); globalThis.__yalps_trace = []; return }
        Object.assign(popped, { status, result: hexd(result), n_pivots: globalThis.__yalps_trace.length / 2,
                                final_sha256: sha(t.matrix), perm_sha256: sha2(t.positionOfVariable, t.variableAtPosition) })
        nodes.push(popped)
      },
      exit: (kind, st) => {
        if (kind === "break") { rec.exit = "break"; rec.break_eval = popped.eval; return }
        if (kind === "integral") { rec.exit = "integral"; return }
        if (rec.exit === "break") return
        const o = Object.assign({ maxIterations: 32768 }, spec.options)
        rec.exit = !(st.iter < o.maxIterations) ? "iterations" : st.empty ? "exhausted"
          : !(st.bestEval >= st.optimalThreshold) ? "threshold" : "timeout"
      },
    }
    globalThis.__yalps_solve = {
      root: (tabmod, status, result) => {
        rec.root = { status, result: hexd(result), n_pivots: globalThis.__yalps_trace.length / 2, final_sha256: sha(tabmod.tableau.matrix) }
      },
      solution: (t, status, result) => {
        rec.best = { status, result: hexd(result), height: t.height, col0_sha256: sha(col0Of(t)),
                     perm_sha256: sha2(t.positionOfVariable.subarray(0, t.width + t.height), t.variableAtPosition.subarray(0, t.width + t.height)) }
      },
    }
    globalThis.__yalps_trace = []
    const t0 = Date.now()
    const sol = solve(spec.model, spec.options)
    rec.wall_ms = Date.now() - t0
    globalThis.__yalps_bnc = undefined; globalThis.__yalps_solve = undefined; globalThis.__yalps_trace = undefined
    rec.nodes = nodes; rec.iterations = nodes.length
    rec.solution = marshal(sol)
    if (spec.zero_flip) {
      const flipped = !(spec.options.includeZeroVariables === true)
      rec.solution_flip = marshal(solve(spec.model, Object.assign({}, spec.options, { includeZeroVariables: flipped })))
    }
    console.log(JSON.stringify(rec))
  }
} else if (mode === "edges") {
  // tableaux of tests/_edges.py, written by gen_golden.py as raw float64 files: argv[3] lists them (JSON)
  for (const spec of JSON.parse(fs.readFileSync(process.argv[3], "utf-8"))) {
    const buf = fs.readFileSync(spec.file)
    const matrix = new Float64Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length))
    const w = spec.N + 1, h = spec.M + 1
    const [pos, vr] = identityPerms(w + h)
    const opts = { precision: spec.precision, maxPivots: spec.maxPivots, checkCycles: spec.checkCycles }
    run({ kind: "edges", family: spec.family, M: spec.M, N: spec.N, seed: spec.seed, layout: spec.layout },
        { matrix, width: w, height: h, positionOfVariable: pos, variableAtPosition: vr }, opts, w * h <= 20000)
  }
} else if (mode === "rounding") {
  // tests/_rounding.py: argv[3] holds {table: [{precision, nums}], states: [...]}, every float as its 64-bit word in hex
  const spec = JSON.parse(fs.readFileSync(process.argv[3], "utf-8"))
  for (const row of spec.table) {
    const p = unhex(row.precision)
    console.log(JSON.stringify({ kind: "round", precision: row.precision, nums: row.nums, outs: row.nums.map((h) => hexw(roundToPrecision(unhex(h), p))) }))
  }
  for (const s of spec.states) {
    const w = spec.n + 1, h = 1 + spec.m_ub + 2 * spec.m_eq
    const matrix = new Float64Array(w * h)
    s.col0.forEach((x, r) => { matrix[r * w] = unhex(x) })
    const tableau = { matrix, width: w, height: h, positionOfVariable: Int32Array.from(s.pos), variableAtPosition: Int32Array.from(s.var) }
    const vars = []
    for (let j = 0; j < spec.n; j++) vars.push([j, []])
    const sol = solution({ tableau, sign: s.sign, variables: vars }, s.status, unhex(s.result), { precision: unhex(s.precision), includeZeroVariables: true })
    console.log(JSON.stringify(Object.assign({ kind: "solution" }, s, { out: { status: sol.status, result: hexw(sol.result), variables: sol.variables.map(([k, v]) => [k, hexw(v)]) } })))
  }
} else if (mode === "rounding_edges") {
  // the family R of tests/_rounding.py (final roundings that end at -0 or NaN), as raw float64 files like "edges"
  for (const spec of JSON.parse(fs.readFileSync(process.argv[3], "utf-8"))) {
    const buf = fs.readFileSync(spec.file)
    const matrix = new Float64Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length))
    const w = spec.N + 1, h = spec.M + 1
    const [pos, vr] = identityPerms(w + h)
    const opts = { precision: spec.precision, maxPivots: spec.maxPivots, checkCycles: spec.checkCycles }
    run({ kind: "rounding_edges", family: spec.family, M: spec.M, N: spec.N, seed: spec.seed, layout: spec.layout },
        { matrix, width: w, height: h, positionOfVariable: pos, variableAtPosition: vr }, opts, false)
  }
} else if (mode === "nonfinite") {
  // tableaux of tests/_nonfinite.py, as raw float64 files; precision and maxPivots travel as strings (JSON has no NaN)
  for (const spec of JSON.parse(fs.readFileSync(process.argv[3], "utf-8"))) {
    const buf = fs.readFileSync(spec.file)
    const matrix = new Float64Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length))
    const w = spec.N + 1, h = spec.M + 1
    const [pos, vr] = identityPerms(w + h)
    const opts = { precision: Number(spec.precision), maxPivots: Number(spec.maxPivots), checkCycles: spec.checkCycles }
    run({ kind: "nonfinite", family: spec.family, M: spec.M, N: spec.N, seed: spec.seed, layout: spec.layout },
        { matrix, width: w, height: h, positionOfVariable: pos, variableAtPosition: vr }, opts, false, true)
  }
}
"""

# The one assumption left in the MILP records: npm `heap` 0.2.7 (the reference's queue, package.json) is not vendored,
# so branchAndCut.ts runs on this stand-in.  heap 0.2.7 is a port of CPython's heapq: push / pop / empty below
# are heapq's heappush / heappop with its _siftdown / _siftup, comparing by the reference's comparator `x[0] - y[0] < 0`.
# tests/test_milp_records.py runs it under node against heapq on push / pop sequences full of ties.
HEAP_MJS = r"""
export default class Heap {
  constructor(cmp) { this.cmp = cmp; this.nodes = [] }
  empty() { return this.nodes.length === 0 }
  push(x) { this.nodes.push(x); this._siftdown(0, this.nodes.length - 1) }
  pop() {
    const last = this.nodes.pop()
    if (this.nodes.length === 0) return last
    const ret = this.nodes[0]
    this.nodes[0] = last
    this._siftup(0)
    return ret
  }
  _siftdown(startpos, pos) {
    const newitem = this.nodes[pos]
    while (pos > startpos) {
      const parentpos = (pos - 1) >> 1
      const parent = this.nodes[parentpos]
      if (this.cmp(newitem, parent) < 0) { this.nodes[pos] = parent; pos = parentpos; continue }
      break
    }
    this.nodes[pos] = newitem
  }
  _siftup(pos) {
    const endpos = this.nodes.length, startpos = pos, newitem = this.nodes[pos]
    let childpos = 2 * pos + 1
    while (childpos < endpos) {
      const rightpos = childpos + 1
      if (rightpos < endpos && !(this.cmp(this.nodes[childpos], this.nodes[rightpos]) < 0)) childpos = rightpos
      this.nodes[pos] = this.nodes[childpos]
      pos = childpos
      childpos = 2 * pos + 1
    }
    this.nodes[pos] = newitem
    this._siftdown(startpos, pos)
  }
}
"""

# the stand-in on its own (argv[2]: a JSON list of operation lists, a number = push [number, id], null = pop): prints, per
# list, the ids popped in order, the heap drained at the end
HEAP_DRIVER = r"""
import Heap from "./heap.mjs"
import * as fs from "fs"
for (const ops of JSON.parse(fs.readFileSync(process.argv[2], "utf-8"))) {
  const h = new Heap((x, y) => x[0] - y[0]), out = []
  ops.forEach((op, id) => { if (op === null) { if (!h.empty()) out.push(h.pop()[1]) } else h.push([op, id]) })
  while (!h.empty()) out.push(h.pop()[1])
  console.log(JSON.stringify(out))
}
"""


def run_driver(erased, mode, *args):
    out = subprocess.run(["node", os.path.join(erased, "golden_driver.mjs"), mode, *map(str, args)],
                         check=True, capture_output=True, text=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def edge_specs(tmp):
    """Writes every tableau of tests/_edges.py to a raw float64 file under `tmp` (outside the repository) and returns the
    list the driver's "edges" mode reads."""
    sys.path.insert(0, REPO)
    from tests import _edges as E
    specs = []
    for i, (family, M, N, seed) in enumerate(E.specs()):
        layout = E.default_layout(M, N)
        m = E.make(family, M, N, seed, layout)
        path = os.path.join(tmp, "edge_%04d.f64" % i)
        m.tofile(path)
        o = E.options(family, M, N, seed)
        specs.append(dict(file=path, family=family, M=M, N=N, seed=seed, layout=[list(layout[0]), list(layout[1])],
                          precision=o["precision"], maxPivots=o["max_pivots"], checkCycles=o["check_cycles"]))
    with open(os.path.join(tmp, "edges.json"), "w") as f:
        json.dump(specs, f)
    return os.path.join(tmp, "edges.json")


def nonfinite_records(erased, tmp):
    """The records of tests/_nonfinite.py, one shape at a time (the raw float64 files of a shape are removed before the
    next one is written)."""
    sys.path.insert(0, REPO)
    from tests import _edges as E
    from tests import _nonfinite as NF
    js = {"nan": "NaN", "inf": "Infinity", "-inf": "-Infinity"}
    recs = []
    for shape in E.SHAPES:
        specs, files = [], []
        for family, M, N, seed in NF.specs():
            if (M, N) != shape:
                continue
            layout = E.default_layout(M, N)
            path = os.path.join(tmp, "nonfinite_%04d.f64" % len(files))
            NF.make(family, M, N, seed, layout).tofile(path)
            files.append(path)
            o = NF.options(family, M, N, seed)
            specs.append(dict(file=path, family=family, M=M, N=N, seed=seed, layout=[list(layout[0]), list(layout[1])],
                              precision=js.get(repr(o["precision"]), repr(o["precision"])),
                              maxPivots=js.get(repr(o["max_pivots"]), repr(o["max_pivots"])), checkCycles=o["check_cycles"]))
        with open(os.path.join(tmp, "nonfinite.json"), "w") as f:
            json.dump(specs, f)
        recs += run_driver(erased, "nonfinite", os.path.join(tmp, "nonfinite.json"))
        for path in files:
            os.remove(path)
    return recs


def rounding_spec(tmp):
    """The table and the states of tests/_rounding.py, as the driver's "rounding" mode reads them."""
    sys.path.insert(0, REPO)
    from tests import _rounding as RD
    spec = dict(n=RD.N, m_ub=RD.M_UB, m_eq=RD.M_EQ,
                table=[dict(precision=RD.hexd(p), nums=[RD.hexd(x) for x in nums]) for p, nums in RD.table()],
                states=[RD.state_spec(s) for s in RD.states()])
    with open(os.path.join(tmp, "rounding.json"), "w") as f:
        json.dump(spec, f)
    return os.path.join(tmp, "rounding.json")


def rounding_edge_records(erased, tmp):
    """The records of the family R of tests/_rounding.py, one shape at a time like nonfinite_records."""
    sys.path.insert(0, REPO)
    from tests import _edges as E
    from tests import _rounding as RD
    recs = []
    for shape in E.SHAPES:
        specs, files = [], []
        for family, M, N, seed in RD.r_specs():
            if (M, N) != shape:
                continue
            layout = E.default_layout(M, N)
            path = os.path.join(tmp, "rounding_%04d.f64" % len(files))
            RD.r_make(family, M, N, seed, layout).tofile(path)
            files.append(path)
            o = RD.r_options(family, M, N, seed)
            specs.append(dict(file=path, family=family, M=M, N=N, seed=seed, layout=[list(layout[0]), list(layout[1])],
                              precision=o["precision"], maxPivots=o["max_pivots"], checkCycles=o["check_cycles"]))
        with open(os.path.join(tmp, "rounding_edges.json"), "w") as f:
            json.dump(specs, f)
        recs += run_driver(erased, "rounding_edges", os.path.join(tmp, "rounding_edges.json"))
        for path in files:
            os.remove(path)
    return recs


def milp_specs(tmp):
    """The models of tests/_milps.py with their options, as the driver's "milp" mode reads them."""
    sys.path.insert(0, REPO)
    from tests import _milps as ML
    specs = []
    for family, seed, variant in ML.specs():
        model, options = ML.make(family, seed, variant)
        specs.append(dict(family=family, seed=seed, variant=variant, model=model, options=options,
                          zero_flip=ML.zero_flip(family, seed, variant)))
    with open(os.path.join(tmp, "milp.json"), "w") as f:
        json.dump(specs, f)
    return os.path.join(tmp, "milp.json")


def compact(rec):
    """Edge records of large tableaux: the permutations as the entries that differ from the identity, and col0 of more
    than 1024 rows as its SHA-256 (final_sha256 covers it as well)."""
    import base64
    import hashlib
    import numpy as np
    for key in ("pos", "var"):
        p = np.frombuffer(base64.b64decode(rec[key]), np.int32)
        idx = np.flatnonzero(p != np.arange(p.size)).astype(np.int32)
        rec[key] = {"n": int(p.size), "idx": base64.b64encode(idx.tobytes()).decode(),
                    "val": base64.b64encode(p[idx].tobytes()).decode()}
    if rec["height"] > 1024:
        rec["col0_canon_sha256" if rec["kind"] == "nonfinite" else "col0_sha256"] = hashlib.sha256(base64.b64decode(rec.pop("col0"))).hexdigest()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-dense", type=int, default=2048)
    ap.add_argument("--erased-dir", default="/tmp/yalps_erased")
    ap.add_argument("--only", nargs="*", default=("cases", "mixed", "dense", "edges", "milp", "nonfinite"))
    args = ap.parse_args()

    erased = erase(args.erased_dir)
    with open(os.path.join(erased, "golden_driver.mjs"), "w") as f:
        f.write(DRIVER)
    with open(os.path.join(erased, "heap.mjs"), "w") as f:
        f.write(HEAP_MJS)
    golden = os.path.join(REPO, "tests", "golden")
    os.makedirs(os.path.join(golden, "cases"), exist_ok=True)

    tmp = tempfile.mkdtemp(prefix="yalps_edges_")
    for mode, extra in (("cases", ()), ("mixed", ()), ("dense", (args.max_dense,)), ("edges", ()), ("milp", ()), ("nonfinite", ()),
                        ("rounding", ()), ("rounding_edges", ())):
        if mode not in args.only:
            continue
        t0 = time.time()
        specs = {"edges": edge_specs, "milp": milp_specs, "rounding": rounding_spec}.get(mode)
        if mode == "nonfinite":
            recs = nonfinite_records(erased, tmp)
        elif mode == "rounding_edges":
            recs = rounding_edge_records(erased, tmp)
        else:
            recs = run_driver(erased, mode, *(extra if specs is None else (specs(tmp),)))
        if mode in ("edges", "nonfinite", "rounding_edges"):
            recs = [compact(r) for r in recs]
        if mode == "rounding_edges":
            for r in recs:
                del r["wall_ms"]
        path = os.path.join(golden, f"simplex_{mode}.json.gz")
        src = {"milp": "YALPS.ts, branchAndCut.ts on the heap stand-in of gen_golden.py", "rounding": "util.ts, YALPS.ts"}.get(mode, "simplex.ts")
        node = subprocess.run(["node", "--version"], capture_output=True, text=True).stdout.strip()
        with gzip.GzipFile(path, "wb", mtime=0) as gz:
            gz.write(json.dumps({"generator": "oracle/tools/gen_golden.py",
                                 "reference": "Ivordir/YALPS src/%s (type-erased, node %s)" % (src, node),
                                 "records": recs}).encode())
        print(f"{mode}: {len(recs)} records -> {path} ({os.path.getsize(path)} bytes, {time.time() - t0:.0f} s)")
    shutil.rmtree(tmp)

    # the reference test-suite's own data files (model + expected), as data
    src = "/root/reference/tests/cases"
    for name in sorted(os.listdir(src)):
        shutil.copyfile(os.path.join(src, name), os.path.join(golden, "cases", name))
    print("copied", len(os.listdir(src)), "case data files")


if __name__ == "__main__":
    main()

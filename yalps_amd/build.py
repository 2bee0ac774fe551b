"""Builds the native pieces in-tree (gfx950 only).  Used by __graft_entry__.build().

  yalps_amd/libyalps_hip.so   HIP kernels + C ABI (include/yalps_hip.h)      hipcc
  yalps_amd/libyalps_lpbatch.so   batches of independent LPs (include/yalps_lpbatch.h)   hipcc
  yalps_amd/libyalps_milpbatch.so batches of independent MILPs (include/yalps_milpbatch.h) hipcc
  yalps_amd/libyalps_lpvar.so     many variants of one LP (include/yalps_lpvar.h)        hipcc
  yalps_amd/libyalps_lpsens.so    LP batches with sensitivity ranges (include/yalps_lpsens.h) hipcc
  yalps_amd/libyalps_lpwarm.so    variants of one LP from its optimal tableau (include/yalps_lpwarm.h) hipcc
  yalps_amd/libyalps_milptree.so  batches of MILPs, every tree walked on the device (include/yalps_milptree.h) hipcc
  yalps_amd/libyalps_lpdense.so   batches of dense LPs of one shape, device tensors in and out (include/yalps_lpdense.h) hipcc
  yalps_amd/libyalps_lpdense_bounds.so   its kernels with variable bounds, linked by libyalps_lpdense.so             hipcc
  yalps_amd/libyalps_lpdense_free.so     its kernels with free variables, linked by libyalps_lpdense.so              hipcc
  yalps_amd/libyalps_milpdense.so batches of dense MILPs of one shape, device tensors in and out, trees walked on the device (include/yalps_milpdense.h) hipcc
  yalps_amd/libyalps_milpdense_bounds.so its root and solution kernels with variable bounds, linked by libyalps_milpdense.so hipcc
  yalps_amd/libyalps_milpdense_free.so   its root and solution kernels with free variables, linked by libyalps_milpdense.so hipcc
  yalps_amd/napi/yalps_napi.node  thin N-API shim over the C ABI (optional)  g++

The .so files are git-ignored but travel to the GPU box with the tree.
"""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libyalps_hip.so")
LIB_STAMPS = os.path.join(HERE, "libyalps_hip_stamps.so")
LINK_LIBS = []
CSRC = os.path.join(HERE, "csrc")
HIP_SRC = os.path.join(CSRC, "yalps_hip.hip")  # host side + C ABI + the launch-per-pivot / single-workgroup / batch kernels
# the persistent kernels' instantiations, one translation unit per group: compiled side by side (the device compile of
# ~40 register-heavy kernels in one unit took 2.5 minutes)
HIP_UNITS = [HIP_SRC] + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.startswith("persistent_") and f.endswith(".hip")]
HIP_DEPS = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".cuh", ".inc", ".h")) and not f.startswith(("lp_batch", "lp_dense", "lp_variants", "lp_sens", "lp_warm", "milp_node", "milp_tree", "milp_dense", "wg_queue", "dense_"))]
# the batch library: one translation unit of its own around the shared workgroup loop, never linked into libyalps_hip.so
LIB_LPBATCH = os.path.join(HERE, "libyalps_lpbatch.so")
LPBATCH_SRC = os.path.join(CSRC, "lp_batch.hip")
QUEUE_DEPS = [os.path.join(CSRC, f) for f in ("wg_queue.cuh", "wg_queue_host.inc", "wg_simplex.cuh", "common.cuh")]  # the queue body and the host pass of all four
LPBATCH_DEPS = [os.path.join(CSRC, f) for f in ("lp_batch_kernel.cuh", "lp_batch_host.inc", "lp_batch_lib.inc")] + QUEUE_DEPS
LPBATCH_HEADER = os.path.join(ROOT, "include", "yalps_lpbatch.h")
# the MILP batch library: the LP batch's root pass compiled again next to milp_node_kernel and the lockstep driver
LIB_MILPBATCH = os.path.join(HERE, "libyalps_milpbatch.so")
MILPBATCH_SRC = os.path.join(CSRC, "milp_batch.hip")
MILPBATCH_DEPS = LPBATCH_DEPS + [os.path.join(CSRC, f) for f in ("milp_node_kernel.cuh", "milp_search.inc")] + [LPBATCH_HEADER]
MILPBATCH_HEADER = os.path.join(ROOT, "include", "yalps_milpbatch.h")
# the variants library: a shared base image plus per-variant patches, one translation unit around the same workgroup loop
LIB_LPVAR = os.path.join(HERE, "libyalps_lpvar.so")
LPVAR_SRC = os.path.join(CSRC, "lp_variants.hip")
LPVAR_DEPS = [os.path.join(CSRC, "lp_variants_kernel.cuh")] + QUEUE_DEPS
LPVAR_HEADER = os.path.join(ROOT, "include", "yalps_lpvar.h")
# the sensitivity library: the LP batch's host code around lp_sens_kernel (lp_batch_kernel's job plus a ranging epilogue)
LIB_LPSENS = os.path.join(HERE, "libyalps_lpsens.so")
LPSENS_SRC = os.path.join(CSRC, "lp_sens.hip")
LPSENS_DEPS = [os.path.join(CSRC, "lp_sens_kernel.cuh")] + LPBATCH_DEPS
LPSENS_HEADER = os.path.join(ROOT, "include", "yalps_lpsens.h")
# the warm-start library: the LP batch's pass for the base (tableau kept), then lp_warm_kernel from the base's final tableau
LIB_LPWARM = os.path.join(HERE, "libyalps_lpwarm.so")
LPWARM_SRC = os.path.join(CSRC, "lp_warm.hip")
LPWARM_DEPS = [os.path.join(CSRC, "lp_warm_kernel.cuh")] + LPBATCH_DEPS + [LPBATCH_HEADER]
LPWARM_HEADER = os.path.join(ROOT, "include", "yalps_lpwarm.h")
# the tree library: the LP batch's root pass compiled again next to milp_tree_kernel, whose search rules the host shares
LIB_MILPTREE = os.path.join(HERE, "libyalps_milptree.so")
MILPTREE_SRC = os.path.join(CSRC, "milp_tree.hip")
MILPTREE_DEPS = LPBATCH_DEPS + [os.path.join(CSRC, f) for f in ("milp_tree_kernel.cuh", "milp_tree_rules.cuh", "milp_tree_host.inc")] + [LPBATCH_HEADER]
MILPTREE_HEADER = os.path.join(ROOT, "include", "yalps_milptree.h")
# the dense library: operands and answers in device memory, one translation unit around the same workgroup loop
LIB_LPDENSE = os.path.join(HERE, "libyalps_lpdense.so")
LPDENSE_SRC = os.path.join(CSRC, "lp_dense.hip")
DENSE_DEPS = [os.path.join(CSRC, f) for f in ("dense_tableau.cuh", "dense_host.inc")] + QUEUE_DEPS  # the tableau's rules and the host checks of both dense libraries
LPDENSE_DEPS = [os.path.join(CSRC, "lp_dense_kernel.cuh")] + DENSE_DEPS
# its kernels with bounds, a code object of their own that libyalps_lpdense.so links: the boundless library's holds the six forms it always held
LIB_LPDENSE_BOUNDS = os.path.join(HERE, "libyalps_lpdense_bounds.so")
LPDENSE_BOUNDS_SRC = os.path.join(CSRC, "lp_dense_bounds.hip")
LPDENSE_HEADER = os.path.join(ROOT, "include", "yalps_lpdense.h")
# and with free variables, likewise a code object of their own that libyalps_lpdense.so links
LIB_LPDENSE_FREE = os.path.join(HERE, "libyalps_lpdense_free.so")
LPDENSE_FREE_SRC = os.path.join(CSRC, "lp_dense_free.hip")
# the dense MILP library: a dense root pass, milp_tree_kernel compiled again on the tree pass both libraries share, and solution() on the device
LIB_MILPDENSE = os.path.join(HERE, "libyalps_milpdense.so")
MILPDENSE_SRC = os.path.join(CSRC, "milp_dense.hip")
MILPDENSE_DEPS = [os.path.join(CSRC, f) for f in ("milp_dense_kernel.cuh", "milp_tree_kernel.cuh", "milp_tree_rules.cuh", "milp_tree_host.inc",
                                                  "lp_batch_kernel.cuh", "milp_dense_bounds_kernel.cuh", "milp_dense_free_kernel.cuh")] + DENSE_DEPS  # (the last two: the sibling kernels' types)
MILPDENSE_HEADER = os.path.join(ROOT, "include", "yalps_milpdense.h")
# its root and solution kernels with bounds, a code object of their own that libyalps_milpdense.so links: the boundless library's holds the kernels it always held
LIB_MILPDENSE_BOUNDS = os.path.join(HERE, "libyalps_milpdense_bounds.so")
MILPDENSE_BOUNDS_SRC = os.path.join(CSRC, "milp_dense_bounds.hip")
MILPDENSE_BOUNDS_DEPS = [os.path.join(CSRC, f) for f in ("milp_dense_bounds_kernel.cuh", "milp_dense_kernel.cuh", "milp_tree_rules.cuh")] + DENSE_DEPS
# and with free variables, likewise a code object of their own that libyalps_milpdense.so links
LIB_MILPDENSE_FREE = os.path.join(HERE, "libyalps_milpdense_free.so")
MILPDENSE_FREE_SRC = os.path.join(CSRC, "milp_dense_free.hip")
MILPDENSE_FREE_DEPS = [os.path.join(CSRC, "milp_dense_free_kernel.cuh")] + MILPDENSE_BOUNDS_DEPS
OBJ_DIR = os.path.join(HERE, "build")
HEADER = os.path.join(ROOT, "include", "yalps_hip.h")
NAPI_SRC = os.path.join(HERE, "napi", "yalps_napi.cc")
NAPI_OUT = os.path.join(HERE, "napi", "yalps_napi.node")

# -ffp-contract=off: the reference (V8) rounds the product and the difference of
# M[r,c] - coef*M[row,c] separately (src/simplex.ts:33); an fma would change pivot paths.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def _stale(out, *srcs):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in srcs if os.path.exists(s))


def kernel_metadata(lib=LIB):
    """{mangled kernel name: {vgpr_count, agpr_count, private_segment_fixed_size, ...}} of the gfx950 code objects inside a
    built library (llvm-objcopy + clang-offload-bundler + llvm-readelf of this image's ROCm)."""
    import re
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([f"{llvm}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        # one bundle per translation unit (yalps_hip.hip + persistent_*.hip), back to back in the section
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        blob = open(fat, "rb").read()
        starts = [i for i in range(len(blob)) if blob.startswith(magic, i)]
        if not starts:
            raise RuntimeError("no offload bundle in .hip_fatbin of %s" % lib)
        notes = ""
        for k, lo in enumerate(starts):
            part = os.path.join(tmp, "part%d.bin" % k)
            with open(part, "wb") as f:
                f.write(blob[lo:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.run([f"{llvm}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
            notes += subprocess.run([f"{llvm}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*(?:- )?\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "agpr_count" and line.lstrip().startswith("- "):  # first key of a kernel's record
            cur = {}
        cur[key] = val
        if key == "name" and val.startswith("_Z"):
            kernels[val] = cur
    return kernels


# Kernels whose rows / tableaux live in registers or LDS behind hand-written sc1 loads and stores: built without
# scratch and without accumulator registers, or not at all.  (Two instantiations that broke this rule computed wrong
# rows on the GPU -- DESIGN.md 4.7 -- so the rule is part of the build, not of an optional test.)
# ("batch_kernel" also matches libyalps_lpbatch.so's lp_batch_kernel.)
NO_SCRATCH = ("lp_sens", "lp_dense", "milp_dense_root_kernel", "milp_dense_solution_kernel", "milp_dense_bounds_root_kernel", "milp_dense_bounds_solution_kernel", "milp_dense_free_root_kernel", "milp_dense_free_solution_kernel", "lp_variants", "lp_warm", "milp_node_kernel", "milp_tree_kernel", "dshard_kernel", "dshard_select_kernel", "dshard_sweep_kernel", "small_kernel", "batch_kernel", "assemble", "resident_kernel", "resident2_kernel", "stream_kernel", "stream2_kernel", "stream3_kernel", "sweep_kernel")


# resident2_kernel<T, J, R>: scalar registers spilled to lanes of vector registers (sgpr_spill_count), at most what each
# instantiation was built with when its rows became slot vectors (before that: 52, 75, 58, 58, 68, 105, 67; the aim of 0
# for <512,2,9> was not reached).  Every reload is a v_readlane on a chain that is instruction-issue bound (DESIGN.md
# 4.2b); the no-scratch rule does not see them.  The counts are this compiler's: if another ROCm moves one up, read the
# kernel's ISA (the loop of resident2_kernel.cuh, v_readlane / v_writelane between the barriers) before raising its
# bound -- a few more spills off the pivot chain cost nothing, a mask or a pointer reloaded on it every pivot does --
# and lower the bounds a newer compiler undercuts.
RESIDENT2_SGPR_SPILLS = {(256, 1, 4): 7, (256, 1, 9): 14, (256, 2, 4): 11, (512, 2, 4): 11, (512, 2, 6): 17, (512, 2, 9): 23,
                         (512, 3, 4): 21}


def check_register_budgets(lib=LIB, min_resident=15):
    """min_resident=0: a library without the register-resident kernels (libyalps_lpbatch.so); the no-scratch rule holds as it is,
    and the kernels under it may not use accumulator registers either."""
    ks = kernel_metadata(lib)
    resident = {k: v for k, v in ks.items() if "resident_kernel" in k or "resident2_kernel" in k}
    bad = []
    if len(resident) < min_resident:
        bad.append("only %d resident_kernel instantiations in the code object" % len(resident))
    for name, md in sorted(ks.items()):
        if ("resident_kernel" in name or "resident2_kernel" in name) and (int(md["vgpr_count"]) > 256 or int(md["agpr_count"]) != 0):
            bad.append("%s: vgpr_count %s agpr_count %s" % (name, md["vgpr_count"], md["agpr_count"]))
        r2 = re.search(r"resident2_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", name)
        if r2:
            shape = tuple(int(x) for x in r2.groups())
            if shape not in RESIDENT2_SGPR_SPILLS:
                bad.append("%s: no sgpr_spill_count bound for this instantiation" % name)
            elif int(md.get("sgpr_spill_count", 0)) > RESIDENT2_SGPR_SPILLS[shape]:
                bad.append("%s: sgpr_spill_count %s, bound %d" % (name, md.get("sgpr_spill_count"), RESIDENT2_SGPR_SPILLS[shape]))
        if any(tag in name for tag in NO_SCRATCH) and int(md["private_segment_fixed_size"]) != 0:
            bad.append("%s: private_segment_fixed_size %s (scratch)" % (name, md["private_segment_fixed_size"]))
        queue = "lp_dense_free_kernel" in name or "lp_dense_bounds_kernel" in name or "lp_batch_kernel" in name or "milp_node_kernel" in name or "lp_variants_kernel" in name or "lp_sens_kernel" in name or "lp_warm_kernel" in name or "milp_tree_kernel" in name or "lp_dense_kernel" in name or "milp_dense_root_kernel" in name or "milp_dense_bounds_root_kernel" in name or "milp_dense_free_root_kernel" in name
        if queue and int(md["agpr_count"]) != 0:
            bad.append("%s: agpr_count %s" % (name, md["agpr_count"]))
        # its dynamic LDS block (tableau and pivot row, swept 16 bytes at a time) starts where the static LDS ends
        if queue and int(md["group_segment_fixed_size"]) % 16 != 0:
            bad.append("%s: group_segment_fixed_size %s is not a multiple of 16 (misaligned 128-bit LDS accesses)" % (name, md["group_segment_fixed_size"]))
    if bad and os.environ.get("YALPS_BUILD_ALLOW_SCRATCH") == "1":  # (experiments only: a same-box A/B of a form that does not fit yet)
        print("register budget violated (YALPS_BUILD_ALLOW_SCRATCH=1: building anyway):\n  " + "\n  ".join(bad))
        return ks
    if bad:
        raise RuntimeError("register budget violated (a spilling variant computes wrong rows):\n  " + "\n  ".join(bad))
    return ks


def build_hip(force=False, verbose=False, stamps=False):
    """stamps=True: the diagnostic build with in-kernel stage stamps (-DYALPS_STAMPS -> libyalps_hip_stamps.so; selected
    with YALPS_HIP_LIB by tools/resident_stages.py, never loaded by default)."""
    lib_out = LIB_STAMPS if stamps else LIB
    obj_dir = OBJ_DIR + ("_stamps" if stamps else "")
    if not force and not _stale(lib_out, HEADER, *HIP_UNITS, *HIP_DEPS):
        return lib_out
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(obj_dir, exist_ok=True)
    objs = [os.path.join(obj_dir, os.path.basename(u)[:-4] + ".o") for u in HIP_UNITS]
    flags = HIPCC_FLAGS + (["-DYALPS_STAMPS"] if stamps else [])

    def compile_unit(pair):
        unit, obj = pair
        if not force and not _stale(obj, unit, HEADER, *HIP_DEPS):
            return
        cmd = [hipcc, *flags, "-c", "-o", obj, unit]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(len(objs), os.cpu_count() or 1)) as pool:
        list(pool.map(compile_unit, zip(HIP_UNITS, objs)))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_out + ".tmp", *objs, *LINK_LIBS]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    if not stamps:
        check_register_budgets(lib_out + ".tmp")  # (the stamped kernels keep their sums in extra scalar registers)
    os.replace(lib_out + ".tmp", lib_out)  # (never a half-written library under the final name)
    return lib_out


def build_single_unit(src, out, deps, header, kernels, force=False, verbose=False, link=()):
    """A library of one translation unit (it includes common.cuh / wg_simplex.cuh itself), same flags as the main library;
    `kernels`: the kernel names its code object must hold; `link`: libraries beside `out` that it links (found again through
    an rpath of $ORIGIN)."""
    if not force and not _stale(out, header, src, *deps):
        return out
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(OBJ_DIR, exist_ok=True)
    obj = os.path.join(OBJ_DIR, os.path.basename(src)[:-4] + ".o")
    for cmd in ([hipcc, *HIPCC_FLAGS, "-c", "-o", obj, src],
                [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out + ".tmp", obj,
                 *(["-L" + os.path.dirname(out), "-Wl,-rpath,$ORIGIN"] if link else []), *("-l:" + os.path.basename(l) for l in link)]):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    ks = check_register_budgets(out + ".tmp", min_resident=0)
    for kernel in kernels:
        if not any(kernel in k for k in ks):
            raise RuntimeError("no %s in the code object of %s" % (kernel, out))
    os.replace(out + ".tmp", out)
    return out


def build_lpbatch(force=False, verbose=False):
    """libyalps_lpbatch.so: lp_batch.hip alone."""
    return build_single_unit(LPBATCH_SRC, LIB_LPBATCH, LPBATCH_DEPS, LPBATCH_HEADER,
                             ("lp_batch_kernel",), force, verbose)


def build_milpbatch(force=False, verbose=False):
    """libyalps_milpbatch.so: milp_batch.hip alone."""
    return build_single_unit(MILPBATCH_SRC, LIB_MILPBATCH, MILPBATCH_DEPS, MILPBATCH_HEADER,
                             ("milp_node_kernel", "lp_batch_kernel"), force, verbose)


def build_lpvar(force=False, verbose=False):
    """libyalps_lpvar.so: lp_variants.hip alone."""
    return build_single_unit(LPVAR_SRC, LIB_LPVAR, LPVAR_DEPS, LPVAR_HEADER,
                             ("lp_variants_kernel", "lp_variants_base_kernel"), force, verbose)


def build_lpsens(force=False, verbose=False):
    """libyalps_lpsens.so: lp_sens.hip alone."""
    return build_single_unit(LPSENS_SRC, LIB_LPSENS, LPSENS_DEPS, LPSENS_HEADER,
                             ("lp_sens_kernel",), force, verbose)


def build_lpwarm(force=False, verbose=False):
    """libyalps_lpwarm.so: lp_warm.hip alone."""
    return build_single_unit(LPWARM_SRC, LIB_LPWARM, LPWARM_DEPS, LPWARM_HEADER,
                             ("lp_warm_kernel", "lp_warm_image_kernel", "lp_batch_kernel"), force, verbose)


def build_milptree(force=False, verbose=False):
    """libyalps_milptree.so: milp_tree.hip alone."""
    return build_single_unit(MILPTREE_SRC, LIB_MILPTREE, MILPTREE_DEPS, MILPTREE_HEADER,
                             ("milp_tree_kernel", "lp_batch_kernel"), force, verbose)


def build_lpdense(force=False, verbose=False):
    """libyalps_lpdense_bounds.so: lp_dense_bounds.hip alone, the six lp_dense_bounds_kernel forms (they pass the same register
    budget: "lp_dense" is under NO_SCRATCH); libyalps_lpdense_free.so: lp_dense_free.hip alone, the six lp_dense_free_kernel forms,
    under the same budget; then libyalps_lpdense.so: lp_dense.hip alone, linking both."""
    bounds = build_single_unit(LPDENSE_BOUNDS_SRC, LIB_LPDENSE_BOUNDS, LPDENSE_DEPS, LPDENSE_HEADER,
                               ("lp_dense_bounds_kernel",), force, verbose)
    free = build_single_unit(LPDENSE_FREE_SRC, LIB_LPDENSE_FREE, LPDENSE_DEPS, LPDENSE_HEADER,
                             ("lp_dense_free_kernel",), force, verbose)
    return build_single_unit(LPDENSE_SRC, LIB_LPDENSE, LPDENSE_DEPS + [bounds, free], LPDENSE_HEADER,
                             ("lp_dense_kernel",), force, verbose, link=(bounds, free))


def build_milpdense(force=False, verbose=False):
    """libyalps_milpdense_bounds.so and libyalps_milpdense_free.so first (build_milpdense_bounds, build_milpdense_free); then
    libyalps_milpdense.so: milp_dense.hip alone, linking both."""
    bounds = build_milpdense_bounds(force, verbose)
    free = build_milpdense_free(force, verbose)
    return build_single_unit(MILPDENSE_SRC, LIB_MILPDENSE, MILPDENSE_DEPS + [bounds, free], MILPDENSE_HEADER,
                             ("milp_dense_root_kernel", "milp_dense_solution_kernel", "milp_tree_kernel"), force, verbose, link=(bounds, free))


def build_milpdense_bounds(force=False, verbose=False):
    """libyalps_milpdense_bounds.so: milp_dense_bounds.hip alone, the six milp_dense_bounds_root_kernel forms and
    milp_dense_bounds_solution_kernel, under the register budget of their boundless siblings."""
    return build_single_unit(MILPDENSE_BOUNDS_SRC, LIB_MILPDENSE_BOUNDS, MILPDENSE_BOUNDS_DEPS, MILPDENSE_HEADER,
                             ("milp_dense_bounds_root_kernel", "milp_dense_bounds_solution_kernel"), force, verbose)


def build_milpdense_free(force=False, verbose=False):
    """libyalps_milpdense_free.so: milp_dense_free.hip alone, the six milp_dense_free_root_kernel forms and
    milp_dense_free_solution_kernel, under the register budget of their bounded siblings."""
    return build_single_unit(MILPDENSE_FREE_SRC, LIB_MILPDENSE_FREE, MILPDENSE_FREE_DEPS, MILPDENSE_HEADER,
                             ("milp_dense_free_root_kernel", "milp_dense_free_solution_kernel"), force, verbose)


def build_napi(force=False, verbose=False):
    """The Node addon; skipped (returns None) where node's headers are absent."""
    inc = "/usr/include/node"
    if not os.path.exists(os.path.join(inc, "node_api.h")) or not os.path.exists(NAPI_SRC):
        return None
    if not force and not _stale(NAPI_OUT, NAPI_SRC, HEADER):
        return NAPI_OUT
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", inc, "-I", os.path.join(ROOT, "include"),
           "-o", NAPI_OUT, NAPI_SRC, "-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return NAPI_OUT


if __name__ == "__main__":
    import sys
    if "stamps" in sys.argv[1:]:
        print(build_hip(verbose=True, stamps=True))
        raise SystemExit(0)
    print(build_hip(force=True, verbose=True))
    print(build_lpbatch(force=True, verbose=True))
    print(build_milpbatch(force=True, verbose=True))
    print(build_lpvar(force=True, verbose=True))
    print(build_lpsens(force=True, verbose=True))
    print(build_lpwarm(force=True, verbose=True))
    print(build_milptree(force=True, verbose=True))
    print(build_lpdense(force=True, verbose=True))
    print(build_milpdense(force=True, verbose=True))
    print(build_napi(force=True, verbose=True))

"""Build libm4ri_amd.so (HIP kernels + engine + C ABI) for gfx950, in-tree.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels to the GPU box with the snapshot.  `python -m m4ri_amd.build` or
`__graft_entry__.build()`.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "csrc", "_obj")
LIB = os.path.join(HERE, "libm4ri_amd.so")
SOURCES = ["m4rm_leaf.hip", "a4_pack.hip", "m4rm8q_leaf.hip", "m4rm_small.hip", "aux_kernels.hip", "scheme_passes.hip", "engine.hip", "mzd_api.hip", "multi.hip", "trsm.hip", "ple.hip", "elim.hip", "echelon.hip", "echelon_batch.hip", "echelon_order_batch.hip", "pivot_exchange_batch.hip", "isd_search_batch.hip", "isd_collide_search_batch.hip", "solve.hip", "solve_batch.hip", "ple_batch.hip", "mul_small_batch.hip", "transpose.hip", "transpose_batch.hip", "reduce_batch.hip", "rowspace_batch.hip", "rowsums_batch.hip", "rowsums_collide_batch.hip", "rowsums_words_batch.hip", "lists_collide_batch.hip", "sort_rows_batch.hip", "assemble_batch.hip", "io.cpp", "small_host.cpp", "host_pipeline_plan.cpp"]
# The test-only library of the fused passes (tests/pass_lib.py binds it; it is not API and not part of the product): the objects of the
# pass sources linked a second time, with the internal launchers the pass tests call as its only exports.  libm4ri_amd.so keeps them local.
PASS_LIB = os.path.join(HERE, "libm4ri_amd_passes.so")
PASS_SOURCES = ["aux_kernels.hip", "scheme_passes.hip", "a4_pack.hip"]
PASS_EXPORTS = ["gf2_launch_pass_down", "gf2_launch_pass_down_pack", "gf2_launch_pass_up", "gf2_pass_down_pack_ok", "gf2_scheme444_rank",
                "gf2_scheme444_leaves", "gf2_scheme444_ok", "gf2_launch_a4_pack_rot", "gf2_m4rm8_a4_words"]
# The test-only library of the M4RM leaves (tests/leaf_lib.py binds it; not API, not part of the product), made the same way: the objects of
# the leaf sources and of the helpers that go with a split launch linked a second time (scheme_passes: what aux_kernels.hip calls), with the
# launchers tests/test_gpu_leaves.py calls as its only exports.
LEAF_LIB = os.path.join(HERE, "libm4ri_amd_leaves.so")
LEAF_SOURCES = ["m4rm_leaf.hip", "a4_pack.hip", "m4rm8q_leaf.hip", "m4rm_small.hip", "aux_kernels.hip", "scheme_passes.hip"]
LEAF_EXPORTS = ["gf2_launch_m4rm_leaf", "gf2_launch_m4rm_leaf_variant", "gf2_launch_m4rm_small", "gf2_m4rm_small_ksplit", "gf2_m4rm8_a4_words",
                "gf2_launch_a4_pack_rot", "gf2_m4rm8q_effective_ksplit", "gf2_launch_m4rm8q", "gf2_launch_reduce_partials", "gf2_launch_zero_tiles"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-fvisibility-inlines-hidden"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libm4ri_amd.so cannot be built (no CPU fallback exists)")
    return exe


def declared_functions() -> list[str]:
    """The functions include/m4ri_amd.h declares: M4RI's own names for this path and the m4ri_amd_* extensions.
    They are the library's whole dynamic symbol table (export_map)."""
    import re
    text = open(os.path.join(HERE, "..", "include", "m4ri_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^[A-Za-z_][\w\s\*]*?\b(\w+)\s*\([^;{]*\)\s*;", text, flags=re.M)
    return sorted(set(n for n in names if n not in ("defined",)))


def export_map() -> str:
    """Linker version script with the explicit export list.  The library is an LD_PRELOAD interposer: every stray
    global (the engine's gf2_* launchers, libstdc++ template instantiations) would be a collision risk in the host
    program, so only the declared names leave the .so; everything else is local."""
    path = os.path.join(OBJ, "exports.map")
    text = "{\n  global:\n" + "".join(f"    {n};\n" for n in declared_functions()) + "  local:\n    *;\n};\n"
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)
    return path


def _test_export_map(name: str, exports: list[str]) -> str:
    path = os.path.join(OBJ, name)
    text = "{\n  global:\n" + "".join(f"    {n};\n" for n in exports) + "  local:\n    *;\n};\n"
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)
    return path


def pass_export_map() -> str:
    """Version script of the test-only pass library: just the names tests/pass_lib.py binds."""
    return _test_export_map("pass_exports.map", PASS_EXPORTS)


def leaf_export_map() -> str:
    """Version script of the test-only leaf library: just the names tests/leaf_lib.py binds."""
    return _test_export_map("leaf_exports.map", LEAF_EXPORTS)


def _stale(target: str, deps: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    hipcc = _hipcc()
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, "gf2_common.h"), os.path.join(CSRC, "gf2_internal.h"), os.path.join(CSRC, "batch_common.h"), os.path.join(CSRC, "dev_scratch.h"), os.path.join(CSRC, "row_gather.h"), os.path.join(CSRC, "subset_rank.h"), os.path.join(CSRC, "join_common.h"), os.path.join(CSRC, "transpose_block.h"), os.path.join(CSRC, "scheme444.h"), os.path.join(HERE, "..", "include", "m4ri_amd.h")]
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
        if force or _stale(o, [s] + headers):
            jobs.append([hipcc, *FLAGS, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print("[m4ri_amd.build]", " ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, os.path.splitext(s)[0] + ".o") for s in SOURCES]
    emap = export_map()
    if force or jobs or _stale(LIB, objs + [emap]):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, f"-Wl,--version-script={emap}", "-ldl", "-lz"])
    pobjs = [os.path.join(OBJ, os.path.splitext(s)[0] + ".o") for s in PASS_SOURCES]
    pmap = pass_export_map()
    if force or jobs or _stale(PASS_LIB, pobjs + [pmap]):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", PASS_LIB, *pobjs, f"-Wl,--version-script={pmap}", "-Wl,--no-undefined"])
    lobjs = [os.path.join(OBJ, os.path.splitext(s)[0] + ".o") for s in LEAF_SOURCES]
    lmap = leaf_export_map()
    if force or jobs or _stale(LEAF_LIB, lobjs + [lmap]):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LEAF_LIB, *lobjs, f"-Wl,--version-script={lmap}", "-Wl,--no-undefined"])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))

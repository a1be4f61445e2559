#!/usr/bin/env python3
"""The parameter table of tests/test_gpu_passes.py against what really ran: which pass kernel instantiations the module's process
launched, by its rocprofv3 kernel trace, compared with the instantiations the table means to reach.

    python tools/pass_coverage.py --table          # the table: row, launcher's answer, form, routing condition
    python tools/pass_coverage.py <results.db>     # the comparison

The argument is the rocpd database of one `rocprofv3 --kernel-trace --stats -- python -m pytest tests/test_gpu_passes.py -m gpu ...` run.
An instantiation the table names and the trace does not hold is a missing test row; exit status 1 then.  (Kernel trace only: counters
belong in a run of their own.)"""
import os
import re
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PASS_KERNEL = re.compile(r"_ZN12_GLOBAL__N_1\d+((?:winograd|scheme)_\w+_kernel|a4_pack_kernel)(?:(I.*?E)Ev|E)")
DEMANGLED = re.compile(r"\b((?:winograd|scheme)_\w+_kernel|a4_pack_kernel)(<[^>]*>)?\(")


def instantiation(mangled: str):
    """'_ZN12_GLOBAL__N_120winograd_down_kernelIDv2_yLb1EEEv...' -> 'winograd_down_kernel<word2,true>' (None: not a pass kernel)."""
    m = PASS_KERNEL.match(mangled)
    if not m:
        d = DEMANGLED.search(mangled)   # a trace that holds demangled names
        if not d or mangled.startswith("_Z"):
            return None
        if not d.group(2):
            return d.group(1)
        args = [a.strip() for a in d.group(2)[1:-1].split(",")]
        args = ["word2" if "__vector(2)" in a or "ext_vector_type(2)" in a else "word" if a.startswith("unsigned long") else re.sub(r"^\(\w+\)", "", a) for a in args]
        return f"{d.group(1)}<{','.join(args)}>"
    name, targs = m.group(1), m.group(2)
    if not targs:
        return name
    out = []
    for tok in re.findall(r"Dv2_y|Lb[01]E|Li\d+E|[ym]", targs[1:-1]):
        out.append("word2" if tok == "Dv2_y" else "word" if tok in "ym" else ("true" if tok == "Lb1E" else "false") if tok.startswith("Lb") else tok[2:-1])
    return f"{name}<{','.join(out)}>"


def traced(path):
    db = sqlite3.connect(path)
    names = dict(db.execute("select id, kernel_name from rocpd_info_kernel_symbol"))
    calls = {}
    for (kid,) in db.execute("select kernel_id from rocpd_kernel_dispatch"):
        k = instantiation(names.get(kid, "").replace(".kd", ""))
        if k:
            calls[k] = calls.get(k, 0) + 1
    return calls


def main(argv):
    import test_gpu_passes as T
    if argv == ["--table"]:
        for r in T.ROWS:
            print(f"{T.row_id(r):64s} rc {r.rc}  {r.reach:40s} {r.why}")
        return 0
    if len(argv) != 1:
        print(__doc__)
        return 2
    want, got = T.kernels_named(), traced(argv[0])
    assert want == T.expected_kernels()   # (test_the_table_names_every_instantiation)
    print(f"== {len(got)} distinct pass kernel instantiations in the trace, {len(want)} named by the table = every one the launchers can start")
    for k in sorted(set(got) | want):
        mark = "ok     " if k in got and k in want else "MISSING" if k in want else "also   "
        print(f"  {mark} {k:48s} {got.get(k, 0):6d} launches")
    return 1 if want - set(got) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

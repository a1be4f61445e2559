"""The read side of the batched calls: m4ri_amd_weight_batch_dev (all three outputs), m4ri_amd_row_span_batch_dev (both outputs) and
m4ri_amd_mismatch_batch_dev on device-resident operands of `--mbytes` MB (dense members back to back, random: fill_dev), each on the
paths it can be routed to (M4RI_AMD_REDUCE_BATCH_PATH0_MAX / _PATH1_MAX), with a device-to-device copy of the same buffer in the same
run as the yardstick.  The table is what the two path bounds are chosen from:
  W0  members of 64 rows and 1, 2, 4, 8, 16 words per row: path 0 (a wave per member) against path 1 (a workgroup per member);
  T1  squares of 64 ... 2048: path 1 against path 2 (chunks of rows, atomics);
and one 65536 x 65536 matrix (512 MB, batch 1) on path 2.  mismatch compares A with a copy of itself, so it reads every word of both
and never leaves early; row_span on random members may leave early on path 2 and is reported for what it is.

All contenders of a shape are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls
between two HIP events sized to `--window` seconds.  Columns: ms per call (median of the windows), the spread of the windows
((max - min) / median), TB/s of operand bytes read, and that rate as a share of the copy's bytes moved per second (a copy of n bytes
moves 2 n).  `clear`: the slowest window of the lower path is faster than the fastest of the higher (the gain exceeds the spread);
`LOSES`: the other way round.

  python tools/bench_reduce_batch.py [--reps 5] [--window 0.3] [--mbytes 256] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

PATH0, PATH1 = "M4RI_AMD_REDUCE_BATCH_PATH0_MAX", "M4RI_AMD_REDUCE_BATCH_PATH1_MAX"
ROUTES = {0: {PATH0: "16"}, 1: {PATH0: "0", PATH1: str(1 << 30)}, 2: {PATH0: "0", PATH1: "0"}}
W0_SWEEP = [(64, 64 * w, (0, 1)) for w in (1, 2, 4, 8, 16)]
T1_SWEEP = [(d, d, (1, 2)) for d in (64, 128, 256, 512, 1024, 2048)]
BIG = [(65536, 65536, (2,))]


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def alternate(fns, args):
    """{name: windows} of the contenders, warmed up, window sizes from a first timing, then `reps` rounds one after the other."""
    for fn in list(fns.values()) * 2:
        fn()
    torch.cuda.synchronize()
    calls = {k: max(3, int(args.window / window(fn, 3)) + 1) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            t[k].append(window(fn, calls[k]))
    return t


def med(v):
    return statistics.median(v)


def spread(v):
    return (max(v) - min(v)) / med(v)


def routed(path, fn):
    def run():
        os.environ.update(ROUTES[path])
        try:
            fn()
        finally:
            for k in ROUTES[path]:
                del os.environ[k]
    return run


def run_shape(nrows, ncols, paths, args):
    w = (ncols + 63) // 64
    words = nrows * w
    batch = max(1, -(-args.mbytes * 1000000 // (8 * words)))
    A = torch.empty(batch * words, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(A.data_ptr(), w, batch * nrows, ncols, 17 + nrows + ncols, 0)
    B, Y = A.clone(), torch.empty_like(A)
    st = torch.cuda.current_stream().cuda_stream
    total = torch.zeros(batch, dtype=torch.int64, device="cuda")
    light = torch.zeros(batch, dtype=torch.int64, device="cuda")
    rows = torch.zeros(batch * nrows, dtype=torch.int32, device="cuda")
    first, end = torch.zeros(batch, dtype=torch.int32, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda")
    a = (A.data_ptr(), w, words)
    weight = lambda: m4ri_amd.weight_batch_dev(*a, 0, 0, 0, nrows, ncols, batch, total.data_ptr(), rows.data_ptr(), light.data_ptr(), stream=st)
    span = lambda: m4ri_amd.row_span_batch_dev(*a, nrows, ncols, batch, first.data_ptr(), end.data_ptr(), stream=st)
    mism = lambda: m4ri_amd.mismatch_batch_dev(*a, B.data_ptr(), w, words, nrows, ncols, batch, first.data_ptr(), stream=st)
    fns = {"copy": lambda: Y.copy_(A)}
    for p in paths:
        fns[f"weight{p}"], fns[f"span{p}"] = routed(p, weight), routed(p, span)
    fns[f"mismatch{paths[0]}"] = routed(paths[0], mism)
    results = {}
    for p in paths:  # the same answers on every path
        fns[f"weight{p}"](); fns[f"span{p}"]()
        torch.cuda.synchronize()
        results[p] = [x.clone() for x in (total, rows, light, first, end)]
    equal = all(torch.equal(x, y) for p in paths[1:] for x, y in zip(results[paths[0]], results[p]))
    equal = equal and int(results[paths[0]][0].sum()) == int(results[paths[0]][1].sum(dtype=torch.int64))
    t = alternate(fns, args)
    nbytes = 8 * batch * words
    copy_rate = 2 * nbytes / med(t["copy"])
    row = dict(nrows=nrows, ncols=ncols, batch=batch, mbytes=nbytes / 1e6, equal=equal, copy_ms=med(t["copy"]) * 1e3, copy_spread=spread(t["copy"]),
               copy_tbytes_per_s=copy_rate / 1e12, calls={}, windows_ms={k: [x * 1e3 for x in v] for k, v in t.items()})
    for k, v in t.items():
        if k == "copy":
            continue
        read = nbytes * (2 if k.startswith("mismatch") else 1)
        row["calls"][k] = dict(ms=med(v) * 1e3, spread=spread(v), tbytes_per_s=read / med(v) / 1e12, of_copy=read / med(v) / copy_rate)
    if len(paths) == 2:
        lo, hi = t[f"weight{paths[0]}"], t[f"weight{paths[1]}"]
        row.update(clear=max(lo) < min(hi), loses=min(lo) > max(hi), hi_over_lo=med(hi) / med(lo))
    for k, c in row["calls"].items():
        print(f"{nrows:>6} {ncols:>6} {batch:>8} {k:>10} {c['ms']:>9.4f} {c['spread'] * 100:>5.1f}% {c['tbytes_per_s']:>6.3f} {c['of_copy'] * 100:>6.1f}%", flush=True)
    verdict = "" if len(paths) < 2 else f"  weight path {paths[1]} / path {paths[0]} = {row['hi_over_lo']:.2f}x, " + (
        "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread")
    print(f"{nrows:>6} {ncols:>6} {batch:>8} {'copy':>10} {row['copy_ms']:>9.4f} {row['copy_spread'] * 100:>5.1f}% {row['copy_tbytes_per_s']:>6.3f} (moved)"
          f"  results {'equal' if equal else 'DIFFER'}{verdict}", flush=True)
    return row


def bound_from(rows):
    """The index of the largest shape of a sweep at which the lower path is clear of the higher, no smaller one losing; -1 = none."""
    best = -1
    for i, r in enumerate(rows):
        if r["loses"] or not r["equal"]:
            break
        if r["clear"]:
            best = i
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--mbytes", type=int, default=256, help="the operand is at least this many MB")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.reps >= 3 and args.window >= 0.3 and 256 <= args.mbytes <= 2000
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    P = m4ri_amd.plan_reduce_batch
    lib_w0 = max(w for w in range(1, 65) if P(64, 64 * w) == 0)
    lib_d1 = max(d for d in range(64, 8193, 64) if P(d, d) != 2)
    print(f"weight / row_span / mismatch _batch_dev, the number after a call's name is its path; ms per call, median of {args.reps} alternating windows of "
          f">= {args.window} s; operand >= {args.mbytes} MB; library bounds: path 0 up to {lib_w0} words per row, path 1 up to the square of {lib_d1}")
    print(f"{'nrows':>6} {'ncols':>6} {'batch':>8} {'call':>10} {'ms':>9} {'spread':>6} {'TB/s':>6} {'of copy':>7}")
    w0_rows = [run_shape(*s, args) for s in W0_SWEEP]
    t1_rows = [run_shape(*s, args) for s in T1_SWEEP]
    big = [run_shape(*s, args) for s in BIG]
    i0, i1 = bound_from(w0_rows), bound_from(t1_rows)
    w0 = W0_SWEEP[i0][1] // 64 if i0 >= 0 else 0
    d1 = T1_SWEEP[i1][0] if i1 >= 0 else 0
    print(f"W0 from this table: {w0} words per row (the largest of the sweep at which path 0 is clear of path 1, no smaller one losing; 0 = none)")
    print(f"T1 from this table: the square of {d1} = {d1 * d1 // 64} words per member (the largest of the sweep at which path 1 is clear of path 2; 0 = none)")
    print(f"all results equal: {'yes' if all(r['equal'] for r in w0_rows + t1_rows + big) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(w0=w0, d1=d1, w0_sweep=w0_rows, t1_sweep=t1_rows, big=big), f, indent=1)


if __name__ == "__main__":
    main()

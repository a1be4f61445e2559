"""Transposes of many small matrices: m4ri_amd_transpose_batch_dev against the batched tile launch and against what the batch cost
before the call existed, a host loop of m4ri_amd_transpose_dev with one call per member -- in the same process on the same
device-resident buffers.  Per shape three contenders:
  a  the new call on its register path: path 0 up to 64, above it path 1 forced with M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX=1024
     whatever T1 the library was built with (the table is what T1 is chosen from);
  b  the batched tile launch, path 2 (M4RI_AMD_TRANSPOSE_BATCH_TILES=1: the same call, every member through the tile kernel);
  c  the loop, one m4ri_amd_transpose_dev per member, over the first min(batch, --loop-members) members; its time is per member,
     and `loop x` = that time over contender a's time per member.
All are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls between two HIP events
sized to `--window` seconds.  Members are dense and back to back (stride = width), random (fill_dev); the batch makes A and D
`--mbytes` MB each or more.  a and b are compared on every word of D (D starts zero, so path 2's zero tail bits are path 1's kept
ones).  In place (D == A) is timed against contender a at 64, 256 and 1024.

Columns: ms per call (median of the windows) and the spread of the windows ((max - min) / median) of a and b; b/a; `clear` = the
slowest window of a is faster than the fastest of b (the gain exceeds the spread), `LOSES` = the other way round; achieved bytes/s of
a from the algorithmic bytes (every word of A read once, every word of D written once) and its share of what a plain device copy of
the same bytes achieves on this box in the same run (a copy of n bytes counts 2 n: n read, n written).

  python tools/bench_transpose_batch.py [--reps 5] [--window 0.3] [--mbytes 256] [--loop-members 20000] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

OVERRIDE, TILES = "M4RI_AMD_TRANSPOSE_BATCH_PATH1_MAX", "M4RI_AMD_TRANSPOSE_BATCH_TILES"
SQUARES = (16, 32, 64, 128, 256, 512, 1024)
SHAPES = [(d, d) for d in SQUARES] + [(48, 64), (64, 200), (1024, 64)]
INPLACE = (64, 256, 1024)
CANDIDATES = (128, 256, 512, 1024)


def w_of(n):
    return (n + 63) // 64


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


def with_env(name, value, fn):
    def run():
        os.environ[name] = value
        try:
            fn()
        finally:
            del os.environ[name]
    return run


def run_shape(nrows, ncols, args):
    wa, wd = w_of(ncols), w_of(nrows)
    a_words, d_words = nrows * wa, ncols * wd
    batch = max(1, -(-args.mbytes * 1000000 // (8 * min(a_words, d_words))))
    A = torch.empty(batch * a_words, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(A.data_ptr(), wa, batch * nrows, ncols, 11 + nrows, 0)
    Da, Db = torch.zeros(batch * d_words, dtype=torch.int64, device="cuda"), torch.zeros(batch * d_words, dtype=torch.int64, device="cuda")
    half = (A.numel() + Da.numel()) // 2  # the copy of the same bytes: half of them read, half written
    X, Y = torch.empty(half, dtype=torch.int64, device="cuda"), torch.zeros(half, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L = m4ri_amd.lib()
    call = lambda D: m4ri_amd.transpose_batch_dev(D.data_ptr(), wd, d_words, A.data_ptr(), wa, a_words, nrows, ncols, batch, stream=st)
    path = 0 if max(nrows, ncols) <= 64 else 1
    nloop = min(batch, args.loop_members)

    def loop():
        pa, pd = A.data_ptr(), Db.data_ptr()
        for b in range(nloop):
            L.m4ri_amd_transpose_dev(pd + 8 * b * d_words, wd, pa + 8 * b * a_words, wa, nrows, ncols, st)

    fns = {"a": with_env(OVERRIDE, "1024", lambda: call(Da)), "b": with_env(TILES, "1", lambda: call(Db)), "c": loop, "copy": lambda: Y.copy_(X)}
    t = alternate(fns, args)
    fns["a"](); fns["b"]()
    torch.cuda.synchronize()
    equal = bool(torch.equal(Da, Db))
    nbytes = 8 * batch * (a_words + d_words)
    m = {k: med(v) for k, v in t.items()}
    rate, copy_rate = nbytes / m["a"], 16 * half / m["copy"]
    row = dict(nrows=nrows, ncols=ncols, batch=batch, path=path, equal=equal, a_ms=m["a"] * 1e3, b_ms=m["b"] * 1e3, a_spread=spread(t["a"]),
               b_spread=spread(t["b"]), b_over_a=m["b"] / m["a"], clear=max(t["a"]) < min(t["b"]), loses=min(t["a"]) > max(t["b"]),
               loop_members=nloop, loop_us_per_member=m["c"] / nloop * 1e6, loop_spread=spread(t["c"]),
               loop_over_a=(m["c"] / nloop) / (m["a"] / batch), mbytes=nbytes / 1e6, tbytes_per_s=rate / 1e12, copy_tbytes_per_s=copy_rate / 1e12,
               of_copy=rate / copy_rate, windows_ms={k: [x * 1e3 for x in v] for k, v in t.items()})
    print(f"{nrows:>5} {ncols:>5} {batch:>8} {path:>4} {row['a_ms']:>9.4f} {row['a_spread'] * 100:>5.1f}% {row['b_ms']:>9.4f} {row['b_spread'] * 100:>5.1f}% "
          f"{row['b_over_a']:>6.2f}x {'yes' if row['clear'] else 'LOSES' if row['loses'] else 'no':>5} {'ok' if equal else 'DIFFER':>6} "
          f"{row['loop_us_per_member']:>9.3f} {row['loop_spread'] * 100:>5.1f}% {row['loop_over_a']:>9.1f}x {row['tbytes_per_s']:>6.3f} "
          f"{row['copy_tbytes_per_s']:>6.3f} {row['of_copy'] * 100:>5.1f}%", flush=True)
    return row


def run_inplace(n, args):
    w = w_of(n)
    words = n * w
    batch = max(1, -(-args.mbytes * 1000000 // (8 * words)))
    A = torch.empty(batch * words, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(A.data_ptr(), w, batch * n, n, 13 + n, 0)
    D, B = torch.zeros_like(A), A.clone()
    st = torch.cuda.current_stream().cuda_stream
    out = with_env(OVERRIDE, "1024", lambda: m4ri_amd.transpose_batch_dev(D.data_ptr(), w, words, A.data_ptr(), w, words, n, n, batch, stream=st))
    inp = lambda: m4ri_amd.transpose_batch_dev(B.data_ptr(), w, words, B.data_ptr(), w, words, n, n, batch, stream=st)
    t = alternate({"out": out, "in": inp}, args)
    B.copy_(A)
    inp(); out()
    torch.cuda.synchronize()
    equal = bool(torch.equal(B, D))
    nbytes = 16 * batch * words
    row = dict(n=n, batch=batch, equal=equal, out_ms=med(t["out"]) * 1e3, in_ms=med(t["in"]) * 1e3, out_spread=spread(t["out"]), in_spread=spread(t["in"]),
               out_over_in=med(t["out"]) / med(t["in"]), in_tbytes_per_s=nbytes / med(t["in"]) / 1e12, out_tbytes_per_s=nbytes / med(t["out"]) / 1e12)
    print(f"{n:>5} {batch:>8} {row['out_ms']:>9.4f} {row['out_spread'] * 100:>5.1f}% {row['in_ms']:>9.4f} {row['in_spread'] * 100:>5.1f}% "
          f"{row['out_over_in']:>6.2f}x {'ok' if equal else 'DIFFER':>6} {row['out_tbytes_per_s']:>6.3f} {row['in_tbytes_per_s']:>6.3f}", flush=True)
    return row


def bound_from(rows):
    """T1: the largest candidate at which path 1 is clear of path 2 while no smaller candidate loses by more than the spread."""
    sq = {r["nrows"]: r for r in rows if r["nrows"] == r["ncols"]}
    t1 = 64
    for d in CANDIDATES:
        if sq[d]["loses"] or not sq[d]["equal"]:
            break
        if sq[d]["clear"]:
            t1 = d
    return t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--mbytes", type=int, default=256, help="A and D are at least this many MB each")
    ap.add_argument("--loop-members", type=int, default=20000, help="the per-member loop runs over at most this many members")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.reps >= 3 and args.window >= 0.3 and 256 <= args.mbytes <= 2000
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    lib_t1 = max(d for d in range(64, 1025, 64) if m4ri_amd.plan_transpose_batch(d, d) != 2)
    print(f"transpose_batch_dev: a = register paths (0 / forced 1), b = batched tile launch (path 2), c = loop of transpose_dev per member; ms per call, "
          f"median of {args.reps} alternating windows of >= {args.window} s; A and D >= {args.mbytes} MB each; library T1 = {lib_t1}")
    print(f"{'nrows':>5} {'ncols':>5} {'batch':>8} {'path':>4} {'a ms':>9} {'spread':>6} {'b ms':>9} {'spread':>6} {'b/a':>7} {'clear':>5} {'a==b':>6} "
          f"{'c us/mem':>9} {'spread':>6} {'loop x':>10} {'TB/s':>6} {'copy':>6} {'of it':>6}")
    rows = [run_shape(r, c, args) for (r, c) in SHAPES]
    print(f"in place (D == A) against out of place (contender a): ms per call, TB/s of 2 x the members' bytes")
    print(f"{'n':>5} {'batch':>8} {'out ms':>9} {'spread':>6} {'in ms':>9} {'spread':>6} {'out/in':>7} {'equal':>6} {'out':>6} {'in':>6}")
    inplace = [run_inplace(n, args) for n in INPLACE]
    t1 = bound_from(rows)
    print(f"T1 from this table: {t1} (the largest of {', '.join(map(str, CANDIDATES))} at which path 1 is clear of path 2 on the square, with no smaller "
          f"one losing by more than the spread; 64 = none)")
    print(f"all results equal: {'yes' if all(r['equal'] for r in rows + inplace) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(t1=t1, rows=rows, inplace=inplace), f, indent=1)


if __name__ == "__main__":
    main()

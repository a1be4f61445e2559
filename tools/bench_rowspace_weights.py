"""m4ri_amd_rowspace_weights_batch_dev on device-resident random generators, on the paths it can be routed to
(M4RI_AMD_ROWSPACE_PATH0_MAX), with and without the histogram (without: lightest alone at w_min = 1, the minimum distance), against
the contender a caller had before: all 2^k words materialised as the product of the 2^k x k message matrix (row x is the word x) with
G (m4ri_amd_mul_small_batch_dev for members, m4ri_amd_m4rm_dev for a single one), their row weights by m4ri_amd_weight_batch_dev, then
torch.bincount and a masked minimum of (wt << 40) | x.  The contender is run up to the k at which its 2^k rows fit (its row count is
an int32, its words 2^k * n bits of memory); its results must equal the call's.
  members  k = 8, 12, 16 at n = 64, 128, 256, 512, 2^24 messages per call (65536, 4096, 256 members), both paths;
  bound    k = 10, 14, 18, 20 at n = 256 besides, the same 2^24 messages: the sweep the path-0 bound K0 is chosen from;
  single   one member of k = 24, 28, 32 at n = 128 and 512 on path 1.

All contenders of a shape are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls
between two HIP events sized to `--window` seconds.  Columns: ms per call (median of the windows), the spread of the windows
((max - min) / median), 10^12 words weighed per second, and the contender's time over the call's (on the path the library takes).
`clear`: the slowest window of path 0 is faster than the fastest of path 1 (the gain exceeds the spread); `LOSES`: the other way round.

  python tools/bench_rowspace_weights.py [--reps 3] [--window 0.3] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

PATH0 = "M4RI_AMD_ROWSPACE_PATH0_MAX"
ROUTES = {0: "26", 1: "-1"}
MESSAGES = 1 << 24
MEMBERS = [(k, n) for k in (8, 12, 16) for n in (64, 128, 256, 512)]
BOUND = [(k, 256) for k in (10, 14, 18, 20)]
SINGLE = [(k, n) for k in (24, 28, 32) for n in (128, 512)]
CONTENDER_K_MAX = 28  # 2^k rows: an int32 row count, and 2^28 x 512 bits are 16 GiB


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
        os.environ[PATH0] = ROUTES[path]
        try:
            fn()
        finally:
            del os.environ[PATH0]
    return run


class Contender:
    """The words themselves: C_b = X * G_b (2^k x n), their row weights, bincount and the masked minimum key."""

    def __init__(self, G, k, n, batch, st):
        w, rows = n // 64, 1 << k
        self.k, self.n, self.batch, self.st, self.w, self.rows = k, n, batch, st, w, rows
        self.G = G
        self.X = torch.arange(rows, dtype=torch.int64, device="cuda")        # row x of the message matrix is the word x
        self.C = torch.empty(batch * rows * w, dtype=torch.int64, device="cuda")
        self.rw = torch.empty(batch * rows, dtype=torch.int32, device="cuda")
        self.offs = (torch.arange(batch, dtype=torch.int64, device="cuda") * (n + 1)).repeat_interleave(rows) if batch > 1 else None
        self.none = torch.tensor(-1, dtype=torch.int64, device="cuda")

    def words(self):
        k, n, w, rows = self.k, self.n, self.w, self.rows
        if self.batch == 1:
            m4ri_amd.m4rm_dev(self.C.data_ptr(), w, self.X.data_ptr(), 1, self.G.data_ptr(), w, rows, k, n, stream=self.st)
        else:
            m4ri_amd.mul_small_batch_dev(self.C.data_ptr(), w, rows * w, self.X.data_ptr(), 1, 0, self.G.data_ptr(), w, k * w, rows, k, n, self.batch,
                                         stream=self.st)
        m4ri_amd.weight_batch_dev(self.C.data_ptr(), w, rows * w, 0, 0, 0, rows, n, self.batch, row_weight=self.rw.data_ptr(), stream=self.st)

    def hist(self):
        idx = self.rw.long()
        if self.offs is not None:
            idx += self.offs
        return torch.bincount(idx, minlength=self.batch * (self.n + 1))

    def lightest(self, w_min):
        wt = self.rw.long().view(self.batch, self.rows)
        key = (wt << 40) | self.X[None, :]
        key = torch.where(wt >= w_min, key, torch.iinfo(torch.int64).max).min(dim=1).values
        return torch.where(key == torch.iinfo(torch.int64).max, self.none, key)

    def run(self, want_hist):
        self.words()
        return (self.hist() if want_hist else None), self.lightest(1)


def run_shape(k, n, paths, args):
    batch = max(1, MESSAGES >> k)
    w = n // 64
    st = torch.cuda.current_stream().cuda_stream
    G = torch.empty(batch * k * w, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(G.data_ptr(), w, batch * k, n, 23 + k + n, 0)
    hist = torch.zeros(batch * (n + 1), dtype=torch.int64, device="cuda")
    light = torch.zeros(batch, dtype=torch.int64, device="cuda")
    g = (G.data_ptr(), w, k * w, k, n, 0, 0, batch, 1)
    lib_path = m4ri_amd.plan_rowspace_weights_batch(k, n)
    con = None
    if k <= CONTENDER_K_MAX:
        try:
            con = Contender(G, k, n, batch, st)
        except torch.cuda.OutOfMemoryError:
            con = None
    rows = []
    for want_hist in (True, False):
        call = lambda: m4ri_amd.rowspace_weights_batch_dev(*g, hist.data_ptr() if want_hist else 0, light.data_ptr(), stream=st)
        fns = {f"path{p}": routed(p, call) for p in paths}
        results = {}
        for p in paths:  # the same answers on every path, and the contender's
            hist.fill_(-7), light.fill_(-7)
            fns[f"path{p}"]()
            torch.cuda.synchronize()
            results[p] = (hist.clone() if want_hist else None, light.clone())
        if con is not None:
            fns["contender"] = lambda: con.run(want_hist)
            results["contender"] = con.run(want_hist)
        first = results[paths[0]]
        equal = all((not want_hist or torch.equal(first[0], r[0])) and torch.equal(first[1], r[1]) for r in results.values())
        equal = equal and (not want_hist or bool((first[0].view(batch, n + 1).sum(dim=1) == 1 << k).all()))
        t = alternate(fns, args)
        words = batch << k
        row = dict(k=k, n=n, batch=batch, hist=want_hist, equal=equal, lib_path=lib_path, calls={}, windows_ms={c: [x * 1e3 for x in v] for c, v in t.items()})
        for c, v in t.items():
            row["calls"][c] = dict(ms=med(v) * 1e3, spread=spread(v), twords_per_s=words / med(v) / 1e12)
        mine = f"path{lib_path}" if f"path{lib_path}" in t else f"path{paths[0]}"
        row["contender_over_call"] = med(t["contender"]) / med(t[mine]) if con is not None else None
        if len(paths) == 2:
            lo, hi = t["path0"], t["path1"]
            row.update(clear=max(lo) < min(hi), loses=min(lo) > max(hi), path1_over_path0=med(hi) / med(lo))
        for c, v in row["calls"].items():
            print(f"{k:>3} {n:>5} {batch:>6} {'hist+light' if want_hist else 'light':>10} {c:>10} {v['ms']:>10.4f} {v['spread'] * 100:>5.1f}% {v['twords_per_s']:>8.4f}", flush=True)
        verdict = "" if len(paths) < 2 else f"  path 1 / path 0 = {row['path1_over_path0']:.2f}x, " + (
            "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread")
        factor = f"  contender / call (path {mine[4:]}) = {row['contender_over_call']:.1f}x" if con is not None else "  contender: does not fit"
        print(f"{k:>3} {n:>5} {batch:>6} {'hist+light' if want_hist else 'light':>10} results {'equal' if equal else 'DIFFER'}{factor}{verdict}", flush=True)
        rows.append(row)
    del con
    torch.cuda.empty_cache()
    return rows


def bound_from(rows):
    """The largest k of the sweep (ascending) at which path 0 is clear of path 1 in both forms, no smaller one losing; -1 = none."""
    best = -1
    for k in sorted({r["k"] for r in rows}):
        at = [r for r in rows if r["k"] == k]
        if any(r["loses"] or not r["equal"] for r in at):
            break
        if all(r["clear"] for r in at):
            best = k
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.reps >= 3 and args.window >= 0.3
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    P = m4ri_amd.plan_rowspace_weights_batch
    lib_k0 = max(k for k in range(41) if P(k, 64) == 0)
    print(f"rowspace_weights_batch_dev; ms per call, median of {args.reps} alternating windows of >= {args.window} s; library bound: path 0 up to k = {lib_k0}")
    print(f"{'k':>3} {'n':>5} {'batch':>6} {'outputs':>10} {'contender':>10} {'ms':>10} {'spread':>6} {'Twords/s':>8}")
    members = [r for s in MEMBERS for r in run_shape(*s, (0, 1), args)]
    bound = [r for s in BOUND for r in run_shape(*s, (0, 1), args)]
    single = [r for s in SINGLE for r in run_shape(*s, (1,), args)]
    k0 = bound_from([r for r in members + bound if r["n"] == 256])
    print(f"K0 from this table: {k0} (the largest k of the n = 256 sweep at which path 0 is clear of path 1 with and without hist, no smaller one losing; -1 = none)")
    slower = [(r["k"], r["n"], r["hist"]) for r in members + bound + single if r["contender_over_call"] is not None and r["contender_over_call"] < 1]
    print(f"slower than the contender at: {slower if slower else 'no measured shape'}")
    print(f"all results equal: {'yes' if all(r['equal'] for r in members + bound + single) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(k0=k0, members=members, bound=bound, single=single), f, indent=1)


if __name__ == "__main__":
    main()

"""m4ri_amd_row_sums_weights_batch_dev on device-resident random generators, on the paths it can be routed to
(M4RI_AMD_ROW_SUMS_PATH0_MAX), with and without the histogram (without: lightest alone at w_min = 1), against the contender a caller
had before: the C(k, t) x k selection matrix materialised once (row r selects the set of colexicographic rank r), its product with G
(m4ri_amd_mul_small_batch_dev for members, m4ri_amd_m4rm_dev for a single one), the row weights of the product by
m4ri_amd_weight_batch_dev, then torch.bincount and a masked minimum of (wt << 40) | r.  The contender's timing leaves the making of the
selection matrix out; it is run where its words fit (CONTENDER_WORDS); its results must equal the call's.
  shapes   k = 16 (t = 2, 3; n = 64, 256; 65 536 members), k = 64 (t = 2, 3, 4; n = 128, 512; 1 024), k = 256 (t = 2, 3; n = 256, 1024; 16),
           k = 1024 (t = 2, 3; n = 1024; one member), k = 512 (t = 4; n = 512; one member);
  bound    t = 2 and t = 3 at n = 256 over a sweep of k, about 2^24 sums per call: what the path-0 bound M0 is chosen from.

All contenders of a shape are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls
between two HIP events sized to `--window` seconds.  Columns: ms per call (median of the windows), the spread of the windows
((max - min) / median), 10^12 words weighed per second (sums x words(n) x members), and the contender's time over the call's (on the
path the library takes).  `clear`: the slowest window of path 0 is faster than the fastest of path 1 (the gain exceeds the spread);
`LOSES`: the other way round.

  python tools/bench_row_sums_weights.py [--reps 3] [--window 0.3] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
from math import comb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

PATH0 = "M4RI_AMD_ROW_SUMS_PATH0_MAX"
M0_MAX = 1 << 24
ROUTES = {0: str(M0_MAX), 1: "-1"}
SUMS = 1 << 24
SHAPES = ([(16, t, n, 65536) for t in (2, 3) for n in (64, 256)] + [(64, t, n, 1024) for t in (2, 3, 4) for n in (128, 512)]
          + [(256, t, n, 16) for t in (2, 3) for n in (256, 1024)] + [(1024, t, 1024, 1) for t in (2, 3)] + [(512, 4, 512, 1)])
BOUND = [(k, 2, 256, None) for k in (16, 32, 46, 64, 91, 128, 182, 256, 362)] + [(k, 3, 256, None) for k in (16, 24, 30, 40, 50, 64)]
CONTENDER_WORDS = 1 << 30  # of the materialised words: 8 GiB


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
    """The words themselves: C_b = S * G_b (C(k, t) x n), their row weights, bincount and the masked minimum key."""

    def __init__(self, G, k, t, n, batch, st):
        w, wk, rows = n // 64, (k + 63) // 64, comb(k, t)
        self.k, self.n, self.batch, self.st, self.w, self.wk, self.rows = k, n, batch, st, w, wk, rows
        self.G = G
        sets = torch.combinations(torch.arange(k, device="cuda"), t)                       # rows x t, ascending in every row
        table = torch.tensor([[comb(i, j + 1) for j in range(t)] for i in range(k)], dtype=torch.int64, device="cuda")
        rank = table[sets, torch.arange(t, device="cuda")[None, :]].sum(dim=1)
        assert rank.numel() == rows and int(rank.max()) == rows - 1
        self.S = torch.zeros(rows * wk, dtype=torch.int64, device="cuda")                  # row r selects the set of rank r
        for j in range(t):
            self.S.index_put_((rank * wk + (sets[:, j] >> 6),), torch.ones_like(rank) << (sets[:, j] & 63), accumulate=True)
        del sets, rank
        self.R = torch.arange(rows, dtype=torch.int64, device="cuda")
        self.C = torch.empty(batch * rows * w, dtype=torch.int64, device="cuda")
        self.rw = torch.empty(batch * rows, dtype=torch.int32, device="cuda")
        self.offs = (torch.arange(batch, dtype=torch.int64, device="cuda") * (n + 1)).repeat_interleave(rows) if batch > 1 else None
        self.none = torch.tensor(-1, dtype=torch.int64, device="cuda")

    def words(self):
        k, n, w, rows = self.k, self.n, self.w, self.rows
        if self.batch == 1:
            m4ri_amd.m4rm_dev(self.C.data_ptr(), w, self.S.data_ptr(), self.wk, self.G.data_ptr(), w, rows, k, n, stream=self.st)
        else:
            m4ri_amd.mul_small_batch_dev(self.C.data_ptr(), w, rows * w, self.S.data_ptr(), self.wk, 0, self.G.data_ptr(), w, k * w, rows, k, n,
                                         self.batch, stream=self.st)
        m4ri_amd.weight_batch_dev(self.C.data_ptr(), w, rows * w, 0, 0, 0, rows, n, self.batch, row_weight=self.rw.data_ptr(), stream=self.st)

    def hist(self):
        idx = self.rw.long()
        if self.offs is not None:
            idx += self.offs
        return torch.bincount(idx, minlength=self.batch * (self.n + 1))

    def lightest(self, w_min):
        wt = self.rw.long().view(self.batch, self.rows)
        key = (wt << 40) | self.R[None, :]
        key = torch.where(wt >= w_min, key, torch.iinfo(torch.int64).max).min(dim=1).values
        return torch.where(key == torch.iinfo(torch.int64).max, self.none, key)

    def run(self, want_hist):
        self.words()
        return (self.hist() if want_hist else None), self.lightest(1)


def run_shape(k, t, n, batch, args):
    sums = comb(k, t)
    batch = batch or max(1, SUMS // sums)
    paths = ([0] if sums <= M0_MAX else []) + [1]
    w = n // 64
    st = torch.cuda.current_stream().cuda_stream
    G = torch.empty(batch * k * w, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(G.data_ptr(), w, batch * k, n, 23 + k + n + t, 0)
    hist = torch.zeros(batch * (n + 1), dtype=torch.int64, device="cuda")
    light = torch.zeros(batch, dtype=torch.int64, device="cuda")
    g = (G.data_ptr(), w, k * w, k, n, 0, 0, batch, t, 1)
    lib_path = m4ri_amd.plan_row_sums_weights_batch(k, n, t)
    con = None
    if sums * batch * w <= CONTENDER_WORDS:
        try:
            con = Contender(G, k, t, n, batch, st)
        except torch.cuda.OutOfMemoryError:
            con = None
    rows = []
    for want_hist in (True, False):
        call = lambda: m4ri_amd.row_sums_weights_batch_dev(*g, hist.data_ptr() if want_hist else 0, light.data_ptr(), stream=st)
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
        equal = equal and (not want_hist or bool((first[0].view(batch, n + 1).sum(dim=1) == sums).all()))
        tm = alternate(fns, args)
        words = sums * w * batch
        row = dict(k=k, t=t, n=n, batch=batch, sums=sums, hist=want_hist, equal=equal, lib_path=lib_path, calls={},
                   windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()})
        for c, v in tm.items():
            row["calls"][c] = dict(ms=med(v) * 1e3, spread=spread(v), twords_per_s=words / med(v) / 1e12)
        mine = f"path{lib_path}" if f"path{lib_path}" in tm else f"path{paths[0]}"
        row["contender_over_call"] = med(tm["contender"]) / med(tm[mine]) if con is not None else None
        if len(paths) == 2:
            lo, hi = tm["path0"], tm["path1"]
            row.update(clear=max(lo) < min(hi), loses=min(lo) > max(hi), path1_over_path0=med(hi) / med(lo))
        what = "hist+light" if want_hist else "light"
        for c, v in row["calls"].items():
            print(f"{k:>4} {t:>1} {n:>5} {batch:>6} {sums:>10} {what:>10} {c:>10} {v['ms']:>10.4f} {v['spread'] * 100:>5.1f}% {v['twords_per_s']:>8.4f}", flush=True)
        verdict = "" if len(paths) < 2 else f"  path 1 / path 0 = {row['path1_over_path0']:.2f}x, " + (
            "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread")
        factor = f"  contender / call (path {mine[4:]}) = {row['contender_over_call']:.1f}x" if con is not None else "  contender: does not fit"
        print(f"{k:>4} {t:>1} {n:>5} {batch:>6} {sums:>10} {what:>10} results {'equal' if equal else 'DIFFER'}{factor}{verdict}", flush=True)
        rows.append(row)
    del con
    torch.cuda.empty_cache()
    return rows


def bound_from(rows):
    """The largest number of sums per member of the sweep (ascending) at which path 0 is clear of path 1 in both forms, no smaller
    one losing; -1 = none."""
    best = -1
    for sums in sorted({r["sums"] for r in rows}):
        at = [r for r in rows if r["sums"] == sums]
        if any(r["loses"] or not r["equal"] for r in at):
            break
        if all(r["clear"] for r in at):
            best = sums
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
    P = m4ri_amd.plan_row_sums_weights_batch
    lib_m0 = max(comb(k, 2) for k in range(2, 1025) if P(k, 64, 2) == 0)
    print(f"row_sums_weights_batch_dev; ms per call, median of {args.reps} alternating windows of >= {args.window} s; library bound: path 0 up to "
          f"C(k, 2) = {lib_m0} sums per member")
    print(f"{'k':>4} {'t':>1} {'n':>5} {'batch':>6} {'sums':>10} {'outputs':>10} {'contender':>10} {'ms':>10} {'spread':>6} {'Twords/s':>8}")
    shapes = [r for s in SHAPES for r in run_shape(*s, args)]
    bound = [r for s in BOUND for r in run_shape(*s, args)]
    m0 = bound_from(bound)
    print(f"M0 from this table: {m0} (the largest number of sums per member of the n = 256 sweep at which path 0 is clear of path 1 with and "
          f"without hist, no smaller one losing; -1 = none)")
    slower = [(r["k"], r["t"], r["n"], r["hist"]) for r in shapes + bound if r["contender_over_call"] is not None and r["contender_over_call"] < 1]
    print(f"slower than the contender at: {slower if slower else 'no measured shape'}")
    print(f"all results equal: {'yes' if all(r['equal'] for r in shapes + bound) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(m0=m0, shapes=shapes, bound=bound), f, indent=1)


if __name__ == "__main__":
    main()

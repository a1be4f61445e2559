"""m4ri_amd_row_sums_collide_batch_dev on device-resident random generators: Stern's collision step (t1 left rows, t2 right rows, zero
on a window of ell columns) on the path the library takes, beside the only way the library had to the same words before: the
unfiltered enumeration m4ri_amd_row_sums_weights_batch_dev at t = t1 + t2 on the same members.  The two do not cover the same sets:
the join covers the N1 * N2 pairs with t1 rows in one half and t2 in the other and weighs the colliding ones, the enumeration weighs all
C(k, t) sets; both counts stand next to the times.
  shapes   (k, n, t1 = t2) = (64, 128, 2), (128, 256, 2), (256, 512, 2), (72, 256, 3), balanced halves, the window the columns 0 .. ell-1,
           ell = 8, 16, 24 (and 0 at the smallest shape); about 2^34 pairs per call, at least 256 and at most 8192 members;
  bound    N1 = C(64, 2) = 2016 against a ladder of N2 = C(k2, 2), n = 256, ell = 16, about 2^32 pairs per call, path 0 against path 1
           (M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX): what the path-0 bound P0 is chosen from.

All contenders of a row are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls between
two HIP events sized to `--window` seconds.  Columns: ms per call (median of the windows), the spread of the windows ((max - min) /
median), 10^9 pairs covered per second, 10^6 collisions weighed per second.  `clear`: the slowest window of path 0 is faster than the
fastest of path 1 (the gain exceeds the spread); `LOSES`: the other way round.

  python tools/bench_row_sums_collide.py [--reps 3] [--window 0.3] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
from math import comb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

PATH0 = "M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX"
P0_MAX = (1 << 32) - 1
ROUTES = {0: str(P0_MAX), 1: "-1"}
SHAPES = [(64, 128, 2, (0, 8, 16, 24)), (128, 256, 2, (8, 16, 24)), (256, 512, 2, (8, 16, 24)), (72, 256, 3, (8, 16, 24))]
PAIRS = 1 << 34        # per call of the shapes
BOUND_K1, BOUND_N, BOUND_ELL = 64, 256, 16
BOUND_K2 = (16, 23, 32, 46, 64, 91, 128, 182, 256, 362, 512)
BOUND_PAIRS = 1 << 32  # per call of the ladder


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


class Members:
    """`batch` random k x n generators, dense, with the outputs of a call."""

    def __init__(self, k, n, batch, seed):
        self.k, self.n, self.batch, self.w = k, n, batch, n // 64
        self.st = torch.cuda.current_stream().cuda_stream
        self.G = torch.empty(batch * k * self.w, dtype=torch.int64, device="cuda")
        m4ri_amd.fill_dev(self.G.data_ptr(), self.w, batch * k, n, seed, 0)
        self.hist = torch.zeros(batch * (n + 1), dtype=torch.int64, device="cuda")
        self.light = torch.zeros(batch, dtype=torch.int64, device="cuda")

    def collide(self, k1, t1, t2, ell):
        m4ri_amd.row_sums_collide_batch_dev(self.G.data_ptr(), self.w, self.k * self.w, self.k, self.n, 0, 0, self.batch, k1, t1, t2, 0, 0, ell, 1,
                                            self.hist.data_ptr(), self.light.data_ptr(), stream=self.st)

    def enumerate(self, t):
        m4ri_amd.row_sums_weights_batch_dev(self.G.data_ptr(), self.w, self.k * self.w, self.k, self.n, 0, 0, self.batch, t, 1, self.hist.data_ptr(),
                                            self.light.data_ptr(), stream=self.st)

    def answers(self, fn):
        self.hist.fill_(-7), self.light.fill_(-7)
        fn()
        torch.cuda.synchronize()
        return self.hist.clone(), self.light.clone()


def run_shape(k, n, t, ells, args):
    k1, n1 = k // 2, comb(k // 2, t)
    pairs, sets = n1 * comb(k - k1, t), comb(k, 2 * t)
    batch = min(8192, max(256, PAIRS // pairs))
    m = Members(k, n, batch, 31 + k + n + t)
    rows = []
    fns = {"enumeration": lambda: m.enumerate(2 * t)}
    for ell in ells:
        fns[f"ell={ell}"] = lambda ell=ell: m.collide(k1, t, t, ell)
    hits = {}
    for ell in ells:
        h, light = m.answers(fns[f"ell={ell}"])
        hits[ell] = int(h.sum())
        for path in (0, 1):   # the same answers on both paths
            if pairs <= P0_MAX:
                h2, l2 = m.answers(routed(path, fns[f"ell={ell}"]))
                assert torch.equal(h, h2) and torch.equal(light, l2), (k, n, t, ell, path)
    if 0 in ells:   # without a window the pairs are the sets of 2t rows with t in each half: the lightest of all is at most as light
        _, le = m.answers(fns["enumeration"])
        _, lc = m.answers(fns["ell=0"])
        assert bool(((le >> 40) <= (lc >> 40)).all())
    tm = alternate(fns, args)
    for name, v in tm.items():
        ell = None if name == "enumeration" else int(name[4:])
        row = dict(k=k, n=n, t1=t, t2=t, k1=k1, batch=batch, call=name, ell=ell, ms=med(v) * 1e3, spread=spread(v), windows_ms=[x * 1e3 for x in v],
                   covered=sets if ell is None else pairs, weighed=sets if ell is None else hits[ell] / batch,
                   lib_path=None if ell is None else m4ri_amd.plan_row_sums_collide_batch(k, n, k1, t, t, ell))
        row["gcovered_per_s"] = row["covered"] * batch / med(v) / 1e9
        row["mweighed_per_s"] = row["weighed"] * batch / med(v) / 1e6
        row["enumeration_over_call"] = med(tm["enumeration"]) / med(v)
        rows.append(row)
        what = f"C({k},{2 * t}) sets" if ell is None else f"N1*N2 pairs, path {row['lib_path']}"
        print(f"{k:>4} {n:>5} {t:>1}+{t:>1} {batch:>6} {name:>12} {row['covered']:>12} {row['weighed']:>14.1f} {row['ms']:>11.4f} {row['spread'] * 100:>5.1f}% "
              f"{row['gcovered_per_s']:>9.2f} {row['mweighed_per_s']:>10.2f} {row['enumeration_over_call']:>8.1f}x  {what}", flush=True)
    del m
    torch.cuda.empty_cache()
    return rows


def run_rung(k2, args):
    k1, n, ell = BOUND_K1, BOUND_N, BOUND_ELL
    k, n1, n2 = k1 + k2, comb(k1, 2), comb(k2, 2)
    pairs = n1 * n2
    batch = max(1, BOUND_PAIRS // pairs)
    m = Members(k, n, batch, 77 + k2)
    call = lambda: m.collide(k1, 2, 2, ell)
    fns = {f"path{p}": routed(p, call) for p in (0, 1)}
    a0, a1 = m.answers(fns["path0"]), m.answers(fns["path1"])
    equal = torch.equal(a0[0], a1[0]) and torch.equal(a0[1], a1[1])
    tm = alternate(fns, args)
    lo, hi = tm["path0"], tm["path1"]
    row = dict(k1=k1, k2=k2, n=n, ell=ell, n1=n1, n2=n2, pairs=pairs, batch=batch, equal=equal, slices=m4ri_amd.row_sums_collide_slices(k, n, k1, 2, 2, ell, batch),
               lib_path=m4ri_amd.plan_row_sums_collide_batch(k, n, k1, 2, 2, ell), ms={c: med(v) * 1e3 for c, v in tm.items()},
               spread={c: spread(v) for c, v in tm.items()}, windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()},
               clear=max(lo) < min(hi), loses=min(lo) > max(hi), path1_over_path0=med(hi) / med(lo))
    verdict = "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread"
    print(f"{k1:>3}+{k2:<4} {n2:>7} {pairs:>11} {batch:>6} {row['slices']:>6} {row['ms']['path0']:>10.4f} {row['spread']['path0'] * 100:>5.1f}% "
          f"{row['ms']['path1']:>10.4f} {row['spread']['path1'] * 100:>5.1f}%  path 1 / path 0 = {row['path1_over_path0']:.2f}x, {verdict}, results "
          f"{'equal' if equal else 'DIFFER'}", flush=True)
    del m
    torch.cuda.empty_cache()
    return row


def bound_from(rows):
    """The largest number of pairs per member of the ladder (ascending) at which path 0 is clear of path 1, no smaller one losing;
    -1 = none."""
    best = -1
    for r in sorted(rows, key=lambda r: r["pairs"]):
        if r["loses"] or not r["equal"]:
            break
        if r["clear"]:
            best = r["pairs"]
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--json")
    ap.add_argument("--only", choices=("shapes", "bound"))
    args = ap.parse_args()
    assert args.reps >= 3 and args.window >= 0.3
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    print(f"row_sums_collide_batch_dev; ms per call, median of {args.reps} alternating windows of >= {args.window} s; both outputs, w_min = 1, no V")
    shapes, bound, p0 = [], [], None
    if args.only != "bound":
        print(f"{'k':>4} {'n':>5} {'t':>3} {'batch':>6} {'call':>12} {'covered/mem':>12} {'weighed/mem':>14} {'ms':>11} {'spread':>6} {'Gcov/s':>9} {'Mweighed/s':>10} "
              f"{'enum/call':>9}")
        shapes = [r for s in SHAPES for r in run_shape(*s, args)]
        behind = [(r["k"], r["n"], r["ell"]) for r in shapes if r["ell"] is not None and r["enumeration_over_call"] < 1]
        print(f"slower than the enumeration at: {behind if behind else 'no measured shape'}")
    if args.only != "shapes":
        print(f"the ladder: N1 = C({BOUND_K1}, 2) = {comb(BOUND_K1, 2)}, n = {BOUND_N}, ell = {BOUND_ELL}, about 2^32 pairs per call")
        print(f"{'k1+k2':>8} {'N2':>7} {'pairs':>11} {'batch':>6} {'slices':>6} {'path0 ms':>10} {'spread':>6} {'path1 ms':>10} {'spread':>6}")
        bound = [run_rung(k2, args) for k2 in BOUND_K2]
        p0 = bound_from(bound)
        print(f"P0 from this ladder: {p0} (the largest number of pairs per member at which path 0 is clear of path 1, no smaller one losing; -1 = none)")
        print(f"all results equal: {'yes' if all(r['equal'] for r in bound) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(p0=p0, shapes=shapes, bound=bound), f, indent=1)


if __name__ == "__main__":
    main()

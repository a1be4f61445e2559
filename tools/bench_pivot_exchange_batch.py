"""m4ri_amd_pivot_exchange_batch_dev on device-resident systematic forms: `steps` exchanges drawn on the device (req = NULL, the order
kept), in place on the forms m4ri_amd_echelonize_order_batch_dev(full = 1) left of ONE shared k x n generator on a random order per
member, against
  re-elimination  what a caller does today to reach the same information sets: m4ri_amd_echelonize_order_batch_dev from scratch, from
                  the shared generator, on order = the new pivots (k entries per member), full = 1;
  copy            a device-to-device copy of the same members: the floor for touching every word once;
  staged, in place  the call itself held on path 1 (the member staged in LDS) and on path 2 (in place in global memory) by the
                  environment: the measurement behind the routing bound between the two.  The call as routed is one of
                  them beyond path 0.
Before anything is timed the tool checks, from one starting state, that the exchanged forms equal the re-eliminated ones bit for bit
(pivots too) and that the forced paths leave the same bytes as the routed call.  The timed calls then chain: every call exchanges on
the state the previous one left.
  shapes   k x n = 32 x 64, 64 x 128, 64 x 1024, 128 x 256, 256 x 512, 512 x 1024, at a batch of 2^23 / (k * words(n)) members held in
           [1024, 65536], steps = 1, 4 and 16;
  pipeline iterations of Lee-Brickell per second with no host round trip, 64 x 128 and 256 x 512: the exchange (steps = 1, 4, 16) and
           m4ri_amd_row_sums_weights_batch_dev at t = 2 (lightest alone, w_min = 1), against random orders, elimination and the same
           enumeration.

The contenders of a row are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls between
two HIP events sized to `--window` seconds.  Columns: ms per call (median of the windows) and the spread of the windows ((max - min) /
median); `clear`: the call's slowest window is faster than the re-elimination's fastest; `LOSES`: the other way round; else `within
the spread`.

  python tools/bench_pivot_exchange_batch.py [--reps 3] [--window 0.3] [--json out.json] [--txt out.txt]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

SHAPES = [(32, 64), (64, 128), (64, 1024), (128, 256), (256, 512), (512, 1024)]
PIPELINE = [(64, 128), (256, 512)]
STEPS = (1, 4, 16)
PATH0_MAX, PATH1_MAX = "M4RI_AMD_PIVOT_EXCHANGE_PATH0_MAX", "M4RI_AMD_PIVOT_EXCHANGE_PATH1_MAX"
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def batch_of(k, n):
    return max(1024, min(65536, (1 << 23) // (k * (n // 64))))


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


class Shape:
    def __init__(self, k, n, seed):
        self.k, self.n, self.w, self.batch = k, n, n // 64, batch_of(k, n)
        w, batch = self.w, self.batch
        self.st = torch.cuda.current_stream().cuda_stream
        self.G = torch.empty(k * w, dtype=torch.int64, device="cuda")
        m4ri_amd.fill_dev(self.G.data_ptr(), w, k, n, seed, 0)
        self.O = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        self.D = torch.empty(batch * k * w, dtype=torch.int64, device="cuda")
        self.D2 = torch.empty_like(self.D)
        self.rank = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.rank2 = torch.empty_like(self.rank)
        self.piv = torch.empty(batch * k, dtype=torch.int32, device="cuda")
        self.piv2 = torch.empty_like(self.piv)
        self.done = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.seeds = iter(range(seed, 1 << 30))
        self.start(seed + 1)
        self.state = (self.D.clone(), self.piv.clone(), self.O.clone())

    def start(self, seed):
        """random orders and the forms on them: the state the exchanges start from"""
        k, n, w = self.k, self.n, self.w
        m4ri_amd.random_orders_batch_dev(self.O.data_ptr(), n, n, self.batch, seed, self.st)
        m4ri_amd.echelonize_order_batch_dev(self.D.data_ptr(), w, k * w, self.G.data_ptr(), w, 0, k, n, k, self.O.data_ptr(), n, n, self.batch, 1,
                                            self.rank.data_ptr(), self.piv.data_ptr(), self.st)

    def reset(self):
        for dst, src in zip((self.D, self.piv, self.O), self.state):
            dst.copy_(src)
        torch.cuda.synchronize()

    def exchange(self, steps, seed=None):
        k, n, w = self.k, self.n, self.w
        m4ri_amd.pivot_exchange_batch_dev(self.D.data_ptr(), w, k * w, k, n, k, self.piv.data_ptr(), self.rank.data_ptr(), self.batch, 0, 0, steps,
                                          next(self.seeds) if seed is None else seed, self.O.data_ptr(), n, n, self.done.data_ptr(), self.st)

    def exchange_on(self, path, steps, seed=None):
        os.environ[PATH0_MAX], os.environ[PATH1_MAX] = "0", "0" if path == 2 else "163840"      # read per call
        try:
            self.exchange(steps, seed)
        finally:
            del os.environ[PATH0_MAX], os.environ[PATH1_MAX]

    def re_eliminate(self):
        """from the shared generator on order = the current pivots, into D2"""
        k, n, w = self.k, self.n, self.w
        m4ri_amd.echelonize_order_batch_dev(self.D2.data_ptr(), w, k * w, self.G.data_ptr(), w, 0, k, n, k, self.piv.data_ptr(), k, k, self.batch, 1,
                                            self.rank2.data_ptr(), self.piv2.data_ptr(), self.st)

    def copy(self):
        self.D2.copy_(self.D)


def check(s, steps):
    """(the exchanged forms equal the re-eliminated ones, the forced paths equal the routed call, steps performed per member)"""
    s.reset()
    s.exchange(steps, seed=99)
    s.D2.fill_(-7)
    s.re_eliminate()
    torch.cuda.synchronize()
    same = torch.equal(s.D, s.D2) and torch.equal(s.piv, s.piv2) and torch.equal(s.rank, s.rank2)
    d1, p1, o1, n1 = s.D.clone(), s.piv.clone(), s.O.clone(), s.done.clone()
    paths = True
    for path in (1, 2):
        s.reset()
        s.exchange_on(path, steps, seed=99)
        torch.cuda.synchronize()
        paths = paths and torch.equal(s.D, d1) and torch.equal(s.piv, p1) and torch.equal(s.O, o1) and torch.equal(s.done, n1)
    return same, paths, float(n1.float().mean())


def run_shape(k, n, args):
    s = Shape(k, n, 31 + k + n)
    torch.cuda.synchronize()
    full_rank = int((s.rank == k).sum())
    rows = []
    for steps in STEPS:
        same, paths, performed = check(s, steps)
        tm = alternate({"call": lambda: s.exchange(steps), "re-elimination": s.re_eliminate, "copy": s.copy,
                        "staged": lambda: s.exchange_on(1, steps), "in place": lambda: s.exchange_on(2, steps)}, args)
        a, b = tm["call"], tm["re-elimination"]
        row = dict(k=k, n=n, batch=s.batch, steps=steps, path=m4ri_amd.plan_pivot_exchange_batch(k, n, steps), equal=same, paths_equal=paths,
                   performed_per_member=performed, full_rank=full_rank, windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()},
                   ms={c: med(v) * 1e3 for c, v in tm.items()}, spread={c: spread(v) for c, v in tm.items()},
                   re_elimination_over_call=med(b) / med(a), call_over_copy=med(a) / med(tm["copy"]),
                   in_place_over_staged=med(tm["in place"]) / med(tm["staged"]), clear=max(a) < min(b), loses=min(a) > max(b),
                   in_place_wins=max(tm["in place"]) < min(tm["staged"]), staged_wins=max(tm["staged"]) < min(tm["in place"]))
        verdict = "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread"
        say(f"{k:>4} {n:>5} {s.batch:>6} {steps:>5} {row['path']:>4} {row['ms']['call']:>9.4f} {row['spread']['call'] * 100:>5.1f}% "
            f"{row['ms']['re-elimination']:>9.4f} {row['spread']['re-elimination'] * 100:>5.1f}% {row['re_elimination_over_call']:>7.2f}x "
            f"{row['ms']['copy']:>9.4f} {row['call_over_copy']:>6.2f}x {row['ms']['staged']:>9.4f} {row['spread']['staged'] * 100:>5.1f}% "
            f"{row['ms']['in place']:>9.4f} {row['spread']['in place'] * 100:>5.1f}% {row['in_place_over_staged']:>6.2f}x  {verdict}; results {'equal' if same and paths else 'DIFFER'}; {performed:.2f} steps performed per member; "
            f"{full_rank} of full rank")
        rows.append(row)
    return rows


def run_pipeline(k, n, args):
    s = Shape(k, n, 57 + k + n)
    w, batch = s.w, s.batch
    light = torch.empty(batch, dtype=torch.int64, device="cuda")

    def weigh():
        m4ri_amd.row_sums_weights_batch_dev(s.D.data_ptr(), w, k * w, k, n, 0, 0, batch, 2, 1, 0, light.data_ptr(), s.st)

    def scratch():
        s.start(next(s.seeds))
        weigh()

    def exchanged(steps):
        def iteration():
            s.exchange(steps)
            weigh()
        return iteration

    tm = alternate(dict({"orders + elimination": scratch}, **{f"exchange, {st} steps": exchanged(st) for st in STEPS}), args)
    rows = []
    for name, v in tm.items():
        row = dict(k=k, n=n, batch=batch, t=2, iteration=name, ms=med(v) * 1e3, spread=spread(v), iterations_per_s=batch / med(v),
                   windows_ms=[x * 1e3 for x in v])
        say(f"{k:>4} {n:>5} {batch:>6}  t = 2  {name:<22} {row['ms']:>10.4f} ms per batch {row['spread'] * 100:>5.1f}%  "
            f"{row['iterations_per_s']:>14.0f} iterations / s")
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    args = ap.parse_args()
    assert args.reps >= 3 and args.window >= 0.3
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    say(f"pivot_exchange_batch_dev (requests drawn on the device, the order kept, in place, chained) against re-elimination from scratch on "
        f"the new pivots, a device copy of the members, and itself held on path 1 (staged in LDS) and on path 2 (in place); ms per call, median of "
        f"{args.reps} alternating windows of >= {args.window} s")
    say(f"{'k':>4} {'n':>5} {'batch':>6} {'steps':>5} {'path':>4} {'call ms':>9} {'spread':>6} {'re-elim':>9} {'spread':>6} {'ratio':>8} {'copy ms':>9} "
        f"{'/copy':>7} {'staged':>9} {'spread':>6} {'in place':>9} {'spread':>6} {'/staged':>7}")
    shapes = [r for (k, n) in SHAPES for r in run_shape(k, n, args)]
    lost = [(r["k"], r["n"], r["steps"], round(r["re_elimination_over_call"], 3)) for r in shapes if r["loses"]]
    say(f"loses to re-elimination beyond the spread at: {lost if lost else 'no measured shape and step count'}")
    won = [(r["k"], r["n"], r["steps"], round(r["in_place_over_staged"], 3)) for r in shapes if r["in_place_wins"]]
    say(f"path 2 beats path 1 beyond the spread at: {won if won else 'no measured shape and step count'}")
    wrong = [(r["k"], r["n"], r["steps"]) for r in shapes if (r["path"] == 1 and r["in_place_wins"]) or (r["path"] == 2 and r["staged_wins"])]
    say(f"routed down the slower of the two beyond the spread at: {wrong if wrong else 'no measured shape and step count'}")
    ok = all(r["equal"] and r["paths_equal"] for r in shapes)
    say(f"all results equal: {'yes' if ok else 'NO'}")
    say("Lee-Brickell: weights of the sums of two rows after random orders and elimination from scratch, or after exchanges on the stored form")
    pipe = [r for (k, n) in PIPELINE for r in run_pipeline(k, n, args)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(shapes=shapes, pipeline=pipe), f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(LINES) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""m4ri_amd_echelonize_order_batch_dev on device-resident random generators: systematic forms (full = 1) of ONE shared k x n generator
on a random column order per member, out of place, against all the library offered before -- the four-launch composition: broadcast
m4ri_amd_copy_block_batch_dev, m4ri_amd_apply_p_right_batch_dev (gather the columns), m4ri_amd_echelonize_batch_dev,
m4ri_amd_apply_p_right_batch_dev with trans (scatter them back).  The composition's transposition sequences are made on the host from
the same orders and uploaded before the clock starts.  Both contenders must leave identical bytes, ranks and pivot columns; the tool
checks that before it times anything.
  shapes   k x n = 32 x 64, 64 x 128, 64 x 1024, 128 x 256, 256 x 512, 512 x 1024, at a batch of 2^23 / (k * words(n)) members held in
           [1024, 65536]: at least four workgroups per compute unit everywhere;
  pipeline for the record, one iteration of Lee-Brickell per member with no host round trip: m4ri_amd_random_orders_batch_dev, the
           systematic forms, m4ri_amd_row_sums_weights_batch_dev at t = 2 (lightest alone, w_min = 1); 64 x 128 and 256 x 512.

The contenders of a shape are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls between
two HIP events sized to `--window` seconds.  Columns: ms per call (median of the windows), the spread of the windows ((max - min) /
median), and the composition's time over the call's.  `clear`: the call's slowest window is faster than the composition's fastest;
`LOSES`: the other way round; else `within the spread`.

  python tools/bench_echelonize_order_batch.py [--reps 3] [--window 0.3] [--json out.json] [--txt out.txt]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import m4ri_amd

SHAPES = [(32, 64), (64, 128), (64, 1024), (128, 256), (256, 512), (512, 1024)]
PIPELINE = [(64, 128), (256, 512)]
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


def transpositions(orders):
    """For every row of `orders` (batch x n permutations) the sequence P that gathers the columns under apply_p_right (trans = 0: the
    swaps (i, P[i]) from i = n - 1 down): afterwards column i is the old column orders[b][i].  All members at once."""
    batch, n = orders.shape
    ar = np.arange(batch)
    at, pos = np.tile(np.arange(n, dtype=np.int32), (batch, 1)), np.tile(np.arange(n, dtype=np.int32), (batch, 1))
    P = np.zeros((batch, n), dtype=np.int32)
    for i in range(n - 1, -1, -1):
        c = orders[:, i]
        p = pos[ar, c]
        a = at[ar, i]
        P[:, i] = p
        at[ar, p], pos[ar, a] = a, p
        at[ar, i], pos[ar, c] = c, i
    return P


class Shape:
    def __init__(self, k, n, seed):
        self.k, self.n, self.w, self.batch = k, n, n // 64, batch_of(k, n)
        k, n, w, batch = self.k, self.n, self.w, self.batch
        self.st = torch.cuda.current_stream().cuda_stream
        self.G = torch.empty(k * w, dtype=torch.int64, device="cuda")
        m4ri_amd.fill_dev(self.G.data_ptr(), w, k, n, seed, 0)
        self.O = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        m4ri_amd.random_orders_batch_dev(self.O.data_ptr(), n, n, batch, seed + 1, self.st)
        torch.cuda.synchronize()
        self.D = torch.empty(batch * k * w, dtype=torch.int64, device="cuda")
        self.rank = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.piv = torch.empty(batch * k, dtype=torch.int32, device="cuda")

    def call(self):
        k, n, w = self.k, self.n, self.w
        m4ri_amd.echelonize_order_batch_dev(self.D.data_ptr(), w, k * w, self.G.data_ptr(), w, 0, k, n, k, self.O.data_ptr(), n, n, self.batch, 1,
                                            self.rank.data_ptr(), self.piv.data_ptr(), self.st)

    def make_composition(self):
        self.P = torch.from_numpy(transpositions(self.O.cpu().numpy().reshape(self.batch, self.n))).cuda().reshape(-1)
        torch.cuda.synchronize()

    def composition(self):
        k, n, w, batch, D, P, st = self.k, self.n, self.w, self.batch, self.D.data_ptr(), self.P.data_ptr(), self.st
        m4ri_amd.copy_block_batch_dev(D, w, k * w, 0, 0, self.G.data_ptr(), w, 0, 0, 0, k, n, batch, st)
        m4ri_amd.apply_p_right_batch_dev(D, w, k * w, k, n, batch, P, n, n, False, 0, st)
        m4ri_amd.echelonize_batch_dev(D, w, k * w, k, n, batch, 1, self.rank.data_ptr(), self.piv.data_ptr(), st)
        m4ri_amd.apply_p_right_batch_dev(D, w, k * w, k, n, batch, P, n, n, True, 0, st)

    def results(self, fn):
        self.D.fill_(-7), self.rank.fill_(-7), self.piv.fill_(-7)
        fn()
        torch.cuda.synchronize()
        return self.D.clone(), self.rank.clone(), self.piv.clone()


def run_shape(k, n, args):
    s = Shape(k, n, 31 + k + n)
    s.make_composition()
    d1, r1, p1 = s.results(s.call)
    d2, r2, p2 = s.results(s.composition)
    # the composition's pivots are positions in the order: through the order they are the call's columns
    o = s.O.view(s.batch, n).long()
    p2 = torch.where(p2.view(s.batch, k) >= 0, torch.gather(o, 1, p2.view(s.batch, k).clamp(min=0).long()), -1).int().reshape(-1)
    equal = torch.equal(d1, d2) and torch.equal(r1, r2) and torch.equal(p1, p2)
    tm = alternate({"call": s.call, "composition": s.composition}, args)
    a, b = tm["call"], tm["composition"]
    row = dict(k=k, n=n, batch=s.batch, path=m4ri_amd.plan_echelonize_order_batch(k, n), equal=equal, full_rank=int((r1 == k).sum()),
               windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()}, call_ms=med(a) * 1e3, call_spread=spread(a),
               composition_ms=med(b) * 1e3, composition_spread=spread(b), composition_over_call=med(b) / med(a), clear=max(a) < min(b),
               loses=min(a) > max(b))
    verdict = "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread"
    say(f"{k:>4} {n:>5} {s.batch:>6} {row['path']:>4} {row['call_ms']:>10.4f} {row['call_spread'] * 100:>5.1f}% {row['composition_ms']:>12.4f} "
        f"{row['composition_spread'] * 100:>5.1f}% {row['composition_over_call']:>8.2f}x  {verdict}; results {'equal' if equal else 'DIFFER'}; "
        f"{row['full_rank']} members of full rank")
    return row


def run_pipeline(k, n, args):
    s = Shape(k, n, 57 + k + n)
    w, batch = s.w, s.batch
    light = torch.empty(batch, dtype=torch.int64, device="cuda")
    seeds = iter(range(1 << 30))

    def iteration():
        m4ri_amd.random_orders_batch_dev(s.O.data_ptr(), n, n, batch, next(seeds), s.st)
        s.call()
        m4ri_amd.row_sums_weights_batch_dev(s.D.data_ptr(), w, k * w, k, n, 0, 0, batch, 2, 1, 0, light.data_ptr(), s.st)

    tm = alternate({"iteration": iteration}, args)["iteration"]
    row = dict(k=k, n=n, batch=batch, t=2, ms=med(tm) * 1e3, spread=spread(tm), iterations_per_s=batch / med(tm), windows_ms=[x * 1e3 for x in tm])
    say(f"{k:>4} {n:>5} {batch:>6}  t = 2 {row['ms']:>10.4f} ms per batch {row['spread'] * 100:>5.1f}%  {row['iterations_per_s']:>14.0f} iterations / s")
    return row


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
    say(f"echelonize_order_batch_dev (one shared generator, a random order per member, full = 1, out of place) against the four-launch "
        f"composition; ms per call, median of {args.reps} alternating windows of >= {args.window} s")
    say(f"{'k':>4} {'n':>5} {'batch':>6} {'path':>4} {'call ms':>10} {'spread':>6} {'composed ms':>12} {'spread':>6} {'ratio':>9}")
    shapes = [run_shape(k, n, args) for (k, n) in SHAPES]
    lost = [(r["k"], r["n"], round(r["composition_over_call"], 3)) for r in shapes if r["loses"]]
    say(f"loses to the composition beyond the spread at: {lost if lost else 'no measured shape'}")
    say(f"all results equal: {'yes' if all(r['equal'] for r in shapes) else 'NO'}")
    say("Lee-Brickell, for the record: random orders, systematic forms, weights of the sums of two rows; one iteration per member")
    pipe = [run_pipeline(k, n, args) for (k, n) in PIPELINE]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(shapes=shapes, pipeline=pipe), f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(LINES) + "\n")
    return 0 if all(r["equal"] for r in shapes) else 1


if __name__ == "__main__":
    sys.exit(main())

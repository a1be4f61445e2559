"""Batched PLUQ decompositions (m4ri_amd_ple_batch_dev, pluq = 1) against the same members through a loop of the per-member call
(m4ri_amd_pluq_dev, recursion_cutoff = 0), and against m4ri_amd_echelonize_batch_dev(full = 0) on the same members: the same
elimination without L compression and without P / Q, the natural floor.  Then "factor once, solve later" (the decomposition plus
m4ri_amd_pluq_solve_left_batch_dev, each timed alone) against one m4ri_amd_solve_left_batch_dev, k right-hand sides per member,
B_b = A_b X_b (every member has a solution).  One GPU, members resident.  Batch times are HIP events around the call (min / median of
`reps` after a warm-up); the in-place calls get fresh members before every repetition, outside the events.  Loop times per member:
the median of `reps` timed loops over a subset of the batch (fresh members each time), scaled to the whole batch.  Where the one-call
solve goes one by one (its path 2) it is timed up to batch 256 only; the other columns are timed at every batch.  Members are random
(fill_dev).

  python tools/ple_batch_timing.py [--reps R] [--k K]
  python tools/ple_batch_timing.py --batch-only --shape 64 64 --batch 4096     # only the batched calls (for a kernel trace)"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import m4ri_amd

SHAPES = [(32, 32), (64, 64), (256, 256), (1024, 1024), (2000, 2000)]
BATCHES = (1, 256, 1024, 4096)


def w_of(n):
    return (n + 63) // 64


def filled(rows, n, seed):
    t = torch.empty(max(1, rows * w_of(n)), dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(t.data_ptr(), w_of(n), rows, n, seed, 0)
    return t


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def timed_in_place(call, work, src, reps):
    """min, median of `reps` calls, `work` refilled from `src` before each (outside the events), after one warm-up."""
    call()
    out = []
    for _ in range(reps):
        work.copy_(src)
        torch.cuda.synchronize()
        out.append(events(call))
    return min(out), statistics.median(out)


class Batch:
    def __init__(self, n, batch, k):
        self.n, self.batch, self.k, self.wa, self.wb = n, batch, k, w_of(n), w_of(k)
        self.src = filled(batch * n, n, 21)
        self.A = self.src.clone()
        self.P = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        self.Q = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        self.rank = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.status = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream
        X = filled(batch * n, k, 22)
        self.B0 = torch.zeros(batch * n * self.wb, dtype=torch.int64, device="cuda")
        m4ri_amd.mul_batch_dev(self.B0.data_ptr(), self.wb, n * self.wb, self.src.data_ptr(), self.wa, n * self.wa, X.data_ptr(), self.wb,
                               n * self.wb, n, n, k, batch, False, 0, self.st)
        self.B = self.B0.clone()
        torch.cuda.synchronize()

    def factor(self):
        m4ri_amd.ple_batch_dev(self.A.data_ptr(), self.wa, self.n * self.wa, self.n, self.n, self.batch, True, self.P.data_ptr(),
                               self.Q.data_ptr(), self.rank.data_ptr(), self.st)

    def echelon(self):
        m4ri_amd.echelonize_batch_dev(self.A.data_ptr(), self.wa, self.n * self.wa, self.n, self.n, self.batch, 0, self.rank.data_ptr(), 0, self.st)

    def solve_from_factors(self):
        m4ri_amd.pluq_solve_left_batch_dev(self.A.data_ptr(), self.wa, self.n * self.wa, self.n, self.n, self.rank.data_ptr(), self.P.data_ptr(),
                                           self.Q.data_ptr(), self.B.data_ptr(), self.wb, self.n * self.wb, self.k, self.batch,
                                           self.status.data_ptr(), self.st)

    def solve_one_call(self):
        m4ri_amd.solve_left_batch_dev(self.A.data_ptr(), self.wa, self.n * self.wa, self.n, self.n, self.B.data_ptr(), self.wb, self.n * self.wb,
                                      self.k, self.batch, self.status.data_ptr(), 0, self.st)


def time_loop(n, members, reps):
    wa = w_of(n)
    A0 = filled(members * n, n, 21)
    A = A0.clone()
    P, Q = np.zeros(n, np.int32), np.zeros(n, np.int32)
    L, r = m4ri_amd.lib(), ctypes.c_int32(0)
    st = torch.cuda.current_stream().cuda_stream
    assert L.m4ri_amd_pluq_dev(A.data_ptr(), wa, n, n, P.ctypes.data, Q.ctypes.data, ctypes.byref(r), 0, st) == 0  # warm

    def loop():
        for b in range(members):
            assert L.m4ri_amd_pluq_dev(A.data_ptr() + 8 * b * n * wa, wa, n, n, P.ctypes.data, Q.ctypes.data, ctypes.byref(r), 0, st) == 0
    out = []
    for _ in range(reps):
        A.copy_(A0)
        torch.cuda.synchronize()
        out.append(events(loop) / members)
    return statistics.median(out)


def batch_only(args):
    n = (args.shape or (64, 64))[0]
    x = Batch(n, args.batch or 4096, args.k)
    for _ in range(args.reps):
        x.A.copy_(x.src)
        x.B.copy_(x.B0)
        x.factor()
        x.solve_from_factors()
    torch.cuda.synchronize()
    print(f"batch-only PLUQ + solve {n} x {n} batch {x.batch} k {x.k}: paths {m4ri_amd.plan_ple_batch(n, n)} / "
          f"{m4ri_amd.plan_pluq_solve_batch(n, n, x.k)}, {args.reps} calls, solved {int((x.status == 0).sum())} of {x.batch}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--shape", type=int, nargs=2)
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    if args.batch_only:
        return batch_only(args)
    print(f"PLUQ of random n x n members and solves with k = {args.k} right-hand sides; batch times = min / median of {args.reps} calls "
          f"(HIP events, ms); loop = m4ri_amd_pluq_dev per member, median of {args.reps} loops over 16 members (4 at n > 1024); echelon = "
          "echelonize_batch_dev(full = 0); one call = solve_left_batch_dev (-: one by one there, timed up to batch 256); paths: ple / "
          "echelon / solve from factors / one-call solve")
    print(f"{'n':>5} {'paths':>7} {'batch':>6} {'pluq min':>10} {'median':>10} {'loop/member':>11} {'loop (all)':>11} {'speedup':>9} "
          f"{'echelon':>10} {'pluq/ech':>8} | {'solve(f)':>10} {'median':>10} {'f + s':>10} {'one call':>10} {'median':>10} {'(f+s)/one':>9}")
    for (n, _) in SHAPES:
        paths = (m4ri_amd.plan_ple_batch(n, n), m4ri_amd.plan_echelonize_batch(n, n), m4ri_amd.plan_pluq_solve_batch(n, n, args.k),
                 m4ri_amd.plan_solve_batch(n, n, args.k))
        per = time_loop(n, 16 if n <= 1024 else 4, args.reps)
        for batch in BATCHES:
            one_call = not (paths[3] == 2 and batch > 256)  # one by one there: more members would only repeat its number
            x = Batch(n, batch, args.k)
            fmin, fmed = timed_in_place(x.factor, x.A, x.src, args.reps)
            emin, _ = timed_in_place(x.echelon, x.A, x.src, args.reps)
            x.A.copy_(x.src)
            x.factor()
            smin, smed = timed_in_place(x.solve_from_factors, x.B, x.B0, args.reps)
            solved = int((x.status == 0).sum())
            assert solved == batch, "B = A X has a solution for every member"
            tail = f"{'-':>10} {'-':>10} {'-':>9}"
            if one_call:
                x.A.copy_(x.src)  # the one-call solve reads the original members
                omin, omed = timed_in_place(x.solve_one_call, x.B, x.B0, args.reps)
                assert batch == int((x.status == 0).sum())
                tail = f"{omin * 1e3:>10.4f} {omed * 1e3:>10.4f} {(fmed + smed) / omed:>9.2f}"
            print(f"{n:>5} {'/'.join(map(str, paths)):>7} {batch:>6} {fmin * 1e3:>10.4f} {fmed * 1e3:>10.4f} {per * 1e3:>11.4f} "
                  f"{per * batch * 1e3:>11.2f} {per * batch / fmed:>8.1f}x {emin * 1e3:>10.4f} {fmin / emin:>8.2f} | {smin * 1e3:>10.4f} "
                  f"{smed * 1e3:>10.4f} {(fmed + smed) * 1e3:>10.4f} {tail}", flush=True)
            del x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

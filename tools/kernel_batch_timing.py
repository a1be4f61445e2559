"""Batched null-space bases (m4ri_amd_kernel_left_batch_dev) against the same members through a loop of the per-member call
(m4ri_amd_kernel_left_pluq_dev, which overwrites A: every member of the loop has its own copy, made before the timed loop, and its own
zeroed R), and against the workaround the batched call replaces: echelonize_batch_dev(full = 1) on copies of the members, the echelon
call alone timed (not the host-side rebuild of the basis from it).  One GPU, members resident.  Batch times are HIP events around the
call (min / median of `reps`; A is read only, so no refill is needed); loop times per member over a subset of the batch, scaled to
the whole batch.  Members are random (fill_dev), kc = n.  For path 0 the HBM floor (every word of A read once, every word of R
written once) at 8 TB/s and the fraction of it reached.

  python tools/kernel_batch_timing.py [--reps R]
  python tools/kernel_batch_timing.py --batch-only --shape 64 64 --batch 4096     # only batched calls (for a kernel trace)"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

SHAPES = [(32, 32), (64, 64), (64, 128), (256, 256), (1024, 1024), (2000, 2000)]
BATCHES = (1, 256, 1024, 4096)
HBM_BYTES_PER_S = 8e12


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


def time_batch(m, n, batch, reps):
    wa = w_of(n)
    A = filled(batch * m, n, 21)
    R = torch.empty(max(1, batch * n * wa), dtype=torch.int64, device="cuda")
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: m4ri_amd.kernel_left_batch_dev(A.data_ptr(), wa, m * wa, m, n, R.data_ptr(), wa, n * wa, n, batch, rank.data_ptr(), st)
    call()  # warm
    out = [events(call) for _ in range(reps)]
    return min(out), statistics.median(out), int(n - rank.max()), int(n - rank.min())


def time_loop(m, n, members):
    wa = w_of(n)
    A0 = filled(members * m, n, 21)
    A = A0.clone()
    R = torch.zeros(members * n * wa, dtype=torch.int64, device="cuda")
    L, r = m4ri_amd.lib(), ctypes.c_int32(0)
    st = torch.cuda.current_stream().cuda_stream
    assert L.m4ri_amd_kernel_left_pluq_dev(A.data_ptr(), wa, m, n, R.data_ptr(), wa, 0, ctypes.byref(r), st) == 0  # warm
    A.copy_(A0)
    R.zero_()
    torch.cuda.synchronize()

    def loop():
        for b in range(members):
            assert L.m4ri_amd_kernel_left_pluq_dev(A.data_ptr() + 8 * b * m * wa, wa, m, n, R.data_ptr() + 8 * b * n * wa, wa, 0,
                                                   ctypes.byref(r), st) == 0
    return events(loop) / members


def time_workaround(m, n, batch, reps):
    wa = w_of(n)
    src = filled(batch * m, n, 21)
    E = src.clone()
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: m4ri_amd.echelonize_batch_dev(E.data_ptr(), wa, m * wa, m, n, batch, 1, rank.data_ptr(), 0, st)
    call()
    out = []
    for _ in range(reps):
        E.copy_(src)
        torch.cuda.synchronize()
        out.append(events(call))
    return min(out), m4ri_amd.plan_echelonize_batch(m, n)


def floor_note(m, n, batch, tmin):
    nbytes = 8 * batch * (m * w_of(n) + n * w_of(n))
    return (f"; HBM floor {nbytes / HBM_BYTES_PER_S * 1e3:.4f} ms, achieved {nbytes / tmin / 1e12:.3f} TB/s "
            f"({nbytes / tmin / HBM_BYTES_PER_S * 100:.1f} % of 8)")


def batch_only(args):
    m, n = args.shape or (64, 64)
    batch = args.batch or 4096
    wa = w_of(n)
    A = filled(batch * m, n, 21)
    R = torch.empty(max(1, batch * n * wa), dtype=torch.int64, device="cuda")
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for _ in range(args.reps):
        m4ri_amd.kernel_left_batch_dev(A.data_ptr(), wa, m * wa, m, n, R.data_ptr(), wa, n * wa, n, batch, rank.data_ptr(), st)
    torch.cuda.synchronize()
    print(f"batch-only kernel {m} x {n} batch {batch} path {m4ri_amd.plan_kernel_batch(m, n)}: {args.reps} calls, "
          f"nullity {n - int(rank.max())}..{n - int(rank.min())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--shape", type=int, nargs=2)
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    if args.batch_only:
        return batch_only(args)
    print(f"null-space bases of random members, kc = n; batch time = min / median of {args.reps} calls (HIP events); loop = "
          "m4ri_amd_kernel_left_pluq_dev per member; workaround = echelonize_batch_dev(full = 1), the echelon call alone")
    print(f"{'m x n':>11} {'path':>4} {'batch':>6} {'batch ms':>10} {'median':>10} {'loop ms/member':>14} {'loop ms (all)':>13} "
          f"{'speedup':>9} {'workaround ms':>13} {'(path)':>6}  extra")
    for (m, n) in SHAPES:
        path = m4ri_amd.plan_kernel_batch(m, n)
        per = time_loop(m, n, 16 if n <= 1024 else 4)
        for batch in BATCHES:
            if path == 2 and batch > 256:
                continue  # one by one: more members would only repeat the loop's number
            tmin, tmed, nlo, nhi = time_batch(m, n, batch, 1 if path == 2 else args.reps)
            wmin, wpath = time_workaround(m, n, batch, 1 if path == 2 else args.reps)
            extra = f"nullity {nlo}..{nhi}"
            if path == 0:
                extra += floor_note(m, n, batch, tmin)
            print(f"{m:>5} x {n:<5} {path:>4} {batch:>6} {tmin * 1e3:>10.4f} {tmed * 1e3:>10.4f} {per * 1e3:>14.4f} {per * batch * 1e3:>13.2f} "
                  f"{per * batch / tmin:>8.1f}x {wmin * 1e3:>13.4f} {wpath:>6}  {extra}", flush=True)


if __name__ == "__main__":
    main()

"""Batched solves and inverses (m4ri_amd_solve_left_batch_dev, m4ri_amd_inv_batch_dev) against the same members through a loop of
the per-member calls (m4ri_amd_solve_left_dev, m4ri_amd_inv_dev), on one GPU with the members resident.  For the inverse also the
workaround the batched call replaces: [A | I] built by hand and m4ri_amd_echelonize_batch_dev(full = 1) on it -- only the echelon
call is timed, not the augmenting or the extraction.  Batch times are HIP events around the call (inputs refilled before every timed
call, outside the events; min / median of `reps`), loop times per member over a subset of the batch, scaled to the whole batch.
The solve's systems are square and consistent (B = A X, made by m4ri_amd_mul_batch_dev).  For path 0 the HBM floor (every word of A
read once, every word of B / Binv read and written once) at 8 TB/s and the fraction of it reached.

  python tools/solve_batch_timing.py [--reps R] [--op solve|inv|both]
  python tools/solve_batch_timing.py --batch-only --op inv --shape 256 256 256 --batch 1024     # only batched calls (for a kernel
        trace): inputs made on the device, no refill and no copy between the calls"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

SOLVE_SHAPES = [(32, 32, 32), (64, 64, 64), (256, 256, 64), (256, 256, 256), (1024, 1024, 64), (2000, 2000, 64)]
INV_SIZES = [32, 64, 256, 768, 1024]
BATCHES = (1, 256, 1024, 4096)
HBM_BYTES_PER_S = 8e12


def w_of(n):
    return (n + 63) // 64


def filled(rows, n, seed):
    t = torch.empty(max(1, rows * w_of(n)), dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(t.data_ptr(), w_of(n), rows, n, seed, 0)
    return t


def solve_inputs(n, k, batch):
    """batch square systems A_b X_b = B_b, A and B back to back (stride = width)."""
    wa, wb = w_of(n), w_of(k)
    A, X = filled(batch * n, n, 11), filled(batch * n, k, 12)
    B = torch.zeros(batch * n * wb, dtype=torch.int64, device="cuda")
    m4ri_amd.mul_batch_dev(B.data_ptr(), wb, n * wb, A.data_ptr(), wa, n * wa, X.data_ptr(), wb, n * wb, n, n, k, batch)
    return A, B


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def time_solve_batch(n, k, batch, reps):
    wa, wb = w_of(n), w_of(k)
    A, Bsrc = solve_inputs(n, k, batch)
    B = Bsrc.clone()
    status = torch.empty(batch, dtype=torch.int32, device="cuda")
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: m4ri_amd.solve_left_batch_dev(A.data_ptr(), wa, n * wa, n, n, B.data_ptr(), wb, n * wb, k, batch, status.data_ptr(),
                                                 rank.data_ptr(), st)
    call()  # warm
    out = []
    for _ in range(reps):
        B.copy_(Bsrc)
        torch.cuda.synchronize()
        out.append(events(call))
    return min(out), statistics.median(out), int((status == 0).sum()), int(rank.min()), int(rank.max())


def time_solve_loop(n, k, members):
    wa, wb = w_of(n), w_of(k)
    A0, B0 = solve_inputs(n, k, members)
    L, ret = m4ri_amd.lib(), ctypes.c_int(0)
    st = torch.cuda.current_stream().cuda_stream
    A, B = A0.clone(), B0.clone()
    assert L.m4ri_amd_solve_left_dev(A.data_ptr(), wa, n, n, B.data_ptr(), wb, n, k, 0, 1, ctypes.byref(ret), st) == 0  # warm
    A.copy_(A0)
    B.copy_(B0)
    torch.cuda.synchronize()

    def loop():
        for b in range(members):
            assert L.m4ri_amd_solve_left_dev(A.data_ptr() + 8 * b * n * wa, wa, n, n, B.data_ptr() + 8 * b * n * wb, wb, n, k, 0, 1,
                                             ctypes.byref(ret), st) == 0
    return events(loop) / members


def time_inv_batch(n, batch, reps):
    w = w_of(n)
    A = filled(batch * n, n, 13)
    X = torch.empty_like(A)
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: m4ri_amd.inv_batch_dev(X.data_ptr(), w, n * w, A.data_ptr(), w, n * w, n, batch, rank.data_ptr(), st)
    call()
    out = []
    for _ in range(reps):
        X.zero_()
        torch.cuda.synchronize()
        out.append(events(call))
    return min(out), statistics.median(out), int((rank == n).sum()), int(rank.min()), int(rank.max())


def time_inv_loop(n, members):
    w = w_of(n)
    A, X = filled(members * n, n, 13), torch.empty(members * n * w, dtype=torch.int64, device="cuda")
    L = m4ri_amd.lib()
    st = torch.cuda.current_stream().cuda_stream
    assert L.m4ri_amd_inv_dev(X.data_ptr(), w, A.data_ptr(), w, n, st) == 0  # warm
    torch.cuda.synchronize()

    def loop():
        for b in range(members):
            assert L.m4ri_amd_inv_dev(X.data_ptr() + 8 * b * n * w, w, A.data_ptr() + 8 * b * n * w, w, n, st) == 0
    return events(loop) / members


def time_inv_workaround(n, batch, reps):
    """[A | 0 | I] (n x 2 * 64 * width, as m4ri_amd_inv_dev lays it out) and echelonize_batch_dev(full = 1): the echelon call only."""
    w = w_of(n)
    A = filled(batch * n, n, 13).view(batch, n, w)
    src = torch.zeros(batch, n, 2 * w, dtype=torch.int64, device="cuda")
    src[:, :, :w] = A
    i = torch.arange(n, device="cuda")
    src[:, i, w + i // 64] |= torch.bitwise_left_shift(torch.ones_like(i), i % 64)
    aug = src.clone()
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda: m4ri_amd.echelonize_batch_dev(aug.data_ptr(), 2 * w, n * 2 * w, n, 2 * w * 64, batch, 1, rank.data_ptr(), 0, st)
    call()
    out = []
    for _ in range(reps):
        aug.copy_(src)
        torch.cuda.synchronize()
        out.append(events(call))
    return min(out), m4ri_amd.plan_echelonize_batch(n, 2 * w * 64)


def floor_note(m, n, k, batch, tmin):
    nbytes = 8 * batch * (m * w_of(n) + 2 * max(m, n) * w_of(k))
    return (f"; HBM floor {nbytes / HBM_BYTES_PER_S * 1e3:.4f} ms, achieved {nbytes / tmin / 1e12:.3f} TB/s "
            f"({nbytes / tmin / HBM_BYTES_PER_S * 100:.1f} % of 8)")


def batch_only(args):
    m, n, k = args.shape or (256, 256, 256)
    batch = args.batch or 1024
    st = torch.cuda.current_stream().cuda_stream
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    if args.op == "inv":
        w = w_of(n)
        A = filled(batch * n, n, 13)
        X = torch.empty_like(A)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            m4ri_amd.inv_batch_dev(X.data_ptr(), w, n * w, A.data_ptr(), w, n * w, n, batch, rank.data_ptr(), st)
    else:
        A, B = solve_inputs(n, k, batch)
        status = torch.empty(batch, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(args.reps):  # after the first call B holds X: the later calls solve A X' = X, same work
            m4ri_amd.solve_left_batch_dev(A.data_ptr(), w_of(n), n * w_of(n), n, n, B.data_ptr(), w_of(k), n * w_of(k), k, batch,
                                          status.data_ptr(), rank.data_ptr(), st)
    torch.cuda.synchronize()
    print(f"batch-only {args.op} {n} x {n} x {k} batch {batch} path {m4ri_amd.plan_solve_batch(n, n, k)}: {args.reps} calls, "
          f"ranks {int(rank.min())}..{int(rank.max())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--op", choices=("solve", "inv", "both"), default="both")
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--shape", type=int, nargs=3)
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    if args.batch_only:
        return batch_only(args)
    if args.op in ("solve", "both"):
        print(f"solve: square consistent systems; batch time = min / median of {args.reps} calls (HIP events); "
              "loop = m4ri_amd_solve_left_dev per member (check on)")
        print(f"{'m x n x k':>16} {'path':>4} {'batch':>6} {'batch ms':>10} {'median':>10} {'loop ms/member':>14} {'loop ms (all)':>13} "
              f"{'speedup':>9}  extra")
        for (m, n, k) in SOLVE_SHAPES:
            path = m4ri_amd.plan_solve_batch(m, n, k)
            per = time_solve_loop(n, k, 16 if n <= 1024 else 4)
            for batch in BATCHES:
                if path == 2 and batch > 256:
                    continue  # one by one: more members would only repeat the loop's number
                tmin, tmed, ok, rlo, rhi = time_solve_batch(n, k, batch, 1 if path == 2 else args.reps)
                extra = f"consistent {ok}/{batch}, ranks {rlo}..{rhi}"
                if path == 0:
                    extra += floor_note(m, n, k, batch, tmin)
                print(f"{m:>5} x {n:>4} x {k:<4} {path:>4} {batch:>6} {tmin * 1e3:>10.4f} {tmed * 1e3:>10.4f} {per * 1e3:>14.4f} "
                      f"{per * batch * 1e3:>13.2f} {per * batch / tmin:>8.1f}x  {extra}", flush=True)
    if args.op in ("inv", "both"):
        print(f"inverse: random members; batch time = min / median of {args.reps} calls (HIP events); loop = m4ri_amd_inv_dev per member; "
              "workaround = echelonize_batch_dev(full = 1) on [A | 0 | I], the echelon call alone")
        print(f"{'n':>6} {'path':>4} {'batch':>6} {'batch ms':>10} {'median':>10} {'loop ms/member':>14} {'loop ms (all)':>13} "
              f"{'speedup':>9} {'workaround ms':>13} {'(path)':>6}  extra")
        for n in INV_SIZES:
            path = m4ri_amd.plan_solve_batch(n, n, n)
            per = time_inv_loop(n, 16)
            for batch in BATCHES:
                if path == 2 and batch > 256:
                    continue
                tmin, tmed, inv, rlo, rhi = time_inv_batch(n, batch, 1 if path == 2 else args.reps)
                wmin, wpath = time_inv_workaround(n, batch, args.reps)
                extra = f"invertible {inv}/{batch}, ranks {rlo}..{rhi}"
                if path == 0:
                    extra += floor_note(n, n, n, batch, tmin)
                print(f"{n:>6} {path:>4} {batch:>6} {tmin * 1e3:>10.4f} {tmed * 1e3:>10.4f} {per * 1e3:>14.4f} {per * batch * 1e3:>13.2f} "
                      f"{per * batch / tmin:>8.1f}x {wmin * 1e3:>13.4f} {wpath:>6}  {extra}", flush=True)


if __name__ == "__main__":
    main()

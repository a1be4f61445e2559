"""Batched echelon forms (m4ri_amd_echelonize_batch_dev) against the same members through a loop of m4ri_amd_echelonize_dev, on
one GPU with the members resident.  Batch times are HIP events around the call (inputs refilled before every timed call, outside
the events; min / median of `reps`), loop times per member over a subset of the batch, scaled to the whole batch.  For path 0 the
HBM floor (every word read and written once) at 8 TB/s and the achieved rate.

  python tools/echelonize_batch_timing.py [--full 0|1] [--reps R]
  python tools/echelonize_batch_timing.py --batch-only --shape 256 256 --batch 1024     # only batched calls (for a kernel trace):
        inputs filled on the device by m4ri_amd_fill_dev, no refill and no copy between the calls"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

SHAPES = [(32, 32), (64, 64), (256, 256), (256, 512), (1024, 1024), (768, 3488), (2100, 2100)]
HBM_BYTES_PER_S = 8e12


def batch_of(m, n, batch, seed):
    """The batch as one (batch * m) x n matrix filled in one launch: member b = its rows b * m ...; a_bs = m * width."""
    w = (n + 63) // 64
    t = torch.empty(batch * m * w, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(t.data_ptr(), w, batch * m, n, seed, 0)
    return t, w, m * w


def time_batch(m, n, batch, full, reps):
    src, w, a_bs = batch_of(m, n, batch, 11)
    A = src.clone()
    rank = torch.empty(batch, dtype=torch.int32, device="cuda")
    piv = torch.empty(batch * min(m, n), dtype=torch.int32, device="cuda")
    call = lambda: m4ri_amd.echelonize_batch_dev(A.data_ptr(), w, a_bs, m, n, batch, full, rank.data_ptr(), piv.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
    call()  # warm
    out = []
    for _ in range(reps):
        A.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    ranks = rank.cpu()
    return min(out), statistics.median(out), int(ranks.min()), int(ranks.max())


def time_loop(m, n, members, full):
    src, w, a_bs = batch_of(m, n, members, 11)
    L, r = m4ri_amd.lib(), ctypes.c_int32(0)
    st = torch.cuda.current_stream().cuda_stream
    A = src.clone()
    assert L.m4ri_amd_echelonize_dev(A.data_ptr(), w, m, n, full, ctypes.byref(r), st) == 0  # warm
    A.copy_(src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for b in range(members):
        assert L.m4ri_amd_echelonize_dev(A.data_ptr() + 8 * b * a_bs, w, m, n, full, ctypes.byref(r), st) == 0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / members


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-only", action="store_true")
    ap.add_argument("--shape", type=int, nargs=2)
    ap.add_argument("--batch", type=int)
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    if args.batch_only:
        m, n = args.shape or (256, 256)
        batch = args.batch or 1024
        A, w, a_bs = batch_of(m, n, batch, 11)
        rank = torch.empty(batch, dtype=torch.int32, device="cuda")
        piv = torch.empty(batch * min(m, n), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(args.reps):
            m4ri_amd.echelonize_batch_dev(A.data_ptr(), w, a_bs, m, n, batch, args.full, rank.data_ptr(), piv.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        print(f"batch-only {m} x {n} batch {batch} path {m4ri_amd.plan_echelonize_batch(m, n)}: {args.reps} calls, ranks {int(rank.min())}..{int(rank.max())}")
        return
    print(f"full={args.full}; batch time = min / median of {args.reps} calls (HIP events); loop = m4ri_amd_echelonize_dev per member")
    print(f"{'shape':>12} {'path':>4} {'batch':>8} {'batch ms':>10} {'median':>10} {'loop ms/member':>14} {'loop ms (all)':>13} {'speedup':>9}  extra")
    rows = [(s, b) for s in SHAPES for b in (1, 256, 1024, 4096)] + [((32, 32), 1 << 20)]
    loop_cache = {}
    for (m, n), batch in rows:
        path = m4ri_amd.plan_echelonize_batch(m, n)
        if path == 3 and batch > 256:
            continue  # one by one: 4096 members of this size would only repeat the loop's number
        reps = 1 if path == 3 else args.reps
        tmin, tmed, rlo, rhi = time_batch(m, n, batch, args.full, reps)
        if (m, n) not in loop_cache:
            loop_cache[(m, n)] = time_loop(m, n, 16 if m * n <= 1 << 22 else 4, args.full)
        per = loop_cache[(m, n)]
        extra = f"ranks {rlo}..{rhi}"
        if path == 0:
            nbytes = 2 * batch * m * 8
            extra += f"; HBM floor {nbytes / HBM_BYTES_PER_S * 1e3:.4f} ms, achieved {nbytes / tmin / 1e12:.3f} TB/s ({nbytes / tmin / HBM_BYTES_PER_S * 100:.1f} % of 8)"
        print(f"{m:>5} x {n:<5} {path:>4} {batch:>8} {tmin * 1e3:>10.4f} {tmed * 1e3:>10.4f} {per * 1e3:>14.4f} {per * batch * 1e3:>13.2f} "
              f"{per * batch / tmin:>8.1f}x  {extra}", flush=True)


if __name__ == "__main__":
    main()

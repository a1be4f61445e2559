"""Block copies and permutations of batches on the device (assemble_batch.hip), in one process on device-resident buffers.

Block copy: m4ri_amd_copy_block_batch_dev of whole n x n members at source shifts 0 and 13, batches of `--mbytes` MiB or more, against
  copy  hipMemcpyAsync device to device of the same byte count (the box's own copy rate, measured in the same run), and, at shift 0,
  loop  what the batch cost before the call existed: a host loop of one hipMemcpy2DAsync per member, over the first
        min(batch, --loop-members) members, its time scaled to the batch.
Bytes moved = every word of the block read once and written once (a copy of n bytes counts 2 n).  Shift 0 runs twice: `dense` members
back to back (odd strides at 64: 8-byte accesses) and `even` strides and bases (16-byte accesses).
Permutations: m4ri_amd_apply_p_left_batch_dev / _right_batch_dev with a random LAPACK-style P per member: path 0 against path 1
(M4RI_AMD_PERM_BATCH_PATH0_MAX=0) at 64 x 64, path 1 against path 2 (M4RI_AMD_PERM_BATCH_PATH1_MAX=0, blocking, over --loop-members / 100
members, scaled) at 1088 x 1088, the largest square of path 1.
All contenders are warmed up and timed alternately `--reps` times, each timing a window of back-to-back calls between two HIP events
sized to `--window` seconds; ms = the median window, spread = (max - min) / median.

  python tools/bench_assemble_batch.py [--reps 5] [--window 0.3] [--mbytes 256] [--loop-members 20000] [--json out.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import m4ri_amd

PATH0, PATH1 = "M4RI_AMD_PERM_BATCH_PATH0_MAX", "M4RI_AMD_PERM_BATCH_PATH1_MAX"
COPY_SIZES = (64, 256, 1024, 16384)
D2D = 3  # hipMemcpyDeviceToDevice


def hip():
    h = ctypes.CDLL("libamdhip64.so")
    P, Z = ctypes.c_void_p, ctypes.c_size_t
    h.hipMemcpyAsync.restype, h.hipMemcpyAsync.argtypes = ctypes.c_int, [P, P, Z, ctypes.c_int, P]
    h.hipMemcpy2DAsync.restype, h.hipMemcpy2DAsync.argtypes = ctypes.c_int, [P, Z, P, Z, Z, Z, ctypes.c_int, P]
    return h


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
    for fn in list(fns.values()) * 2:
        fn()
    torch.cuda.synchronize()
    calls = {k: max(2, int(args.window / window(fn, 2)) + 1) for k, fn in fns.items()}
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


def copy_case(n, shift, even, args, h):
    w = w_of(n)
    sa, sd = w_of(n + shift), w
    if even:
        sa, sd = sa + (sa & 1), sd + (sd & 1)
    a_words, d_words = n * sa, n * sd
    batch = max(1, -(-args.mbytes * (1 << 20) // (8 * n * w)))
    A = torch.empty(batch * a_words + 2, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(A.data_ptr(), sa, batch * n, 64 * sa, 7 + n, 0)
    D = torch.zeros(batch * d_words + 2, dtype=torch.int64, device="cuda")
    moved = 8 * batch * n * w  # bytes read; as many written
    X, Y = torch.empty(moved // 8, dtype=torch.int64, device="cuda"), torch.zeros(moved // 8, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    off = 0 if even else 8 * (w & 1)  # dense members of an odd width: an 8-byte aligned base as well
    pa, pd = A.data_ptr() + off, D.data_ptr() + off
    fns = {"call": lambda: m4ri_amd.copy_block_batch_dev(pd, sd, d_words, 0, 0, pa, sa, a_words, 0, shift, n, n, batch, stream=st),
           "copy": lambda: h.hipMemcpyAsync(Y.data_ptr(), X.data_ptr(), moved, D2D, st)}
    nloop = min(batch, args.loop_members)
    if shift == 0:
        def loop():
            for b in range(nloop):
                h.hipMemcpy2DAsync(pd + 8 * b * d_words, 8 * sd, pa + 8 * b * a_words, 8 * sa, 8 * w, n, D2D, st)
        fns["loop"] = loop
    t = alternate(fns, args)
    m = {k: med(v) for k, v in t.items()}
    r = dict(kind="copy", n=n, shift=shift, layout="even" if even else "dense", batch=batch, ms=m["call"] * 1e3, spread=spread(t["call"]),
             gbs=2 * moved / m["call"] / 1e9, copy_gbs=2 * moved / m["copy"] / 1e9, copy_spread=spread(t["copy"]))
    r["of_copy"] = r["gbs"] / r["copy_gbs"]
    if shift == 0:
        r["loop_ms"] = m["loop"] * 1e3 * batch / nloop
        r["loop_x"] = r["loop_ms"] / r["ms"]
    return r


def perm_case(n, right, slow_env, slow_members, args):
    """The routed path against the path `slow_env` = "0" forces, on the same members and permutations."""
    w = w_of(n)
    batch = max(1, -(-args.mbytes * (1 << 20) // (8 * n * w)))
    A = torch.empty(batch * n * w, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(A.data_ptr(), w, batch * n, n, 9 + n, 0)
    rng = np.random.default_rng(n + right)
    hp = (np.arange(n)[None, :] + (rng.random((min(batch, 4096), n)) * (n - np.arange(n))[None, :]).astype(np.int64)).astype(np.int32)
    P = torch.from_numpy(np.tile(hp, (-(-batch // hp.shape[0]), 1))[:batch].copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    fn = m4ri_amd.apply_p_right_batch_dev if right else m4ri_amd.apply_p_left_batch_dev
    nslow = min(batch, slow_members)
    fast = lambda: fn(A.data_ptr(), w, n * w, n, n, batch, P.data_ptr(), n, n, False, 0, stream=st)
    slow = with_env(slow_env, "0", lambda: fn(A.data_ptr(), w, n * w, n, n, nslow, P.data_ptr(), n, n, False, 0, stream=st))
    t = alternate({"fast": fast, "slow": slow}, args)
    m = {k: med(v) for k, v in t.items()}
    path = m4ri_amd.plan_perm_batch(n, n, right)
    r = dict(kind="perm", n=n, side="right" if right else "left", batch=batch, path=path, ms=m["fast"] * 1e3, spread=spread(t["fast"]),
             other_path=path + 1, other_ms=m["slow"] * 1e3 * batch / nslow, other_spread=spread(t["slow"]), gbs=2 * 8 * batch * n * w / m["fast"] / 1e9)
    r["other_x"] = r["other_ms"] / r["ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--mbytes", type=int, default=256)
    ap.add_argument("--loop-members", type=int, default=20000)
    ap.add_argument("--json")
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    h = hip()
    rows = []
    print(f"{'n':>6} {'shift':>5} {'layout':>6} {'batch':>8} {'ms':>9} {'spread':>7} {'GB/s':>8} {'copy GB/s':>10} {'of copy':>8} {'loop ms':>10} {'loop x':>8}")
    for n in COPY_SIZES:
        for shift, even in ((0, False), (0, True), (13, False)):
            r = copy_case(n, shift, even, args, h)
            rows.append(r)
            loop = f"{r['loop_ms']:10.2f} {r['loop_x']:8.1f}" if "loop_ms" in r else f"{'-':>10} {'-':>8}"
            print(f"{n:6d} {shift:5d} {r['layout']:>6} {r['batch']:8d} {r['ms']:9.3f} {r['spread']:7.1%} {r['gbs']:8.0f} {r['copy_gbs']:10.0f} {r['of_copy']:8.1%} {loop}",
                  flush=True)
    print(f"\n{'n':>6} {'side':>6} {'batch':>8} {'path':>4} {'ms':>9} {'spread':>7} {'GB/s':>8} {'other':>5} {'other ms':>10} {'spread':>7} {'other/this':>10}")
    for n, env, members in ((64, PATH0, 1 << 30), (1088, PATH1, max(1, args.loop_members // 100))):
        for right in (0, 1):
            r = perm_case(n, right, env, members, args)
            rows.append(r)
            print(f"{n:6d} {r['side']:>6} {r['batch']:8d} {r['path']:4d} {r['ms']:9.3f} {r['spread']:7.1%} {r['gbs']:8.0f} {r['other_path']:5d} {r['other_ms']:10.2f} "
                  f"{r['other_spread']:7.1%} {r['other_x']:10.1f}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

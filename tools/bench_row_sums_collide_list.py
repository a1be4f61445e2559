"""m4ri_amd_row_sums_collide_list_batch_dev and m4ri_amd_row_sums_words_batch_dev on device-resident random generators, with the
protocol of tools/bench_row_sums_collide.py (contenders warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of
back-to-back calls between two HIP events sized to `--window` seconds; ms per call = the median of the windows, spread = (max - min) /
median).
  meant    the shapes of tools/bench_row_sums_collide.py at ell = 16 and 24 (balanced halves, the window the columns 0 .. ell-1, no V,
           w_min = 1): the existing call with hist and lightest (the yardstick) against the list call with hist, lightest, list and
           count, w_max the smallest weight at which the yardstick's own histogram leaves the batch at least two keys per member on
           average, cap = 64.  `over`: list / yardstick - 1.
  flood    ell = 0 and 8 with w_max = n, so that every colliding pair is emitted, on both paths (M4RI_AMD_ROW_SUMS_COLLIDE_PATH0_MAX);
           the batch cut so that the lists stay below 1 GiB.  10^6 keys per second, and on path 1 that rate over the 88 * 10^6 returning
           adds per second one word takes.  Documentation, not a gate.
  words    64 x 128, 256 x 512 and 1024 x 1024 generators, t1 + t2 = 4 (balanced halves) and 16 (t1 = t2 = 8 on the first 48 rows: with
           more rows C(k1, 8) * C(k2, 8) is beyond the 2^40 ranks), cap = 1024 random valid keys per member, no count; 10^9 bytes
           written per second beside a device-to-device hipMemcpyAsync of W's byte count timed in the same rounds (bytes written per
           second: what tools/bench_assemble_batch.py calls the copy rate is twice that, reads and writes).

  python tools/bench_row_sums_collide_list.py [--reps 3] [--window 0.3] [--json out.json] [--only meant|flood|words]"""
import argparse
import ctypes
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
SHAPES = [(64, 128, 2), (128, 256, 2), (256, 512, 2), (72, 256, 3)]
PAIRS = 1 << 34                 # per call of the shapes, as in tools/bench_row_sums_collide.py
CAP = 64
FLOOD = [(64, 128, 2, 0), (64, 128, 2, 8), (128, 256, 2, 8)]
FLOOD_KEYS = 1 << 27            # list entries per call at most: 1 GiB
ATOMIC_RATE = 88e6              # returning 64-bit adds per second on one word (MI355X)
WORDS = [(64, 128), (256, 512), (1024, 1024)]
WORDS_CAP = 1024
WORDS_BYTES = 1 << 28
D2D = 3


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

    def __init__(self, k, n, batch, seed, cap):
        self.k, self.n, self.batch, self.w, self.cap = k, n, batch, n // 64, cap
        self.st = torch.cuda.current_stream().cuda_stream
        self.G = torch.empty(batch * k * self.w, dtype=torch.int64, device="cuda")
        m4ri_amd.fill_dev(self.G.data_ptr(), self.w, batch * k, n, seed, 0)
        self.hist = torch.zeros(batch * (n + 1), dtype=torch.int64, device="cuda")
        self.light = torch.zeros(batch, dtype=torch.int64, device="cuda")
        self.list = torch.zeros(batch * cap, dtype=torch.int64, device="cuda")
        self.count = torch.zeros(batch, dtype=torch.int64, device="cuda")

    def plain(self, k1, t1, t2, ell):
        m4ri_amd.row_sums_collide_batch_dev(self.G.data_ptr(), self.w, self.k * self.w, self.k, self.n, 0, 0, self.batch, k1, t1, t2, 0, 0, ell, 1,
                                            self.hist.data_ptr(), self.light.data_ptr(), stream=self.st)

    def listed(self, k1, t1, t2, ell, w_max, both=True):
        m4ri_amd.row_sums_collide_list_batch_dev(self.G.data_ptr(), self.w, self.k * self.w, self.k, self.n, 0, 0, self.batch, k1, t1, t2, 0, 0, ell, 1, w_max,
                                                 self.hist.data_ptr() if both else 0, self.light.data_ptr() if both else 0, self.list.data_ptr(), self.cap,
                                                 self.cap, self.count.data_ptr(), stream=self.st)


def run_meant(k, n, t, args):
    k1 = k // 2
    pairs = comb(k1, t) * comb(k - k1, t)
    batch = min(8192, max(256, PAIRS // pairs))
    m = Members(k, n, batch, 31 + k + n + t, CAP)
    rows = []
    for ell in (16, 24):
        m.plain(k1, t, t, ell)
        torch.cuda.synchronize()
        h = m.hist.view(batch, n + 1).sum(dim=0).cpu().tolist()
        want_hist, want_light = m.hist.clone(), m.light.clone()
        run, w_max = 0, n
        for w in range(1, n + 1):
            run += h[w]
            if run >= 2 * batch:
                w_max = w
                break
        fns = {"yardstick": lambda ell=ell: m.plain(k1, t, t, ell), "list": lambda ell=ell, w_max=w_max: m.listed(k1, t, t, ell, w_max)}
        m.hist.fill_(-7), m.light.fill_(-7)
        fns["list"]()
        torch.cuda.synchronize()
        band = want_hist.view(batch, n + 1)[:, 1:w_max + 1].sum(dim=1)
        assert torch.equal(m.hist, want_hist) and torch.equal(m.light, want_light) and torch.equal(m.count, band), (k, n, ell)
        tm = alternate(fns, args)
        y, l = tm["yardstick"], tm["list"]
        row = dict(k=k, n=n, t1=t, t2=t, batch=batch, ell=ell, w_max=w_max, keys_per_member=float(band.sum()) / batch, most_keys=int(band.max()),
                   lib_path=m4ri_amd.plan_row_sums_collide_batch(k, n, k1, t, t, ell), ms={c: med(v) * 1e3 for c, v in tm.items()},
                   spread={c: spread(v) for c, v in tm.items()}, windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()}, over=med(l) / med(y) - 1)
        rows.append(row)
        print(f"{k:>4} {n:>5} {t}+{t} {batch:>6} {ell:>3} {w_max:>5} {row['keys_per_member']:>9.2f} {row['most_keys']:>5} {row['lib_path']:>4} {row['ms']['yardstick']:>10.4f} "
              f"{row['spread']['yardstick'] * 100:>5.1f}% {row['ms']['list']:>10.4f} {row['spread']['list'] * 100:>5.1f}% {row['over'] * 100:>+6.1f}%", flush=True)
    del m
    torch.cuda.empty_cache()
    return rows


def run_flood(k, n, t, ell, args):
    k1 = k // 2
    pairs = comb(k1, t) * comb(k - k1, t)
    per = pairs >> ell                      # about this many collisions per member
    batch = max(1, min(8192, PAIRS // pairs, FLOOD_KEYS // max(per * 2, 1)))
    probe = Members(k, n, batch, 31 + k + n + t, 0)
    probe.listed(k1, t, t, ell, n)
    torch.cuda.synchronize()
    cap, keys = int(probe.count.max()), int(probe.count.sum())
    del probe
    m = Members(k, n, batch, 31 + k + n + t, cap)
    fns = {}
    for path in (0, 1):
        fns[f"path{path} both"] = routed(path, lambda: m.listed(k1, t, t, ell, n))
        fns[f"path{path} list alone"] = routed(path, lambda: m.listed(k1, t, t, ell, n, both=False))
        fns[f"path{path} yardstick"] = routed(path, lambda: m.plain(k1, t, t, ell))
    sorted_lists = {}
    for path in (0, 1):
        m.list.fill_(-7)
        fns[f"path{path} both"]()
        torch.cuda.synchronize()
        assert int(m.count.sum()) == keys
        sorted_lists[path] = torch.sort(m.list.view(batch, cap), dim=1).values.clone()
    assert torch.equal(sorted_lists[0], sorted_lists[1]), "the two paths list different sets"
    tm = alternate(fns, args)
    rows = []
    for name, v in tm.items():
        row = dict(k=k, n=n, t1=t, t2=t, batch=batch, ell=ell, call=name, keys=keys, ms=med(v) * 1e3, spread=spread(v), windows_ms=[x * 1e3 for x in v],
                   mkeys_per_s=0.0 if name.endswith("yardstick") else keys / med(v) / 1e6)
        row["of_atomic_rate"] = row["mkeys_per_s"] * 1e6 / ATOMIC_RATE if name.startswith("path1") and not name.endswith("yardstick") else None
        rows.append(row)
        tail = "" if row["of_atomic_rate"] is None else f"  {row['of_atomic_rate']:.1f}x the one-word atomic rate"
        print(f"{k:>4} {n:>5} {t}+{t} {batch:>6} {ell:>3} {name:>18} {keys:>11} {row['ms']:>10.4f} {row['spread'] * 100:>5.1f}% {row['mkeys_per_s']:>10.1f}{tail}", flush=True)
    del m
    torch.cuda.empty_cache()
    return rows


def run_words(k, n, t, args, hip):
    kk = k if t == 2 else min(k, 48)        # the rows the keys name
    k1 = kk // 2
    pairs, w = comb(k1, t) * comb(kk - k1, t), n // 64
    batch = max(1, WORDS_BYTES // (WORDS_CAP * w * 8))
    st = torch.cuda.current_stream().cuda_stream
    G = torch.empty(batch * k * w, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(G.data_ptr(), w, batch * k, n, 5 + k, 0)
    keys = torch.randint(0, pairs, (batch * WORDS_CAP,), dtype=torch.int64, device="cuda")
    W, X = torch.zeros(batch * WORDS_CAP * w, dtype=torch.int64, device="cuda"), torch.zeros(batch * WORDS_CAP * w, dtype=torch.int64, device="cuda")
    skipped = torch.zeros(batch, dtype=torch.int32, device="cuda")
    nbytes = batch * WORDS_CAP * w * 8
    fns = {"call": lambda: m4ri_amd.row_sums_words_batch_dev(G.data_ptr(), w, k * w, kk, n, 0, 0, batch, k1, t, t, keys.data_ptr(), WORDS_CAP, WORDS_CAP, 0,
                                                              W.data_ptr(), w, WORDS_CAP * w, skipped.data_ptr(), stream=st),
           "copy": lambda: hip.hipMemcpyAsync(X.data_ptr(), W.data_ptr(), nbytes, D2D, st)}
    fns["call"]()
    torch.cuda.synchronize()
    assert int(skipped.sum()) == 0 and int((W != 0).sum()) > 0
    tm = alternate(fns, args)
    row = dict(k=k, n=n, rows_named=kk, t1=t, t2=t, batch=batch, cap=WORDS_CAP, bytes=nbytes, ms={c: med(v) * 1e3 for c, v in tm.items()},
               spread={c: spread(v) for c, v in tm.items()}, windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()},
               written_gbs=nbytes / med(tm["call"]) / 1e9, copy_written_gbs=nbytes / med(tm["copy"]) / 1e9)
    row["of_copy"] = row["written_gbs"] / row["copy_written_gbs"]
    print(f"{k:>5} {n:>5} {kk:>5} {t}+{t} {batch:>6} {row['ms']['call']:>9.4f} {row['spread']['call'] * 100:>5.1f}% {row['written_gbs']:>9.1f} {row['ms']['copy']:>9.4f} "
          f"{row['spread']['copy'] * 100:>5.1f}% {row['copy_written_gbs']:>9.1f} {row['of_copy'] * 100:>6.1f}%", flush=True)
    del G, keys, W, X
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--json")
    ap.add_argument("--only", choices=("meant", "flood", "words"))
    args = ap.parse_args()
    assert args.reps >= 3 and args.window >= 0.3
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype, hip.hipMemcpyAsync.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    print(f"ms per call, median of {args.reps} alternating windows of >= {args.window} s; no V, w_min = 1")
    meant, flood, words = [], [], []
    if args.only in (None, "meant"):
        print(f"the list call where it is meant to run: hist + lightest (yardstick) against hist + lightest + list + count, cap = {CAP}")
        print(f"{'k':>4} {'n':>5} {'t':>3} {'batch':>6} {'ell':>3} {'w_max':>5} {'keys/mem':>9} {'most':>5} {'path':>4} {'yard ms':>10} {'spread':>6} {'list ms':>10} {'spread':>6} {'over':>7}")
        meant = [r for s in SHAPES for r in run_meant(*s, args)]
        print(f"over 3 %: {[(r['k'], r['n'], r['ell']) for r in meant if r['over'] > 0.03] or 'no measured row'}")
    if args.only in (None, "flood"):
        print("every colliding pair emitted (w_max = n): keys per second on both paths")
        print(f"{'k':>4} {'n':>5} {'t':>3} {'batch':>6} {'ell':>3} {'call':>18} {'keys':>11} {'ms':>10} {'spread':>6} {'Mkeys/s':>10}")
        flood = [r for s in FLOOD for r in run_flood(*s, args)]
    if args.only in (None, "words"):
        print(f"the words call: cap = {WORDS_CAP} keys per member, bytes written per second beside a device-to-device copy of W's bytes")
        print(f"{'k':>5} {'n':>5} {'rows':>5} {'t':>3} {'batch':>6} {'call ms':>9} {'spread':>6} {'GB/s':>9} {'copy ms':>9} {'spread':>6} {'GB/s':>9} {'of copy':>7}")
        words = [run_words(k, n, t, args, hip) for k, n in WORDS for t in (2, 8)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(meant=meant, flood=flood, words=words), f, indent=1)


if __name__ == "__main__":
    main()

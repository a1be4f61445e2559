"""Products of many tiny matrices: m4ri_amd_mul_small_batch_dev against what the batch cost before it existed, m4ri_amd_m4rm_batch_dev,
in the same process on the same device-resident buffers.  Per shape: both entries warmed up, then timed ALTERNATELY `--reps` times
each, every timing a window of back-to-back calls between two HIP events sized to `--window` seconds; the two results compared on
C's valid bits.  Shapes with a dimension above 64 run with M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX=256, i.e. on path 1 whatever D1 the
library was built with: the table is what D1 is chosen from.  Members are dense and back to back (stride = width), random
(fill_dev), add = 0; the batch makes the operands (A, B and C) total about `--mbytes` MB.

Columns: ms per call (median of the windows) and the spread of the windows ((max - min) / median) for each entry; speed-up = old
median / new median; `clear` = the slowest new window is faster than the fastest old one (the gain exceeds the spread); achieved
bytes/s of the new entry from the algorithmic bytes (every word of A and B read once, every word of C written once) and its share of
the HBM peak; the two floors of the new kernels -- HBM at the peak, and vector issue: the unrolled loop's instructions (one signed
field extract and a v_readlane + v_bitop3_b32 pair per live half of C's word, per inner bit in groups of eight) at two cycles per
wave instruction on every SIMD of the chip -- and which of them is the larger.

  python tools/bench_mul_small_batch.py [--reps 5] [--window 0.3] [--mbytes 256 | --batch N] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

HBM_PEAK = 8.0e12          # bytes/s, the specification figure; about 6.3e12 is what a plain copy achieves
SIMDS, CLOCK = 1024, 2.4e9  # 256 CUs x 4 SIMDs
OVERRIDE = "M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX"
CUBES = (16, 32, 64, 128, 192, 256)
SHAPES = [(d, d, d, False) for d in CUBES] + [(64, 64, 64, True), (128, 64, 64, False), (64, 128, 64, False), (64, 64, 128, False)]


def w_of(n):
    return (n + 63) // 64


def filled(rows, n, seed):
    t = torch.empty(max(1, rows * w_of(n)), dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(t.data_ptr(), w_of(n), rows, n, seed, 0)
    return t


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def valu_floor(m, l, n, batch):
    """Seconds the unrolled loop needs at full vector issue: waves x instructions x 2 cycles over every SIMD."""
    waves = batch * ((m + 63) // 64) * w_of(n)
    per_bit = 1 + 2 * (2 if n > 32 else 1)
    groups = sum((min(64, l - 64 * q) + 7) // 8 for q in range(w_of(l)))
    return waves * groups * 8 * per_bit * 2 / (SIMDS * CLOCK)


def run_shape(m, l, n, share_b, args):
    wl, wn = w_of(l), w_of(n)
    member_bytes = 8 * (m * wl + l * wn + m * wn)
    batch = args.batch or max(1, args.mbytes * 1000000 // member_bytes)
    A = filled(batch * m, l, 11)
    B = filled((1 if share_b else batch) * l, n, 12)
    Cn = torch.full((batch * m * wn,), 0x5555555555555555, dtype=torch.int64, device="cuda")
    Co = Cn.clone()
    st = torch.cuda.current_stream().cuda_stream
    bbs = 0 if share_b else l * wn
    common = (A.data_ptr(), wl, m * wl, B.data_ptr(), wn, bbs, m, l, n, batch)
    L = m4ri_amd.lib()
    new = lambda: m4ri_amd.mul_small_batch_dev(Cn.data_ptr(), wn, m * wn, *common, add=False, stream=st)

    def old():
        rc = L.m4ri_amd_m4rm_batch_dev(Co.data_ptr(), wn, m * wn, *common, 0, st)
        assert rc == 0, rc

    if max(m, l, n) > 64:
        os.environ[OVERRIDE] = "256"
    else:
        os.environ.pop(OVERRIDE, None)
    path = 0 if max(m, l, n) <= 64 else 1
    for fn in (new, old, new, old):  # warm-up
        fn()
    torch.cuda.synchronize()
    gen = int(m4ri_amd.get_stats().leaf_gen)
    mask = torch.full((wn,), -1, dtype=torch.int64, device="cuda")
    if n % 64:
        mask[-1] = (1 << (n % 64)) - 1
    equal = not bool((((Cn ^ Co).view(-1, wn)) & mask).any())
    calls = {}
    for name, fn in (("new", new), ("old", old)):
        t1 = window(fn, 3)
        calls[name] = max(3, int(args.window / t1) + 1)
    t = {"new": [], "old": []}
    for _ in range(args.reps):
        t["new"].append(window(new, calls["new"]))
        t["old"].append(window(old, calls["old"]))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    nbytes = member_bytes * batch - (8 * l * wn * (batch - 1) if share_b else 0)
    hbm, valu = nbytes / HBM_PEAK, valu_floor(m, l, n, batch)
    row = dict(m=m, l=l, n=n, share_b=share_b, batch=batch, path=path, old_gen=gen, equal=equal, new_ms=med["new"] * 1e3, old_ms=med["old"] * 1e3,
               new_spread=spread["new"], old_spread=spread["old"], speedup=med["old"] / med["new"], clear=max(t["new"]) < min(t["old"]),
               new_windows_ms=[x * 1e3 for x in t["new"]], old_windows_ms=[x * 1e3 for x in t["old"]], calls=calls, mbytes=nbytes / 1e6,
               tbytes_per_s=nbytes / med["new"] / 1e12, hbm_share=nbytes / med["new"] / HBM_PEAK, hbm_floor_ms=hbm * 1e3, valu_floor_ms=valu * 1e3,
               bound="HBM" if hbm >= valu else "VALU issue")
    print(f"{m:>4} {l:>4} {n:>4} {'shared B' if share_b else '':>8} {batch:>8} {path:>4} {gen:>3} {row['new_ms']:>9.4f} {spread['new'] * 100:>5.1f}% "
          f"{row['old_ms']:>10.4f} {spread['old'] * 100:>5.1f}% {row['speedup']:>8.2f}x {'yes' if row['clear'] else 'NO':>5} {'ok' if equal else 'DIFFER':>6} "
          f"{row['tbytes_per_s']:>6.3f} {row['hbm_share'] * 100:>5.1f}% {row['hbm_floor_ms']:>8.4f} {row['valu_floor_ms']:>8.4f}  {row['bound']}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--mbytes", type=int, default=256)
    ap.add_argument("--batch", type=int, help="this many members for every shape instead of --mbytes (a smaller batch sends the old path "
                    "to another leaf generation, column `gen`)")
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.reps >= 5 and 64 <= args.mbytes <= 1000
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    print(f"mul_small_batch_dev (new) against m4rm_batch_dev (old): ms per call, median of {args.reps} alternating windows of >= {args.window} s; "
          f"{'batch ' + str(args.batch) if args.batch else 'operands about ' + str(args.mbytes) + ' MB'}; library D1 = {max(d for d in (64, 128, 192, 256) if m4ri_amd.plan_mul_small_batch(d, d, d) != 2)}")
    print(f"{'m':>4} {'l':>4} {'n':>4} {'':>8} {'batch':>8} {'path':>4} {'gen':>3} {'new ms':>9} {'spread':>6} {'old ms':>10} {'spread':>6} {'speed-up':>9} "
          f"{'clear':>5} {'bits':>6} {'TB/s':>6} {'of 8':>6} {'HBM ms':>8} {'VALU ms':>8}  floor")
    rows = [run_shape(m, l, n, s, args) for (m, l, n, s) in SHAPES]
    cube = {r["m"]: r for r in rows if r["m"] == r["l"] == r["n"] and not r["share_b"]}
    d1 = 64
    for d in (128, 192, 256):
        if not (cube[d]["clear"] and cube[d]["equal"]):
            break
        d1 = d
    small = all(cube[d]["clear"] and cube[d]["equal"] for d in (16, 32, 64))
    print(f"D1 from this table: {d1} (the largest of 128, 192, 256 at which path 1 is clear of the old path on the cube, and at every smaller one; 64 = none)")
    print(f"path 0 clear of the old path at every cube <= 64: {'yes' if small else 'NO'}; all results equal on the valid bits: "
          f"{'yes' if all(r['equal'] for r in rows) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(d1=d1, path0_clear=small, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

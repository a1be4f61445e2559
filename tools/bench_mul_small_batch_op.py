"""Products of many tiny matrices with transposed operands: m4ri_amd_mul_small_batch_op_dev (one launch, no scratch) against what the
library offered before it, m4ri_amd_transpose_batch_dev of every transposed operand into a scratch buffer followed by
m4ri_amd_mul_small_batch_dev on the same stream, and against the untransposed call of the same shape, which is what the fused
transposes cost.  The protocol is tools/bench_mul_small_batch.py's: the operands (A, B and C; the scratch of the composition comes on
top) total about `--mbytes` MB and stay resident, every contender is warmed up, then they are timed ALTERNATELY `--reps` times each,
every timing a window of back-to-back calls between two HIP events sized to `--window` seconds.  Members are dense and back to back
(stride = width), random (fill_dev), add = 0.  Shapes with a dimension above 64 run with M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX=256, i.e.
on path 1 whatever D1op the library was built with: the table is what D1op is chosen from.

Columns: ms per call (median of the windows) and the spread of the windows ((max - min) / median) of the fused call and of the
composition; `x comp` = composition median / fused median; `ok` = the fused call is not slower than the composition by more than the
spread (fused median <= composition median * (1 + the larger of the two spreads)); the untransposed call's ms and `x NN` = fused
median / its median; achieved bytes/s of the fused call from the algorithmic bytes (every word of the stored A and B read once, a
shared or aliased operand counted once, every word of C written once); `bits` = the whole buffers of C of the fused call and of the
composition are equal.

  python tools/bench_mul_small_batch_op.py [--reps 5] [--window 0.3] [--mbytes 256] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

OVERRIDE = "M4RI_AMD_MUL_SMALL_BATCH_PATH1_MAX"
NT, TN, TT = (0, 1), (1, 0), (1, 1)
NAME = {NT: "NT", TN: "TN", TT: "TT"}
CANDIDATES = (128, 192, 256)
# (m, l, n, op, variant): variant "" | "gram" (B == A, the same pointer) | "shared B" (b_bs = 0)
SHAPES = ([(d, d, d, op, "") for d in (16, 32, 64) for op in (NT, TN, TT)] + [(64, 64, 64, NT, "gram"), (64, 64, 64, NT, "shared B")]
          + [(d, d, d, op, "") for d in CANDIDATES for op in (NT, TN, TT)] + [(128, 64, 64, NT, ""), (64, 128, 64, NT, "")])


def w_of(n):
    return (n + 63) // 64


def filled(count, rows, cols, seed):
    """`count` dense members of rows x cols, back to back, as one matrix of count * rows rows."""
    t = torch.empty(max(1, count * rows * w_of(cols)), dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(t.data_ptr(), w_of(cols), count * rows, cols, seed, 0)
    return t


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def run_shape(m, l, n, op, variant, args):
    ta, tb = op
    gram, share_b = variant == "gram", variant == "shared B"
    (ra, ca), (rb, cb) = ((l, m) if ta else (m, l)), ((n, l) if tb else (l, n))  # as stored
    wa, wb, wl, wn = w_of(ca), w_of(cb), w_of(l), w_of(n)
    a_words, b_words, c_words = ra * wa, (0 if gram else rb * wb), m * wn
    batch = max(1, args.mbytes * 1000000 // (8 * (a_words + b_words + c_words)))
    nb = 1 if share_b else batch
    A = filled(batch, ra, ca, 11)
    B = A if gram else filled(nb, rb, cb, 12)
    assert not gram or (ra, ca) == (rb, cb)
    b_bs = 0 if share_b else rb * wb
    Cf = torch.full((batch * c_words,), 0x5555555555555555, dtype=torch.int64, device="cuda")
    Cc, Cn = Cf.clone(), Cf.clone()
    st = torch.cuda.current_stream().cuda_stream
    # the composition's scratch, the caller's to own: the transposes, dense
    sA = torch.empty(batch * m * wl, dtype=torch.int64, device="cuda") if ta else None
    sB = torch.empty(nb * l * wn, dtype=torch.int64, device="cuda") if tb else None
    # the untransposed call of the same (m, l, n): operands of its own where the stored shapes differ
    An = A if (ra, ca) == (m, l) else filled(batch, m, l, 13)
    Bn = B if (rb, cb) == (l, n) else filled(nb, l, n, 14)

    def fused():
        m4ri_amd.mul_small_batch_op_dev(Cf.data_ptr(), wn, c_words, A.data_ptr(), wa, ra * wa, B.data_ptr(), wb, b_bs, m, l, n, batch, trans_a=bool(ta),
                                        trans_b=bool(tb), add=False, stream=st)

    def comp():
        a, b = (A.data_ptr(), wa, ra * wa), (B.data_ptr(), wb, b_bs)
        if ta:
            m4ri_amd.transpose_batch_dev(sA.data_ptr(), wl, m * wl, *a, l, m, batch, stream=st)
            a = (sA.data_ptr(), wl, m * wl)
        if tb:
            m4ri_amd.transpose_batch_dev(sB.data_ptr(), wn, l * wn, *b, n, l, nb, stream=st)
            b = (sB.data_ptr(), wn, 0 if share_b else l * wn)
        m4ri_amd.mul_small_batch_dev(Cc.data_ptr(), wn, c_words, *a, *b, m, l, n, batch, add=False, stream=st)

    def nn():
        m4ri_amd.mul_small_batch_dev(Cn.data_ptr(), wn, c_words, An.data_ptr(), wl, m * wl, Bn.data_ptr(), wn, 0 if share_b else l * wn, m, l, n, batch,
                                     add=False, stream=st)

    if max(m, l, n) > 64:
        os.environ[OVERRIDE] = "256"
    else:
        os.environ.pop(OVERRIDE, None)
    fns = dict(fused=fused, comp=comp, nn=nn)
    for fn in list(fns.values()) * 2:  # warm-up
        fn()
    torch.cuda.synchronize()
    equal = bool(torch.equal(Cf, Cc))
    calls = {k: max(3, int(args.window / window(fn, 3)) + 1) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(args.reps):
        for k, fn in fns.items():
            t[k].append(window(fn, calls[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
    nbytes = 8 * (batch * a_words + (0 if gram else nb * rb * wb) + batch * c_words)
    ok = med["fused"] <= med["comp"] * (1 + max(spread["fused"], spread["comp"]))
    row = dict(m=m, l=l, n=n, op=NAME[op], variant=variant, batch=batch, path=0 if max(m, l, n) <= 64 else 1, equal=equal,
               fused_ms=med["fused"] * 1e3, comp_ms=med["comp"] * 1e3, nn_ms=med["nn"] * 1e3, fused_spread=spread["fused"], comp_spread=spread["comp"],
               nn_spread=spread["nn"], over_comp=med["comp"] / med["fused"], over_nn=med["fused"] / med["nn"], not_slower=ok,
               windows_ms={k: [x * 1e3 for x in v] for k, v in t.items()}, calls=calls, mbytes=nbytes / 1e6, tbytes_per_s=nbytes / med["fused"] / 1e12)
    print(f"{m:>4} {l:>4} {n:>4} {NAME[op]:>3} {variant:>8} {batch:>8} {row['path']:>4} {row['fused_ms']:>9.4f} {spread['fused'] * 100:>5.1f}% "
          f"{row['comp_ms']:>9.4f} {spread['comp'] * 100:>5.1f}% {row['over_comp']:>7.2f}x {'yes' if ok else 'NO':>4} {row['nn_ms']:>9.4f} "
          f"{spread['nn'] * 100:>5.1f}% {row['over_nn']:>6.2f}x {row['tbytes_per_s']:>6.3f} {'ok' if equal else 'DIFFER':>6}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--mbytes", type=int, default=256)
    ap.add_argument("--json")
    args = ap.parse_args()
    assert args.reps >= 5 and 64 <= args.mbytes <= 1000
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device: nothing to measure"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    built = max(d for d in (64, 128, 192, 256) if m4ri_amd.plan_mul_small_batch_op(d, d, d, True, True) != 2)
    print(f"mul_small_batch_op_dev (fused) against transpose_batch_dev into scratch + mul_small_batch_dev (comp) and against the untransposed "
          f"mul_small_batch_dev of the same shape (NN): ms per call, median of {args.reps} alternating windows of >= {args.window} s; operands about "
          f"{args.mbytes} MB; library D1op = {built}")
    print(f"{'m':>4} {'l':>4} {'n':>4} {'op':>3} {'':>8} {'batch':>8} {'path':>4} {'fused ms':>9} {'spread':>6} {'comp ms':>9} {'spread':>6} {'x comp':>8} "
          f"{'ok':>4} {'NN ms':>9} {'spread':>6} {'x NN':>7} {'TB/s':>6} {'bits':>6}")
    rows = [run_shape(*s, args) for s in SHAPES]
    good = lambda d: all(r["not_slower"] and r["equal"] for r in rows if r["m"] == r["l"] == r["n"] == d and not r["variant"])
    d1op = 64
    for d in CANDIDATES:
        if not good(d):
            break
        d1op = d
    path0 = all(r["not_slower"] and r["equal"] for r in rows if r["path"] == 0)
    print(f"D1op from this table: {d1op} (the largest of 128, 192, 256 at which the fused call is not slower than the composition by more than the "
          f"spread on the cube for every op, and at every smaller one; 64 = none)")
    print(f"path 0 not slower than the composition at every shape <= 64: {'yes' if path0 else 'NO'}; all results equal: "
          f"{'yes' if all(r['equal'] for r in rows) else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(d1op=d1op, path0_not_slower=path0, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

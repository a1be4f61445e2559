"""m4ri_amd_isd_collide_search_dev against the loop it fuses, on device-resident systematic forms with a received word stacked under
each: 16 iterations of "exchange `steps` pivots, then Stern's collision step on the window order[k : k + ell]" (w_min = 1) for every
member of a batch,
  fused      one call of m4ri_amd_isd_collide_search_dev(iters = 16, w_stop = -1), the best word written out;
  two calls  the same 16 iterations as m4ri_amd_pivot_exchange_batch_dev(seed = isd_iteration_seed(seed, it)) and
             m4ri_amd_row_sums_collide_batch_dev(cols = order + k, lightest only), 31 calls, the 16 keys per member left in an array (the
             loop has no running minimum and writes no word: it does less),
each as plain launches and replayed from one captured graph.  The baseline is the two-call loop of the same build; it is never the new
call.  Before anything is timed the tool checks from one starting state that both leave the same D, pivots and order bit for bit and
that best is the lightest of the loop's keys, the earliest among equal weights.  The timed calls then chain: every call goes on from
the state the previous one left.
  shapes   k x n = 32 x 64 (k1 = 16, t = 1 + 1, ell = 4) and 64 x 128 (k1 = 32; t = 1 + 1, ell = 5 and t = 2 + 2, ell = 9) at 65 536
           members, 256 x 512 (k1 = 128, t = 2 + 2, ell = 13) at 4 096, steps = 1 and 4;
  threads  every shape at steps = 1 again with the workgroup forced to 64 ... 1024 threads (M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS) beside
           the size the call chooses: what the rule of DESIGN 3.18 rests on;
  stop     64 x 128, t = 1 + 1, steps = 1: the fused call with w_stop = the median of the members' best weights after 16 iterations, so
           that about half of the members stop early: what the stop saves.

The contenders of a row are warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of back-to-back calls between
two HIP events sized to `--window` seconds.  Columns: ms per 16 iterations of the batch (median of the windows), the spread of the
windows ((max - min) / median) and iterations per second (members * 16 / time); `clear`: the fused call's slowest window is faster
than the two-call loop's fastest, both taken the faster of plain and graph; `LOSES`: the other way round; else `within the spread`.

  python tools/bench_isd_collide_search.py [--reps 3] [--window 0.3] [--json out.json] [--txt out.txt]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import m4ri_amd

# (k, n, members, k1, t1, t2, ell)
SHAPES = [(32, 64, 65536, 16, 1, 1, 4), (64, 128, 65536, 32, 1, 1, 5), (64, 128, 65536, 32, 2, 2, 9), (256, 512, 4096, 128, 2, 2, 13)]
STEPS = (1, 4)
ITERS, W_MIN, SEED = 16, 1, 2027
THREADS = "M4RI_AMD_ISD_COLLIDE_SEARCH_THREADS"
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


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
    def __init__(self, k, n, batch, k1, t1, t2, ell, seed):
        self.k, self.n, self.w, self.batch, self.split = k, n, n // 64, batch, (k1, t1, t2, ell)
        w, m = self.w, k + 1                      # row k: the received word
        self.m = m
        G = torch.empty(m * w, dtype=torch.int64, device="cuda")
        m4ri_amd.fill_dev(G.data_ptr(), w, m, n, seed, 0)
        self.O = torch.empty(batch * n, dtype=torch.int32, device="cuda")
        self.D = torch.empty(batch * m * w, dtype=torch.int64, device="cuda")
        self.rank = torch.empty(batch, dtype=torch.int32, device="cuda")
        self.piv = torch.empty(batch * k, dtype=torch.int32, device="cuda")
        self.best = torch.empty(batch, dtype=torch.int64, device="cuda")
        self.best_iter, self.run, self.done = (torch.empty(batch, dtype=torch.int32, device="cuda") for _ in range(3))
        self.W = torch.empty(batch * w, dtype=torch.int64, device="cuda")
        self.keys = torch.empty((ITERS, batch), dtype=torch.int64, device="cuda")
        m4ri_amd.random_orders_batch_dev(self.O.data_ptr(), n, n, batch, seed + 1, 0)
        m4ri_amd.echelonize_order_batch_dev(self.D.data_ptr(), w, m * w, G.data_ptr(), w, 0, m, n, k, self.O.data_ptr(), n, n, batch, 1, self.rank.data_ptr(),
                                            self.piv.data_ptr(), 0)
        torch.cuda.synchronize()
        self.state = (self.D.clone(), self.piv.clone(), self.O.clone())
        self.seeds = [m4ri_amd.isd_iteration_seed(SEED, it) for it in range(ITERS)]

    def reset(self):
        for dst, src in zip((self.D, self.piv, self.O), self.state):
            dst.copy_(src)
        torch.cuda.synchronize()

    def fused(self, steps, w_stop=-1, stream=0):
        k, n, w, m = self.k, self.n, self.w, self.m
        m4ri_amd.isd_collide_search_dev(self.D.data_ptr(), w, m * w, m, n, k, self.piv.data_ptr(), self.rank.data_ptr(), self.batch, ITERS, steps, SEED,
                                        *self.split, W_MIN, w_stop, self.best.data_ptr(), self.O.data_ptr(), n, n, self.best_iter.data_ptr(), self.run.data_ptr(),
                                        self.done.data_ptr(), self.W.data_ptr(), w, stream)

    def two_calls(self, steps, stream=0):
        k, n, w, m = self.k, self.n, self.w, self.m
        k1, t1, t2, ell = self.split
        call = m4ri_amd.lib().m4ri_amd_row_sums_collide_batch_dev
        for it in range(ITERS):
            if it:
                m4ri_amd.pivot_exchange_batch_dev(self.D.data_ptr(), w, m * w, m, n, k, self.piv.data_ptr(), self.rank.data_ptr(), self.batch, 0, 0, steps,
                                                  self.seeds[it], self.O.data_ptr(), n, n, 0, stream)
            rc = call(self.D.data_ptr(), w, m * w, k, n, self.D.data_ptr() + 8 * k * w, m * w, self.batch, k1, t1, t2, self.O.data_ptr() + 4 * k, n, ell, W_MIN,
                      None, self.keys[it].data_ptr(), stream or None)
            assert rc == 0, rc

    def graph(self, fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return g.replay


def check(s, steps):
    """from one starting state: the same D, pivots and order, and best the lightest of the loop's keys, the earliest among equal weights"""
    s.reset()
    s.fused(steps)
    torch.cuda.synchronize()
    d, p, o = s.D.clone(), s.piv.clone(), s.O.clone()
    best, best_iter = s.best.cpu().numpy(), s.best_iter.cpu().numpy()
    s.reset()
    s.two_calls(steps)
    torch.cuda.synchronize()
    same = torch.equal(s.D, d) and torch.equal(s.piv, p) and torch.equal(s.O, o)
    keys = s.keys.cpu().numpy()
    weights = np.where(keys < 0, 1 << 30, keys >> 40)
    first = weights.argmin(axis=0)                 # NumPy: the first of equal minima
    lightest = keys[first, np.arange(s.batch)]
    same = same and np.array_equal(best, lightest) and np.array_equal(best_iter, np.where(lightest < 0, -1, first))
    return same, float(s.done.float().mean()), best


def run_shape(k, n, batch, k1, t1, t2, ell, args):
    s = Shape(k, n, batch, k1, t1, t2, ell, 31 + k + n)
    rows = []
    for steps in STEPS:
        same, performed, _best = check(s, steps)
        g_fused, g_two = s.graph(lambda st: s.fused(steps, stream=st)), s.graph(lambda st: s.two_calls(steps, stream=st))
        tm = alternate({"fused": lambda: s.fused(steps), "fused, graph": g_fused, "two calls": lambda: s.two_calls(steps), "two calls, graph": g_two}, args)
        a = min((tm["fused"], tm["fused, graph"]), key=med)
        b = min((tm["two calls"], tm["two calls, graph"]), key=med)
        row = dict(k=k, n=n, batch=batch, steps=steps, iters=ITERS, k1=k1, t1=t1, t2=t2, ell=ell, path=f"{t1}+{t2}", equal=same,
                   performed_per_member=performed, windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()}, ms={c: med(v) * 1e3 for c, v in tm.items()},
                   spread={c: spread(v) for c, v in tm.items()}, iterations_per_s={c: batch * ITERS / med(v) for c, v in tm.items()},
                   two_calls_over_fused=med(b) / med(a), clear=max(a) < min(b), loses=min(a) > max(b))
        verdict = "clear" if row["clear"] else "LOSES" if row["loses"] else "within the spread"
        for c in tm:
            say(f"{k:>4} {n:>5} {batch:>6} {steps:>5} {row['path']:>4}  {c:<17} {row['ms'][c]:>10.4f} ms {row['spread'][c] * 100:>5.1f}%  "
                f"{row['iterations_per_s'][c]:>14.0f} iterations / s")
        say(f"{k:>4} {n:>5} {batch:>6} {steps:>5}       two calls / fused {row['two_calls_over_fused']:.2f}x, {verdict}; results {'equal' if same else 'DIFFER'}; "
            f"{performed:.2f} steps performed per member")
        rows.append(row)
    return rows


def run_threads(k, n, batch, k1, t1, t2, ell, args):
    """steps = 1: the fused call at the size it chooses and at every forced size"""
    s = Shape(k, n, batch, k1, t1, t2, ell, 31 + k + n)
    s.reset()

    def forced(threads):
        def fn():
            if threads:
                os.environ[THREADS] = str(threads)
            s.fused(1)
            os.environ.pop(THREADS, None)
        return fn

    tm = alternate({("chosen" if not t else f"{t} threads"): forced(t) for t in (0, 64, 128, 256, 512, 1024)}, args)
    row = dict(k=k, n=n, batch=batch, k1=k1, t1=t1, t2=t2, ell=ell, ms={c: med(v) * 1e3 for c, v in tm.items()}, spread={c: spread(v) for c, v in tm.items()},
               windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()})
    for c in tm:
        say(f"{k:>4} {n:>5} {batch:>6} {1:>5} {t1}+{t2:<2}  {c:<17} {row['ms'][c]:>10.4f} ms {row['spread'][c] * 100:>5.1f}%")
    return row


def run_stop(k, n, batch, k1, t1, t2, ell, steps, args):
    s = Shape(k, n, batch, k1, t1, t2, ell, 31 + k + n)
    same, _performed, best = check(s, steps)
    w_stop = int(np.median(best[best >= 0] >> 40))
    s.reset()
    s.fused(steps, w_stop)
    torch.cuda.synchronize()
    run = s.run.float().mean().item()

    def stopped():          # from the same state every time: a member that has stopped would stop at once in a chained call
        for dst, src in zip((s.D, s.piv, s.O), s.state):
            dst.copy_(src)
        s.fused(steps, w_stop)

    def unstopped():
        for dst, src in zip((s.D, s.piv, s.O), s.state):
            dst.copy_(src)
        s.fused(steps)

    def copies():
        for dst, src in zip((s.D, s.piv, s.O), s.state):
            dst.copy_(src)

    tm = alternate({"w_stop = -1": unstopped, f"w_stop = {w_stop}": stopped, "the copies alone": copies}, args)
    row = dict(k=k, n=n, batch=batch, steps=steps, w_stop=w_stop, iterations_run_per_member=run, equal=same, ms={c: med(v) * 1e3 for c, v in tm.items()},
               spread={c: spread(v) for c, v in tm.items()}, windows_ms={c: [x * 1e3 for x in v] for c, v in tm.items()})
    for c in tm:
        say(f"{k:>4} {n:>5} {batch:>6} {steps:>5}  {c:<17} {row['ms'][c]:>10.4f} ms {row['spread'][c] * 100:>5.1f}%")
    say(f"{k:>4} {n:>5} {batch:>6} {steps:>5}  with w_stop = {w_stop} a member runs {run:.2f} of {ITERS} iterations on average")
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
    say(f"isd_collide_search_dev (iters = {ITERS}, w_min = {W_MIN}, w_stop = -1, a received word, the order kept, all outputs) against the same {ITERS} iterations "
        f"as pivot_exchange_batch_dev + row_sums_collide_batch_dev (lightest only), as plain launches and replayed from one captured graph; ms per {ITERS} iterations of "
        f"the batch, median of {args.reps} alternating windows of >= {args.window} s")
    say(f"{'k':>4} {'n':>5} {'batch':>6} {'steps':>5} {'t':>4}  {'variant':<17} {'ms':>13} {'spread':>6}")
    shapes = [r for shape in SHAPES for r in run_shape(*shape, args)]
    lost = [(r["k"], r["n"], r["path"], r["steps"], round(r["two_calls_over_fused"], 3)) for r in shapes if r["loses"]]
    say(f"the fused call loses to the two-call loop beyond the spread at: {lost if lost else 'no measured shape and step count'}")
    say("the stop: the fused call from the same starting state every time (the device copies that restore it are in every variant, and alone)")
    stop = run_stop(*SHAPES[1], 1, args)
    say("the workgroup: the fused call, steps = 1, at the size it chooses and at forced sizes")
    threads = [run_threads(*shape, args) for shape in SHAPES]
    ok = all(r["equal"] for r in shapes) and stop["equal"]
    say(f"all results equal: {'yes' if ok else 'NO'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(shapes=shapes, stop=stop, threads=threads), f, indent=1)
    if args.txt:
        with open(args.txt, "w") as f:
            f.write("\n".join(LINES) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""m4ri_amd_sort_rows_batch_dev on device-resident lists against what it replaces, with the protocol of tools/bench_lists_collide.py
(contenders warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of >= `--window` seconds of back-to-back calls
between two events; medians and (max - min) / median spreads).  Every output is asked for (order, ucount, uniq, mult).

  batch    batches of short lists of random rows: 2^10 .. 2^13 rows by 1024 .. 16 members, n = 128 and 512, cols = NULL, ell = 16 and 32
  long     one long list of random rows: 2^16 .. 2^22 rows, n = 128 and 512, ell = 32
  join     the words of a real join, where the duplicates are: X_b and Y_b drawn from small pools, joined on 4 columns, the listed pairs
           written out by lists_words_batch_dev; those rows sorted on the next 16 columns with xcount = the join's count

Against, in the same run on the same device:
  unique   a loop of torch.unique(dim=0, return_inverse=False, return_counts=True) over the members on the (rows x words) int64 tensor: what
           a caller does today; its output size is dynamic, so every member synchronises with the host
  keysort  ONE torch.sort of the (batch x rows) int64 window keys alone: the floor of a library sort, which settles no equal keys, reads
           no rows, removes no duplicates and gives no multiplicities

  python tools/bench_sort_rows.py [--reps 3] [--window 0.2] [--json profiles/sort_rows_bench.json] [--txt profiles/sort_rows_bench.txt]
                                  [--only batch|long|join]"""
import argparse
import json
import os
import statistics
import sys
import traceback

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd


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


def random_words(rows, w, seed):
    """rows x w random words, dense"""
    t = torch.empty(rows * w, dtype=torch.int64, device="cuda")
    m4ri_amd.fill_dev(t.data_ptr(), w, rows, 64 * w, seed, 0)
    return t


class Sorter:
    """The call on `batch` lists of nx rows of n bits at X (dense), window = the columns 0 .. ell-1 or `cols`, every output asked for."""

    def __init__(self, X, nx, n, batch, ell, cols=None, xcount=None):
        self.X, self.nx, self.n, self.batch, self.ell, self.cols, self.xcount, self.w = X, nx, n, batch, ell, cols, xcount, n // 64
        self.order, self.uniq, self.mult = (torch.zeros(batch * nx, dtype=torch.int64, device="cuda") for _ in range(3))
        self.ucount = torch.zeros(batch, dtype=torch.int64, device="cuda")
        self.need = m4ri_amd.sort_rows_scratch_bytes(nx, n, ell, batch)
        self.scratch = torch.empty(max(self.need, 16), dtype=torch.uint8, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def __call__(self):
        m4ri_amd.sort_rows_batch_dev(self.X.data_ptr(), self.w, self.nx * self.w, self.nx, self.n, self.xcount.data_ptr() if self.xcount is not None else 0,
                                     self.batch, self.cols.data_ptr() if self.cols is not None else 0, 0, self.ell, self.order.data_ptr(), self.ucount.data_ptr(),
                                     self.uniq.data_ptr(), self.mult.data_ptr(), self.nx, self.scratch.data_ptr(), self.need, self.st)


def contenders(s, keys, rows_of):
    """The call and its two baselines on the same lists.  keys: (batch x nx) int64 window keys; rows_of(b): member b's (m_b x words) rows."""
    def unique():
        for b in range(s.batch):
            torch.unique(rows_of(b), dim=0, return_counts=True)
    return {"sort_rows": s, "unique": unique, "keysort": lambda: torch.sort(keys, dim=1)}


def measure(s, keys, rows_of, args, **shape):
    fns = contenders(s, keys, rows_of)
    s()
    torch.cuda.synchronize()
    distinct = s.ucount.sum().item()
    check = sum(int(torch.unique(rows_of(b), dim=0).shape[0]) for b in range(min(s.batch, 2)))
    tm = alternate(fns, args)
    return dict(shape, path=m4ri_amd.plan_sort_rows_batch(s.nx, s.n, s.ell, s.batch), launches=m4ri_amd.sort_rows_units(s.nx, s.n, s.ell, s.batch)[2],
                distinct=int(distinct), agrees=bool(check == int(s.ucount[:2].sum().item())), ms={c: med(v) * 1e3 for c, v in tm.items()},
                spread={c: spread(v) for c, v in tm.items()}, rows_per_s=shape["rows"] / med(tm["sort_rows"]),
                unique_over_sort_rows=med(tm["unique"]) / med(tm["sort_rows"]), sort_rows_over_keysort=med(tm["sort_rows"]) / med(tm["keysort"]))


def run_random(args, shapes):
    out = []
    for nx, batch, n, ell in shapes:
        w = n // 64
        X = random_words(batch * nx, w, 51 + ell)
        V = X.view(batch, nx, w)
        keys = (V[:, :, 0] & ((1 << ell) - 1)).contiguous()
        out.append(measure(Sorter(X, nx, n, batch, ell), keys, lambda b: V[b], args, nx=nx, batch=batch, n=n, ell=ell, rows=batch * nx))
        del X, V, keys
    return out


def run_batch(args):
    return run_random(args, [(nx, batch, n, ell) for n in (128, 512) for nx, batch in ((1 << 10, 1024), (1 << 11, 256), (1 << 12, 64), (1 << 13, 16)) for ell in (16, 32)])


def run_long(args):
    return run_random(args, [(1 << e, 1, n, 32) for n in (128, 512) for e in (16, 18, 20, 22)])


def run_join(args):
    """Lists drawn from pools, joined on the columns 0 .. 3; the words of the listed pairs sorted on the columns 4 .. 19."""
    out = []
    st = torch.cuda.current_stream().cuda_stream
    for rows, pool, batch, cap, n in ((256, 64, 64, 8192, 128), (1024, 128, 4, 1 << 17, 128)):
        w = n // 64
        g = torch.Generator(device="cuda").manual_seed(rows)
        lists = []
        for seed in (61, 62):
            P = random_words(batch * pool, w, seed).view(batch, pool, w)
            pick = torch.randint(0, pool, (batch, rows), device="cuda", generator=g)
            lists.append(torch.gather(P, 1, pick[:, :, None].expand(batch, rows, w)).contiguous())
        X, Y = lists
        K, N = torch.zeros(batch * cap, dtype=torch.int64, device="cuda"), torch.zeros(batch, dtype=torch.int64, device="cuda")
        W = torch.zeros(batch * cap * w, dtype=torch.int64, device="cuda")
        m4ri_amd.lists_collide_batch_dev(X.data_ptr(), w, rows * w, rows, Y.data_ptr(), w, rows * w, rows, n, 0, 0, batch, 0, 0, 4, 0, n, list=K.data_ptr(), l_bs=cap,
                                         cap=cap, count=N.data_ptr(), stream=st)
        m4ri_amd.lists_words_batch_dev(X.data_ptr(), w, rows * w, rows, Y.data_ptr(), w, rows * w, rows, n, 0, 0, batch, K.data_ptr(), cap, cap, N.data_ptr(),
                                       W.data_ptr(), w, cap * w, stream=st)
        torch.cuda.synchronize()
        counts = N.cpu().tolist()
        assert max(counts) <= cap, (max(counts), cap)
        cols = torch.arange(4, 20, dtype=torch.int32, device="cuda")
        V = W.view(batch, cap, w)
        keys = ((V[:, :, 0] >> 4) & 0xFFFF).contiguous()
        s = Sorter(W, cap, n, batch, 16, cols=cols, xcount=N)
        out.append(measure(s, keys, lambda b: V[b, :counts[b]], args, nx=cap, batch=batch, n=n, ell=16, rows=sum(counts), joined_rows=rows, pool=pool))
    return out


def text(res):
    out = [f"sort_rows_batch_dev on {res['device']}; ms per call, medians of {res['reps']} alternating windows of >= {res['window']} s",
           "unique: a loop of torch.unique(dim=0, return_counts=True) over the members; keysort: one torch.sort of the window keys alone", ""]
    head = "       nx  batch     n  ell  path  launches       rows   distinct  agrees  sort_rows ms   unique ms  keysort ms  unique/sort_rows  sort_rows/keysort    Mrows/s  spreads"
    for name, title in (("batch", "batch: short lists of random rows, cols = NULL"), ("long", "long: one list of random rows, cols = NULL"),
                        ("join", "join: the words of a join of pooled lists on 4 columns, sorted on the next 16; nx = cap, rows = the join's counts")):
        if name in res:
            out += [title, head]
            for r in res[name]:
                out.append(f"  {r['nx']:7d}  {r['batch']:5d}  {r['n']:4d}  {r['ell']:3d}  {r['path']:4d}  {r['launches']:8d}  {r['rows']:9d}  {r['distinct']:9d}  {str(r['agrees']):6s}  "
                           f"{r['ms']['sort_rows']:12.4f}  {r['ms']['unique']:10.4f}  {r['ms']['keysort']:10.4f}  {r['unique_over_sort_rows']:16.2f}  "
                           f"{r['sort_rows_over_keysort']:17.2f}  {r['rows_per_s'] / 1e6:9.1f}  " + " ".join(f"{v:.1%}" for v in r["spread"].values()))
            out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--json", default="profiles/sort_rows_bench.json")
    ap.add_argument("--txt", default="profiles/sort_rows_bench.txt")
    ap.add_argument("--only", choices=["batch", "long", "join"])
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, window=args.window)
    for name, fn in (("batch", run_batch), ("long", run_long), ("join", run_join)):
        if args.only in (None, name):
            res[name] = fn(args)
    for path, body in ((args.json, json.dumps(res, indent=1) + "\n"), (args.txt, text(res))):
        with open(path, "w") as f:
            f.write(body)
    print(text(res))


if __name__ == "__main__":
    try:
        main()
    except Exception:
        traceback.print_exc()
        sys.exit(1)

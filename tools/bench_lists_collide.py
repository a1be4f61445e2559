"""m4ri_amd_lists_collide_batch_dev and m4ri_amd_lists_words_batch_dev on device-resident random lists, with the protocol of
tools/bench_row_sums_collide.py (contenders warmed up, then timed ALTERNATELY `--reps` times each, every timing a window of >= `--window`
seconds of back-to-back calls between two events; medians and (max - min) / median spreads).

  stern    Stern at k = 256, k1 = 128, t = 2 + 2, n = 512, ell = 16 and 24, where both calls apply: row_sums_collide_list_batch_dev on
           the generators against the new join on the two MATERIALISED lists (8128 rows each), the join alone and with the two
           row_sums_words_batch_dev calls that write the lists.  hist, lightest and count are checked equal first.
  beyond   past the old bound, random rows: nx = ny = 32 640 (k = 512) at n = 512, ell = 24 and 30, one member and 32; nx = ny = 2^20 at
           n = 128, ell = 32 and 40; and a ladder of nx against ny = 2^20, time against the number of chunks.  Right rows walked per
           second (chunks * ny per member), bytes read per second (every row of X once, every row of Y once per chunk, whole rows) as a
           share of what a device-to-device copy reads per second on the same device.
  flood    ell = 0 on small lists: every pair is weighed; pairs per second.
  words    lists_words_batch_dev: bytes of W written per second against a device-to-device copy of W.

  python tools/bench_lists_collide.py [--reps 3] [--window 0.3] [--json profiles/lists_collide_bench.json] [--txt profiles/lists_collide_bench.txt]
                                      [--only stern|beyond|flood|words]"""
import argparse
import json
import os
import statistics
import sys
import traceback
from math import comb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch

import m4ri_amd

CAP = 64
COPY_WORDS = 1 << 27            # the device-to-device copy: 1 GiB


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


class Outs:
    def __init__(self, batch, n, cap=CAP):
        self.hist = torch.zeros(batch * (n + 1), dtype=torch.int64, device="cuda")
        self.light = torch.zeros(batch, dtype=torch.int64, device="cuda")
        self.list = torch.zeros(batch * cap, dtype=torch.int64, device="cuda")
        self.count = torch.zeros(batch, dtype=torch.int64, device="cuda")
        self.cap = cap


def join(X, Y, nx, ny, n, batch, ell, w_min, w_max, o, st):
    w = n // 64
    m4ri_amd.lists_collide_batch_dev(X.data_ptr(), w, nx * w, nx, Y.data_ptr(), w, ny * w, ny, n, 0, 0, batch, 0, 0, ell, w_min, w_max, o.hist.data_ptr(),
                                     o.light.data_ptr(), o.list.data_ptr(), o.cap, o.cap, o.count.data_ptr(), stream=st)


def copy_rate(args):
    a, b = random_words(COPY_WORDS // 16, 16, 1), torch.empty(COPY_WORDS, dtype=torch.int64, device="cuda")
    t = alternate({"copy": lambda: b.copy_(a)}, args)["copy"]
    return dict(bytes=8 * COPY_WORDS, ms=med(t) * 1e3, spread=spread(t), bytes_per_s=8 * COPY_WORDS / med(t))


def run_stern(args):
    k, k1, t, n = 256, 128, 2, 512
    w, N = n // 64, comb(k1, t)
    batch = 64
    st = torch.cuda.current_stream().cuda_stream
    G = random_words(batch * k, w, 11)
    X, Y = torch.empty(batch * N * w, dtype=torch.int64, device="cuda"), torch.empty(batch * N * w, dtype=torch.int64, device="cuda")
    iota = torch.arange(N, dtype=torch.int64, device="cuda").repeat(batch)
    old, new = Outs(batch, n), Outs(batch, n)

    def words():
        for dst, off in ((X, 0), (Y, k1 * w)):
            m4ri_amd.row_sums_words_batch_dev(G.data_ptr() + 8 * off, w, k * w, k1, n, 0, 0, batch, k1, t, 0, iota.data_ptr(), N, N, 0, dst.data_ptr(), w, N * w,
                                              stream=st)

    rows = []
    for ell in (16, 24):
        m4ri_amd.row_sums_collide_batch_dev(G.data_ptr(), w, k * w, k, n, 0, 0, batch, k1, t, t, 0, 0, ell, 1, old.hist.data_ptr(), old.light.data_ptr(), stream=st)
        torch.cuda.synchronize()
        h, run, w_max = old.hist.view(batch, n + 1).sum(dim=0).cpu().tolist(), 0, n
        for wt in range(1, n + 1):
            run += h[wt]
            if run >= 2 * batch:
                w_max = wt
                break
        fns = {"row_sums": lambda ell=ell, w_max=w_max: m4ri_amd.row_sums_collide_list_batch_dev(
                   G.data_ptr(), w, k * w, k, n, 0, 0, batch, k1, t, t, 0, 0, ell, 1, w_max, old.hist.data_ptr(), old.light.data_ptr(), old.list.data_ptr(), CAP, CAP,
                   old.count.data_ptr(), stream=st),
               "join": lambda ell=ell, w_max=w_max: join(X, Y, N, N, n, batch, ell, 1, w_max, new, st),
               "words+join": lambda ell=ell, w_max=w_max: (words(), join(X, Y, N, N, n, batch, ell, 1, w_max, new, st))}
        words()
        fns["row_sums"](), fns["join"]()
        torch.cuda.synchronize()
        equal = bool(torch.equal(old.hist, new.hist) and torch.equal(old.light, new.light) and torch.equal(old.count, new.count))
        tm = alternate(fns, args)
        rows.append(dict(k=k, k1=k1, t=t, n=n, ell=ell, batch=batch, rows=N, w_max=w_max, equal=equal, collisions_per_member=sum(h) / batch,
                         units=m4ri_amd.lists_collide_units(N, N, n, ell, batch), path=m4ri_amd.plan_lists_collide_batch(N, N, n, ell, batch),
                         ms={c: med(v) * 1e3 for c, v in tm.items()}, spread={c: spread(v) for c, v in tm.items()},
                         join_over_row_sums=med(tm["join"]) / med(tm["row_sums"]), words_join_over_row_sums=med(tm["words+join"]) / med(tm["row_sums"])))
    return rows


def run_beyond(args, copy):
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    shapes = [(32640, 32640, 512, 24, 1), (32640, 32640, 512, 30, 1), (32640, 32640, 512, 24, 32), (32640, 32640, 512, 30, 32),
              (1 << 20, 1 << 20, 128, 32, 1), (1 << 20, 1 << 20, 128, 40, 1)]
    shapes += [(nx, 1 << 20, 128, 32, 1) for nx in (1 << 13, 1 << 15, 1 << 17, 1 << 19)]
    for nx, ny, n, ell, batch in shapes:
        w = n // 64
        X, Y, o = random_words(batch * nx, w, 21 + ell), random_words(batch * ny, w, 22 + ell), Outs(batch, n)
        fn = lambda: join(X, Y, nx, ny, n, batch, ell, 0, n, o, st)
        fn()
        torch.cuda.synchronize()
        found = int(o.hist.sum().item())
        tm = alternate({"join": fn}, args)["join"]
        c, chunks, slices = m4ri_amd.lists_collide_units(nx, ny, n, ell, batch)
        walked, read = batch * chunks * ny, batch * (nx + chunks * ny) * w * 8
        rows.append(dict(nx=nx, ny=ny, n=n, ell=ell, batch=batch, chunks=chunks, slices=slices, workgroups=batch * chunks * slices, collisions=found,
                         expected=batch * nx * ny / 2.0**ell, ms=med(tm) * 1e3, spread=spread(tm), right_rows_per_s=walked / med(tm),
                         bytes_read_per_s=read / med(tm), share_of_copy=read / med(tm) / copy["bytes_per_s"], ms_per_chunk=med(tm) * 1e3 / chunks))
        del X, Y
    return rows


def run_flood(args):
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for nx, n, batch in ((64, 256, 4096), (256, 256, 1024), (1024, 256, 64)):
        w = n // 64
        X, Y, o = random_words(batch * nx, w, 31), random_words(batch * nx, w, 32), Outs(batch, n, 1)
        fn = lambda: m4ri_amd.lists_collide_batch_dev(X.data_ptr(), w, nx * w, nx, Y.data_ptr(), w, nx * w, nx, n, 0, 0, batch, 0, 0, 0, 0, n, o.hist.data_ptr(),
                                                      o.light.data_ptr(), stream=st)
        fn()
        torch.cuda.synchronize()
        assert int(o.hist.sum().item()) == batch * nx * nx
        tm = alternate({"join": fn}, args)["join"]
        rows.append(dict(nx=nx, ny=nx, n=n, batch=batch, path=m4ri_amd.plan_lists_collide_batch(nx, nx, n, 0, batch), ms=med(tm) * 1e3, spread=spread(tm),
                         pairs_per_s=batch * nx * nx / med(tm)))
    return rows


def run_words(args):
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for n, nx, batch, cap in ((128, 4096, 2048, 4096), (1024, 4096, 256, 4096)):
        w = n // 64
        X, Y = random_words(batch * nx, w, 41), random_words(batch * nx, w, 42)
        keys = torch.randint(0, nx * nx, (batch * cap,), dtype=torch.int64, device="cuda")
        W, W2 = torch.zeros(batch * cap * w, dtype=torch.int64, device="cuda"), torch.empty(batch * cap * w, dtype=torch.int64, device="cuda")
        fns = {"words": lambda: m4ri_amd.lists_words_batch_dev(X.data_ptr(), w, nx * w, nx, Y.data_ptr(), w, nx * w, nx, n, 0, 0, batch, keys.data_ptr(), cap, cap, 0,
                                                               W.data_ptr(), w, cap * w, stream=st),
               "copy": lambda: W2.copy_(W)}
        tm = alternate(fns, args)
        nbytes = batch * cap * w * 8
        rows.append(dict(n=n, nx=nx, ny=nx, batch=batch, cap=cap, bytes=nbytes, ms={c: med(v) * 1e3 for c, v in tm.items()}, spread={c: spread(v) for c, v in tm.items()},
                         bytes_written_per_s=nbytes / med(tm["words"]), over_copy=med(tm["words"]) / med(tm["copy"])))
    return rows


def text(res):
    out = [f"lists_collide_batch_dev / lists_words_batch_dev on {res['device']}; ms per call, medians of {res['reps']} alternating windows of >= {res['window']} s",
           f"device-to-device copy of {res['copy']['bytes'] >> 20} MiB: {res['copy']['ms']:.3f} ms, {res['copy']['bytes_per_s'] / 1e12:.3f} TB/s copied (spread {res['copy']['spread']:.1%})", ""]
    if "stern" in res:
        out.append("stern: k = 256, k1 = 128, t = 2 + 2, n = 512, batch 64, 8128 x 8128 rows per member; hist, lightest, list; the band 1 .. w_max")
        out.append("  ell  w_max  equal  collisions/member  row_sums ms   join ms  words+join ms  join/row_sums  words+join/row_sums  spreads")
        for r in res["stern"]:
            out.append(f"  {r['ell']:3d}  {r['w_max']:5d}  {str(r['equal']):5s}  {r['collisions_per_member']:17.1f}  {r['ms']['row_sums']:11.4f}  {r['ms']['join']:8.4f}  "
                       f"{r['ms']['words+join']:13.4f}  {r['join_over_row_sums']:13.3f}  {r['words_join_over_row_sums']:19.3f}  "
                       + " ".join(f"{v:.1%}" for v in r["spread"].values()))
        out.append("")
    if "beyond" in res:
        out.append("beyond: random rows, cols = NULL, hist + lightest + list (all weights, cap 64); bytes read = (nx + chunks * ny) rows, whole rows")
        out.append("       nx       ny     n  ell  batch  chunks  slices  workgroups  collisions        ms  spread  right rows/s  read GB/s  share of copy  ms/chunk")
        for r in res["beyond"]:
            out.append(f"  {r['nx']:7d}  {r['ny']:7d}  {r['n']:4d}  {r['ell']:3d}  {r['batch']:5d}  {r['chunks']:6d}  {r['slices']:6d}  {r['workgroups']:10d}  {r['collisions']:10d}  "
                       f"{r['ms']:8.4f}  {r['spread']:6.1%}  {r['right_rows_per_s']:12.4g}  {r['bytes_read_per_s'] / 1e9:9.1f}  {r['share_of_copy']:13.3f}  {r['ms_per_chunk']:8.4f}")
        out.append("")
    if "flood" in res:
        out.append("flood: ell = 0, every pair weighed, n = 256, hist + lightest")
        out.append("    nx    ny  batch  path        ms  spread      pairs/s")
        for r in res["flood"]:
            out.append(f"  {r['nx']:4d}  {r['ny']:4d}  {r['batch']:5d}  {r['path']:4d}  {r['ms']:8.4f}  {r['spread']:6.1%}  {r['pairs_per_s']:11.4g}")
        out.append("")
    if "words" in res:
        out.append("words: cap random keys per member, count = NULL, no V")
        out.append("     n  batch   cap   MiB of W  words ms   copy ms  written GB/s  words/copy  spreads")
        for r in res["words"]:
            out.append(f"  {r['n']:4d}  {r['batch']:5d}  {r['cap']:4d}  {r['bytes'] / 2**20:9.1f}  {r['ms']['words']:8.4f}  {r['ms']['copy']:8.4f}  {r['bytes_written_per_s'] / 1e9:12.1f}  "
                       f"{r['over_copy']:10.3f}  " + " ".join(f"{v:.1%}" for v in r["spread"].values()))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--json", default="profiles/lists_collide_bench.json")
    ap.add_argument("--txt", default="profiles/lists_collide_bench.txt")
    ap.add_argument("--only", choices=["stern", "beyond", "flood", "words"])
    args = ap.parse_args()
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, window=args.window, copy=copy_rate(args))
    for name, fn in (("stern", run_stern), ("beyond", lambda a: run_beyond(a, res["copy"])), ("flood", run_flood), ("words", run_words)):
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

#!/usr/bin/env python3
"""Return codes of the batched calls on a fixed grid of arguments: the recorder behind tests/golden/batch_arg_codes.json.

    python tools/record_batch_arg_codes.py --lib PATH/libm4ri_amd.so --out tests/golden/batch_arg_codes.json   # record
    python tools/record_batch_arg_codes.py --check tests/golden/batch_arg_codes.json                           # compare, exit 1 on a difference

The fixture is recorded from the library of the commit BEFORE a change to the host side of the batched calls, never
from the code under test; tests/test_batch_argument_grid.py runs --check on the library of the tree.

Every call here is meant to return before its first HIP call, so the operands are addresses that are never touched (2^44 bytes apart,
far more than a span of the grid: every value is at most 2^20, no product of a check reaches 2^63).  The process hides the GPUs from
the HIP runtime before the library is loaded, so a grid point that does get past the checks fails with hipErrorNoDevice instead of
launching on those addresses; it is recorded as 'x' -- past the checks -- and what it computes is the GPU suite's business.

One string per call, a character per grid point: 0 success, 1 hipErrorInvalidValue, N hipErrorNotSupported, x past the checks; the
plan helpers: m for -1, the path's digit.  The helpers that return numbers are recorded as lists.
"""
import argparse
import ctypes
import json
import os
import sys

for _v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
    os.environ[_v] = ""  # before the library loads: no call of this process can reach a GPU

I64, I32, U64, PTR = ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p
SIZES = (-1, 0, 1, 63, 64, 65, 1024, 1025, 1 << 20)
CHAR = {-1: "m", 0: "0", 1: "1", 2: "2", 3: "3", 801: "N", 100: "x"}
FAR = 1 << 44  # bytes between two operands' addresses


def W(n):
    return (n + 63) // 64 if n > 0 else 0


def mem(rows, stride, width):
    return (rows - 1) * stride + width if rows > 0 and width > 0 else 0


# An argument: (kind, name, ...)
#   p  pointer; then the operand's bytes per member, its batch stride's name (None: one entry per member) and the unit in bytes
#   s  size, walked over SIZES; then its base value (65 unless given)
#   t  row stride; then its width as a function of the arguments
#   b  batch stride; then the member's size as a function of the arguments
#   n  the batch
#   v  another scalar; then its values, the first one the base; then its C type
def p(name, member=None, bs=None, unit=8):
    return ("p", name, member or (lambda a: 1), bs, unit)


def s(name, base=65):
    return ("s", name, base)


def t(name, width):
    return ("t", name, width)


def b(name, member):
    return ("b", name, member)


def v(name, values, ctype=I64):
    return ("v", name, values, ctype)


N = ("n", "batch")
ST = v("stream", (None,), PTR)
mn = lambda a, x, y: max(min(a[x], a[y]), 0)

# rows operands: name, rows, stride, width
def rows_op(name, rows, stride, width, bs):
    return p(name, lambda a: mem(rows(a), a[stride], width(a)), bs)


def matrix(name, stride, bs, rows, cols):
    """pointer, stride and batch stride of a rows x cols matrix operand, in the order the calls take them"""
    wf = lambda a: W(a[cols]) if isinstance(cols, str) else cols(a)
    rf = lambda a: a[rows] if isinstance(rows, str) else rows(a)
    return [rows_op(name, rf, stride, wf, bs), t(stride, wf), b(bs, lambda a: mem(rf(a), a[stride], wf(a)))]


def block(name, stride, bs, col):
    """the same of a block of `rows` rows and `cols` columns from column `col` on: the stride covers the row up to the block's end"""
    words = lambda a: W(a[col] + a["cols"]) - (max(a[col], 0) >> 6)
    return [rows_op(name, lambda a: a["rows"], stride, words, bs), t(stride, lambda a: W(a[col] + a["cols"])),
            b(bs, lambda a: mem(a["rows"], a[stride], words(a)))]


R = lambda a: max(a["m"], a["n"])
JOIN_OUT = [p("hist", lambda a: a["n"] + 1), p("lightest")]
CALLS = {
    "m4ri_amd_echelonize_batch_dev": matrix("A", "stride", "a_bs", "nrows", "ncols") + [s("nrows"), s("ncols"), N, v("full", (0, 1), I32), p("rank", unit=4),
                                                                                         p("pivots", lambda a: mn(a, "nrows", "ncols"), unit=4), ST],
    "m4ri_amd_echelonize_order_batch_dev": matrix("D", "d_stride", "d_bs", "nrows", "ncols") + matrix("A", "a_stride", "a_bs", "nrows", "ncols") + [
        s("nrows"), s("ncols"), s("pivot_rows", 33), p("order", lambda a: a["olen"], "o_bs", 4), b("o_bs", lambda a: a["olen"]), s("olen", 40), N,
        v("full", (1, 0), I32), p("rank", unit=4), p("pivots", lambda a: mn(a, "pivot_rows", "ncols"), unit=4), ST],
    "m4ri_amd_random_orders_batch_dev": [p("order", lambda a: a["n"], "o_bs", 4), b("o_bs", lambda a: a["n"]), s("n"), N, v("seed", (7,), U64), ST],
    "m4ri_amd_pivot_exchange_batch_dev": matrix("D", "d_stride", "d_bs", "nrows", "ncols") + [
        s("nrows"), s("ncols"), s("pivot_rows", 33), p("pivots", lambda a: mn(a, "pivot_rows", "ncols"), unit=4), p("rank", unit=4), N,
        p("req", lambda a: 2 * a["steps"], "r_bs", 4), b("r_bs", lambda a: 2 * a["steps"]), s("steps", 3), v("seed", (7,), U64),
        p("order", lambda a: a["olen"], "o_bs", 4), b("o_bs", lambda a: a["olen"]), s("olen", 40), p("done", unit=4), ST],
    "m4ri_amd_solve_left_batch_dev": matrix("A", "a_stride", "a_bs", "m", "n")[:3] + [s("m"), s("n")] + matrix("B", "b_stride", "b_bs", R, "k") + [
        s("k"), N, p("status", unit=4), p("rank", unit=4), ST],
    "m4ri_amd_inv_batch_dev": matrix("Binv", "b_stride", "b_bs", "n", "n") + matrix("A", "a_stride", "a_bs", "n", "n") + [s("n"), N, p("rank", unit=4), ST],
    "m4ri_amd_kernel_left_batch_dev": matrix("A", "a_stride", "a_bs", "m", "n") + [s("m"), s("n")] + matrix("R", "r_stride", "r_bs", "n", "kc") + [
        s("kc", 40), N, p("rank", unit=4), ST],
    "m4ri_amd_ple_batch_dev": matrix("A", "stride", "a_bs", "nrows", "ncols") + [s("nrows"), s("ncols"), N, v("pluq", (0, 1), I32),
                                                                                  p("P", lambda a: a["nrows"], unit=4), p("Q", lambda a: a["ncols"], unit=4),
                                                                                  p("rank", unit=4), ST],
    "m4ri_amd_pluq_solve_left_batch_dev": matrix("A", "a_stride", "a_bs", "m", "n") + [s("m"), s("n"), p("rank", unit=4), p("P", lambda a: a["m"], unit=4),
                                                                                       p("Q", lambda a: a["n"], unit=4)] +
    matrix("B", "b_stride", "b_bs", R, "k") + [s("k"), N, p("status", unit=4), ST],
    "m4ri_amd_mul_small_batch_dev": matrix("C", "c_stride", "c_bs", "m", "n") + matrix("A", "a_stride", "a_bs", "m", "l") +
    matrix("B", "b_stride", "b_bs", "l", "n") + [s("m"), s("l"), s("n"), N, v("add", (0, 1), I32), ST],
    "m4ri_amd_mul_small_batch_op_dev": matrix("C", "c_stride", "c_bs", "m", "n") +
    matrix("A", "a_stride", "a_bs", lambda a: a["l"] if a["trans_a"] else a["m"], lambda a: W(a["m"] if a["trans_a"] else a["l"])) +
    matrix("B", "b_stride", "b_bs", lambda a: a["n"] if a["trans_b"] else a["l"], lambda a: W(a["l"] if a["trans_b"] else a["n"])) +
    [s("m"), s("l"), s("n"), N, v("trans_a", (1, 0), I32), v("trans_b", (0, 1), I32), v("add", (0, 1), I32), ST],
    "m4ri_amd_transpose_batch_dev": matrix("D", "d_stride", "d_bs", "ncols", "nrows") + matrix("A", "a_stride", "a_bs", "nrows", "ncols") + [
        s("nrows"), s("ncols"), N, ST],
    "m4ri_amd_weight_batch_dev": matrix("A", "a_stride", "a_bs", "nrows", "ncols") + matrix("B", "b_stride", "b_bs", "nrows", "ncols") + [
        s("nrows"), s("ncols"), N, p("total"), p("row_weight", lambda a: a["nrows"], unit=4), p("lightest"), ST],
    "m4ri_amd_mismatch_batch_dev": matrix("A", "a_stride", "a_bs", "nrows", "ncols") + matrix("B", "b_stride", "b_bs", "nrows", "ncols") + [
        s("nrows"), s("ncols"), N, p("first_row", unit=4), ST],
    "m4ri_amd_row_span_batch_dev": matrix("A", "a_stride", "a_bs", "nrows", "ncols") + [s("nrows"), s("ncols"), N, p("first", unit=4), p("end", unit=4), ST],
    "m4ri_amd_copy_block_batch_dev": block("D", "d_stride", "d_bs", "d_col") + [s("d_row", 3), s("d_col", 70)] + block("A", "a_stride", "a_bs", "a_col") + [
        s("a_row", 2), s("a_col", 5), s("rows"), s("cols"), N, ST],
    "m4ri_amd_extract_tri_batch_dev": matrix("D", "d_stride", "d_bs", lambda a: mn(a, "nrows", "ncols") if a["upper"] else a["nrows"],
                                             lambda a: W(a["ncols"] if a["upper"] else mn(a, "nrows", "ncols"))) +
    matrix("A", "a_stride", "a_bs", "nrows", "ncols") + [s("nrows"), s("ncols"), N, v("upper", (1, 0), I32), v("diag", (0, 1, 2, 3, -1), I32),
                                                          p("rank", unit=4), ST],
    "m4ri_amd_rowspace_weights_batch_dev": matrix("G", "g_stride", "g_bs", "k", "n") + [s("k", 8), s("n"), p("V", lambda a: W(a["n"]), "v_bs"),
                                                                                         b("v_bs", lambda a: W(a["n"])), N, v("w_min", (0, 3, -1))] + JOIN_OUT + [ST],
    "m4ri_amd_row_sums_weights_batch_dev": matrix("G", "g_stride", "g_bs", "k", "n") + [s("k", 20), s("n"), p("V", lambda a: W(a["n"]), "v_bs"),
                                                                                         b("v_bs", lambda a: W(a["n"])), N, v("t", (2, 0, 1, 5, -1)),
                                                                                         v("w_min", (0, 3, -1))] + JOIN_OUT + [ST],
    "m4ri_amd_sort_rows_batch_dev": matrix("X", "x_stride", "x_bs", "nx", "n") + [
        s("nx", 100), s("n"), p("xcount"), N, p("cols", lambda a: a["ell"], "c_bs", 4), b("c_bs", lambda a: a["ell"]), s("ell", 20),
        p("order", lambda a: a["nx"], "l_bs"), p("ucount"), p("uniq", lambda a: a["nx"], "l_bs"), p("mult", lambda a: a["nx"], "l_bs"),
        b("l_bs", lambda a: a["nx"]), p("scratch", lambda a: a["scratch_bytes"], unit=1), v("scratch_bytes", (1 << 30, 0, -1, 8)), ST],
}
for _side in ("left", "right"):
    CALLS["m4ri_amd_apply_p_%s_batch_dev" % _side] = matrix("A", "stride", "a_bs", "nrows", "ncols") + [
        s("nrows"), s("ncols"), N, p("P", lambda a: a["length"], "p_bs", 4), b("p_bs", lambda a: a["length"]), s("length", 30), v("trans", (0, 1), I32),
        p("status", unit=4), ST]

# the joins: the generator's calls take (G, k1, t1, t2), the lists' calls (X, Y)
_GEN = matrix("G", "g_stride", "g_bs", "k", "n") + [s("k", 20), s("n"), p("V", lambda a: W(a["n"]), "v_bs"), b("v_bs", lambda a: W(a["n"])), N,
                                                     v("k1", (10, 0, 20, 21, -1)), v("t1", (1, 0, 2, 5, -1)), v("t2", (1, 0, 2, 5, -1))]
_LISTS = matrix("X", "x_stride", "x_bs", "nx", "n")[:3] + [s("nx", 100)] + matrix("Y", "y_stride", "y_bs", "ny", "n") + [
    s("ny", 70), s("n"), p("V", lambda a: W(a["n"]), "v_bs"), b("v_bs", lambda a: W(a["n"])), N]
_WINDOW = [p("cols", lambda a: a["ell"], "c_bs", 4), b("c_bs", lambda a: a["ell"]), s("ell", 20), v("w_min", (0, 3, -1))]
_LIST = [p("list", lambda a: a["cap"], "l_bs"), b("l_bs", lambda a: a["cap"]), s("cap", 50), p("count")]
_WORDS = [p("keys", lambda a: a["cap"], "l_bs"), b("l_bs", lambda a: a["cap"]), s("cap", 50), p("count"),
          rows_op("W", lambda a: a["cap"], "w_stride", lambda a: W(a["n"]), "w_bs"), t("w_stride", lambda a: W(a["n"])),
          b("w_bs", lambda a: mem(a["cap"], a["w_stride"], W(a["n"]))), p("skipped", unit=4), ST]
CALLS["m4ri_amd_row_sums_collide_batch_dev"] = _GEN + _WINDOW + JOIN_OUT + [ST]
CALLS["m4ri_amd_row_sums_collide_list_batch_dev"] = _GEN + _WINDOW + [v("w_max", (9, 0, -1))] + JOIN_OUT + _LIST + [ST]
CALLS["m4ri_amd_row_sums_words_batch_dev"] = _GEN + _WORDS
CALLS["m4ri_amd_lists_collide_batch_dev"] = _LISTS + _WINDOW + [v("w_max", (9, 0, -1))] + JOIN_OUT + _LIST + [ST]
CALLS["m4ri_amd_lists_words_batch_dev"] = _LISTS + _WORDS

# the helpers: name, the number of sizes, flags behind them, int64 outputs behind those, the result's C type
HELPERS = {
    "m4ri_amd_plan_echelonize_batch": (2, 0, 0, I32), "m4ri_amd_plan_echelonize_order_batch": (2, 0, 0, I32),
    "m4ri_amd_plan_pivot_exchange_batch": (3, 0, 0, I32), "m4ri_amd_plan_solve_batch": (3, 0, 0, I32), "m4ri_amd_plan_kernel_batch": (2, 0, 0, I32),
    "m4ri_amd_plan_ple_batch": (2, 0, 0, I32), "m4ri_amd_plan_pluq_solve_batch": (3, 0, 0, I32), "m4ri_amd_plan_mul_small_batch": (3, 0, 0, I32),
    "m4ri_amd_plan_mul_small_batch_op": (3, 2, 0, I32), "m4ri_amd_plan_transpose_batch": (2, 0, 0, I32), "m4ri_amd_plan_reduce_batch": (2, 0, 0, I32),
    "m4ri_amd_plan_perm_batch": (2, 1, 0, I32), "m4ri_amd_plan_rowspace_weights_batch": (2, 0, 0, I32),
    "m4ri_amd_plan_row_sums_weights_batch": (3, 0, 0, I32), "m4ri_amd_plan_row_sums_collide_batch": (6, 0, 0, I32),
    "m4ri_amd_row_sums_collide_slices": (7, 0, 0, I64), "m4ri_amd_plan_lists_collide_batch": (5, 0, 0, I32),
    "m4ri_amd_lists_collide_units": (5, 0, 3, I32), "m4ri_amd_plan_sort_rows_batch": (4, 0, 0, I32), "m4ri_amd_sort_rows_units": (4, 0, 3, I32),
    "m4ri_amd_sort_rows_scratch_bytes": (4, 0, 0, I64),
}


def points(spec):
    """the grid of a call: a list of {argument: override}; what is not overridden takes its base value"""
    sizes = [x[1] for x in spec if x[0] == "s"]
    out = []
    for bt in (0, 1, 2):
        for name in sizes:
            out += [{"batch": bt, name: val} for val in SIZES]
        plain = [x[1] for x in spec if x[0] == "s" and x[2] == 65]
        out += [dict({"batch": bt}, **{name: val for name in plain}) for val in SIZES]
        if len(sizes) >= 2:
            out += [{"batch": bt, sizes[0]: x, sizes[1]: y} for x in SIZES for y in SIZES]
    ptrs = [x[1] for x in spec if x[0] == "p"]
    for bt in (1, 2):
        for x in spec:
            if x[0] == "t":
                out += [{"batch": bt, x[1]: ("w", d)} for d in (None, 0, -1, 0.5, 1)]  # -1, 0, width - 1, width, width + 1
            if x[0] == "b":
                out += [{"batch": bt, x[1]: ("w", d)} for d in (None, 0, -1, 0.5)]  # -1, 0, the member's size - 1, the member's size
            if x[0] == "v":
                out += [{"batch": bt, x[1]: val} for val in x[2]]
        for name in ptrs:
            out.append({"batch": bt, name: None})
            for other in ptrs:
                if other != name:
                    out += [{"batch": bt, name: ("first", other)}, {"batch": bt, name: ("last", other)}]
    return out


def arguments(spec, over):
    a = {"batch": over.get("batch", 1)}
    for x in spec:  # sizes and scalars first: widths and members are functions of them
        if x[0] in ("s", "v"):
            a[x[1]] = over.get(x[1], x[2] if x[0] == "s" else x[2][0])
    for kind in ("t", "b"):  # then the row strides, then the batch strides
        for x in spec:
            if x[0] == kind:
                full, o = x[2](a), over.get(x[1])
                a[x[1]] = full if o is None else -1 if o[1] is None else 0 if o[1] == 0 else full - 1 if o[1] == -1 else full if o[1] == 0.5 else full + 1
    ptrs = [x for x in spec if x[0] == "p"]
    base = {x[1]: FAR * (i + 1) for i, x in enumerate(ptrs)}

    def extent(x):
        bs = a[x[3]] if x[3] else x[2](a)
        per = x[2](a)
        return ((a["batch"] - 1) * bs + per) * x[4] if a["batch"] > 0 and per > 0 else 0

    for x in ptrs:
        o = over.get(x[1], "own")
        if o == "own":
            a[x[1]] = base[x[1]]
        elif o is None:
            a[x[1]] = None
        else:
            y = next(q for q in ptrs if q[1] == o[1])
            a[x[1]] = base[o[1]] + (max(extent(y) - 1, 0) if o[0] == "last" else 0)
    return a


def ctype_of(x):
    return {"p": PTR, "s": I64, "t": I64, "b": I64, "n": I64}.get(x[0]) or x[3]


def walk(lib):
    codes = {}
    for name in sorted(CALLS):
        spec = CALLS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = I32, [ctype_of(x) for x in spec]
        out = []
        for over in points(spec):
            a = arguments(spec, over)
            out.append(CHAR.get(fn(*[a[x[1]] for x in spec]), "?"))
        codes[name] = "".join(out)
    for name in sorted(HELPERS):
        nsizes, nflags, nouts, restype = HELPERS[name]
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, [I64] * nsizes + [I32] * nflags + [ctypes.POINTER(I64)] * nouts
        grid = [[val] * nsizes for val in SIZES] + [[20] * i + [val] + [20] * (nsizes - i - 1) for i in range(nsizes) for val in SIZES]
        if nsizes >= 2:
            grid += [[x, y] + [20] * (nsizes - 2) for x in SIZES for y in SIZES]
        out = []
        for sizes in grid:
            for flags in range(1 << nflags):
                outs = [I64(-7) for _ in range(nouts)]
                r = fn(*sizes, *[(flags >> i) & 1 for i in range(nflags)], *[ctypes.byref(o) for o in outs])
                out.append([r] + [o.value for o in outs] if nouts or restype is I64 else CHAR.get(r, "?"))
        codes[name] = out if nouts or restype is I64 else "".join(out)
    return codes


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "m4ri_amd", "libm4ri_amd.so"))
    ap.add_argument("--out")
    ap.add_argument("--check")
    args = ap.parse_args()
    codes = walk(ctypes.CDLL(args.lib))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(codes, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    if args.check:
        want = json.load(open(args.check))
        bad = 0
        for name in sorted(set(want) | set(codes)):
            w, g = want.get(name), codes.get(name)
            if w != g:
                bad += 1
                at = next((i for i in range(min(len(w or ""), len(g or ""))) if w[i] != g[i]), -1)
                print("DIFFERS %s: first at grid point %d: recorded %r, now %r" % (name, at, w[at] if w and at >= 0 else None, g[at] if g and at >= 0 else None))
        print("%d calls, %d differ" % (len(codes), bad))
        sys.exit(1 if bad else 0)
    if not args.out:
        for name, c in codes.items():
            print(name, len(c), c if isinstance(c, str) else "...")


if __name__ == "__main__":
    main()

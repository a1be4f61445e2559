"""What m4ri_amd_pivot_exchange_batch_dev (include/m4ri_amd.h) has to give, in NumPy and plain Python on the unpacked bits of one
member, written literally from the header.  tests/test_pivot_exchange_plan.py pins it to tests/order_cases.py's ech_order from scratch
on the new pivots; tests/test_gpu_pivot_exchange_batch.py judges the kernels with it."""
import numpy as np

from order_cases import from_words, splitmix, to_words


def draw(seed, b, steps, s, R, ncols):
    """(r, start) of step s of member b without requests: output number b * steps + s of the stream, R >= 1."""
    h = splitmix(seed, b * steps + s)
    return (h >> 32) % R, (h & 0xFFFFFFFF) % ncols


def scan(row, own, start):
    """The first column in the cyclic order start, start + 1, ..., ncols - 1, 0, ..., start - 1 with the bit set, `own` not counted;
    None if there is none."""
    ncols = len(row)
    for j in range(ncols):
        c = (start + j) % ncols
        if row[c] and c != own:
            return c
    return None


def exchange(bits, pivots, rank, pivot_rows, steps, req=None, seed=0, b=0, order=None):
    """The rule, steps 0 .. steps-1 in this order.  bits: uint8 nrows x ncols; pivots: min(pivot_rows, ncols) entries; req: steps pairs
    (r, c), or None: drawn from the stream seeded `seed` for member b; order: the entries kept, or None.
    Returns (bits, pivots, order, done, the requests met: one (r, c) or None per step); the arguments are not written."""
    bits = np.array(bits, dtype=np.uint8) & 1
    nrows, ncols = bits.shape
    pivots = np.array(pivots, dtype=np.int32)
    order = None if order is None else np.array(order, dtype=np.int32)
    pm = min(pivot_rows, ncols)
    assert len(pivots) == pm
    R = min(max(int(rank), 0), pm)
    M = to_words(bits)   # the rows as packed words: a row addition is one XOR
    done, met = 0, []

    def bit(i, c):
        return int((int(M[i, c >> 6]) >> (c & 63)) & 1)

    for s in range(steps):
        if req is not None:
            r, c = int(req[s][0]), int(req[s][1])
        else:
            if R == 0:
                met.append(None)
                continue
            r, start = draw(seed, b, steps, s, R, ncols)
            c = scan(from_words(M[r:r + 1], ncols)[0], int(pivots[r]), start)
            if c is None:
                met.append(None)
                continue
        met.append((r, c))
        if not (0 <= r < R and 0 <= c < ncols and bit(r, c) and c != int(pivots[r])):
            continue
        col = (M[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1)
        col[r] = 0                                   # every row i != r with the bit, followers included
        M[np.flatnonzero(col)] ^= M[r]
        old = int(pivots[r])
        pivots[r] = c
        if order is not None:
            p, q = np.flatnonzero(order == old), np.flatnonzero(order == c)
            if p.size and q.size:
                order[p[0]], order[q[0]] = c, old
        done += 1
    return from_words(M, ncols), pivots, order, done, met

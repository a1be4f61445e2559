"""What m4ri_amd_lists_collide_batch_dev and m4ri_amd_lists_words_batch_dev (include/m4ri_amd.h) have to give, in NumPy on the
unpacked bits of one member: X (nx x n, uint8), Y (ny x n), V (n, or None) and a window `cols`.  The word of pair (i, j) is
V ^ X[i] ^ Y[j], its rank i * ny + j; it COLLIDES iff it is 0 at every window column.  The rule is written TWICE -- brute() takes every
pair, join() sorts the left keys and looks the right ones up -- and tests/test_lists_collide_plan.py holds the two to each other;
tests/test_gpu_lists_collide.py judges the kernels with them (brute force where the lists are small, the join where they are not).
pack() lays bit rows out as the 64-bit words the library reads, with dirt wherever the library must not look."""
import numpy as np

RANK_MASK = (1 << 40) - 1
REFUSED_HIST, REFUSED_LIGHTEST, REFUSED_COUNT = -1, -2, -1


def refused(n, cols):
    return any(c < 0 or c >= n for c in cols)


def _v(V, n):
    return np.zeros(n, dtype=np.uint8) if V is None else np.asarray(V, dtype=np.uint8)


def window_keys(A, cols):
    """The window bits of every row of A as one uint64: bit j = column cols[j] (repeated and unsorted entries as they come)."""
    key = np.zeros(A.shape[0], dtype=np.uint64)
    for j, c in enumerate(cols):
        key |= A[:, c].astype(np.uint64) << np.uint64(j)
    return key


def brute(X, Y, V, cols):
    """(weights, ranks) of the colliding pairs, every pair taken: small lists only."""
    nx, n = X.shape
    ny = Y.shape[0]
    c = X[:, None, :] ^ Y[None, :, :] ^ _v(V, n)[None, None, :]
    hit = ~c[:, :, list(cols)].any(axis=2) if len(cols) else np.ones((nx, ny), dtype=bool)
    i, j = np.nonzero(hit)
    return c[i, j].sum(axis=1).astype(np.int64), i.astype(np.int64) * ny + j


def join(X, Y, V, cols):
    """The same by a sorted join: the left keys sorted, every right key (with V's) looked up, the matches weighed."""
    nx, n = X.shape
    ny = Y.shape[0]
    v = _v(V, n)
    kx, ky = window_keys(X, cols), window_keys(Y, cols) ^ window_keys(v[None, :], cols)[0]
    order = np.argsort(kx, kind="stable")
    sx = kx[order]
    lo, hi = np.searchsorted(sx, ky, "left"), np.searchsorted(sx, ky, "right")
    cnt = hi - lo
    j = np.repeat(np.arange(ny, dtype=np.int64), cnt)
    pos = np.arange(cnt.sum(), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    i = order[pos].astype(np.int64)
    w = np.zeros(len(i), dtype=np.int64)
    for s in range(0, len(i), 1 << 16):       # the matches a block at a time
        w[s:s + (1 << 16)] = (X[i[s:s + (1 << 16)]] ^ Y[j[s:s + (1 << 16)]] ^ v[None, :]).sum(axis=1)
    return w, i * ny + j


def keys_of(w, r, w_min, w_max):
    take = (w >= w_min) & (w <= w_max)
    return np.sort((w[take] << 40) | r[take])


def expect(X, Y, V, cols, w_min, w_max, rule=join):
    """(hist, lightest, sorted keys of the band, count) of one member; the refused forms for a window entry outside 0 .. n-1."""
    n = X.shape[1]
    if refused(n, cols):
        return np.full(n + 1, REFUSED_HIST, dtype=np.int64), REFUSED_LIGHTEST, np.zeros(0, dtype=np.int64), REFUSED_COUNT
    w, r = rule(X, Y, V, cols)
    hist = np.bincount(w, minlength=n + 1).astype(np.int64)
    cand = ((w << 40) | r)[w >= w_min]
    keys = keys_of(w, r, w_min, min(w_max, n))
    return hist, int(cand.min()) if len(cand) else -1, keys, len(keys)


def words_of(X, Y, V, ranks):
    """The words (len(ranks) x n) of these pair ranks."""
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    ny = Y.shape[0]
    assert ((ranks >= 0) & (ranks < X.shape[0] * ny)).all()
    return X[ranks // ny] ^ Y[ranks % ny] ^ _v(V, X.shape[1])[None, :]


def width(n):
    return (n + 63) // 64


def pack(bits, stride=None, rng=None):
    """Bit rows (rows x n, uint8) as int64 words, `stride` words per row.  rng: the bits behind column n and the padding words are
    random dirt (the library must ignore them); None: they are 0."""
    bits = np.asarray(bits, dtype=np.uint8)
    rows, n = bits.shape
    w = width(n)
    stride = w if stride is None else stride
    assert stride >= w
    full = np.zeros((rows, 64 * stride), dtype=np.uint8)
    if rng is not None:
        full[:] = rng.integers(0, 2, size=full.shape, dtype=np.uint8)
    full[:, :n] = bits
    return np.packbits(full, axis=1, bitorder="little").view(np.uint64).reshape(rows, stride).view(np.int64)


def unpack(words, n):
    """The n valid bits of packed rows (rows x >= width(n) words)."""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return b[:, :n]

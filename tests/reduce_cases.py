"""What m4ri_amd_weight_batch_dev, m4ri_amd_mismatch_batch_dev and m4ri_amd_row_span_batch_dev (include/m4ri_amd.h) have to give,
in NumPy on the unpacked bits of one member (uint8, nrows x ncols).  tests/test_reduce_batch_plan.py pins these to the reference's
mzd_equal, mzd_is_zero and mzd_first_zero_row; tests/test_gpu_reduce_batch.py judges the kernels with them."""
import numpy as np


def row_weights(bits):
    return bits.sum(axis=1, dtype=np.int64).astype(np.int32)


def total(bits):
    return int(bits.sum(dtype=np.int64))


def lightest(bits):
    """(the smallest row weight << 32) | the first row that has it; -1 without rows."""
    if bits.shape[0] == 0:
        return -1
    w = row_weights(bits)
    i = int(np.argmin(w))  # the first of equals
    return (int(w[i]) << 32) | i


def _nonzero_rows(bits):
    return np.flatnonzero(bits.any(axis=1)) if bits.shape[1] else np.zeros(0, dtype=np.int64)


def first_mismatch(a, b):
    """The first row at which a and b differ, -1 if none."""
    rows = _nonzero_rows(a != b)
    return int(rows[0]) if rows.size else -1


def first_nonzero(bits):
    rows = _nonzero_rows(bits)
    return int(rows[0]) if rows.size else bits.shape[0]


def end_nonzero(bits):
    """One past the last non-zero row: mzd_first_zero_row."""
    rows = _nonzero_rows(bits)
    return int(rows[-1]) + 1 if rows.size else 0


def single(nrows, ncols, r, c):
    b = np.zeros((nrows, ncols), dtype=np.uint8)
    b[r, c] = 1
    return b


def corners(nrows, ncols):
    """The positions of the single-bit members: the corners, and columns 63 and 64 (a word's last bit, the next word's first) in a
    middle row."""
    r = nrows // 2
    pos = [(0, 0), (0, ncols - 1), (nrows - 1, 0), (nrows - 1, ncols - 1)] + [(r, c) for c in (63, 64) if c < ncols]
    return sorted(set(pos))

"""CPU checks of the helpers of tests/test_gpu_dev_api.py (tests/dev_frame.py): the plain NumPy column gather that serves as the
reference of the wide m4ri_amd_apply_p_right_dev cases, against the oracle's apply_p_right at widths where both run, and the
frame's geometry."""
import numpy as np
import pytest

import dev_frame as df
from m4ri_amd.mzd import Mzd


@pytest.mark.parametrize("m,n", [(1, 1), (3, 64), (4, 65), (7, 200), (5, 1000), (2, 4097)])
@pytest.mark.parametrize("trans", [False, True])
def test_numpy_gather_is_the_oracles_apply_p_right(oracle, m, n, trans):
    rng = np.random.default_rng(31 * m + n)
    A = Mzd.random(m, n, 17 + n)
    for P in (np.array([rng.integers(0, n) if rng.random() < 0.6 else i for i in range(n)], dtype=np.int32),   # any target, chains
              np.array([rng.integers(i, n) for i in range(n)], dtype=np.int32),                                   # LAPACK style
              np.arange(n, dtype=np.int32)):
        want = A.copy()
        oracle.apply_p_right(want, P, trans)
        got = df.pack_bits(df.apply_p_right_bits(A.to_bits(), P, trans))
        assert np.array_equal(got.valid_words(), want.valid_words())
        short = P[: max(1, n // 2)]   # length < ncols
        if np.all(short < n):
            want = A.copy()
            oracle.apply_p_right(want, short, trans)
            assert np.array_equal(df.pack_bits(df.apply_p_right_bits(A.to_bits(), short, trans)).valid_words(), want.valid_words())


@pytest.mark.parametrize("width", [1, 2, 3, 4, 65, 130])
def test_frame_geometry(width):
    s, b = df.geometry(width, "even")
    assert s % 2 == 0 and s - width in (0, 1) and b % 2 == 0
    s, b = df.geometry(width, "odd")
    assert s % 2 == 1 and s > width and b % 2 == 1
    s, b = df.geometry(width, "wide")
    assert s == width + 3 and b % 2 == 0
    for layout in df.LAYOUTS:
        s, b = df.geometry(width, layout)
        assert b >= df.GUARD * s


@pytest.mark.parametrize("layout", df.LAYOUTS)
@pytest.mark.parametrize("dirty", [False, True])
def test_frame_places_the_operand(layout, dirty):
    M = Mzd.random(5, 130, 3)
    f = df.Frame(M, layout, 9, dirty_tail=dirty)
    v = f.view(f.before)
    assert np.array_equal(v[:, :-1], M.valid_words()[:, :-1]) and np.array_equal(v[:, -1] & f.mask, M.valid_words()[:, -1])
    tail = v[:, -1] & ~f.mask
    assert np.all(tail != 0) if dirty else np.all(tail == 0)
    assert f.outside.sum() == f.before.size - 5 * 3 and not f.outside[f.base] and f.outside[f.base - 1] and f.outside[f.base + 3]


@pytest.mark.parametrize("mb,nb", [(1, 2), (5, 64), (70, 65), (33, 200), (130, 513)])
@pytest.mark.parametrize("upper", [False, True])
def test_right_solve_by_transposition_is_the_oracles_right_solve(oracle, mb, nb, upper):
    T = df.unit_diag(Mzd.random(nb, nb, 3 + nb))   # the other triangle is junk on both routes
    B = Mzd.random(mb, nb, 4 + mb)
    want = (oracle.trsm_upper_right if upper else oracle.trsm_lower_right)(T, B.copy())
    got = df.trsm_right_by_transposition(oracle, T, B, upper)
    assert np.array_equal(got.valid_words(), want.valid_words())

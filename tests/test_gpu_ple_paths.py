"""Every path of the PLE's pivot searches and every variant of its trailing update (m4ri_amd/csrc/ple.hip) on the GPU, against
the oracle, bit for bit on matrix, P, Q and rank.  The inputs are the shelf cases of tests/ple_paths.py;
tests/test_ple_paths_cpu.py shows from the oracle's results that between them they reach the one-wave search's high slot, both
outcomes of a deferral, the general search's catch-up pass and its scans beyond the window (s_head, global memory, later chunks),
and blocks of both kinds next to each other.  The file runs again in child processes with the switches that are read once per
process: the general search for every block, the other tile widths and row counts of the rank update, the panel step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import m4ri_amd
from m4ri_amd.mzd import Mzd
from ple_paths import CASES, WIDE_CASES, classify, expected
from test_gpu_ple import _same

pytestmark = pytest.mark.gpu

FLAVOURS = (("mzd_ple", "ple"), ("_mzd_ple_russian", "flat"), ("mzd_pluq", "pluq"))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)


def _check(oracle, case):
    A, want = expected(oracle, case)
    for which, flavour in FLAVOURS:
        (rank, P, Q), Ao = want[flavour]
        Ag = A.copy()
        try:
            _same(m4ri_amd.mzd_ple(Ag, 0, which), (rank, P, Q), Ag, Ao)
        except AssertionError as e:
            raise AssertionError(f"{case.name} {which}: {e.args}; paths of the case: {sorted(classify(P, Q, rank, case.m, case.n))}") from None


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_path_matches_oracle(oracle, case):
    _check(oracle, case)


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: c.name)
def test_wide_rank_updates_match_oracle(oracle, case):
    """Both searches in the first block, then the rank update over 68 and 18 words: whole and partial column tiles of every tile
    width, an odd word count."""
    _check(oracle, case)


@pytest.mark.parametrize("stride,r0", [(11, 6), (12, 5)])
def test_paths_on_an_unaligned_window_keep_the_parent(oracle, stride, r0):
    """The alternating case in place on a window of a pinned parent that starts at an odd word offset, the parent's row stride odd
    (11) or even (12): the rank update's scalar path, its tile origin not rounded down, real neighbouring words on both sides.
    The parent must come back unchanged outside the window."""
    case = next(c for c in CASES if c.name == "alternating")
    A, want = expected(oracle, case)
    c0 = 3 * 64
    assert (r0 * stride + c0 // 64) % 2 == 1 and case.n % 64 == 0
    rows, cols = r0 + case.m + 5, 64 * 11
    for which, flavour in (("_mzd_ple_russian", "flat"), ("mzd_pluq", "pluq")):
        (rank, P, Q), Ao = want[flavour]
        P0 = Mzd(rows, cols, rowstride=stride)
        P0.fill_splitmix(91)
        if stride > P0.width:
            P0.rows()[:, P0.width:] = Mzd.random(rows, 64 * (stride - P0.width), 92).valid_words()  # the padding words too
        Pg = Mzd(rows, cols, buf=P0.buf.copy(), rowstride=stride)
        wg = Pg.window(r0, c0, r0 + case.m, c0 + case.n)
        wg.valid_words()[:, :] = A.valid_words()
        before = Pg.buf.copy()
        m4ri_amd.pin(Pg)
        try:
            got = m4ri_amd.mzd_ple(wg, 0, which)
        finally:
            m4ri_amd.unpin(Pg)
        _same(got, (rank, P, Q), wg, Ao)
        outside = np.ones((rows, stride), dtype=bool)
        outside[r0:r0 + case.m, c0 // 64:c0 // 64 + wg.width] = False
        assert np.array_equal(Pg.rows()[outside], Mzd(rows, cols, buf=before, rowstride=stride).rows()[outside]), which + ": the parent changed outside the window"


SWITCHES = [
    {"M4RI_AMD_PLE_WAVE": "0"},
    {"M4RI_AMD_RU_TW": "16", "M4RI_AMD_RU_ROWS": "96"},
    {"M4RI_AMD_RU_TW": "64", "M4RI_AMD_RU_ROWS": "160"},
    {"M4RI_AMD_PLE_WAVE": "0", "M4RI_AMD_PLE_PANELS": "1", "M4RI_AMD_PLE_PANEL": "1"},
    {"M4RI_AMD_PLE_PANELS": "1", "M4RI_AMD_PLE_PANEL": "2"},
]


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: ",".join(k[9:] + "=" + v for k, v in s.items()))
def test_paths_under_switched_variants(switches):
    """The rest of this file in a child process with the general search for every block, the 16- and 64-word instantiations of the
    rank update with row counts per workgroup that divide no case, and the panel step with either search (the switches are read
    once per process)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_ple_paths.py"), "-x", "-q", "-m", "gpu", "-k", "not switched",
                        "-p", "no:cacheprovider"], cwd=os.path.dirname(here), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert " passed" in r.stdout

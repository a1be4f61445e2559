"""Every branch of the engine's leaf launch (engine.hip launch_leaf_one), run through the entry points callers use -- m4rm_dev,
m4rm_batch_dev, mul_batch_dev at level 0 -- and compared word for word with the NumPy GF(2) product of tests/leaf_reference.py.

A case names its branch; tests/leaf_launch_cases.py run() first asks m4ri_amd_plan_leaf_launch, for the compute-unit count of the device
the test runs on, whether that branch is what the engine will do (tile counts are derived from the count: cus, cus + 1, cus + 44 tiles),
and fails when it is not -- a device or a cost model under which a case would test another branch says so.  Then, with add off and on
and C starting from random words: the entry on operands with pattern-filled words between rows, between members and around the
buffers; every word of C against NumPy; every other word untouched; leaf_gen, one launch, `batch` products in the stats.

Each case runs with one contiguous C (zero_c clears it with one memset) and with rows and members of C apart (one clearing pass per
member).  The NumPy side of the largest cases is 2 to 3 x 10^10 bit operations, computed once per shape and shared by the layouts and
by add off and on; measured on 8 CPU cores: 300 products of 192 x 1024 x 512 1.3 s, 256 of 192 x 704 x 512 1.0 s, 200 x 1024 x 153523
0.7 s, 356 of 256 x 512 x 512 0.5 s, everything else below 0.4 s.  The whole file takes about 10 s on an MI355X."""
import os
import subprocess
import sys

import pytest
import torch

import m4ri_amd
import leaf_launch_cases as cases

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "strided"])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible: the gpu tests have nothing to run on"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    for k in ("M4RI_AMD_LEAF_GEN", "M4RI_AMD_SMALL_LEAF", "M4RI_AMD_SMALL_LEAF_WORK", "M4RI_AMD_SMALL_KS", "M4RI_AMD_TAIL_KSPLIT"):
        assert not os.environ.get(k), f"{k} is set: the cases of this file are about the engine's own plan"


# ---- the table of tests/test_leaf_plan_cpu.py, at its shapes ----------------------------------------------------------------------------
@LAYOUTS
def test_full_round_of_packed_a_tiles_unsplit(strided):
    """cus products of 192 x 704 x 512, one tile each: generation 4, one launch, plain stores."""
    cases.run("mul_batch_dev", "gen4 unsplit", 192, 704, 512, batch=cases.cus(), strided=strided, seed=1, more=dict(tiles=cases.cus()))


@LAYOUTS
@pytest.mark.parametrize("extra", [44, 1])
def test_full_round_then_split_tail_of_a_batch(strided, extra):
    """cus + 44 (cus + 1) products of 192 x 1024 x 512: one round unsplit, the 44 tiles (the one tile) left over in a second launch with
    their inner dimension split into slabs, one reduce pass over the tail's tiles alone."""
    cases.run("mul_batch_dev", "gen4 hybrid slabs", 192, 1024, 512, batch=cases.cus() + extra, strided=strided, seed=2,
              more=dict(tail_tiles=extra, tiles=cases.cus() + extra))


@LAYOUTS
def test_full_round_then_split_tail_of_one_ragged_product(strided):
    """One product of cus + 44 column tiles, the last one 435 columns wide and its last word ragged: the tail is the last 44 column tiles."""
    n = (cases.cus() + 44) * 512 - 77
    cases.run("m4rm_dev", "gen4 hybrid slabs", 200, 1024, n, strided=strided, seed=3, more=dict(tail_tiles=44, tiles_n=cases.cus() + 44))


@LAYOUTS
def test_whole_launch_split_in_slabs_few_tiles_per_cu(strided):
    """100 tiles on 256 CUs (the same share of any other count): every tile split, slabs, one reduce pass over all tiles."""
    cases.run("mul_batch_dev", "gen4 split slabs", 192, 2048, 512, batch=max(2, cases.cus() * 100 // 256), strided=strided, seed=4)


@LAYOUTS
def test_whole_launch_split_many_ways_in_slabs(strided):
    """9 products of 300 x 8192 x 1000, 18 tiles with a ragged second column tile: split 13 ways on 256 CUs."""
    cases.run("mul_batch_dev", "gen4 split slabs", 300, 8192, 1000, batch=9, strided=strided, seed=5, more=dict(ksplit=lambda k: k >= 4, tiles=18))


@LAYOUTS
def test_requested_split_beyond_the_slab_region_meets_by_atomics(strided):
    """192 x 512 x 51200 with ksplit = 8: 100 tiles x 8 splits are more slabs than the 768 there are, so all of C is cleared and the splits
    meet by atomic XOR."""
    cases.run("m4rm_dev", "gen4 split atomics", 192, 512, 51200, ksplit=8, strided=strided, seed=6, more=dict(ksplit=8, tiles=100))


@LAYOUTS
def test_requested_split_of_the_plain_a_kernel(strided):
    """100 x 2048 x 3000 with ksplit = 4: generation 1 in 512-row tiles, atomics into a cleared C."""
    cases.run("m4rm_dev", "gen1 split atomics", 100, 2048, 3000, ksplit=4, strided=strided, seed=7, more=dict(rg=16, tile_rows=512, ksplit=4))


@LAYOUTS
def test_small_leaf_with_an_inner_split(strided):
    """Few tiles and a long inner dimension: the one-launch small leaf splits it, atomics into a cleared C -- one product, and a batch
    (whose C, when not contiguous, is cleared member by member)."""
    cases.run("m4rm_dev", "small leaf split", 256, 8192, 512, strided=strided, seed=8)
    cases.run("mul_batch_dev", "small leaf split", 300, 4096, 600, batch=3, strided=strided, seed=9)


@LAYOUTS
def test_work_bound_of_the_small_leaf(strided):
    """1024 x 1024 x 16384 is 2^34 bit operations, the most the small leaf takes (here unsplit: 128 of its tiles); one column more and
    the product is generation 4's, 33 tiles with a one-column last tile, split into slabs."""
    cases.run("m4rm_dev", "small leaf unsplit", 1024, 1024, 16384, strided=strided, seed=14, more=dict(tiles=128))
    cases.run("m4rm_dev", "gen4 split slabs", 1024, 1024, 16385, strided=strided, seed=15, more=dict(tiles=33))


# ---- m4rm_batch_dev: the one entry that does not reserve the packed-A scratch ------------------------------------------------------------
def _reserve_for(m, l, batch):
    """An m4rm_dev call that leaves a packed-A scratch large enough for `batch` members of m x l behind: 4096 rows of A, as long as needed."""
    need = cases.a4_words(m, l, batch)
    l1 = 64 * -(-need // 4096)
    assert cases.reserved_words(4096, l1) >= need
    t = torch.zeros(4096 * (l1 // 64) + l1 + 4096, dtype=torch.int64, device="cuda")

    def call():
        m4ri_amd.m4rm_dev(t.data_ptr() + 8 * (4096 * (l1 // 64) + l1), 1, t.data_ptr(), l1 // 64, t.data_ptr() + 8 * 4096 * (l1 // 64), 1, 4096, l1, 64)
        torch.cuda.synchronize()
    return call


@LAYOUTS
@pytest.mark.parametrize("m,l,n,extra,on_gen4,on_gen1", [(192, 1024, 512, 44, "gen4 hybrid slabs", "gen1 fallback"),
                                                           (300, 8192, 1000, None, "gen4 split slabs", "gen1 fallback split")])
def test_batch_entry_takes_the_scratch_the_previous_call_left(strided, m, l, n, extra, on_gen4, on_gen1):
    """m4rm_batch_dev straight after the workspace was released (no scratch: generation 1 in 1024-row tiles, the launch's split kept and met
    by atomics), after an m4rm_dev call whose reservation holds the batch (generation 4, the plan of the table) and after one whose
    reservation is too small (generation 1 again): three times the NumPy product."""
    batch = cases.cus() + extra if extra else 9
    assert cases.reserved_words(64, 64) < cases.a4_words(m, l, batch)
    kw = dict(batch=batch, strided=strided, seed=10)
    cases.run("m4rm_batch_dev", on_gen1, m, l, n, scratch_ok=False, before=m4ri_amd.lib().m4ri_amd_release_workspace, **kw)
    cases.run("m4rm_batch_dev", on_gen4, m, l, n, scratch_ok=True, before=_reserve_for(m, l, batch), **kw)
    cases.run("m4rm_batch_dev", on_gen1, m, l, n, scratch_ok=False, before=cases.tiny_product, **kw)


# ---- edges of the inner dimension ----------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_more_splits_requested_than_the_inner_dimension_has(strided):
    """ksplit = 64 at l = 100: generation 4 makes the 2 splits its four dwords of A allow (slabs sized for 2), generation 1 is handed
    the 64 and rounds them in its launcher; both clear nothing they should not."""
    cases.run("m4rm_dev", "gen4 split slabs", 300, 100, 1000, ksplit=64, strided=strided, seed=11, more=dict(ksplit=2))
    cases.run("m4rm_dev", "gen1 split atomics", 100, 100, 3000, ksplit=64, strided=strided, seed=12, more=dict(ksplit=64))


@LAYOUTS
def test_empty_inner_dimension_clears_or_keeps_c(strided):
    """l = 0: C = 0 (the members' words, nothing between them) or C kept, no kernel of the leaf."""
    cases.run("m4rm_batch_dev", "empty inner dimension", 70, 0, 130, batch=3, strided=strided, seed=13)
    cases.run("m4rm_dev", "empty inner dimension", 70, 0, 130, strided=strided, seed=13)


# ---- switches read once per process: one child each ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CHILDREN))
def test_branches_behind_a_developer_switch(name):
    """tail_ksplit: M4RI_AMD_TAIL_KSPLIT=8 on a short last round of 100 tiles -- the hybrid plan WITHOUT slabs (zero_tiles + atomics in the
    tail), which the cost model alone never picks.  no_small_leaf: M4RI_AMD_SMALL_LEAF=0 and the branches above at inner dimensions of
    64 ... 256 bits (leaf_launch_cases.py child_tail_ksplit / child_no_small_leaf)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, **cases.CHILDREN[name][1])
    r = subprocess.run([sys.executable, os.path.join(here, "leaf_launch_cases.py"), name], cwd=os.path.dirname(here), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert " cases passed" in r.stdout

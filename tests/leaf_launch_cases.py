"""What tests/test_gpu_leaf_launch.py runs for one case, and the two child processes it starts (python tests/leaf_launch_cases.py NAME):
a product through an entry point callers use, on operands with pattern-filled words between rows, between members and around the
buffers, asserted -- through m4ri_amd_plan_leaf_launch, for the device's own compute-unit count -- to have taken the branch of
engine.hip launch_leaf_one the case is named for, and compared word for word with the NumPy product of tests/leaf_reference.py.

The plan is asked with the scratch flag the entry guarantees: True for m4rm_dev and mul_batch_dev (they reserve first), and for
m4rm_batch_dev what the case knows of the previous call (`scratch_ok`)."""
from __future__ import annotations

import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:  # run as a script (the child processes): the package is beside tests/
    sys.path.insert(0, _ROOT)

import m4ri_amd  # noqa: E402
import leaf_reference as ref  # noqa: E402

GUARD = 67          # pattern words before and after C (odd: a strided C starts 8- but not 16-byte aligned)
_rng = np.random.default_rng


def cus() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def a4_words(m: int, l: int, batch: int) -> int:
    """Words of packed-A scratch a generation-4 launch needs (a4_pack.hip gf2_m4rm8_a4_words: two dwords per word of A, rows padded to 4)."""
    return (batch * ((m + 3) & ~3) * 2 * ref.words_of(l) + 1) // 2


def reserved_words(m: int, l: int) -> int:
    """Words of packed-A scratch an m4rm_dev call of this shape leaves behind (engine.hip reserve_apk: whole 256-byte granules)."""
    return (a4_words(m, l, 1) + 31) & ~31


def product(A: np.ndarray, B: np.ndarray, l: int) -> np.ndarray:
    """leaf_reference.product, 256 words of columns at a time (the float matrices of a 150000-column B stay small)."""
    wn = B.shape[1]
    if wn <= 256:
        return ref.product(A, B, l)
    return np.concatenate([ref.product(A, np.ascontiguousarray(B[:, w:w + 256]), l) for w in range(0, wn, 256)], axis=1)


class Operands:
    """A, B and the NumPy product of every member, made once per shape and shared by the add / layout variants of a case (read-only)."""

    def __init__(self, m, l, n, batch, seed):
        self.m, self.l, self.n, self.batch = m, l, n, batch
        self.wl, self.wn = ref.words_of(l), ref.words_of(n)
        r = _rng(seed)
        self.sa, self.sb = self.wl + 1, self.wn + 3                  # rows of A and B a little apart, members too
        self.abs, self.bbs = m * self.sa + 5, l * self.sb + 2
        self.hA = r.integers(0, 1 << 64, size=max(batch * self.abs, 1), dtype=np.uint64)   # bits of A beyond column l: whatever
        self.hB = r.integers(0, 1 << 64, size=max(batch * self.bbs, 1), dtype=np.uint64)
        self.P = np.zeros((batch, m, self.wn), dtype=np.uint64)
        for b in range(batch):
            Ab = self.hA[b * self.abs: b * self.abs + m * self.sa].reshape(m, self.sa)[:, :self.wl]
            Bb = self.hB[b * self.bbs: b * self.bbs + l * self.sb].reshape(l, self.sb)[:, :self.wn]
            self.P[b] = product(Ab, Bb, l)
        for x in (self.hA, self.hB, self.P):
            x.setflags(write=False)
        self.tA = self.tB = None

    def upload(self):
        import torch
        if self.tA is None:
            self.tA, self.tB = (torch.from_numpy(x.view(np.int64).copy()).cuda() for x in (self.hA, self.hB))
        return self


_operands = {}


def operands(m, l, n, batch, seed=1) -> Operands:
    key = (m, l, n, batch, seed)
    if key not in _operands:
        if len(_operands) >= 2:   # a case's variants follow each other: two shapes are all that is ever live
            _operands.pop(next(iter(_operands)))
        _operands[key] = Operands(m, l, n, batch, seed)
    return _operands[key]


class CFrame:
    """`batch` members of m rows of wn words inside a pattern-filled buffer.  strided: rows c_stride = wn + 3 words apart, members
    m * c_stride + 7, the first word at an odd word of the allocation; else one contiguous block (c_stride = wn, c_bs = m * wn)."""

    def __init__(self, m, wn, batch, strided, seed):
        self.m, self.wn, self.batch = m, wn, batch
        self.cs = wn + 3 if strided else wn
        self.cbs = m * self.cs + (7 if strided else 0)
        self.base = GUARD if strided else GUARD + 1
        total = self.base + (batch - 1) * self.cbs + m * self.cs + GUARD
        self.before = _rng(seed).integers(0, 1 << 64, size=total, dtype=np.uint64)
        self.inside = np.zeros(total, dtype=bool)
        self.members(self.inside)[:] = True

    def members(self, flat):
        """(batch, m, wn) view of the members' words inside a flat buffer of this geometry."""
        it = flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.base:], shape=(self.batch, self.m, self.wn), strides=(it * self.cbs, it * self.cs, it), writeable=True)

    def upload(self):
        import torch
        self.t = torch.from_numpy(self.before.view(np.int64).copy()).cuda()
        return self

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.base

    def check(self, P, add, what):
        """Every word between rows, between members and around the frame as before; every word of every member the product (XORed
        into what was there when accumulating)."""
        after = self.t.cpu().numpy().view(np.uint64)
        moved = np.flatnonzero((after != self.before) & ~self.inside)
        assert moved.size == 0, (f"{what}: {moved.size} words outside the members of C changed, the first at word {int(moved[0]) - self.base} from C "
                                 f"(c_stride {self.cs}, c_bs {self.cbs}, {self.batch} x {self.m} rows of {self.wn} words)")
        got, was = self.members(after), self.members(self.before)
        want = was ^ P if add else P
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} words of C differ from the NumPy product, the first at (member, row, word) {tuple(int(x) for x in bad[0])}"


def expect(plan, **want):
    """The plan is the branch the case is named for: every named field has the named value (a callable: holds for the value)."""
    for k, v in want.items():
        got = getattr(plan, k)
        assert (v(got) if callable(v) else got == v), f"the plan is not the case's branch: {k} = {got}; {plan}"


BRANCHES = {   # name -> what the plan must say
    "gen4 unsplit": dict(gen=4, ksplit=1, tail_tiles=0, mode=lambda x: x in (0, 1), slabs=0, zero=0, pack_a=1),
    "gen4 hybrid slabs": dict(gen=4, ksplit=1, tail_tiles=lambda x: x > 0, tail_ksplit=lambda x: x > 1, tail_mode=2, slabs=1, zero=0, pack_a=1),
    "gen4 hybrid atomics": dict(gen=4, ksplit=1, tail_tiles=lambda x: x > 0, tail_ksplit=lambda x: x > 1, tail_mode=1, slabs=0, pack_a=1),
    "gen4 split slabs": dict(gen=4, ksplit=lambda x: x > 1, tail_tiles=0, mode=2, slabs=1, zero=0, pack_a=1),
    "gen4 split atomics": dict(gen=4, ksplit=lambda x: x > 1, tail_tiles=0, mode=1, slabs=0, pack_a=1),
    "gen1 fallback": dict(gen=1, rg=32, tile_rows=1024, tail_tiles=0, slabs=0, pack_a=0),
    "gen1 fallback split": dict(gen=1, rg=32, tile_rows=1024, ksplit=lambda x: x > 1, tail_tiles=0, mode=1, slabs=0, pack_a=0),
    "gen1 split atomics": dict(gen=1, ksplit=lambda x: x > 1, mode=1, slabs=0, pack_a=0),
    "small leaf split": dict(gen=5, ksplit=lambda x: x > 1, mode=1, slabs=0, pack_a=0),
    "small leaf unsplit": dict(gen=5, ksplit=1, slabs=0, zero=0, pack_a=0),
    "empty inner dimension": dict(gen=0),
}


def planned(branch, m, l, n, batch, add, ksplit, ncu, scratch_ok, more=None):
    """The plan of the launch, asserted to be `branch` (and `more`), and to clear what that branch needs cleared."""
    plan = m4ri_amd.plan_leaf_launch(m, l, n, batch, add=add, ksplit=ksplit, cus=ncu, scratch_ok=scratch_ok)
    expect(plan, **BRANCHES[branch])
    expect(plan, **(more or {}))
    atomics = (plan.ksplit > 1 or plan.tail_tiles > 0) and not plan.slabs
    expect(plan, zero=(0 if add or not atomics else 2 if plan.tail_tiles else 1) if l else (0 if add else 1))
    return plan


def run(entry, branch, m, l, n, batch=1, ksplit=0, strided=False, scratch_ok=True, adds=(False, True), seed=1, more=None, before=None):
    """One case: the plan for this device is `branch` (and `more`); then, with add off and on, the entry on a fresh C and the checks.
    before: called ahead of every launch (what puts the engine's scratch in the state the case is about).  Returns the plan."""
    import torch
    ncu = cus()
    what = f"{entry} {batch} x ({m} x {l} x {n}), ksplit {ksplit}, {'strided' if strided else 'contiguous'} C, {ncu} CUs: {branch}"
    ops = operands(m, l, n, batch, seed).upload()
    for add in adds:
        plan = planned(branch, m, l, n, batch, add, ksplit, ncu, scratch_ok, more)
        if before is not None:
            before()
        C = CFrame(m, ops.wn, batch, strided, seed + 100 + int(add)).upload()
        if entry == "m4rm_dev":
            assert batch == 1
            m4ri_amd.m4rm_dev(C.ptr, C.cs, ops.tA.data_ptr(), ops.sa, ops.tB.data_ptr(), ops.sb, m, l, n, add=add, ksplit=ksplit)
        elif entry == "mul_batch_dev":
            assert ksplit == 0
            m4ri_amd.mul_batch_dev(C.ptr, C.cs, C.cbs, ops.tA.data_ptr(), ops.sa, ops.abs, ops.tB.data_ptr(), ops.sb, ops.bbs, m, l, n, batch, add, 1 << 20, 0)
        elif entry == "m4rm_batch_dev":
            assert ksplit == 0
            rc = m4ri_amd.lib().m4ri_amd_m4rm_batch_dev(C.ptr, C.cs, C.cbs, ops.tA.data_ptr(), ops.sa, ops.abs, ops.tB.data_ptr(), ops.sb, ops.bbs, m, l, n, batch, int(add), None)
            assert rc == 0, f"{what}: hipError_t {rc}"
        else:
            raise ValueError(entry)
        torch.cuda.synchronize()
        st = m4ri_amd.get_stats()
        assert st.levels == 0, f"{what}: {st.levels} Strassen levels"
        if plan.gen:
            assert (st.leaf_gen, st.leaf_launches, st.leaf_products) == (plan.gen, 1, batch), \
                f"{what}, add={add}: generation {st.leaf_gen}, {st.leaf_launches} launches, {st.leaf_products} products; {plan}"
        else:
            assert (st.leaf_launches, st.leaf_products) == (0, 0), f"{what}: nothing to launch, yet {st.leaf_launches} launches"
        C.check(ops.P, add, f"{what}, add={add}")
    return plan


def tiny_product():
    """An m4rm_dev call whose reservation is too small for any batch of the cases: 64 x 64 x 64."""
    import torch
    t = torch.zeros(3 * 64, dtype=torch.int64, device="cuda")
    m4ri_amd.m4rm_dev(t.data_ptr(), 1, t.data_ptr() + 8 * 64, 1, t.data_ptr() + 8 * 128, 1, 64, 64, 64)
    torch.cuda.synchronize()


# ---- the child processes: one per set of switches, each read once per process --------------------------------------------------------
def child_tail_ksplit():
    """M4RI_AMD_TAIL_KSPLIT=8 and a short last round of 100 tiles: 800 slabs are more than the 768 there are, so the tail's splits meet by
    atomic XOR in tiles cleared by zero_tiles -- the hybrid plan without slabs, which the cost model alone never reaches."""
    assert os.environ.get("M4RI_AMD_TAIL_KSPLIT") == "8"
    ncu = cus()
    for strided in (False, True):
        run("mul_batch_dev", "gen4 hybrid atomics", 256, 512, 512, batch=ncu + 100, strided=strided, seed=31,
            more=dict(tail_tiles=100, tail_ksplit=8))
    # one product, its last column tile and last word ragged: the tail is the last 100 column tiles
    run("m4rm_dev", "gen4 hybrid atomics", 250, 512, (ncu + 100) * 512 - 77, strided=True, seed=32, more=dict(tail_tiles=100, tail_ksplit=8))
    return 3


def child_no_small_leaf():
    """M4RI_AMD_SMALL_LEAF=0: generations 4 and 1 at inner dimensions of 64 to 256 bits, where the 2^34 rule otherwise sends every one of
    these launches to the small leaf.  At so few stages the cost model itself splits nothing (a split's fixed cost is more than the whole
    inner loop: the plans below say so for one, two and a ragged number of rounds), so the split branches are reached by a requested
    ksplit: slabs, atomics beyond the slab region, generation 1; and the fallback of m4rm_batch_dev runs unsplit."""
    assert os.environ.get("M4RI_AMD_SMALL_LEAF") == "0"
    ncu = cus()
    release = m4ri_amd.lib().m4ri_amd_release_workspace
    done = 0
    for strided in (False, True):
        kw = dict(strided=strided, seed=41)
        for l in (64, 200):
            run("mul_batch_dev", "gen4 unsplit", 192, l, 512, batch=ncu + 44, **kw)          # two rounds, the second short: no tail at this length
        run("mul_batch_dev", "gen4 unsplit", 192, 128, 512, batch=ncu + 1, **kw)
        run("mul_batch_dev", "gen4 unsplit", 192, 256, 512, batch=ncu, **kw)
        run("m4rm_dev", "gen4 unsplit", 200, 256, (ncu + 44) * 512 - 77, **kw)
        run("mul_batch_dev", "gen4 unsplit", 300, 256, 1000, batch=9, **kw)
        run("m4rm_dev", "gen4 split slabs", 192, 100, 51200, ksplit=8, more=dict(ksplit=2), **kw)
        run("m4rm_dev", "gen4 split slabs", 192, 256, 51200, ksplit=8, more=dict(ksplit=4), **kw)
        run("m4rm_dev", "gen4 split atomics", 192, 256, 250 * 512, ksplit=8, more=dict(ksplit=4, tiles=250), **kw)   # 1000 slabs wanted
        for l in (64, 200):
            run("m4rm_dev", "gen1 split atomics", 100, l, 3000, ksplit=4, **kw)
        run("m4rm_batch_dev", "gen1 fallback", 192, 64, 512, batch=ncu + 44, scratch_ok=False, before=release, **kw)
        run("m4rm_batch_dev", "gen1 fallback", 300, 256, 1000, batch=9, scratch_ok=False, before=tiny_product, **kw)
        done += 13
    return done


CHILDREN = {"tail_ksplit": (child_tail_ksplit, {"M4RI_AMD_TAIL_KSPLIT": "8"}), "no_small_leaf": (child_no_small_leaf, {"M4RI_AMD_SMALL_LEAF": "0"})}

if __name__ == "__main__":
    import torch
    assert m4ri_amd.lib().m4ri_amd_device_count() >= 1, "no HIP device visible"
    m4ri_amd.init(0)
    torch.cuda.set_device(0)
    print(f"leaf launch child {sys.argv[1]}: {CHILDREN[sys.argv[1]][0]()} cases passed", flush=True)

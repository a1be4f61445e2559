"""What keeps the shape sweep of tests/test_gpu_batch_shape_sweep.py from being hollow, pinned on the oracle and NumPy alone: the
domain is complete, every kind of member and every scheduled size occurs where it has to, the members split into full-rank and
deficient, solvable and unsolvable, invertible and singular ones at every size, the plan functions route the domain as the sweep
supposes, and the arena packer puts the members where it says and nowhere else."""
import numpy as np
import pytest

import m4ri_amd
import sweep_cases as sc

ALL = sc.S0 + sc.S1


def test_the_domain_is_complete():
    assert len(sc.S0) == len(set(sc.S0)) == 4096 and set(sc.S0) == {(m, n) for m in range(1, 65) for n in range(1, 65)}
    edge, thin = {65, 66, 127, 128, 129}, set(range(1, 67)) | {127, 128, 129}
    assert set(sc.S1) == {(m, n) for m in thin | edge for n in thin | edge if (m in edge and n in thin) or (m in thin and n in edge)}
    assert len(sc.S1) == len(set(sc.S1)) == 665 and not set(sc.S0) & set(sc.S1)
    assert sc.SQUARES == list(range(1, 131))
    rows = sc.rows_of(ALL)
    assert [r[0][0] for r in rows] == sorted({m for m, _ in ALL}) and sum(len(r) for r in rows) == len(ALL)
    assert all(len({m for m, _ in r}) == 1 for r in rows)


def test_the_plan_functions_route_the_domain_as_the_sweep_supposes():
    """Path 0 on every shape up to 64 x 64 for every call; path 1 beyond for the elimination calls."""
    for m, n in ALL:
        want = 0 if max(m, n) <= 64 else 1
        k, got = sc.k_of(m, n), {}
        got["echelonize"] = m4ri_amd.plan_echelonize_batch(m, n)
        got["order"] = m4ri_amd.plan_echelonize_order_batch(m, n)
        got["ple"] = m4ri_amd.plan_ple_batch(m, n)
        got["solve"] = m4ri_amd.plan_solve_batch(m, n, k)
        got["kernel"] = m4ri_amd.plan_kernel_batch(m, n)
        got["pluq_solve"] = m4ri_amd.plan_pluq_solve_batch(m, n, k)
        assert set(got.values()) == {want}, ((m, n, k), got)
    for n in sc.SQUARES:
        assert m4ri_amd.plan_solve_batch(n, n, n) == (0 if n <= 64 else 1), n
    for m, n in sc.S0:
        assert m4ri_amd.plan_transpose_batch(m, n) == 0
        for plane, op in [(p, sc.NN) for p in sc.PLANES] + list(zip(sc.PLANES, (sc.NT, sc.TN, sc.TT))):
            assert m4ri_amd.plan_mul_small_batch_op(*sc.triple(plane, m, n), *op) == 0
        assert m4ri_amd.plan_mul_small_batch(*sc.triple("ml", m, n)) == 0


def test_every_kind_occurs_with_every_row_and_column_count():
    for sizes, axis in ((sorted({m for m, _ in ALL}), 0), (sorted({n for _, n in ALL}), 1)):
        for x in sizes:
            kinds = {sc.kind_of(m, n, b) for m, n in ALL if (m, n)[axis] == x for b in range(sc.BATCH)}
            assert kinds == set(sc.KINDS), (axis, x, kinds)
    for m in sc.SMALL:   # and within the shapes up to 64 x 64 alone
        assert {sc.kind_of(m, n, b) for n in sc.SMALL for b in range(sc.BATCH)} == set(sc.KINDS)
        assert {sc.kind_of(n, m, b) for n in sc.SMALL for b in range(sc.BATCH)} == set(sc.KINDS)


def test_the_kinds_are_what_they_say_and_the_seeds_depend_on_the_shape_and_member_alone():
    for m, n in [(1, 1), (2, 1), (8, 8), (64, 64), (47, 64), (64, 3), (129, 66)]:
        rng = lambda: np.random.default_rng(m * n)
        low, sparse, zc, halves, perm, ones = (sc.bits_of(k, m, n, rng()) for k in sc.KINDS[1:])
        assert sc.rank_np(low) <= max(1, min(m, n) // 3)
        assert sparse.any() and (m <= 4 or sparse.sum() <= 4 * n)
        assert not zc[:, 0].any() and (~zc.any(axis=0)).sum() >= max(1, n // 3)
        assert np.array_equal(halves[m - m // 2:], halves[: m // 2])
        assert (perm.sum(axis=0) <= 1).all() and (perm.sum(axis=1) <= 1).all() and (min(m, n) + 1) // 2 <= perm.sum() <= min(m, n)
        assert ones.all()
        for b in range(sc.BATCH):
            assert np.array_equal(sc.member(m, n, b), sc.member(m, n, b)) and sc.member(m, n, b).shape == (m, n)
    assert sc.bits_of("sparse", 8, 8, np.random.default_rng(1)).any(), "a sparse 8 x 8 member that is all zero says nothing"


def test_every_scheduled_size_occurs():
    every = set(range(1, 65))
    ks = [sc.k_of(m, n) for m, n in sc.S0]
    assert set(ks) == every and ks.count(64) >= 1024 and {sc.k_of(m, n) for m, n in sc.S1} <= every
    assert {sc.kc_of(m, n) for m, n in sc.S0} == every and all(1 <= sc.kc_of(m, n) <= n for m, n in ALL)
    for m in sc.SMALL:   # the null space's three cases at every row count: one column, all of them, some
        assert {(sc.kc_of(m, n) == 1, sc.kc_of(m, n) == n) for n in range(4, 65)} == {(True, False), (False, True), (False, False)}
    for plane, at in (("ml", 2), ("ln", 0), ("mn", 1)):
        for a in sc.SMALL:
            assert {sc.triple(plane, a, b)[at] for b in sc.SMALL} == every, (plane, a)
        for a, b in ALL:
            t = sc.triple(plane, a, b)
            assert 1 <= t[at] <= 64 and tuple(x for i, x in enumerate(t) if i != at) == (a, b)


def test_full_rank_and_deficient_members_at_every_row_count(oracle):
    for m in sorted({m for m, _ in ALL}):
        full = deficient = False
        for n in [n for mm, n in ALL if mm == m]:
            for G in sc.members(m, n):
                r = sc.rank_of(oracle, G)
                assert r == sc.rank_np(G)
                full, deficient = full or r == min(m, n), deficient or r < min(m, n)
            if full and deficient:
                break
        assert full and (deficient or m < 2), m


def test_solvable_and_unsolvable_systems_at_every_row_count(oracle):
    """Status 0 and status -1 for every m >= 4, taken over all n; the consistent members are B = A X, so their status is 0."""
    for m in sorted({m for m, _ in ALL}):
        seen = set()
        for n in [n for mm, n in ALL if mm == m]:
            c = sc.solve_case(oracle, m, n)
            assert (c["status"][[0, 1, 3, 4]] == 0).all(), (m, n)
            seen |= set(c["status"].tolist())
            if seen == {0, -1}:
                break
        assert 0 in seen and (-1 in seen or m < 4), m
    for n in (1, 5, 40, 64, 66, 129):   # one decomposition for all: the same low-rank A, solvable and unsolvable members
        c = sc.solve_case(oracle, n, n, shared=True)
        assert (c["status"][[0, 1, 3, 4]] == 0).all() and (n < 4 or c["status"][2] == -1) and len(set(c["rank"].tolist())) == 1


def test_invertible_and_singular_members_at_every_size(oracle):
    for n in sc.SQUARES:
        c = sc.inv_case(oracle, n)
        assert (c["rank"][:4] == n).all() and c["rank"][4] < n, n
        for G, W in zip(c["A"][:4], c["inv"][:4]):   # and the oracle's inverse is one
            X = sc.from_words(W[None], n)[0]
            assert np.array_equal((G.astype(np.int64) @ X.astype(np.int64)) & 1, np.eye(n, dtype=np.int64)), n
    assert {n % 3 for n in sc.SQUARES} == {0, 1, 2}   # a repeated row, a zero column, a random singular matrix


def test_the_arena_packer_round_trips_and_covers_the_buffer_exactly():
    shapes = [(1, 1), (5, 64), (64, 64), (3, 65), (129, 128), (2, 129)]
    arena = sc.Arena()
    blocks = [arena.add(s, *s, pad=1 + i % 2, gap=3 + i) for i, s in enumerate(shapes)]
    image, other = arena.dirt(1), arena.dirt(2)
    for blk in blocks:
        for h in (image, other):
            sc.put(h, blk, sc.to_words(sc.members(blk.rows, blk.cols)))
    inside = arena.inside()
    # the members come back; outside them the image is the dirt it started as, inside it does not depend on the dirt
    for blk in blocks:
        assert np.array_equal(sc.from_words(sc.get(image, blk), blk.cols), sc.members(blk.rows, blk.cols))
        assert blk.stride > (blk.cols + 63) // 64 and blk.bs > blk.rows * blk.stride
    assert np.array_equal(image & ~inside, arena.dirt(1) & ~inside) and np.array_equal(image & inside, other & inside)
    assert (image & ~inside != other & ~inside).any()
    # no two members share a word, and the mask holds exactly the members' bits
    words = np.concatenate([blk.idx.reshape(-1) for blk in blocks])
    assert np.unique(words).size == words.size and words.max() < arena.size == image.size
    bits = sum(bin(int(x)).count("1") for x in inside)
    assert bits == sum(sc.BATCH * m * n for m, n in shapes)
    assert (inside == 0).sum() == arena.size - sum(sc.BATCH * m * ((n + 63) // 64) for m, n in shapes)
    # every word is found again: the members' own words and the gap behind a member
    blk = blocks[3]
    j = np.searchsorted(arena.offsets(), int(blk.idx[2, 1, 1]), side="right") - 1
    assert arena.locate(int(j), int(blk.idx[2, 1, 1])) == ((3, 65), 2, blk.stride + 1)
    assert arena.locate(3, blk.off + 2 * blk.bs - 1) == ((3, 65), 1, blk.bs - 1)
    ints = sc.Ints()
    offs = [ints.add(s, min(s)) for s in shapes]
    assert ints.size == sum(sc.BATCH * min(s) + 3 for s in shapes) and (ints.image() == -7).all()
    assert ints.locate(2, offs[2] + 64 * 3 + 5) == ((64, 64), 3, 64 * 3 + 5)


def test_a_job_reports_what_differs_and_where(oracle):
    """The comparison the GPU sweep relies on, fed by hand: the expected buffers pass; one flipped bit, one written gap word and one
    wrong rank are found and named by shape, member and word."""
    shapes = [(m, n) for m in (5, 47) for n in (3, 64, 65)]
    job = sc.ech_job(oracle, shapes, 1)
    assert [k for k, _, _ in job.launches] == shapes and not job.failures({k: v.copy() for k, v in job.want.items()})
    assert job.failures({k: v.copy() for k, v in job.bufs.items()}), "the forms of these members differ from the members"
    got = {k: v.copy() for k, v in job.want.items()}
    blk = job.where["A"].blocks[4]
    got["A"][blk.idx[3, 46, 0]] ^= np.uint64(1)       # a valid bit of member 3
    got["A"][blk.off + blk.bs - 1] ^= np.uint64(1)    # the last word of the gap behind member 0
    got["rank"][job.where["rank"].offs[1] + 2] += 1
    fails = job.failures(got)
    assert sorted(t for _, t in fails) == sorted([f"(47, 64) member 0 A[{blk.bs - 1}]", f"(47, 64) member 3 A[{46 * blk.stride}]",
                                                  "(5, 64) member 2 rank[2]"])
    with pytest.raises(AssertionError, match=r"echelonize_batch_dev \(full=1\): 2 of 6 shapes differ.*\(47, 64\) member 0"):
        sc.verdict(job.call, job.flags, fails, len(shapes))
    sc.verdict(job.call, job.flags, [], len(shapes))


def test_every_job_keeps_its_launches_inside_its_buffers(oracle):
    """Every kind of job on a few shapes either side of 64: each pointer of each launch names a buffer of the job and an element of
    it, one launch per shape, and a buffer nobody may write is expected back as it went."""
    shapes = [(1, 1), (47, 64), (64, 47), (64, 64), (65, 3), (2, 129), (129, 128)]
    squares = [(n, n) for n in (1, 64, 65, 129)]
    pairs = [(9, 11), (64, 64), (129, 5), (7, 128)]
    jobs = [sc.ech_job(oracle, shapes, 0), sc.ech_job(oracle, shapes, 1, order=True), sc.order_job(shapes), sc.ple_job(oracle, shapes, 0),
            sc.ple_job(oracle, shapes, 1), sc.solve_job(oracle, shapes), sc.pluq_solve_job(oracle, shapes),
            sc.pluq_solve_job(oracle, squares, shared=True), sc.inv_job(oracle, [1, 64, 65, 130], False), sc.inv_job(oracle, [1, 64, 65, 130], True),
            sc.kernel_job(oracle, shapes), sc.transpose_job(shapes), sc.transpose_job(squares, inplace=True)]
    jobs += [sc.mul_job(plane, pairs, add, results_only={(129, 5), (7, 128)}) for plane in sc.PLANES for add in (0, 1)]
    jobs += [sc.mul_job(plane, pairs, 0, op, refused={(129, 5)}) for plane, op in zip(sc.PLANES, (sc.NT, sc.TN, sc.TT))]
    for job in jobs:
        assert len(job.launches) == len({k for k, _, _ in job.launches}) and set(job.want) == set(job.bufs) == set(job.where)
        for key, args, error in job.launches:
            ptrs = [a for a in args if isinstance(a, sc.Ptr)]
            assert ptrs and all(0 <= a.off < job.bufs[a.name].size for a in ptrs), (job.call, key)
            assert all(isinstance(a, (int, np.integer)) for a in args if not isinstance(a, sc.Ptr)), (job.call, key, args)
            assert error in (None, 801)
        assert not job.failures({k: v.copy() for k, v in job.want.items()})
        for name in job.bufs:
            assert job.bufs[name].size == job.want[name].size == job.where[name].size and job.bufs[name].dtype == job.want[name].dtype
    solve = jobs[5]
    assert solve.want["A"] is solve.bufs["A"] and not np.array_equal(solve.want["B"], solve.bufs["B"])
    refused = jobs[-1]   # a refused shape is expected back untouched, the others are not
    blocks = {blk.key: blk for blk in refused.where["C"].blocks}
    (key,) = [k for k, _, e in refused.launches if e]
    assert max(key) == 129 and np.array_equal(sc.get(refused.want["C"], blocks[key]), sc.get(refused.bufs["C"], blocks[key]))
    assert sum(not np.array_equal(sc.get(refused.want["C"], b), sc.get(refused.bufs["C"], b)) for b in blocks.values()) == 3
    only = jobs[13].mask["C"]   # results only: nothing but the valid bits of such a shape is compared, everything of the others
    for (a, b), blk in zip(pairs, jobs[13].where["C"].blocks):
        span = only[blk.off:blk.end]
        assert (span != 0).sum() == (blk.idx.size if a > 64 or b > 64 else span.size), (a, b)


def test_the_reference_products_and_transposes_are_numpy_s(oracle):
    """The NumPy references of the products against the oracle on a few shapes, stored operands transposed included."""
    from m4ri_amd.mzd import Mzd
    for plane, op, a, b in [("ml", sc.NN, 64, 64), ("ln", sc.TN, 47, 64), ("mn", sc.TT, 13, 7), ("ml", sc.NT, 129, 66)]:
        (m, l, n), A, B, C0, AB = sc.product_expected(plane, op, a, b)
        assert A.shape[1:] == ((l, m) if op[0] else (m, l)) and B.shape[1:] == ((n, l) if op[1] else (l, n)) and C0.shape[1:] == (m, n)
        for i in range(sc.BATCH):
            X, Y = (A[i].T if op[0] else A[i]), (B[i].T if op[1] else B[i])
            want = oracle.mul(None, Mzd.from_bits(np.ascontiguousarray(X)), Mzd.from_bits(np.ascontiguousarray(Y)), 0)
            assert np.array_equal(want.to_bits(), AB[i]), (plane, op, a, b, i)

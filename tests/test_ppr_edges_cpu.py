"""CPU: the inputs of tests/test_gpu_ppr_edges.py are what they claim to be (tests/ppr_edges.py).  The colliding ids hash to their
slots and their chain wraps past the last slot, the graphs are simple and symmetric, the oracle accepts every case, every case lies
on its side of the accept / refuse bounds of the push kernel, the tie cases tie at the cut of the top-K, and the plain per-row
restatement of the DEG / SPD union rules equals the reference's sparse algebra as SciPy runs it (oracle.encoding_scipy)."""
import numpy as np
import pytest

import ppr_edges as E
from oracle import oracle as orc

CAP = 1024
COLLIDING = [(190, [1023]), (256, [1023, 0]), (300, [1023, 1022])]


def _row(indptr, indices, root, alpha=E.ALPHA, eps=E.EPS, topk=4096):
    off, ids, vals, pushes = orc.ppr_topk(indptr, indices, [root], alpha, eps, topk, table_log2=16)
    return ids, vals, pushes


@pytest.mark.parametrize("root_slot", [None, 1023])
@pytest.mark.parametrize("K,slots", COLLIDING)
def test_colliding_star_hashes_wraps_and_is_accepted(K, slots, root_slot):
    indptr, indices, root, leaves = E.colliding_star(K, slots, root_slot=root_slot)
    assert E.is_simple_symmetric(indptr, indices)
    assert set(E.khash(leaves, 10).tolist()) == set(slots)
    assert int(E.khash([root], 10)[0]) == (1023 if root_slot is not None else (slots[0] + 512) % 1024)
    assert np.array_equal(indices[indptr[root]:indptr[root + 1]], leaves)
    # more ids than slots from the first of them to the end of the table: the chain runs on at slot 0
    assert K + (root_slot is not None) > CAP - min(s for s in slots if s > 512)
    for alpha, eps in ((E.ALPHA, E.EPS), (0.3, 1e-3)):
        for r in [root] + leaves[[0, K // 2, K - 1]].tolist():
            ids, vals, pushes = _row(indptr, indices, r, alpha, eps)
            touched = E.touched_count(indptr, indices, ids)
            print(f"K = {K}, slots {slots}, ({alpha}, {eps}), root {r}: np = {len(ids)}, touched = {touched}, pushes = {pushes}")
            assert touched == K + 1 and E.certainly_accepted(touched, CAP)


def test_khash_counts_per_slot():
    c = np.bincount(E.khash(np.arange(200_000), 10).astype(np.int64), minlength=CAP)
    print(f"ids below 200,000 per slot of 1,024: {c.min()} .. {c.max()}")
    assert c.min() >= 191           # 190 leaves and a root on one slot


@pytest.mark.parametrize("d", [1, 63, 64, 65, 255, 256, 257, 382])
def test_star_degrees_are_accepted(d):
    indptr, indices = E.star(d)
    assert E.is_simple_symmetric(indptr, indices)
    for alpha, eps in [(0.5, 1e-4)] + ([(0.15, 1e-5)] if d <= 65 else []):
        for r in (0, 1):
            ids, vals, pushes = _row(indptr, indices, r, alpha, eps)
            touched = E.touched_count(indptr, indices, ids)
            print(f"star({d}) ({alpha}, {eps}) root {r}: np = {len(ids)}, touched = {touched}, pushes = {pushes}")
            assert touched == d + 1 and E.certainly_accepted(touched, CAP)
            assert pushes < 80_000


@pytest.mark.parametrize("d,side", [(510, None), (511, None), (512, "refused"), (600, "refused")])
def test_star_refusal_bound(d, side):
    indptr, indices = E.star(d)
    for r in (0, 1):
        ids, _, _ = _row(indptr, indices, r)
        touched = E.touched_count(indptr, indices, ids)
        assert touched == d + 1
        assert E.certainly_refused(touched, CAP) == (side == "refused")
        assert not E.certainly_accepted(touched, CAP)
    assert E.certainly_accepted(383, CAP) and not E.certainly_accepted(384, CAP)
    assert E.certainly_refused(513, CAP) and not E.certainly_refused(512, CAP)


def test_mixed_graph_sides():
    indptr, indices, parts = E.mixed_graph()
    assert E.is_simple_symmetric(indptr, indices)
    want = {"colliding": True, "star512": False, "star600": False, "star7": True}
    for name, (hub, leaves) in parts.items():
        for r in (hub, int(leaves[0])):
            ids, _, _ = _row(indptr, indices, r)
            touched = E.touched_count(indptr, indices, ids)
            assert touched == len(leaves) + 1
            assert E.certainly_accepted(touched, CAP) == want[name] and E.certainly_refused(touched, CAP) == (not want[name])


@pytest.mark.parametrize("d", [255, 512])
def test_star_rows_tie_at_the_cut(d):
    """few distinct scores among np entries: the cut of the top-K falls between equal scores, which the order of entry decides"""
    indptr, indices = E.star(d)
    for r in (0, 1):
        ids, vals, _ = _row(indptr, indices, r)
        n_p = len(ids)
        distinct = len(np.unique(vals))
        s = np.sort(vals)
        tied = [k for k in (1, 2, 63, 64, 65, n_p - 1) if s[n_p - k] == s[n_p - k - 1]]
        print(f"star({d}) root {r}: np = {n_p}, {distinct} distinct scores, ties at the cut for topk in {tied}")
        assert n_p == d + 1 and distinct <= 5
        assert {63, 64, 65, n_p - 1} <= set(tied)


def test_bipartite_hub_keeps_one_entry_of_hundreds_touched():
    indptr, indices = E.complete_bipartite(20, 300)
    ids, vals, pushes = _row(indptr, indices, 0)
    assert ids.tolist() == [0] and pushes == 1 and E.touched_count(indptr, indices, ids) == 301


def test_alpha_one_cuts_among_zero_scores():
    indptr, indices = E.directed_graph(1500, 9000, 4)
    off, ids, vals, _ = orc.ppr_topk(indptr, indices, np.arange(1500), 1.0, 1e-4, 100, table_log2=16)
    lens = np.diff(off)
    print(f"alpha = 1: rows of {lens.min()} .. {lens.max()} entries, {(vals == 0).sum()} zero scores")
    assert lens.min() == 1 and lens.max() > 5 and (vals == 0).sum() > 1000      # topk = 5 cuts rows whose scores are all-zero bits


def test_star_1500_is_one_push():
    """the case the retry ceiling of ppr.ppr_topk used to refuse: one push, 1,501 nodes touched, one entry kept"""
    indptr, indices = E.star(1500)
    ids, vals, pushes = _row(indptr, indices, 0, 0.5, 1e-2)
    assert ids.tolist() == [0] and vals.tolist() == [0.5] and pushes == 1
    assert E.touched_count(indptr, indices, ids) == 1501 and E.certainly_refused(1501, 2048)


def test_repeated_entry_star_passes_no_table_up_to_the_ceiling():
    indptr, indices = E.repeated_entry_star()
    N = len(indptr) - 1
    assert not E.is_simple_symmetric(indptr, indices)
    ceiling = 1 << (2 * N + 257 - 1).bit_length()
    assert E.certainly_refused(1 + 4 * (N - 1), ceiling)


@pytest.mark.parametrize("mode", ["DEG", "SPD"])
def test_union_restatement_equals_scipy(mode):
    X, A = E.edge_inputs_for_encoders()
    N = X.shape[0]
    assert (A != A.T).nnz == 0 and A.diagonal().nonzero()[0].tolist() == [0, N // 2, N - 1] and (X.data > 0).all()
    deg, xlen = A.getnnz(axis=1), X.getnnz(axis=1)
    assert {63, 64, 65, 130, 257} <= set(deg.tolist()) and deg[E.ISOLATED] == 0
    assert {0, 1, 63, 64, 65, 129, N} <= set(xlen.tolist()) and xlen[E.ISOLATED] == 0
    has = lambda m, i: i in m.indices[m.indptr[i]:m.indptr[i + 1]]
    assert [(has(A, i), has(X, i)) for i in (0, N // 2, 1, 2)] == [(True, True), (True, False), (False, True), (False, False)]
    row = lambda i: np.union1d(A.indices[A.indptr[i]:A.indptr[i + 1]], X.indices[X.indptr[i]:X.indptr[i + 1]])
    assert row(0).min() == 0 and row(1).min() == 1 and row(N - 1).max() == N - 1 and row(N - 2).max() == N - 2
    assert row(2).min() > 2 and row(N - 3).max() < N - 3
    want, wagg = orc.encoding_scipy(X, A, mode)
    indptr, ids, val, agg = E.encode_union(X, A, mode)
    np.testing.assert_array_equal(want.indptr, indptr)
    np.testing.assert_array_equal(want.indices, ids)
    np.testing.assert_array_equal(want.data.astype(np.float64).view(np.int64), val.view(np.int64))
    if mode == "DEG":
        np.testing.assert_array_equal(wagg.indices, ids)
        np.testing.assert_array_equal(wagg.data.view(np.int64), agg.view(np.int64))
    else:
        assert wagg is None and agg is None


def test_long_row_sizes_the_lds_of_the_fill():
    for kmax, above in ((6551, False), (6552, True), (8192, True)):
        X, A, s = E.long_row_inputs(kmax)
        assert X.getnnz(axis=1).max() == kmax == X.getnnz(axis=1)[s] and A.getnnz(axis=1)[s] == 65
        assert np.sort(X.getnnz(axis=1))[-2] <= 3 and (A != A.T).nnz == 0
        assert (10 * kmax + 20 > 64 * 1024) == above


def test_packed_rows_layout():
    indptr, indices = E.directed_graph(1500, 9000, 4)
    deg = np.diff(indptr)
    sinks, nonsinks = np.flatnonzero(deg == 0), np.flatnonzero(deg > 0)
    for nnz in (0, 1, 255, 256, 257, 1000):
        roots, row_off, ids, vals = E.packed_rows(nnz, 1500, sinks, nonsinks)
        lens = np.diff(row_off)
        assert row_off[-1] == nnz == len(ids) == len(vals) and lens[0] == 0 and lens[-1] == 0 and lens[2] == lens[3] == 0
        assert deg[roots[0]] == 0 and (deg[ids] == 0).any() == (nnz > 0)
        if nnz:
            last = np.flatnonzero(lens)[-1]
            assert deg[roots[last]] > 0 and vals.argmax() == nnz - 1

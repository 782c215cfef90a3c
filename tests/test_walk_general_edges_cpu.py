"""CPU: the shapes and graphs of tests/walk_general_edges.py reach the branches of walk_sets_kernel, walk_sets_kernel<SPG>
(csrc/walk.hip), walk_pipe_kernel (csrc/walk_pipe.hip) and compact_sets_kernel that tests/test_gpu_walk_general_edges.py means them
for -- shown with the oracle's sets and the plain-Python restatements of the launcher and the general SPG epilogue.  No kernel runs
here; the two LDS refusals go through the C ABI, which refuses them before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import walk_general_edges as G
import walk_rows_edges as W
from surel_plus_amd import sampler

SEED = 13


def _sets(g, q, M, m, rng, bucket=-1):
    ref = G.reference(g, q, M, m, rng, SEED, bucket)
    return ref, [ref["ids"][ref["off"][i]: ref["off"][i + 1]] for i in range(len(q))]


# ---------------------------------------------------------------------------------------------------------------- the launcher
def test_restatement_agrees_with_walk_kernel_name():
    """kernel_for against sampler.walk_kernel_name over M = 1 .. 300, 1 .. 6 hops, plain and fused, with and without a truncating
    bucket (a bucket of exactly Q truncates nothing: the launcher keeps walk_rows_kernel where the host predicate says general, as
    test_walk_rows_edges_cpu.py records)"""
    for M in range(1, 301):
        for m in range(1, 7):
            Q = M * m + 1
            assert G.kernel_for(M, m) == sampler.walk_kernel_name(None, M, m, False), (M, m)
            for bucket in (-1, 1, Q - 1, Q + 1):
                k = G.kernel_for(M, m, "table", bucket=bucket)
                if not k.startswith("refused"):
                    assert k == sampler.walk_kernel_name(None, M, m, True, bucket), (M, m, bucket)
            assert G.kernel_for(M, m, "table", bucket=Q) == G.kernel_for(M, m, "table")
    # everything the pipe declines goes to walk_sets_kernel: raw walks, step-major order, a plain first hop, replayed positions,
    # seven hops, M = 257
    for kw in (dict(emit_walks=True), dict(order="step"), dict(first_hop_wo=False), dict(walk_pos=True)):
        assert G.kernel_for(100, 3, **kw) == "walk_sets_kernel", kw
    assert G.kernel_for(100, 7) == G.kernel_for(257, 2) == "walk_sets_kernel" and G.kernel_for(256, 2) == "walk_pipe_kernel"
    assert G.kernel_for(100, 3, "table", walk_pos=True) == "walk_sets_kernel<SPG>" and G.kernel_for(100, 3, "table") == "walk_rows_kernel"
    assert G.kernel_for(100, 3, "table", emit_walks=True).startswith("refused")
    assert G.kernel_for(255, 9) == "refused: key width" and G.kernel_for(205, 4, "table") == "refused: LDS"


def test_table_pairs_fall_on_both_sides_of_every_doubling():
    """A: Q = 51|52 .. 819|820 -- the full side has want == T exactly, the other one the next power of two; raw walks send every one
    of them to walk_sets_kernel; the full tree (one hop: the star) has exactly Q members under both RNGs, and roots of one and two
    members stand beside it; at a full table linear probing steps from the last slot to the first"""
    wraps = []
    for (a, b_), T in zip(G.TABLE_PAIRS, (64, 128, 256, 512, 1024)):
        Qa, Qb = a[0] * a[1] + 1, b_[0] * b_[1] + 1
        assert Qb == Qa + 1 and Qa + Qa // 4 + 1 == T == G.table_size_for(Qa) and G.table_size_for(Qb) == 2 * T
        assert max(a[1], b_[1]) >= 2
        for M, m in (a, b_):
            assert G.kernel_for(M, m, emit_walks=True) == "walk_sets_kernel" and not G.needs_attribute(M, m)
            g = G.edge_graph(M, m)
            for rng in G.RNGS:
                ref, sets = _sets(g, g["batch"], M, m, rng)
                assert ref["nsize"][g["rows"]["full"][0]] == M * m + 1, (M, m, rng)
                assert sorted(ref["nsize"][g["rows"]["self_loop"]].tolist()) == [1, 2, 2] and ref["nsize"][g["rows"]["isolated"][0]] == 1
            if (M, m) == a:
                wraps.append(G.probe_wraps(sets[g["rows"]["full"][0]], T))
    # shapes that need no raw walks to stay out of the pipe: seven hops, M > 256
    assert [G.kernel_for(M, m) for M, m in ((29, 7), (409, 1), (409, 2), (273, 3))] == ["walk_sets_kernel"] * 4
    print("probes from the last slot to slot 0 in the full tables:", wraps)
    assert all(w >= 1 for w in wraps), wraps


def test_bitmap_pairs():
    """A: Q = 32|33 and 64|65 -- one bitmap word more on the far side; the full set carries every first-visit number up to Q - 1, so
    31, 32 (and 33 at Q = 65) are all present"""
    for (a, b_), words in zip(G.BITMAP_PAIRS, (1, 2)):
        for (M, m), nw in ((a, words), (b_, words + 1)):
            Q = M * m + 1
            assert (Q + 31) // 32 == nw and G.kernel_for(M, m, emit_walks=True) == "walk_sets_kernel"
            g = G.edge_graph(M, m)
            ref, _ = _sets(g, g["batch"], M, m, "philox")
            assert ref["nsize"][g["rows"]["full"][0]] == Q        # Q distinct members: visit numbers 0 .. Q - 1 are all first visits
    assert G.BITMAP_PAIRS[1][1][0] * G.BITMAP_PAIRS[1][1][1] + 1 == 65


def test_walk_loop_trips_and_first_hops():
    """A: M = 255|256|257 and 511|512|513 -- one, two and three trips of `for (w = tid; w < M; w += 256)`; the ladder holds roots of
    degree M - 1, M (the last modulo pick), M + 1 (the first shuffled one) and 2M"""
    assert [-(-M // 256) for M, _ in G.TRIP_SHAPES] == [1, 1, 2, 2, 2, 3]
    for M, m in G.TRIP_SHAPES:
        g = G.edge_graph(M, m)
        degs = g["degrees"]
        assert {M - 1, M, M + 1, 2 * M} <= set(degs.tolist())
        assert np.array_equal(W.out_degree(g, g["roots"]["ladder"]), degs)
        assert [W.first_hop(d, M) for d in (0, M - 1, M, M + 1, 2 * M)] == ["isolated", "modulo", "modulo", "shuffled", "shuffled"]
        assert G.kernel_for(M, m, emit_walks=True) == "walk_sets_kernel"
        assert (G.kernel_for(M, m) == "walk_pipe_kernel") == (M <= 256)


def test_dynamic_lds_edges_and_the_two_refusals():
    """A: the largest shape of a 2,048-slot table stays below 64 KiB, the smallest 4,096-slot shape needs the attribute, an 8,192-slot
    shape fits 160 KiB.  Refused before anything is launched, through the C ABI with dummy pointers: the smallest Q whose table has
    16,384 slots, and the largest 8,192-slot shape -- its tables alone would fit, the 4 * M bytes of Fisher-Yates draws do not"""
    from surel_plus_amd import _lib
    (Ma, ma), (Mb, mb), (Mc, mc) = G.LDS_SHAPES
    assert G.lds_edge_shapes() == (Ma, ma)
    assert G.table_size_for(Ma * ma + 1) == 2048 and G.table_size_for(Ma * ma + 2) == 4096 and not G.needs_attribute(Ma, ma)
    assert Mb * mb + 1 == Ma * ma + 2 and G.needs_attribute(Mb, mb) and G.kernel_for(Mb, mb) == "walk_sets_kernel"
    assert G.table_size_for(Mc * mc + 1) == 8192 and 64 * 1024 < G.lds_of(Mc, mc) <= G.LDS_BYTES and G.kernel_for(Mc, mc) == "walk_sets_kernel"
    print("LDS bytes:", [G.lds_of(M, m) for M, m in G.LDS_SHAPES])
    _lib.build()
    L = _lib.lib()
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)

    def sets(M, m):
        cfg = _lib.WalkCfg(M, m, -1, _lib.RNG_PHILOX, 111413, 1, _lib.ORDER_WALK_MAJOR, 1, 0, 0, None, 0, 0, None, 0)
        return L.subgacc_walk_sets(C.byref(cfg), here, here, 10, here, 4, None, None, here, here, here, None, here, None)

    assert G.table_size_for(6553) == 8192 and G.table_size_for(6554) == 16384
    assert G.kernel_for(6553, 1) == "refused: LDS" and sets(6553, 1) == _lib.ERR_LDS and b"LDS" in L.subgacc_last_error()
    Q = 6553
    assert G.lds_of(6552, 1) > G.LDS_BYTES >= G.lds_of(6552, 1) - 4 * 6552 and G.lds_of(3276, 2) <= G.LDS_BYTES
    assert G.kernel_for(6552, 1) == "refused: LDS" and G.kernel_for(3276, 2) == "walk_sets_kernel" and 3276 * 2 + 1 == Q
    assert sets(6552, 1) == _lib.ERR_LDS and b"per-root tables need" in L.subgacc_last_error()
    with pytest.raises(ValueError):
        _lib.check(sets(6552, 1))


def test_bucket_cases():
    """A: the buckets around a set of known size and around Q: nsize = min(ns, bucket), flags[1] = the roots cut"""
    M, m = G.BUCKET_SHAPE
    Q = M * m + 1
    g = G.edge_graph(M, m)
    row = g["rows"]["short5"][0]
    full, _ = _sets(g, g["batch"], M, m, "philox")
    ns = int(full["nsize"][row])
    assert ns == Q - 5 and G.buckets_for(Q, ns) == [1, 2, ns - 1, ns, ns + 1, Q - 1, Q, Q + 1]
    for bucket in G.buckets_for(Q, ns):
        assert G.kernel_for(M, m, bucket=bucket, emit_walks=True) == "walk_sets_kernel" and G.kernel_for(M, m, bucket=bucket) == "walk_pipe_kernel"
        ref, sets = _sets(g, g["batch"], M, m, "philox", bucket)
        assert np.array_equal(ref["nsize"], np.minimum(full["nsize"], bucket))
        assert np.array_equal(sets[row], full["ids"][full["off"][row]: full["off"][row] + min(ns, bucket)])
        assert (int((full["nsize"] > bucket).sum()) > 0) == (bucket < Q)


def test_orders_differ_and_the_recount_is_the_oracle():
    """A: on the dense graph the walk-major and the step-major first-visit orders of a root differ; the plain-Python recount of the
    oracle's raw walks gives oracle.gset_sampler's sets walk-major and oracle.walk_sampler's step-major, under both RNGs -- the
    recount is what the GPU file checks emitted walks with"""
    M, m = G.ORDER_SHAPE
    g = G.dense_graph(40, 4, 1)
    q = g["batch"]
    for rng in G.RNGS:
        ref = G.reference(g, q, M, m, rng, SEED)
        wr = G.walk_reference(g, q, M, m, rng, SEED)
        ns, ids, keys, _ = G.recount(wr["walks"], M, m, "walk")
        assert np.array_equal(ns, ref["nsize"]) and np.array_equal(ids, ref["ids"]) and np.array_equal(keys, ref["keys"]), rng
        ns2, ids2, keys2, _ = G.recount(wr["walks"], M, m, "step")
        assert np.array_equal(ns2, wr["nsize"]) and np.array_equal(ids2, wr["ids"]) and np.array_equal(keys2, wr["keys"]), rng
        assert np.array_equal(ns, ns2) and not np.array_equal(ids, ids2), "the two orders agree on this graph"
        for bucket in (3, 7):
            rb = G.reference(g, q, M, m, rng, SEED, bucket)
            nb, ib, kb, tot = G.recount(wr["walks"], M, m, "walk", bucket)
            assert np.array_equal(nb, rb["nsize"]) and np.array_equal(ib, rb["ids"]) and np.array_equal(kb, rb["keys"])
        plain = G.walk_reference(g, q, M, m, rng, SEED, first_hop_wo=False)
        assert not np.array_equal(plain["walks"], wr["walks"])
    assert G.kernel_for(M, m, order="step", emit_walks=True) == G.kernel_for(M, m, first_hop_wo=False) == "walk_sets_kernel"


def test_dead_end_and_root_cases():
    """A: replayed positions and every kind of root go where they are meant to"""
    for M, m in G.DEAD_SHAPES:
        g = W.dead_ends(M, m)
        assert G.kernel_for(M, m, walk_pos=True) == "walk_sets_kernel" and (np.diff(g["indptr"]) == 0).sum() >= 400
    assert [G.kernel_for(M, m) for M, m in G.ROOT_SHAPES] == ["walk_sets_kernel", "walk_pipe_kernel"]
    for M, m in G.ROOT_SHAPES:
        g = G.edge_graph(M, m)
        N = g["num_nodes"]
        assert {0, N - 1} <= set(g["batch"].tolist()) and W.out_degree(g, g["roots"]["isolated"])[0] == 0
        assert G.in_graph([-1, N, G.INT32_MAX, G.NO_ROOT, 0, N - 1], N).tolist() == [False] * 4 + [True] * 2
        a = g["roots"]["self_loop"][0]
        assert g["indices"][g["indptr"][a]: g["indptr"][a + 1]].tolist() == [a]


# ------------------------------------------------------------------------------------------------------- B. the SPG epilogue
def test_spg_shapes_reach_both_forms_of_the_epilogue():
    """B: every shape goes to walk_sets_kernel<SPG>; without a bucket nothing is ranked and the fold table lies over inv, a truncating
    bucket ranks; level-1 geometry from one member up to B = min(T / 4, 256); staged on both sides at T = 1,024 and, with a
    bucket, at T = 256"""
    seen = set()
    for M, m in G.SPG_SHAPES:
        assert G.kernel_for(M, m, "table") == "walk_sets_kernel<SPG>", (M, m)
        assert G.lds_of(M, m, True) <= 64 * 1024 and G.lds_of(M, m, True, 2) <= 64 * 1024
        g = G.edge_graph(M, m, crowd=(M, m) == G.CROWD_SHAPE)
        ref, sets = _sets(g, g["batch"], M, m, "philox")
        eps = [G.spg_epilogue(s, M, m) for s in sets]
        assert not any(e["ranked"] for e in eps)
        small = [eps[r] for r in g["rows"]["small"]]
        assert [e["ns"] for e in small] == g["small"] and (small[0]["B"], small[0]["bshift"]) == (1, 0)
        assert [e["B"] for e in small[:5]] == [1, 2, 4, 4, 8][: len(small)]
        fe = eps[g["rows"]["full"][0]]
        assert fe["ns"] == M * m + 1 and fe["B"] == min(fe["T"] // 4, 256)
        seen.add((fe["T"], fe["B"], fe["staged"]))
        for r in g["rows"]["run"]:                      # consecutive ids at 0 and at N - 1: one id per bucket where B reaches ns
            assert eps[r]["ns"] == min(M + 1, W.RUN) and (eps[r]["bshift"] == 0) == (eps[r]["B"] >= eps[r]["ns"])
        assert sets[g["rows"]["run"][0]].min() == 0 and sets[g["rows"]["run"][1]].max() == g["num_nodes"] - 1
    print("full sets (T, B, staged):", sorted(seen))
    assert {(1024, 256, True), (1024, 256, False), (256, 64, True), (64, 16, False)} <= seen
    (Ma, ma), (Mb, mb) = G.STAGED_PAIR
    assert (Ma * ma + 1, Mb * mb + 1) == G.staged_edge(1024) == (682, 683)
    M, m = G.STAGED_BUCKET
    lo, hi = G.staged_edge(256)
    assert (lo, hi) == (170, 171) and hi < M * m + 1
    g = G.edge_graph(M, m)
    for bucket, st in ((lo, True), (hi, False)):
        assert G.kernel_for(M, m, "table", bucket=bucket) == "walk_sets_kernel<SPG>"
        ref, sets = _sets(g, g["batch"], M, m, "philox", bucket)
        e = G.spg_epilogue(sets[g["rows"]["full"][0]], M, m, bucket)
        assert e["ranked"] and e["staged"] == st and e["ns"] == bucket


def test_crowded_sets_admit_level_two():
    """B: 12 | 13 | 24 members in one level-1 bucket: level 1 alone, level 2, level 2 with a crowded part"""
    M, m = G.CROWD_SHAPE
    g = G.edge_graph(M, m, crowd=True)
    ref, sets = _sets(g, g["batch"], M, m, "philox")
    eps = [G.spg_epilogue(sets[r], M, m) for r in g["rows"]["crowded"]]
    assert [e["maxc"] for e in eps] == list(W.CROWD) and [e["level2"] for e in eps] == [False, True, True]
    assert [e["ns"] for e in eps] == [W.SPREAD + k + 1 for k in W.CROWD]


def test_conditions_of_the_spg_epilogue_no_shape_reaches():
    """B: level 2 is admitted by maxc > kFineAbove && W2 <= CW * kWalkThreads && W2 <= T / 2 - 2.  The fused form is refused above a
    1,024-slot table (Q <= 819), and for every Q it admits and every set size ns <= Q the two room checks hold: no launch makes
    either false; only maxc decides"""
    for Q in range(2, 820):
        T = G.table_size_for(Q)
        assert T <= G.SPG_PER_LANE * G.WALK_THREADS
        W2 = (Q + 2) // 2 + 1                                     # the largest W2 of the shape (ns = Q)
        assert W2 <= G.CW * G.WALK_THREADS and W2 <= T // 2 - 2, Q
    assert G.table_size_for(820) == 2048 and (819 + 2) // 2 + 1 == 411


def test_fold_table_cases():
    """B: distinct LP rows per set, from the oracle's enc: the edge graph's sets hold at most kSpgFold / 2, the dense graph's more than
    kSpgFold (keys that find no slot in 16 probes go straight to the HBM table)"""
    for M, m in G.FOLD_SHAPES:
        assert G.kernel_for(M, m, "table") == "walk_sets_kernel<SPG>"
        g = G.fold_graph(M, m)
        for rng in G.RNGS:
            ref = G.reference(g, g["batch"], M, m, rng, SEED)
            rows = [G.fold_rows(ref["keys"][ref["off"][i]: ref["off"][i + 1]]) for i in range(len(g["batch"]))]
            print(f"M = {M}, m = {m}, {rng}: distinct LP rows per set {min(rows)} .. {max(rows)}")
            assert max(rows) > G.SPG_FOLD
        e = G.edge_graph(M, m)
        ref = G.reference(e, e["batch"], M, m, "philox", SEED)
        rows = [G.fold_rows(ref["keys"][ref["off"][i]: ref["off"][i + 1]]) for i in range(len(e["batch"]))]
        assert max(rows) <= G.SPG_FOLD // 2


# --------------------------------------------------------------------------------------------------------------- C. the pipe
def test_every_pipe_instantiation_is_launched():
    """C: 6 hop counts x 2 RNGs x 2 offset widths"""
    got = {G.pipe_instantiation(m, rng, i) for M, m, rng, i in G.pipe_launches() if G.kernel_for(M, m) == "walk_pipe_kernel"}
    assert got == G.PIPE_INSTANTIATIONS and len(got) == 24
    assert [G.kernel_for(M, m) for M, m in G.PIPE_WALKS] == ["walk_pipe_kernel"] * 6 and G.kernel_for(257, 2) == "walk_sets_kernel"
    assert G.kernel_for(4, 7) == "walk_sets_kernel" and [M for M, _ in G.PIPE_WALKS] == [1, 63, 64, 65, 255, 256]


def test_grid_edges():
    """C: whatever c = 1..8 the occupancy query yields, n = 256c - 1, 256c, 256c + 1 and 2 * 256c + 1 are launched: one root short of
    the grid, exactly the grid, one workgroup with a second root, every workgroup with two roots and one with three"""
    for c in range(1, 9):
        assert {256 * c - 1, 256 * c, 256 * c + 1, 2 * 256 * c + 1} <= set(G.GRID_NS)
        assert min(256 * c, 256 * c - 1) == 256 * c - 1 and 256 * c in G.pipe_grids(256 * c + 1)
    assert {1, 2} <= set(G.GRID_NS) and max(G.GRID_NS) == 4097 and G.kernel_for(*G.GRID_SHAPE) == "walk_pipe_kernel"


def test_root_kind_transitions():
    """C: in the query of 3 * 2,048 roots every ordered pair of kinds stands at distance G = 256c for every c = 1..8 (consecutive
    roots of one workgroup), every kind is some workgroup's first and last root, and some root of the graph stands twice at
    distance G.  The kinds are what they are named: shown with the oracle (Philox: a set is a function of its root)"""
    M, m = G.GRID_SHAPE
    Q = M * m + 1
    g, pools = G.transition_graph()
    q, kind = G.transition_query()
    K = len(G.KINDS)
    assert len(q) == G.TRANSITION_ROOTS
    for c in range(1, 9):
        D = 256 * c
        pairs = set(zip(kind[:-D].tolist(), kind[D:].tolist()))
        assert len(pairs) == K * K, (c, len(pairs))
        assert set(kind[:D].tolist()) == set(range(K)) and set(kind[-D:].tolist()) == set(range(K))
        same = (q[:-D] == q[D:]) & G.in_graph(q[:-D], g["num_nodes"])
        assert same.sum() >= 5, c
    deg = np.diff(g["indptr"])
    size = {}
    for k, ids in pools.items():
        if k in ("outside", "no_root"):
            assert not G.in_graph(ids, g["num_nodes"]).any()
            continue
        ref = G.reference(g, ids, M, m, "philox", SEED)
        size[k] = ref["nsize"].tolist()
    assert set(size["full"]) == {Q} and set(size["truncated"]) == {Q - 2} and set(size["ordinary"]) == {3}
    assert set(size["dead_end"]) == {4} and size["self_loop"] == [1, 2] and set(size["isolated"]) == {1}
    assert (deg[pools["shuffled"]] > M).all() and (deg[pools["isolated"]] == 0).all() and min(size["shuffled"]) > G.TRANSITION_BUCKET
    for k in ("ordinary", "isolated", "dead_end", "self_loop"):
        assert max(size[k]) <= G.TRANSITION_BUCKET
    assert Q - 2 > G.TRANSITION_BUCKET


# ------------------------------------------------------------------------------------------------------------- D. compaction
def test_compact_cases():
    """D: n = 1, 3, 4, 5 rows (four waves to a workgroup), sizes 0, 63, 64, 65 and one set of 300 distinct keys -- more than the 256
    slots of a wave's fold table, so some go straight to the HBM table and are found again by probing"""
    sizes = set()
    for n in (1, 3, 4, 5):
        c = G.compact_case(n)
        sizes |= set(c["nsize"].tolist())
        assert len(np.unique(c["keys"][-1, :300])) == 300 > G.COMPACT_FOLD
        ids, keys, ukeys = G.compact_expected(c)
        assert len(ids) == c["row_off"][-1] == c["nsize"].sum() and len(np.unique(ukeys)) == len(ukeys) >= 300
    assert sizes == {0, 63, 64, 65, 300}

"""CPU: the shapes and graphs of tests/walk_small_edges.py reach the branches of csrc/walk_small.hip that
tests/test_gpu_walk_small_edges.py means them for -- shown with the oracle's sets and the plain-Python restatements of SmallShape, the
launcher, the hash and the wave's table.  No kernel runs here."""
import numpy as np
import pytest

import walk_rows_edges as W
import walk_small_edges as E
from surel_plus_amd import sampler


# ------------------------------------------------------------------------------------------------- the restatement and the table
def test_small_shape_is_the_header_written_out():
    """the constants of all twelve instantiations, by hand from SmallShape's text; the launcher's table against the host predicate"""
    by_hand = {  # (T, MH): (QMAX, MMAX, WPL, SPL, EPL, TSHIFT)
        (64, 1): (51, 50, 1, 1, 1, 26), (64, 2): (51, 25, 1, 1, 1, 26), (64, 3): (51, 16, 1, 1, 1, 26), (64, 4): (51, 12, 1, 1, 1, 26),
        (128, 1): (102, 101, 2, 2, 2, 25), (128, 2): (102, 50, 1, 2, 2, 25), (128, 3): (102, 33, 1, 2, 2, 25), (128, 4): (102, 25, 1, 2, 2, 25),
        (256, 1): (204, 203, 4, 4, 4, 24), (256, 2): (204, 101, 2, 4, 4, 24), (256, 3): (204, 67, 2, 4, 4, 24), (256, 4): (204, 50, 1, 4, 4, 24),
    }
    seen = set()
    for m in range(1, 5):
        for M in range(1, 204):
            if not sampler.small_rows_form(M, m):
                assert M * m + 1 > E.MAX_Q
                continue
            s = E.small_shape(M, m)
            seen.add((s["T"], s["MH"]))
            assert tuple(s[k] for k in ("QMAX", "MMAX", "WPL", "SPL", "EPL", "TSHIFT")) == by_hand[(s["T"], m)], (M, m)
            assert s["T"] == W.table_size_for(M * m + 1) and 1 << (32 - s["TSHIFT"]) == s["T"]       # the hash fills the table exactly
            assert s["shift"] == int(M).bit_length() and s["bits"] == m * s["shift"] + 1 <= 25
            assert M <= s["WPL"] * E.WAVE and M * m + 1 <= s["EPL"] * E.WAVE and M * m + 1 < s["T"]
    assert seen == set(by_hand)
    with pytest.raises(AssertionError):
        E.small_shape(204, 1)
    assert E.small_shape(32, 4)["bits"] == 25 and E.small_shape(203, 1)["bits"] == 9                 # the widest key, the widest field


def test_the_shape_table_covers_every_instantiation_lane_boundary_and_key_shift():
    pairs = {(E.small_shape(M, m)["T"], m) for M, m in E.SHAPES}
    assert pairs == {(T, MH) for T in (64, 128, 256) for MH in (1, 2, 3, 4)}
    for T, shapes in E.INSTANTIATIONS.items():
        for MH in (1, 2, 3, 4):
            Ms = sorted(M for M, m in shapes if m == MH)
            assert len(Ms) == 2 and all(E.small_shape(M, MH)["T"] == T for M in Ms)
            # both ends of the instantiation's range of M: one walk less or more is another table (or no small shape at all)
            lo, hi = Ms
            assert lo == 1 or E.small_shape(lo - 1, MH)["T"] < T
            assert hi * MH + 1 + MH > E.MAX_Q or E.small_shape(hi + 1, MH)["T"] > T
    Ms = {M for M, _ in E.SHAPES}
    assert set(E.LANE_MS) <= Ms and set(E.SHIFT_MS) <= Ms
    lanes = [s for v in E.LANES.values() for s in v]
    assert {M for M, _ in lanes} == set(E.LANE_MS)
    assert (E.small_shape(63, 1)["T"], E.small_shape(63, 1)["WPL"]) == (128, 2) and E.small_shape(127, 1)["WPL"] == 4
    assert all(E.small_shape(M, m)["T"] == 256 and E.small_shape(M, m)["WPL"] == 2 for M, m in E.LANES["T = 256"])
    # a key shift turns where M gains a bit
    shifts = {M: E.small_shape(M, m)["shift"] for M, m in E.SHAPES}
    for a, b in ((1, 2), (3, 4), (7, 8), (15, 16), (31, 32), (127, 128)):
        assert shifts[b] == shifts[a] + 1
    assert shifts[2] == shifts[3] == 2
    assert max(E.small_shape(M, m)["bits"] for M, m in E.SHAPES) == 25 == E.small_shape(32, 4)["bits"]
    print(sorted(pairs), sorted(Ms & set(E.LANE_MS)), sorted(Ms & set(E.SHIFT_MS)))


def test_lane_boundaries_turn_the_trace_back():
    """`if (k2 * kWave >= M) continue` and `min(kWave, M - k2 * kWave)`: the blocks and trips on either side of 64, 128 and 192 walks"""
    tb = lambda M, m: E.traceback_blocks(M, E.small_shape(M, m)["WPL"])      # noqa: E731
    assert [tb(M, 1) for M in (63, 64, 65)] == [[(0, 63)], [(0, 64)], [(1, 1), (0, 64)]]              # WPL 2: the block of 63 skipped
    for m in (2, 3):
        assert [tb(M, m) for M in (63, 64, 65)] == [[(0, 63)], [(0, 64)], [(1, 1), (0, 64)]]
    assert [tb(M, 1) for M in (127, 128, 129)] == [[(1, 63), (0, 64)], [(1, 64), (0, 64)], [(2, 1), (1, 64), (0, 64)]]
    assert [tb(M, 1) for M in (191, 192, 193)] == [[(2, 63), (1, 64), (0, 64)], [(2, 64), (1, 64), (0, 64)], [(3, 1), (2, 64), (1, 64), (0, 64)]]
    for M, m in E.SHAPES:
        s = E.small_shape(M, m)
        blocks = E.traceback_blocks(M, s["WPL"])
        assert sum(t for _, t in blocks) == M and len(blocks) == (M + 63) // 64 <= s["WPL"]


# -------------------------------------------------------------------------------------------------------- the hash and the table
def test_the_hash_against_a_plain_loop():
    ids = np.concatenate([np.arange(3000), np.random.default_rng(0).integers(0, 2 ** 31, 3000), [2 ** 31 - 1, W.N_IDS - 1]])
    for T, tshift in ((64, 26), (128, 25), (256, 24)):
        plain = [((int(i) * 2654435761) % 2 ** 32) >> tshift for i in ids]
        assert E.home(ids, T).tolist() == plain and 0 <= min(plain) and max(plain) == T - 1
    # how many ids below 2^20 the hash sends to the last slot
    assert [len(E.ids_with_home(T, T - 1)) for T in (64, 128, 256)] == [16384, 8191, 4096]


def test_the_table_model_against_a_plain_loop():
    """insert-or-find with linear probing over random ids with repeats: every id ends in the first slot at or behind its home that the
    ids before it left free, an id seen again is found where it was put, nothing is lost"""
    rng = np.random.default_rng(1)
    for T in (64, 128, 256):
        ids = rng.integers(0, W.N_IDS, 3 * T // 4)
        visits = np.concatenate([ids[1:], ids[1: T // 4]])
        keys, placed = E.table_model(T, ids[0], visits)
        slot_of = {int(ids[0]): int(E.home(ids[0], T))}
        for v, (h, path) in zip(visits.tolist(), placed):
            if v in slot_of:
                assert h == slot_of[v]
            else:
                want = int(E.home(v, T))
                while want in slot_of.values():
                    want = (want + 1) % T
                assert h == want
                slot_of[v] = h
            assert path == [(int(E.home(v, T)) + i) % T for i in range(len(path))] and (not path or (path[-1] + 1) % T == h)
        assert {k: keys.index(k) for k in keys if k != -1} == slot_of


@pytest.mark.parametrize("M,m", E.CLUSTER_SHAPES)
def test_cluster_chains_wrap_and_step_over_the_root(M, m):
    g = E.cluster_graph(M, m)
    T = g["T"]
    assert T == E.small_shape(M, m)["T"] and len(g["batch"]) == 13 and g["rows"]["cluster"].tolist() == [0, 1, 2]
    homes = []
    for r in g["roots"]["cluster"]:
        nb = g["indices"][g["indptr"][r]: g["indptr"][r + 1]]
        assert len(nb) == M and len(set(nb.tolist())) == M and set(E.home(nb, T).tolist()) == {T - 2}
        nxt = [g["indices"][g["indptr"][v]: g["indptr"][v + 1]] for v in nb]
        assert all(len(x) == 1 for x in nxt) and [int(x[0]) for x in nxt] == np.roll(nb, -1).tolist()      # a cycle: the set is closed
        hr = int(E.home(r, T))
        homes.append(hr)
        # hop 1 in walk order (any order fills the same slots: the homes are equal); the later hops only find
        visits = np.concatenate([np.roll(nb, -s) for s in range(m)])
        keys, placed = E.table_model(T, r, visits)
        assert sum(k != -1 for k in keys) == M + 1
        paths = [p + [h] for h, p in placed]
        assert any((a, b) == (T - 1, 0) for p in paths for a, b in zip(p, p[1:])), "no chain wraps from slot T - 1 to slot 0"
        assert any(hr in p[:-1] for p in paths), "no chain steps over the root's slot"
        assert max(len(p) - 1 for p in paths) >= M
        assert {i for i, k in enumerate(keys) if k != -1} == {(T - 2 + i) % T for i in range(M + 1)}      # one run, the root inside it
    assert homes == [1, T - 1, T - 2]
    for rng in E.RNGS:
        exp = E.rows("cluster", M, m, rng)
        assert (exp["nsize"] == M + 1).all()


# ---------------------------------------------------------------------------------------------------- the graphs reach their branch
@pytest.mark.parametrize("M,m", E.SHAPES)
def test_edge_graph_at_every_shape(M, m):
    """the root degrees on every side of the first hop's branches, a set of exactly Q members, every residue of ns % 4 (the ranking's
    sentinel padding), in both RNGs"""
    g, Q = E.graph("edge", M, m), M * m + 1
    degs = set(W.out_degree(g, g["batch"]).tolist())
    assert {0, 1, M - 1, M, M + 1, 2 * M} <= degs
    assert {W.first_hop(d, M) for d in degs} == {"isolated", "modulo", "shuffled"}
    assert len(np.unique(g["batch"])) < len(g["batch"]) < 400
    for rng in E.RNGS:
        ns = E.rows("edge", M, m, rng)["nsize"]
        assert int(ns.max()) == Q and int(ns.min()) == 1
        if Q >= 5:      # with the rows of sizes_graph: the edge graph alone lacks a residue at (1, 4) and (3, 4)
            more = E.rows("sizes", M, m, rng)["nsize"]
            assert int(more.max()) <= Q and set((np.concatenate([ns, more]) % 4).tolist()) == {0, 1, 2, 3}
            trimmed = min(3, M - 1) if m >= 2 else 0
            assert more.tolist() == [Q - k for k in range(1, trimmed + 1)] + [min(m, 2) + 1, min(m, 3) + 1]
        # the shuffled roots' sets: the trace-back ran (degree M + 1: M draws over M + 1 values, the densest it meets here)
        assert ns[g["rows"]["tree_shuffled"][0]] == Q


@pytest.mark.parametrize("M,m", E.LADDER_SHAPES)
def test_ladder_all(M, m):
    g = E.ladder_graph(M, m)
    deg = W.out_degree(g, g["batch"])
    assert deg.tolist() == list(range(1, M + 9)) == g["degrees"].tolist()
    assert [W.first_hop(int(d), M) for d in deg] == ["modulo"] * M + ["shuffled"] * 8
    d_all = np.diff(g["indptr"])
    assert (d_all[np.unique(g["indices"])] > 0).all()                            # no dead ends: both RNGs run it
    for rng in E.RNGS:
        ns = E.rows("ladder", M, m, rng)["nsize"]
        if m == 1:                                                               # distinct neighbours: min(deg, M) of them and the root
            assert ns.tolist() == [min(int(d), M) + 1 for d in deg]


def test_the_reciprocal_is_exact_at_every_degree():
    """w - ((w * inv) >> 16) * deg == w % deg for every walk w < 256 and every degree the modulo branch can meet"""
    assert all(W.reciprocal_is_exact(d) for d in range(1, 257))
    w = np.arange(256)
    for d in range(1, 257):
        inv = 65535 // d + 1
        assert np.array_equal(w - ((w * inv) >> 16) * d, w % d)


@pytest.mark.parametrize("M,m", E.DEAD_SHAPES + (E.DEAD_ONE_HOP,))
def test_dead_ends(M, m):
    """walks stand on a node without out-edges with a hop left (m >= 2) -- and never with one hop"""
    import oracle
    g = E.graph("dead", M, m)
    d = np.diff(g["indptr"])
    N = g["num_nodes"]
    assert g["roots"]["owner"][0] == N - 401 and g["indptr"][N - 401] + d[N - 401] == len(g["indices"])
    nsize, remap, enc, raw = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=E.SEED,
                                                 rng="philox", debug=True)
    off = np.concatenate([[0], np.cumsum(nsize)])
    dead = d[remap[0]] == 0
    stayed = dead & (raw[:, 1:m].sum(axis=1) > 0)                                # landed on a dead end before the last hop
    if m == 1:
        assert not stayed.any() and dead.any()
    else:
        assert stayed.any()
        for s, r in zip(range(1, m), g["rows"]["stops"]):
            assert nsize[r] == 1 + 7 * (s + 1) and raw[off[r]: off[r + 1]][:, s + 1:].sum() == (m - s) * M
    assert (nsize[g["rows"]["dead"]] == 1).all() and 200 <= len(g["batch"]) <= 210


def test_hub_cap():
    g = E.graph("hub", 50, 1)
    deg = W.out_degree(g, g["batch"])
    assert deg.tolist()[:3] == [W.NEIGH_CAP, W.NEIGH_CAP + 1, 1]
    for M, m in E.HUB_SHAPES:
        assert [W.first_hop(int(x), M) for x in deg[:3]] == ["shuffled", "capped", "modulo"]
        for rng in E.RNGS:
            assert int(E.rows("hub", M, m, rng)["nsize"].max()) == M * m + 1      # 51, 201 and 49 members


@pytest.mark.parametrize("M,m", E.SYM_SHAPES)
def test_symmetric_version(M, m):
    g, d = E.graph("sym", M, m), E.graph("edge", M, m)
    deg = np.diff(g["indptr"])
    assert np.array_equal(g["batch"], d["batch"]) and deg[g["roots"]["self_loop"]].tolist() == [0, 1, 1]
    assert (deg[np.unique(g["indices"])] > 0).all()
    assert int(deg[np.unique(g["indices"])].max()) >= 255                        # hubs among the reached nodes


@pytest.mark.parametrize("M,m", E.LAST_SHAPES)
def test_last_node_graph(M, m):
    g = E.graph("last", M, m)
    N = g["num_nodes"]
    assert g["batch"][0] == g["batch"][-1] == N - 1 and g["batch"][1] == N - 2
    assert g["indptr"][N] - g["indptr"][N - 1] == M + 2 and g["indices"][-1] != N - 1 and (g["indices"] == N - 1).sum() == 10
    ns = E.rows("last", M, m, "philox")["nsize"]
    assert ns[1] == 1 and ns[0] > 1


def test_isolated_graph():
    g = E.isolated_graph()
    assert not g["indptr"].any() and len(g["indices"]) == 1 and len(g["batch"]) > 2 * E.WAVES
    for M, m in E.ISOLATED_SHAPES:
        s = E.small_shape(M, m)
        key = (1 << (m * s["shift"])) | sum(M << (j * s["shift"]) for j in range(m))
        for rng in E.RNGS:
            exp = E.rows("isolated", M, m, rng)
            assert (exp["nsize"] == 1).all() and np.array_equal(exp["ids"], g["batch"]) and (exp["keys"] == key).all()


# ------------------------------------------------------------------------------------------------ every case's reference is usable
@pytest.mark.parametrize("kind,M,m", E.CASES)
def test_the_oracle_keys_are_unique_and_fit_the_key(kind, M, m):
    import oracle
    g = E.graph(kind, M, m)
    bits = E.small_shape(M, m)["bits"]
    assert g["num_nodes"] <= 2 ** 21 and int(g["batch"].min()) >= 0 and int(g["batch"].max()) < g["num_nodes"]
    for rng in E.RNGS:
        _, _, enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=E.SEED, rng=rng)
        ukeys = W.lp_keys(enc, M, m)
        assert len(np.unique(ukeys)) == len(ukeys) and int(ukeys.max()) < 1 << bits <= 1 << 25
        exp = E.rows(kind, M, m, rng)
        assert 1 <= int(exp["nsize"].min()) and int(exp["nsize"].max()) <= M * m + 1
        assert (np.diff(exp["ids"])[np.diff(np.repeat(np.arange(len(exp["nsize"])), exp["nsize"])) == 0] > 0).all()     # ascending, distinct

"""CPU: the shapes and graphs of tests/walk_rows_edges.py reach the branches of csrc/walk_rows.hip that tests/test_gpu_walk_rows_edges.py
means them for -- shown with the oracle's sets and the plain-Python restatements of the launcher and the epilogues.  No kernel runs
here."""
import numpy as np
import pytest

import walk_rows_edges as W
from surel_plus_amd import sampler


def _all_launches():
    """(idx64, rng, instantiation) of every launch of the GPU file's parametrisation"""
    out = set()
    for m, M in W.SHAPES:
        for form, idx64, rec in W.launches(M, m):
            tup = W.variant(M, m, form, idx64, bool(rec))
            assert tup is not None, (M, m, form)
            for rng in ("rand_r", "philox"):
                out.add((idx64, rng, tup))
    return out


def test_shape_table_gives_the_instantiations_written_next_to_it():
    assert set(W.SHAPE_TABLE) == set(W.SHAPES)
    for (m, M), forms in W.SHAPE_TABLE.items():
        assert set(forms) | ({"tags"} if "keys32" in forms else set()) == set(W.forms_of(M, m))
        for form, tup in forms.items():
            assert W.variant(M, m, form) == tup, (M, m, form)
        assert W.variant(M, m, "tags") == (forms["table"] if "keys32" in forms else W.variant(M, m, "tags"))
    Q = {(m, M): M * m + 1 for m, M in W.SHAPES + W.GENERAL + (W.REFUSED,)}
    assert sorted(Q[s] for s in W.SHAPES) == [205, 205, 205, 409, 409, 409, 411, 412, 413, 509, 513, 513, 640, 643, 682, 685, 769, 817]
    assert [Q[s] for s in W.GENERAL[:2]] == [203, 202] and Q[W.REFUSED] == 821
    # the table edges: 256 | 512 at Q = 205, 512 | 1,024 at 410, 1,024 | 2,048 at 820
    assert [W.table_size_for(q) for q in (203, 204, 205, 409, 410, 411, 412, 413, 817, 819, 820, 821)] == \
        [256, 256, 512, 512, 1024, 1024, 1024, 1024, 1024, 1024, 2048, 2048]
    # 29 | 33 bits at M = 127 | 128, four hops
    assert (W.key_bits(127, 4), W.key_bits(128, 4)) == (29, 33)
    assert "keys32" in W.SHAPE_TABLE[(4, 127)] and "keys64" in W.SHAPE_TABLE[(4, 128)]
    # EPLP of the key rows at stride 640 | 643, of nothing else at three hops
    assert (W.variant(213, 3, "keys32")[6], W.variant(214, 3, "keys32")[6]) == (5, 0)
    # 12 * stride <= 8 * T of the 32-bit-count table form at stride 682 | 685
    assert 12 * 682 <= 8 * 1024 < 12 * 685 and W.variant(227, 3, "table") == W.variant(228, 3, "table") == (3, 8, 128, 0, True, False, 0)


def test_key_rows_ask_for_lds_a_launch_gets_without_an_attribute():
    """launch_walk_rows sets no hipFuncAttributeMaxDynamicSharedMemorySize: what it asks for (kr_red_offset + the reduction words for
    key rows, walk_lds_bytes for the table form) stays below 64 KiB at every served shape, the largest included"""
    for M in range(1, 257):
        for m in (2, 3, 4):
            Q = M * m + 1
            for form in ("keys32", "keys64"):
                for idx64 in (False, True):
                    tup = W.variant(M, m, form, idx64)
                    if tup:
                        assert W.kr_red_offset(tup[1] * tup[2], M, Q, tup[2], not tup[4]) + 64 + 16 <= 64 * 1024
                        assert (Q + 2) // 2 + 1 <= 4 * tup[2] and Q <= (tup[6] or (7 if tup[1:3] == (8, 64) else tup[1])) * tup[2]
            if W.variant(M, m, "table"):
                assert W.walk_lds_bytes(W.table_size_for(Q), (Q + 31) // 32, M, Q, True, False) <= 64 * 1024
    assert W.kr_red_offset(1024, 204, 817, 128, True) == 817 * 16 + 132 * 4 + 512 * 4       # the sort outgrows the walk tables
    assert W.kr_red_offset(512, 102, 205, 64, False) == 512 * 8 + 102 * 4 + 8               # ... and here it does not


def test_dispatch_neighbours():
    for m, M in W.GENERAL:
        assert W.variant(M, m, "table") is None and W.outcome(M, m, "table") == "walk_sets_kernel<SPG>"
        assert W.outcome(M, m, "tags").startswith("refused") and W.outcome(M, m, "keys32").startswith("refused")
    assert W.outcome(200, 3, "table", bucket=50) == "walk_sets_kernel<SPG>" and W.variant(200, 3, "table", bucket=50) is None
    # (a bucket of exactly M * m + 1 truncates nothing: the launcher keeps the fused-row kernel, the host predicate says "general" --
    #  it only ever errs towards not handing a work list over)
    assert W.outcome(200, 3, "table", bucket=601) == "walk_rows_kernel" and not sampler.rows_kernel_takes(200, 3, 601)
    m, M = W.REFUSED
    assert all(W.outcome(M, m, f) == "refused: LDS" for f in ("table", "tags", "keys64"))
    assert W.outcome(204, 4, "keys32") == "refused: key rows" and W.outcome(127, 4, "keys64") == "refused: walk_keyrows64"
    assert W.outcome(255, 9, "table").startswith("refused: key width")


def test_variant_agrees_with_the_host_predicates():
    """rows_kernel_takes, key_rows_form and walk_kernel_name over every M in 1 .. 300 and m in 1 .. 6"""
    for M in range(1, 301):
        for m in range(1, 7):
            for bucket in (-1, 50):
                takes = sampler.rows_kernel_takes(M, m, bucket)
                for idx64 in (False, True):
                    for rec in (False, True):
                        tup = W.variant(M, m, "table", idx64, rec, bucket=bucket)
                        if M * m + 1 <= sampler.FUSED_MAX_Q or not takes:
                            assert (tup is not None) == takes, (M, m, bucket)
                        if bucket == -1 and W.outcome(M, m, "table") != "refused: LDS":
                            name = sampler.walk_kernel_name(None, M, m, True, bucket)
                            assert name == W.outcome(M, m, "table", idx64, rec), (M, m)
            kf = sampler.key_rows_form(M, m)
            for idx64 in (False, True):
                assert (W.variant(M, m, "keys32", idx64) is not None) == (kf == 32), (M, m)
                assert (W.variant(M, m, "keys64", idx64) is not None) == (kf == 64), (M, m)
            assert (M * m + 1 > sampler.FUSED_MAX_Q) == (W.table_size_for(M * m + 1) > 1024)


def test_the_gpu_launches_cover_every_reachable_instantiation():
    """brute force over every shape = the list written out in the helper = what the GPU file's parametrisation launches"""
    brute = set()
    for M in range(1, 301):
        for m in range(1, 7):
            for form in W.FORMS:
                for idx64 in (False, True):
                    for rec in (False, True):
                        tup = W.variant(M, m, form, idx64, rec)
                        if tup is not None:
                            brute.add((idx64, tup))
    assert brute == W.REACHABLE
    launched = _all_launches()
    assert {(i, t) for i, _, t in launched} == W.REACHABLE
    assert launched == {(i, r, t) for i, t in W.REACHABLE for r in ("rand_r", "philox")}
    # forms the source no longer has because no shape reaches them: EPLP = 0 of the 64-bit key rows and of the 2- and
    # 4-hop 32-bit key rows at 1,024 slots, two slots per lane x 256 lanes, 64-bit counts at 1,024 slots for 2 and 3 hops over int32
    # offsets -- an invariant of the launcher now (rows_form declines them), not only of the shapes
    assert not any(t[:3] == (4, 8, 128) and t[5] and not t[4] and t[6] == 0 for _, t in brute)
    assert not any(t[1] == 2 for _, t in brute)
    assert all(max(M * 4 + 1 for M in range(128, 205)) <= 7 * 128 for _ in (0,))


@pytest.mark.parametrize("m,M", W.SHAPES + W.GENERAL)
def test_degree_ladder_and_first_hops(m, M):
    g = W.edge_graph(M, m)
    deg = W.out_degree(g, g["roots"]["ladder"])
    assert np.array_equal(deg, g["degrees"]) and set(range(M + 3)) <= set(deg.tolist()) and {2 * M, 4 * M + 1} <= set(deg.tolist())
    hops = [W.first_hop(int(d), M) for d in deg]
    assert hops[0] == "isolated" and set(hops[1: M + 1]) == {"modulo"} and set(hops[M + 1:]) == {"shuffled"}
    assert all(W.reciprocal_is_exact(d) for d in range(1, 257))
    # the narrowest Fisher-Yates draw: degree M + 1, whose last swap k = M - 1 draws below rdeg - k == 2 (rdeg - k == 1 would take a root
    # of degree M, which is the modulo branch's); and degree M + 2
    assert M + 1 in deg and M + 2 in deg
    # no walk stands on a node without out-edges while it has hops left: reached nodes with out-degree 0 are the trees' last nodes
    d_all = np.diff(g["indptr"])
    reached = np.unique(g["indices"])
    ends = reached[d_all[reached] == 0]
    n_trees = sum(1 for k in g["roots"] if k.startswith("tree"))
    assert len(ends) <= n_trees * (M + 3)
    # a reached hub whose degree does not fit 8 bits
    assert (d_all[reached] >= 255).any()


@pytest.mark.parametrize("rng", ["rand_r", "philox"])
@pytest.mark.parametrize("m,M", W.SHAPES)
def test_sets_reach_their_branches(m, M, rng):
    g = W.edge_graph(M, m)
    exp = W.expected_rows("edge", M, m, rng)
    Q, rows = M * m + 1, g["rows"]
    ns = exp["nsize"]
    # trees: ns == Q exactly, from the modulo and from the shuffled first hop; the trimmed ones on both sides of `staged`
    assert ns[rows["tree"][0]] == Q and ns[rows["tree_shuffled"][0]] == Q
    assert W.first_hop(int(W.out_degree(g, g["roots"]["tree"])[0]), M) == "modulo"
    assert W.first_hop(int(W.out_degree(g, g["roots"]["tree_shuffled"])[0]), M) == "shuffled"
    for idx64 in (False, True):
        tup = W.variant(M, m, "table", idx64)
        T, NT, K32 = tup[1] * tup[2], tup[2], tup[4]
        edge = W.staged_edge(M, m, tup)
        if edge:
            lo, hi = (W.table_epilogue(W.row_of(exp, rows[f"tree_{e}"][0]), T, NT, K32, Q) for e in edge)
            assert (lo["ns"], hi["ns"]) == edge and lo["staged"] and not hi["staged"]
            assert not W.table_epilogue(W.row_of(exp, rows["tree"][0]), T, NT, K32, Q)["staged"]
        full = W.table_epilogue(W.row_of(exp, rows["tree"][0]), T, NT, K32, Q)
        assert full["staged"] == (Q + full["B"] + 1 <= T and (not K32 or 12 * Q <= 8 * T))
        # runs: the set is the consecutive ids, bshift == 0
        for r, base in zip(rows["run"], (0, W.N_IDS - min(M + 1, W.RUN))):
            ids = W.row_of(exp, r)
            assert np.array_equal(ids, base + np.arange(min(M + 1, W.RUN)))
            assert W.table_epilogue(ids, T, NT, K32, Q)["bshift"] == 0
        # crowded: 12 stays at level 1, 13 and 24 go to level 2
        got = [W.table_epilogue(W.row_of(exp, r), T, NT, K32, Q) for r in rows["crowded"]]
        assert [e["maxc"] for e in got] == list(W.CROWD) and [e["level2"] for e in got] == [False, True, True]
        assert [e["ns"] for e in got] == [1 + W.SPREAD + k for k in W.CROWD] and got[0]["bshift"] == 14
        for form in ("keys32", "keys64"):
            kt = W.variant(M, m, form, idx64)
            if kt is None:
                continue
            kT, kNT = kt[1] * kt[2], kt[2]
            lv = [W.key_row_levels(W.row_of(exp, r), kT, kNT) for r in rows["crowded"]]
            assert [e["levels"] for e in lv] == ([1, 2, 2] if kNT == 64 else [1, 2, 3]), lv
            assert all(W.key_row_levels(W.row_of(exp, r), kT, kNT)["bshift"] == 0 for r in rows["run"])
            assert ns.max() <= (kt[6] if kt[6] else (7 if (kNT == 64 and kt[1] == 8) else kt[1])) * kNT       # ns <= EPL * NT
    # self loops: one member through the main path; two members
    assert ns[rows["self_loop"]].tolist() == [1, 2, 2]
    assert W.out_degree(g, g["roots"]["self_loop"]).tolist() == [1, 2, 1]
    # the ladder's isolated root, and a set for every degree
    assert ns[rows["ladder"][0]] == 1 and (ns[rows["ladder"][1:]] > 1).all()
    # repeated roots: the same set under Philox (a function of seed and root)
    if rng == "philox":
        n = len(g["batch"])
        assert np.array_equal(W.row_of(exp, n - 4), W.row_of(exp, rows["ladder"][5])) and np.array_equal(W.row_of(exp, n - 1), W.row_of(exp, rows["tree"][0]))
    assert len(g["batch"]) < 400


@pytest.mark.parametrize("m,M", W.WORKLIST_SHAPES)
def test_symmetric_version(m, M):
    """the symmetrised edge graph: no self loop is left, no reached node is a dead end, the ladder keeps a root for every first hop"""
    g, d = W.symmetric_edge_graph(M, m), W.edge_graph(M, m)
    deg = np.diff(g["indptr"])
    src = np.repeat(np.arange(g["num_nodes"]), deg)
    assert not (src == g["indices"]).any() and (deg[np.unique(g["indices"])] > 0).all()
    assert np.array_equal(g["batch"], d["batch"]) and deg[g["roots"]["self_loop"]].tolist() == [0, 1, 1]
    assert {"isolated", "modulo", "shuffled"} == {W.first_hop(int(x), M) for x in deg[g["roots"]["ladder"]]} | {"isolated"}
    assert deg[g["roots"]["self_loop"][0]] == 0


def test_both_store_paths_run_at_every_shape():
    for m, M in W.SHAPES:
        Q = M * m + 1
        ps = W.pitches(Q)
        assert ps[0] == 0 and {W.wide_rows(p, Q) for p in ps} == {False, True}
        assert all(p == 0 or p > Q for p in ps) and ps[1] % 32 == 0
    assert any((M * m + 1) % 4 == 0 for m, M in W.SHAPES)                         # a default pitch that is wide by itself


@pytest.mark.parametrize("m,M", [(2, 204), (3, 256), (4, 128)])
def test_dead_ends_graph(m, M):
    import oracle
    g = W.dead_ends(M, m)
    d = np.diff(g["indptr"])
    N = g["num_nodes"]
    assert (d[N - 400:] == 0).all() and d[N - 401] > 0 and g["roots"]["owner"][0] == N - 401
    assert g["indptr"][N - 401] + d[N - 401] == len(g["indices"])                 # the owner of the last adjacency entry
    nsize, remap, enc, raw = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=13, rng="philox",
                                                 debug=True)
    off = np.concatenate([[0], np.cumsum(nsize)])
    for s, r in zip(range(1, m), g["rows"]["stops"]):                             # walks that stop after hop s: 7 chains of s nodes + a dead end
        assert nsize[r] == 1 + 7 * (s + 1)
        counts = raw[off[r]: off[r + 1]]
        assert counts[:, s + 1:].sum() == (m - s) * M and (counts[1:, s + 1:].sum(axis=1) > 0).sum() == 7      # they stay on the 7 dead ends
    assert (nsize[g["rows"]["dead"]] == 1).all()


def test_hub_cap_graph():
    g = W.hub_cap()
    deg = W.out_degree(g, g["batch"])
    assert deg.tolist()[:2] == [W.NEIGH_CAP, W.NEIGH_CAP + 1] and int((deg > W.NEIGH_CAP).sum()) == 2       # node 1, listed twice
    assert len(set(g["batch"][deg > W.NEIGH_CAP].tolist())) == 1                  # rdeg64 > kNeighCap for exactly one root
    assert [W.first_hop(int(x), 200) for x in deg[:3]] == ["shuffled", "capped", "modulo"]
    assert W.first_hop(W.NEIGH_CAP + 1, 200, cap=False) == "shuffled"
    assert g["num_nodes"] == W.HUB_NODES and len(g["batch"]) <= 8
    assert int(g["indices"].max()) < g["num_nodes"] and int(g["indices"].min()) >= 0

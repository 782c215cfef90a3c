"""GPU (MI355X): the one-wave key-row walk (csrc/walk_small.hip: walk_small_kernel behind subgacc_walk_keyrows_small) driven through
the C ABI at every edge of its instantiations, of the lanes' share of the walks, of the key's fields and of the wave's table, with the
shapes and graphs of tests/walk_small_edges.py -- tests/test_walk_small_edges_cpu.py shows on the host that every case reaches the
branch it is here for.

The reference is the oracle's sets of the same batch made into rows (ids ascending, keys from walk_rows_edges.lp_keys), computed once
per (graph, shape, rng) and shared; every comparison is bit for bit.  Every output is poisoned before the launch and stands between
two poisoned guards: the guards, the tail of every row behind its last member, the words between a row's capacity and the pitch and
every row that is not listed must come back untouched (test_gpu_walk_rows_edges._check)."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_walk_rows_edges as R
import test_gpu_walk_small as S
import walk_rows_edges as W
import walk_small_edges as E
from gpu_helpers import sp  # noqa: F401
from walk_rows_edges import POISON

pytestmark = pytest.mark.gpu

RNGS = E.RNGS
assert S.SEED == E.SEED == R.SEED


# --------------------------------------------------------------------------------------------------------------------- plumbing
@functools.lru_cache(maxsize=2)
def _csrs(kind, M, m):
    """{idx64: DeviceCSR} of one graph of walk_small_edges.graph (the edge graph: test_gpu_walk_small's own)"""
    from surel_plus_amd.sampler import DeviceCSR
    g = E.graph(kind, M, m)
    return {False: DeviceCSR(g["indptr"], g["indices"]), True: DeviceCSR(g["indptr"].astype(np.int64), g["indices"])}


def _pitches(Q):
    return (0, (Q + 31) // 32 * 32)


def _run_all(kind, M, m, rngs=RNGS, pitches=(0,), flags=(0, 0, 0, 0)):
    """the graph's batch in every RNG, with int32 and int64 row offsets, at every pitch given, against the oracle's rows"""
    g, csrs = E.graph(kind, M, m), _csrs(kind, M, m)
    out = []
    for rng in rngs:
        exp = E.rows(kind, M, m, rng)
        for idx64 in (False, True):
            for pitch in pitches:
                got = S._launch(csrs[idx64], g["batch"], M, m, rng, pitch)
                R._check(got, exp, flags=flags, what=(kind, M, m, rng, idx64, pitch))
                out.append(got)
    return out


# --------------------------------------------------------------------------------------- (a) every shape of the table, directly
@pytest.mark.parametrize("M,m", E.SHAPES)
def test_every_shape_on_its_edge_graph(sp, M, m):
    """both RNGs, int32 and int64 row offsets, pitch Q and Q rounded up to 32.  Among the rows: root degrees 0, 1, M - 1, M, M + 1 and
    2M, a set of exactly Q members and -- from Q = 5 on, with the rows of walk_small_edges.sizes_graph -- every residue of nsize % 4"""
    g, csrs, Q = S._graph(M, m), S._csrs(M, m), M * m + 1
    assert g is E.graph("edge", M, m)
    assert {0, 1, M - 1, M, M + 1, 2 * M} <= set(W.out_degree(g, g["batch"]).tolist())
    for rng in RNGS:
        exp = S._expected(M, m, rng)
        for idx64 in (False, True):
            for pitch in _pitches(Q):
                got = S._launch(csrs[idx64], g["batch"], M, m, rng, pitch)
                R._check(got, exp, what=(rng, idx64, pitch))
                ns = got["nsize"]
                assert int(ns.max()) == Q and int(ns.min()) == 1
                if Q >= 5:
                    more = S._launch(_csrs("sizes", M, m)[idx64], E.graph("sizes", M, m)["batch"], M, m, rng, pitch)
                    R._check(more, E.rows("sizes", M, m, rng), what=("sizes", rng, idx64, pitch))
                    assert set((np.concatenate([ns, more["nsize"]]) % 4).tolist()) == {0, 1, 2, 3}
    s = E.small_shape(M, m)
    print(f"M = {M}, m = {m}: walk_small_kernel<.., {s['MH']}, {s['T']}>, Q = {Q}, WPL = {s['WPL']}, key bits = {s['bits']}, "
          f"rows = {len(g['batch'])}; here for {E.SHAPE_TABLE[(M, m)]}")


# -------------------------------------------------------------------------------------------------- (b) cluster and ladder_all
@pytest.mark.parametrize("M,m", E.CLUSTER_SHAPES)
def test_sets_that_collide_in_the_table(sp, M, m):
    """three roots whose M + 1 members share one home: chains that fill slots T - 2 and T - 1, wrap to slot 0 and step over the root's
    slot, in all four tables of a workgroup at once (where a member sits shows in no row: the evidence that the chains do wrap is the
    table model of test_walk_small_edges_cpu.py; here the rows must be the oracle's and the neighbouring waves' rows their own)"""
    for got in _run_all("cluster", M, m):
        assert (got["nsize"] == M + 1).all()


@pytest.mark.parametrize("M,m", E.LADDER_SHAPES)
def test_a_root_of_every_degree(sp, M, m):
    """out-degrees 1 .. M + 8: the modulo first hop at every divisor, the trace-back with M draws over M + 1 .. M + 8 values"""
    assert W.out_degree(E.graph("ladder", M, m), E.graph("ladder", M, m)["batch"]).tolist() == list(range(1, M + 9))
    _run_all("ladder", M, m, pitches=_pitches(M * m + 1))


# ---------------------------------------------------------------------------------------------------------------- (c) dead ends
@pytest.mark.parametrize("M,m", E.DEAD_SHAPES)
def test_dead_ends(sp, M, m):
    """walks that stop after hop 1 .. m - 1, dead ends whose rows begin at nnz, the owner of the last adjacency entry as a root.  Philox:
    the oracle's rows, no flag.  rand_r: the stream is no longer the sequential one, so the kernel says so (flags[0] & 1) and stays
    inside its rows: every size in [1, Q], nothing written behind a row's members or outside the outputs"""
    g, csrs, Q = E.graph("dead", M, m), _csrs("dead", M, m), M * m + 1
    _run_all("dead", M, m, rngs=("philox",), pitches=_pitches(Q))
    for idx64 in (False, True):
        for pitch in _pitches(Q):
            got = S._launch(csrs[idx64], g["batch"], M, m, "rand_r", pitch)       # (_back has looked at the guards)
            assert got["flags"].tolist() == [1, 0, 0, 0]
            ns = got["nsize"]
            assert (ns >= 1).all() and (ns <= Q).all()
            member = np.arange(got["P"])[None, :] < ns[:, None]
            assert (got["ids"][~member] == POISON).all() and (got["pay"][~member] == POISON).all()
            assert (got["ids"][member] >= 0).all() and (got["ids"][member] < g["num_nodes"]).all() and (got["pay"][member] > 0).all()
            assert ((got["ids"] == g["batch"][:, None]) & member).sum(axis=1).tolist() == [1] * len(ns)      # the root, once
            rows_ascend = np.diff(got["ids"].astype(np.int64), axis=1) > 0
            assert (rows_ascend | ~member[:, 1:]).all()


def test_one_hop_meets_no_dead_end(sp):
    """the graph of dead ends walked with one hop: no walk has a hop left on a dead end, so rand_r too is the oracle's, flags zero"""
    M, m = E.DEAD_ONE_HOP
    assert m == 1 and E.graph("dead", M, m) is W.dead_ends(M, 2)
    _run_all("dead", M, m, pitches=_pitches(M * m + 1))


# ----------------------------------------------------------------------------------------------------------- (d) the degree cap
@pytest.mark.parametrize("M,m", E.HUB_SHAPES)
def test_root_degree_cap(sp, M, m):
    """roots of degree 1,000,000 and 1,000,001.  With cap_root_degree: the oracle's rows (the reference draws from the first 1,000,000
    neighbours).  Without it: every other root unchanged, and the root of 1,000,001 what the general kernel gives with the same
    setting -- ids, and keys through its table of distinct rows (test_gpu_walk_small.py::test_rows_equal_the_general_kernels)"""
    from surel_plus_amd import sampler
    g, csrs, Q = E.graph("hub", M, m), _csrs("hub", M, m), M * m + 1
    q = g["batch"]
    _run_all("hub", M, m)
    big = q == 1
    assert big.sum() == 2 and W.out_degree(g, q)[big].tolist() == [W.NEIGH_CAP + 1] * 2
    for rng in RNGS:
        exp = E.rows("hub", M, m, rng)
        for idx64 in (False, True):
            csr = csrs[idx64]
            got = S._launch(csr, q, M, m, rng, 0, cap_root=False)
            hide = lambda a: np.where(big if a.ndim == 1 else big[:, None], POISON, a)      # noqa: E731
            R._check(dict(got, nsize=hide(got["nsize"]), ids=hide(got["ids"]), pay=hide(got["pay"])), exp, listed=np.nonzero(~big)[0],
                     what=("uncapped, the other roots", rng, idx64))
            sets = sampler.sample_sets(csr, q, num_walks=M, num_steps=m, seed=S.SEED, rng=rng, cap_root_degree=False, fused_rows=True,
                                       strided=True, key_rows=False)
            assert sets.strided and not sets.keyrows and sets.stride == Q
            ns = sets.nsize.cpu().numpy()
            assert np.array_equal(got["nsize"], ns)
            member = np.arange(Q)[None, :] < ns[:, None]
            ids, slot = sets.ids.cpu().numpy().reshape(-1, Q), sets.slot.cpu().numpy().reshape(-1, Q)
            tkeys = sets.table[: sets.capacity * 8].view(torch.int64).cpu().numpy()
            assert np.array_equal(got["ids"][member], ids[member])
            assert np.array_equal(got["pay"][member].astype(np.int64), tkeys[slot[member]])
            assert (got["ids"][~member] == POISON).all() and (got["pay"][~member] == POISON).all()
            differs = False
            for i in np.nonzero(big)[0]:
                k = int(ns[i])
                differs |= k != exp["nsize"][i] or not np.array_equal(got["ids"][i, :k], exp["ids"][exp["off"][i]: exp["off"][i + 1]])
            assert differs, "1,000,001 neighbours drew like 1,000,000"


# ------------------------------------------------------------------------------------------------ (e) the symmetrised edge graph
@pytest.mark.parametrize("M,m", E.SYM_SHAPES)
def test_symmetric_version_of_the_edge_graph(sp, M, m):
    """the edge graph as the reference's loader would hand it over: hubs among the reached nodes, a root without edges where the lone
    self loop was"""
    _run_all("sym", M, m, pitches=_pitches(M * m + 1))


# ---------------------------------------------------------------------------------------------------------------- (f) work lists
@pytest.mark.parametrize("M,m", E.WORKLIST_SHAPES)
def test_work_list_entries_outside_the_batch(sp, M, m):
    """-1, n, n + 7, 2^31 - 1 and -2^31 among valid rows: passed over -- the valid rows are the oracle's, nothing else is written, no flag"""
    g, csrs = S._graph(M, m), S._csrs(M, m)
    q = g["batch"]
    n = len(q)
    valid = np.arange(0, n, 3)
    wl = valid.astype(np.int64).tolist()
    for at, bad in ((0, -1), (3, n), (9, n + 7), (len(wl) // 2, 2 ** 31 - 1), (len(wl) + 3, -2 ** 31), (len(wl) + 5, -1)):
        wl.insert(at, bad)
    assert len(wl) <= n and wl[0] == -1 and wl[-1] == -1 and {n, n + 7, 2 ** 31 - 1, -2 ** 31} <= set(wl)
    for rng in RNGS:
        exp = S._expected(M, m, rng)
        for idx64 in (False, True):
            got = S._launch(csrs[idx64], q, M, m, rng, 0, work=np.array(wl, dtype=np.int32), n_work=len(wl))
            R._check(got, exp, listed=valid, what=(rng, idx64))


@pytest.mark.parametrize("M,m", E.WORKLIST_SHAPES)
def test_work_list_naming_a_row_three_times(sp, M, m):
    """three waves write one row: under Philox all three write the oracle's row.  And a list of one entry with *n_work = 1 at n = 5: the
    second workgroup has nothing to do"""
    g, csrs = S._graph(M, m), S._csrs(M, m)
    q = g["batch"]
    row = int(g["rows"]["tree"][0])                                  # the largest set
    exp = S._expected(M, m, "philox")
    assert exp["nsize"][row] == M * m + 1
    wl = np.array([2, row, 5, row, 7, row, 11, 0], dtype=np.int32)
    for idx64 in (False, True):
        got = S._launch(csrs[idx64], q, M, m, "philox", 0, work=wl, n_work=len(wl))
        R._check(got, exp, listed=np.unique(wl), what=("three times", idx64))
    for rng in RNGS:
        exp = S._expected(M, m, rng)
        for only in (0, 3, 4):
            got = S._launch(csrs[False], q[:5], M, m, rng, 0, work=np.array([only], dtype=np.int32), n_work=1)
            assert got["n"] == 5
            R._check(got, exp, listed=[only], what=("one entry", rng, only))


# -------------------------------------------------------------------------------------------------------------- (g) graph edges
@pytest.mark.parametrize("M,m", E.LAST_SHAPES)
def test_the_last_node_as_a_root(sp, M, m):
    """the root is num_nodes - 1 and owns the last adjacency entry (its row's end is indptr[num_nodes]); walks come back to it with hops left"""
    g = E.graph("last", M, m)
    assert g["batch"][0] == g["num_nodes"] - 1 and g["indptr"][-1] == len(g["indices"]) > g["indptr"][-2]
    _run_all("last", M, m, pitches=_pitches(M * m + 1))


@pytest.mark.parametrize("M,m", E.ISOLATED_SHAPES)
def test_a_graph_without_edges(sp, M, m):
    """indptr[num_nodes] == 0 (the clamp value is -1) and an indices array of one word: every root gives one member, itself, whose key
    holds M in every field plus the lead bit"""
    g = E.graph("isolated", M, m)
    assert not g["indptr"].any() and len(g["indices"]) == 1
    shift = E.small_shape(M, m)["shift"]
    key = (1 << (m * shift)) | sum(M << (j * shift) for j in range(m))
    for got in _run_all("isolated", M, m, pitches=_pitches(M * m + 1)):
        assert (got["nsize"] == 1).all() and np.array_equal(got["ids"][:, 0], g["batch"]) and (got["pay"][:, 0] == key).all()

"""Shapes and graphs that sit on the branch points of the one-wave key-row walk (csrc/walk_small.hip: walk_small_kernel behind
subgacc_walk_keyrows_small), and plain-Python restatements of those branch points.  No GPU here: tests/test_walk_small_edges_cpu.py
shows with the oracle that every case reaches the branch it is named for, tests/test_gpu_walk_small_edges.py drives the kernel through
the C ABI.

The restatements (small_shape, traceback_blocks, home, table_model) follow SmallShape, the launcher and the kernel's text line by line.
They say WHICH instantiation a launch runs and WHERE a member sits in the wave's table, never what a row is: the expected rows are
always the oracle's (rows)."""
import functools

import numpy as np

import walk_rows_edges as W
from walk_rows_edges import N_IDS, POOL, HUB_DEG, _Builder, key_bits, key_shift, lp_keys, table_size_for  # noqa: F401

WAVE = 64                    # kWave
WAVES = 4                    # kSmallWaves: roots per workgroup, their tables side by side in LDS
MAX_Q = 204                  # kSmallMaxQ
HASH_MUL = 2654435761        # the table's hash: (id * HASH_MUL mod 2^32) >> TSHIFT
SEED = 13
RNGS = ("rand_r", "philox")


# ------------------------------------------------------------------------------------- restatements: SmallShape and the launcher
def small_shape(M, m):
    """SmallShape<T, MH> of the walk_small_kernel<.., MH, T> that subgacc_walk_keyrows_small launches for (M, m), with the launcher's
    key shift: dict(T, MH, QMAX, MMAX, WPL, SPL, EPL, TSHIFT, shift, bits)"""
    Q = M * m + 1
    assert M >= 1 and 1 <= m <= 4 and Q <= MAX_Q, (M, m)
    T = table_size_for(Q)                                          # small_launch_table
    QMAX = 51 if T == 64 else (102 if T == 128 else MAX_Q)
    MMAX = (QMAX - 1) // m
    out = dict(T=T, MH=m, QMAX=QMAX, MMAX=MMAX, WPL=(MMAX + WAVE - 1) // WAVE, SPL=T // WAVE, EPL=(QMAX + WAVE - 1) // WAVE,
               TSHIFT=26 if T == 64 else (25 if T == 128 else 24), shift=key_shift(M), bits=key_bits(M, m))
    assert Q <= QMAX and M <= MMAX
    return out


def traceback_blocks(M, WPL):
    """the first-hop trace-back of a shuffled root: [(k2, trips)] of the 64-walk blocks it runs, last block first --
    `if (k2 * kWave >= M) continue` and `min(kWave, M - k2 * kWave)` trips"""
    return [(k2, min(WAVE, M - k2 * WAVE)) for k2 in range(WPL - 1, -1, -1) if k2 * WAVE < M]


def home(ids, T):
    """the slot a node id hashes to in a table of T slots"""
    tshift = {64: 26, 128: 25, 256: 24}[T]
    return (((np.asarray(ids).astype(np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(tshift)).astype(np.int64)


def table_model(T, root, visits):
    """the wave's open-addressing table: the root placed in its home slot, then insert-or-find of every visit in the order given
    with h = (h + 1) & (T - 1).  -> (keys [T], [(slot, the slots probed before it)] per visit)"""
    keys = [-1] * T
    keys[int(home(root, T))] = int(root)
    out = []
    for v in visits:
        v, h, path = int(v), int(home(v, T)), []
        while keys[h] != -1 and keys[h] != v:
            path.append(h)
            h = (h + 1) & (T - 1)
        keys[h] = v
        out.append((h, path))
    return keys, out


# ------------------------------------------------------------------------------------------------------------ the shape table
# (M, m): the smallest shapes at which each edge of the kernel exists, every one labelled with the edge it is here for
INSTANTIATIONS = {      # every (T, MH), at both ends of its Q range where it has two
    64: ((1, 1), (50, 1), (1, 2), (25, 2), (1, 3), (16, 3), (1, 4), (12, 4)),
    128: ((51, 1), (101, 1), (26, 2), (50, 2), (17, 3), (33, 3), (13, 4), (25, 4)),
    256: ((102, 1), (203, 1), (51, 2), (101, 2), (34, 3), (67, 3), (26, 4), (50, 4)),
}
LANES = {               # M on either side of a multiple of 64 walks
    "T = 128, WPL 2": ((63, 1), (64, 1), (65, 1)),
    "T = 256": ((63, 2), (64, 2), (65, 2), (63, 3), (64, 3), (65, 3)),
    "T = 256, WPL 4": ((127, 1), (128, 1), (129, 1), (191, 1), (192, 1), (193, 1)),
}
KEY_SHIFTS = ((2, 4), (3, 4), (4, 4), (7, 4), (8, 4), (15, 4), (16, 4), (31, 4), (32, 4))       # and (127, 1) | (128, 1), above
LANE_MS = (63, 64, 65, 127, 128, 129, 191, 192, 193)
SHIFT_MS = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 127, 128)


def _table():
    out = {}
    for T, shapes in INSTANTIATIONS.items():
        for s in shapes:
            out.setdefault(s, []).append(f"instantiation T = {T}, MH = {s[1]}")
    for name, shapes in LANES.items():
        for s in shapes:
            out.setdefault(s, []).append(f"lane boundary ({name})")
    for s in KEY_SHIFTS:
        out.setdefault(s, []).append("key shift")
    return out


SHAPE_TABLE = _table()               # {(M, m): [the edges it is here for]}
SHAPES = tuple(SHAPE_TABLE)

CLUSTER_SHAPES = ((50, 1), (101, 1), (203, 1), (12, 4), (25, 4), (50, 4))       # the fullest table of every T at one hop; four hops
LADDER_SHAPES = ((203, 1), (64, 3))
DEAD_SHAPES = ((12, 4), (25, 2), (25, 4), (67, 3), (101, 2), (50, 4))           # per T: the fewest hops that can stop early, the most
DEAD_ONE_HOP = (50, 1)                                                          # dead_ends(50, 2) walked with one hop
HUB_SHAPES = ((50, 1), (100, 2), (12, 4))
SYM_SHAPES = ((25, 2), (33, 3), (50, 4))
WORKLIST_SHAPES = ((25, 2), (203, 1))
LAST_SHAPES = ((12, 4), (33, 3), (203, 1))
ISOLATED_SHAPES = ((1, 1), (32, 4), (203, 1))


# -------------------------------------------------------------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def _homes(T):
    return home(np.arange(N_IDS), T)


def ids_with_home(T, slot):
    """the node ids below 2^20 whose home is `slot`, ascending"""
    return np.nonzero(_homes(T) == slot)[0]


def cluster(b, T, M, m):
    """three roots whose whole set collides in a table of T slots; the M neighbours of each have ONE home and point to the next one in a
    cycle (the set is closed: M + 1 members for any m; the root's degree is M: walk w takes neighbour w):
      root 1  home 1, neighbours' home T - 2: the chain fills T - 2, T - 1, wraps to 0, steps over the root's slot and goes on;
      root 2  home T - 1, neighbours' home T - 2: the root stands on the chain's second slot, in front of the wrap;
      root 3  home T - 2, the neighbours' own: the root sits in the slot where their probes begin.
    -> the roots"""
    assert m >= 1 and 4 <= M < T - 4
    pool = ids_with_home(T, T - 2)
    assert len(pool) >= 3 * M + 1
    rids = (ids_with_home(T, 1)[0], ids_with_home(T, T - 1)[0], pool[3 * M])
    roots = []
    for k, rid in enumerate(rids):
        nodes = b.new(M, pool[k * M: (k + 1) * M])
        r = b.new(1, [rid])[0]
        b.edges(r, nodes)
        b.edges(nodes, np.roll(nodes, -1))
        roots.append(r)
    return np.array(roots)


def ladder_all(b, M):
    """walk_rows_edges.degree_ladder with a longer tail: one root of every out-degree 1 .. M + 8 over the same kind of pool (three
    out-edges a node, a hub of HUB_DEG that every tenth node points to: no dead ends).  Up to M the modulo first hop runs its remainder at
    every divisor; M + 1 .. M + 8 are the Fisher-Yates draws with the fewest values to choose from.  -> (roots, their degrees)"""
    pool = b.new(POOL)
    b.edges(np.repeat(pool[1:], 3), pool[b.rng.integers(0, POOL, 3 * (POOL - 1))])
    b.edges(pool[0], pool[b.rng.permutation(POOL - 1)[:HUB_DEG] + 1])
    b.edges(pool[10::10], pool[0])
    degs = np.arange(1, M + 9)
    roots = b.new(len(degs))
    for r, d in zip(roots, degs):
        b.edges(r, pool[b.rng.permutation(POOL)[:d]])
    return roots, degs


def _finished(b, N, roots, order, batch=None, **more):
    indptr, indices, ids = b.finish(N)
    roots = {k: ids[np.atleast_1d(v)] for k, v in roots.items()}
    where, at = {}, 0
    for k in order:
        where[k] = np.arange(at, at + len(roots[k]))
        at += len(roots[k])
    first = np.concatenate([roots[k] for k in order])
    batch = first if batch is None else np.concatenate([first, ids[np.atleast_1d(batch)]])
    return dict(indptr=indptr, indices=indices, num_nodes=N, roots=roots, rows=where, batch=batch.astype(np.int32), **more)


@functools.lru_cache(maxsize=None)
def cluster_graph(M, m):
    """the three cluster roots of the shape's table and nothing else; the batch names them so that every workgroup's four waves fill
    their tables side by side (13 rows: the last workgroup has one)"""
    b = _Builder([M, m, 2])
    T = small_shape(M, m)["T"]
    r = cluster(b, T, M, m)
    return _finished(b, N_IDS, {"cluster": r}, ["cluster"], batch=r[[0, 1, 2, 0, 1, 2, 0, 1, 2, 2]], T=T)


@functools.lru_cache(maxsize=None)
def ladder_graph(M, m):
    b = _Builder([M, m, 3])
    r, degs = ladder_all(b, M)
    return _finished(b, N_IDS, {"ladder": r}, ["ladder"], degrees=degs)


LAST_NODES = 2000


@functools.lru_cache(maxsize=None)
def last_node_graph(M, m):
    """the root is the LAST node, num_nodes - 1, and owns the last adjacency entry: its row ends at nnz, and indptr[num_nodes] is read as
    its end.  M + 2 neighbours in a pool of 500 nodes with three out-edges each; every 50th pool node points back to it, so that walks
    stand on it with hops left as well.  The node in front of it has no edges.  -> as edge_graph"""
    b = _Builder([M, m, 4])
    N = LAST_NODES
    pool = b.new(500)
    b.edges(np.repeat(pool, 3), pool[b.rng.integers(0, 500, 1500)])
    owner = b.new(1, [N - 1])[0]
    lone = b.new(1, [N - 2])[0]
    b.edges(pool[::50], owner)
    b.edges(owner, pool[b.rng.permutation(500)[: M + 2]])
    g = _finished(b, N, {"owner": [owner], "lone": [lone], "pool": pool[:9]}, ["owner", "lone", "pool"], batch=[owner])
    assert g["indptr"][N - 1] < g["indptr"][N] == len(g["indices"]) and g["indptr"][N - 2] == g["indptr"][N - 1]
    return g


@functools.lru_cache(maxsize=None)
def isolated_graph():
    """nine nodes without an edge: indptr[num_nodes] == 0, the kernel's clamp value is -1; the indices array is one word long"""
    N = 9
    return dict(indptr=np.zeros(N + 1, dtype=np.int32), indices=np.zeros(1, dtype=np.int32), num_nodes=N,
                batch=np.array(list(range(N)) + [N - 1, 0], dtype=np.int32))


SIZES_NODES = 4096


@functools.lru_cache(maxsize=None)
def sizes_graph(M, m):
    """set sizes the edge graph does not promise at the smallest M (its sets have 1, 2 or about Q members there): walk_rows_edges.tree
    trimmed by one, two and three members as far as M allows (ns = Q - 1, Q - 2, Q - 3 exactly), and two roots with one edge each, into
    a directed ring of two and of three nodes (ns = min(m, 2) + 1 and min(m, 3) + 1 exactly, whatever M is).  With the edge graph's
    rows every residue of ns % 4 -- every length of the ranking's sentinel padding -- occurs at every shape with Q >= 5;
    tests/test_walk_small_edges_cpu.py asserts it.  -> as edge_graph"""
    b = _Builder([M, m, 5])
    Q = M * m + 1
    trees = [W.tree(b, M, m, ns=Q - k) for k in range(1, min(3, M - 1) + 1)] if m >= 2 else []
    rings = []
    for k in (2, 3):
        r, ring = b.new(1)[0], b.new(k)
        b.edges(r, ring[0])
        b.edges(ring, np.roll(ring, -1))
        rings.append(r)
    roots = dict(tree=trees, ring=rings) if trees else dict(ring=rings)
    return _finished(b, SIZES_NODES, roots, list(roots))


def graph(kind, M, m):
    """the graph of one case.  The builders that need two hops to be built (trees, chains into dead ends) give a one-hop shape the
    two-hop graph of its M"""
    if kind == "edge":
        return W.edge_graph(M, max(m, 2))
    if kind == "sym":
        return W.symmetric_edge_graph(M, max(m, 2))
    if kind == "dead":
        return W.dead_ends(M, max(m, 2))
    if kind == "hub":
        return W.hub_cap()
    if kind == "isolated":
        return isolated_graph()
    return {"sizes": sizes_graph, "cluster": cluster_graph, "ladder": ladder_graph, "last": last_node_graph}[kind](M, m)


# every (graph, M, m) the GPU file launches (the work lists run on edge graphs of the shape table)
assert set(WORKLIST_SHAPES) <= set(SHAPE_TABLE)
CASES = tuple([("edge", M, m) for M, m in SHAPES] + [("sizes", M, m) for M, m in SHAPES if M * m + 1 >= 5]
              + [("cluster", M, m) for M, m in CLUSTER_SHAPES]
              + [("ladder", M, m) for M, m in LADDER_SHAPES] + [("dead", M, m) for M, m in DEAD_SHAPES + (DEAD_ONE_HOP,)]
              + [("hub", M, m) for M, m in HUB_SHAPES] + [("sym", M, m) for M, m in SYM_SHAPES]
              + [("last", M, m) for M, m in LAST_SHAPES] + [("isolated", M, m) for M, m in ISOLATED_SHAPES])


# ------------------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def rows(kind, M, m, rng):
    """THE reference, once per (graph, shape, rng): the oracle's sets of the graph's batch as finished rows -- ids ascending inside every
    row, keys the member's LP key (what test_gpu_walk_small._expected makes of the edge graph) -> dict(nsize, off, ids, keys)"""
    import oracle
    g = graph(kind, M, m)
    nsize, remap, enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng)
    off = np.concatenate([[0], np.cumsum(nsize)]).astype(np.int64)
    order = np.lexsort((remap[0], np.repeat(np.arange(len(nsize)), nsize)))
    ukeys = lp_keys(enc, M, m)
    assert len(np.unique(ukeys)) == len(ukeys) and int(ukeys.max()) < 1 << small_shape(M, m)["bits"]
    out = dict(nsize=nsize, off=off, ids=remap[0][order], keys=ukeys[remap[1][order]])
    for v in out.values():
        v.setflags(write=False)
    return out

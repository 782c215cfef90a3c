"""Shapes, fixed graphs and plain-Python restatements for the three kernels that serve every walk walk_rows_kernel declines:
walk_sets_kernel<SPG = false> and <SPG = true> (csrc/walk.hip) and the persistent walk_pipe_kernel (csrc/walk_pipe.hip), and for
subgacc_compact_sets.  No GPU here: tests/test_walk_general_edges_cpu.py shows with the oracle that every case reaches the branch it
is named for, tests/test_gpu_walk_general_edges.py drives the kernels through the C ABI.

The restatements (kernel_for, spg_epilogue, sets_from_walks) say WHICH kernel a launch runs and WHICH branch a set takes; what a row
must hold is always the oracle's (reference)."""
import functools

import numpy as np

import walk_rows_edges as W
from walk_rows_edges import (GUARD, POISON, _Builder, crowded, dead_ends, degree_ladder, lp_keys, run,  # noqa: F401
                             self_loop, table_size_for, tree, walk_lds_bytes)

NO_ROOT = W.NO_ROOT
INT32_MAX = 2 ** 31 - 1
WALK_THREADS = W.WALK_THREADS
SPG_FOLD = W.SPG_FOLD            # kSpgFold: slots of the block-local table of a set's distinct LP keys
SPG_PER_LANE = 4                 # kSpgPerLane
FINE_ABOVE = W.FINE_ABOVE        # kFineAbove of the general epilogue
CW = 2                           # level-2 counter words per lane
LDS_BYTES = W.LDS_BYTES
COMPACT_FOLD = 256               # kFoldSlots: the wave-local table of compact_sets_kernel<INSERT>
RNGS = ("rand_r", "philox")


# ------------------------------------------------------------------------------------------------- restatements: the launcher
def lds_of(M, m, spg=False, bucket=-1):
    Q = M * m + 1
    stride = bucket if bucket > 0 else Q
    return walk_lds_bytes(table_size_for(Q), (Q + 31) // 32, M, Q, spg, stride < Q)


def kernel_for(M, m, form="sets", bucket=-1, order="walk", emit_walks=False, first_hop_wo=True, walk_pos=False):
    """launch_walk's choice (csrc/walk.hip) for subgacc_walk_sets (form "sets") and subgacc_walk_spg with a table (form "table"):
    'walk_pipe_kernel', 'walk_rows_kernel', 'walk_sets_kernel', 'walk_sets_kernel<SPG>' or 'refused: ...'"""
    assert form in ("sets", "table") and order in ("walk", "step")
    bits = W.key_bits(M, m)
    if bits > 64 or (bits == 64 and M == (1 << W.key_shift(M)) - 1):
        return "refused: key width"
    Q = M * m + 1
    if Q > 1 << 20:
        return "refused: LDS"
    spg = form == "table"
    if spg and (emit_walks or order != "walk"):
        return "refused: walk_spg"                                 # the entry point's own check
    T = table_size_for(Q)
    if spg and T > SPG_PER_LANE * WALK_THREADS:
        return "refused: LDS"
    if T > 65536 or lds_of(M, m, spg, bucket) > LDS_BYTES:
        return "refused: LDS"
    if not spg and first_hop_wo and order == "walk" and not emit_walks and M <= WALK_THREADS and 1 <= m <= 6 and not walk_pos:
        return "walk_pipe_kernel"
    if spg and not walk_pos and lds_of(M, m, True, bucket) <= 64 * 1024 and W.variant(M, m, "table", bucket=bucket) is not None:
        return "walk_rows_kernel"
    return "walk_sets_kernel<SPG>" if spg else "walk_sets_kernel"


def needs_attribute(M, m, spg=False, bucket=-1):
    """more than 64 KiB of dynamic LDS: the launch goes through hipFuncSetAttribute first"""
    return lds_of(M, m, spg, bucket) > 64 * 1024


def pipe_instantiation(m, rng, idx64):
    """(IDX64, RNG, MH) of walk_pipe_kernel<.., NT = 256, WPL = 1>: what a product build holds for 1..6 hops"""
    return (bool(idx64), rng, int(m))


PIPE_INSTANTIATIONS = frozenset((i, r, h) for i in (False, True) for r in RNGS for h in range(1, 7))


def pipe_grids(n):
    """the grids launch_hops may choose for n roots: min(256 * c, n), c = 1..8 from the occupancy query"""
    return sorted({min(256 * c, n) for c in range(1, 9)})


# --------------------------------------------------------------------------------- restatements: the general SPG epilogue
def staged(T, stride):
    """the sorted row is assembled in LDS (ids over minq, slots behind A) when both fit: (T - stride - 1) * 8 >= 4 * stride"""
    return (T - stride - 1) * 8 >= 4 * stride


def staged_edge(T):
    """(the largest stride that is staged, the smallest that is not) == ((2T - 2) // 3, + 1)"""
    e = (2 * T - 2) // 3
    assert staged(T, e) and not staged(T, e + 1)
    return e, e + 1


def spg_epilogue(ids, M, m, bucket=-1):
    """dict(ns, T, ranked, B, logb, bshift, maxc, W2, level2, staged) of one set (its kept members' ids) in walk_sets_kernel<SPG>:
    level 1 of the sort is W.level1 with NT = kWalkThreads lanes, level 2 is admitted by maxc > kFineAbove and the two room checks"""
    Q = M * m + 1
    T = table_size_for(Q)
    stride = bucket if bucket > 0 else Q
    ns, B, bshift, bk, counts = W.level1(ids, T, WALK_THREADS)
    assert ns <= stride and B <= min(T // 4, 256)
    maxc = int(counts.max())
    W2 = (ns + 2) // 2 + 1
    room = (W2 <= CW * WALK_THREADS, W2 <= T // 2 - 2)
    return dict(ns=ns, T=T, ranked=stride < Q, B=B, logb=B.bit_length() - 1, bshift=bshift, maxc=maxc, W2=W2, room=room,
                level2=bool(maxc > FINE_ABOVE and all(room)), staged=bool(staged(T, stride)))


def fold_rows(keys):
    """the distinct LP keys of one set: at most kSpgFold / 2 sit in the block-local table without long probe chains, more than kSpgFold
    cannot all fit (the 16-probe overflow goes straight to the HBM table)"""
    return len(np.unique(np.asarray(keys)))


# ----------------------------------------------------------------------------------- restatement: a set from its raw walks
def sets_from_walks(walks, M, m, order, bucket=-1):
    """plain-Python recount of one root's set from its raw walks [M, m + 1]: (ids in first-visit order under `order`, counts
    [ns, m + 1] with counts[0, 0] = M for the root and counts[k, s] = landings of step s on member k, total members before the
    bucket cut).  Members ranked past the bucket are dropped with all their visits."""
    walks = np.asarray(walks).reshape(M, m + 1)
    root = int(walks[0, 0])
    slot, ids, cnt = {root: 0}, [root], [[M] + [0] * m]
    visits = [(w, s) for w in range(M) for s in range(1, m + 1)] if order == "walk" else \
             [(w, s) for s in range(1, m + 1) for w in range(M)]
    for w, s in visits:
        v = int(walks[w, s])
        if v not in slot:
            slot[v] = len(ids)
            ids.append(v)
            cnt.append([0] * (m + 1))
        cnt[slot[v]][s] += 1
    total = len(ids)
    keep = total if bucket <= 0 else min(total, bucket)
    return np.array(ids[:keep], dtype=np.int32), np.array(cnt[:keep], dtype=np.int64), total


def count_keys(counts, M, m):
    """lp_keys of per-member counts [X, m + 1] (column 0: M on a root's row, else 0)"""
    return lp_keys(counts, M, m)


# ------------------------------------------------------------------------------------------------------------ the shape tables
# A. walk_sets_kernel, sets form: (M, m) on both sides of every table doubling -- Q = M * m + 1, want = Q + Q / 4 + 1
TABLE_PAIRS = (((25, 2), (17, 3)),            # Q = 51 | 52:   64 | 128 slots
               ((101, 1), (51, 2)),           # Q = 102 | 103: 128 | 256
               ((29, 7), (102, 2)),           # Q = 204 | 205: 256 | 512
               ((204, 2), (409, 1)),          # Q = 409 | 410: 512 | 1,024
               ((409, 2), (273, 3)))          # Q = 819 | 820: 1,024 | 2,048
BITMAP_PAIRS = (((31, 1), (16, 2)), ((21, 3), (32, 2)))           # Q = 32 | 33, 64 | 65: the last bit of a bitmap word, the first of the next
TRIP_SHAPES = ((255, 2), (256, 2), (257, 2), (511, 1), (512, 1), (513, 1))      # one, two and three trips of the walk loop
LDS_SHAPES = ((1637, 1), (273, 6), (546, 6))  # T = 2,048 (its largest shape), 4,096 (its smallest: the attribute path), 8,192
BUCKET_SHAPE = (25, 2)
ORDER_SHAPE = (6, 3)
DEAD_SHAPES = ((7, 3), (300, 2))
ROOT_SHAPES = ((7, 7), (4, 2))                # m = 7: the general kernel; (4, 2): the pipe and the general kernel side by side
# B. walk_sets_kernel<SPG>
SPG_SHAPES = ((25, 2), (101, 2), (100, 5), (257, 3), (681, 1), (341, 2), (60, 2), (136, 6))
FOLD_SHAPES = ((136, 6),)             # (random graphs at M = 257, m = 3 and at five hops stay below kSpgFold distinct rows: 53 and 128 at most)
STAGED_PAIR = ((681, 1), (341, 2))            # Q = 682 | 683 at T = 1,024
STAGED_BUCKET = (101, 2)                      # T = 256: bucket 170 | 171
CROWD_SHAPE = (60, 2)
# C. walk_pipe_kernel
PIPE_HOPS = tuple((4, m) for m in range(1, 7))
PIPE_WALKS = tuple((M, 2) for M in (1, 63, 64, 65, 255, 256))
GRID_SHAPE = (4, 2)
GRID_NS = tuple(sorted({1, 2} | {256 * c + d for c in range(1, 9) for d in (-1, 0, 1)} | {2 * 256 * c + 1 for c in range(1, 9)}))
KINDS = ("ordinary", "shuffled", "isolated", "outside", "no_root", "truncated", "full", "dead_end", "self_loop")
TRANSITION_BUCKET = 5                         # the second launch of the transition query: sets of more than 5 members are cut
TRANSITION_ROOTS = 3 * 2048


def pipe_launches():
    """(M, m, rng, idx64) of every launch of the GPU file's hop-count crossing"""
    return [(M, m, rng, idx64) for M, m in PIPE_HOPS for rng in RNGS for idx64 in (False, True)]


def buckets_for(Q, ns):
    return sorted({1, 2, ns - 1, ns, ns + 1, Q - 1, Q, Q + 1})


def probe_wraps(ids, T):
    """how many probes of the open-addressing table of T slots step from slot T - 1 to slot 0 while `ids` are inserted (the number does
    not depend on the order: it is the overflow of the cluster at the table's end)"""
    sh = 32 - (T.bit_length() - 1)
    used, wraps = set(), 0
    for v in np.asarray(ids).astype(np.int64):
        h = ((int(v) * 2654435761) & 0xFFFFFFFF) >> sh
        while h in used:
            wraps += h == T - 1
            h = (h + 1) & (T - 1)
        used.add(h)
    return wraps


def lds_edge_shapes():
    """((M, m) of the largest lds with T = 2,048, the smallest Q with T = 4,096, a T = 8,192 shape that fits): derived, compared with
    LDS_SHAPES by the CPU test"""
    best = None
    for Q in range(2, 1639):
        if table_size_for(Q) == 2048:
            for m in range(1, 8):
                if (Q - 1) % m == 0 and kernel_for((Q - 1) // m, m, emit_walks=True) == "walk_sets_kernel":
                    cand = (lds_of((Q - 1) // m, m), Q, ((Q - 1) // m, m))
                    best = cand if best is None or cand[:2] > best[:2] else best
    return best[2]


# -------------------------------------------------------------------------------------------------------------------- graphs
N_SMALL = 1 << 16
GRAPH_SEED = {(25, 2): 14}        # (ids are drawn at random: a seed under which the full set's probes wrap at the end of its 64-slot table)


def star(b, M, children=None):
    """a root with `children` (default M) children that nobody else reaches: with one hop the set has exactly M + 1 members"""
    root = b.new(1)[0]
    b.edges(root, b.new(children or M))
    return root


@functools.lru_cache(maxsize=8)
def edge_graph(M, m, ladder=True, crowd=False):
    """One directed graph per shape, no dead ends on any walk: degree_ladder (roots of out-degree 0 .. M + 2, 2M, 4M + 1), the full
    tree (ns = Q exactly; one hop: a star), a tree one member short, a tree of M + 3 children (shuffled), self_loop (1, 2 and 2
    members), runs of 1 .. 5 consecutive ids, runs at id 0 and at N - 1, and (crowd) W.crowded's three sets.
    -> dict(indptr, indices, num_nodes, roots, rows, batch, Q, degrees)"""
    b = _Builder([M, m, GRAPH_SEED.get((M, m), 7)])
    Q = M * m + 1
    N = W.N_IDS if crowd else max(N_SMALL, 1 << int(4 * Q + 6000).bit_length())
    parts = {}
    degs = None
    if ladder:
        parts["ladder"], degs = degree_ladder(b, M)
    if m >= 2:
        parts["full"] = np.array([tree(b, M, m)])
        if M >= 2:
            parts["short"] = np.array([tree(b, M, m, ns=Q - 1)])
        if M >= 6:
            parts["short5"] = np.array([tree(b, M, m, ns=Q - 5)])
        parts["shuffled"] = np.array([tree(b, M, m, children=M + 3)])
    else:
        parts["full"] = np.array([star(b, M)])
        parts["shuffled"] = np.array([star(b, M, M + 3)])
    parts["self_loop"] = self_loop(b)
    parts["isolated"] = b.new(1)
    small = [k for k in (1, 2, 3, 4, 5) if k <= M + 1]
    parts["small"] = np.array([run(b, k, 1000 * (i + 1)) for i, k in enumerate(small)])
    rs = min(M + 1, W.RUN)
    parts["run"] = np.array([run(b, rs, 0), run(b, rs, N - rs)])
    if crowd:
        assert M >= W.SPREAD + max(W.CROWD)
        parts["crowded"] = crowded(b)
    indptr, indices, ids = b.finish(N)
    order = list(parts)
    roots = {k: ids[np.asarray(v)] for k, v in parts.items()}
    assert roots["run"].tolist() == [0, N - 1]
    batch = np.concatenate([roots[k] for k in order] + [roots["full"], roots["run"][:1], roots["self_loop"][:1]])
    where, at = {}, 0
    for k in order:
        where[k] = np.arange(at, at + len(roots[k]))
        at += len(roots[k])
    return dict(indptr=indptr, indices=indices, num_nodes=N, roots=roots, rows=where, degrees=degs, batch=batch.astype(np.int32), Q=Q,
                small=small)


@functools.lru_cache(maxsize=4)
def dense_graph(N, deg, seed):
    """N nodes of `deg` random out-edges each (repeats and self loops allowed): sets overlap, so the walk-major and the step-major
    first-visit orders differ and a set carries many distinct LP rows"""
    rng = np.random.default_rng([N, deg, seed])
    indptr = (np.arange(N + 1) * deg).astype(np.int32)
    indices = rng.integers(0, N, N * deg).astype(np.int32)
    return dict(indptr=indptr, indices=indices, num_nodes=N, batch=np.arange(min(N, 48), dtype=np.int32))


def fold_graph(M, m):
    """the dense graph of a fold-table shape: enough reached nodes for more than kSpgFold distinct LP rows in one set"""
    return dense_graph(200, 48, M * 10 + m)


@functools.lru_cache(maxsize=2)
def transition_graph():
    """the graph of the root-kind transitions at GRID_SHAPE (M = 4, two hops, Q = 9): pools of roots of every kind that is a property
    of the node -> (graph dict, {kind: node ids})"""
    M, m = GRID_SHAPE
    b = _Builder([M, m, 11])
    ladder, degs = degree_ladder(b, M)                  # degrees 0 .. 6, 8, 17
    full = np.array([tree(b, M, m) for _ in range(3)])
    trunc = np.array([tree(b, M, m, ns=M * m + 1 - 2) for _ in range(3)])         # 7 members: cut by TRANSITION_BUCKET, not full
    loops = self_loop(b)
    dead = []
    for _ in range(3):                                  # three children without out-edges: every walk stops after its first hop
        r = b.new(1)[0]
        b.edges(r, b.new(3))
        dead.append(r)
    small = np.array([run(b, 3, 50000 + 10 * i) for i in range(3)])               # three members
    indptr, indices, ids = b.finish(N_SMALL)
    N = N_SMALL
    pools = dict(ordinary=ids[small], shuffled=ids[ladder[degs > M]], isolated=ids[ladder[degs == 0]].repeat(2),
                 outside=np.array([-1, N, INT32_MAX, -7]), no_root=np.array([NO_ROOT]), truncated=ids[trunc], full=ids[full],
                 dead_end=ids[np.array(dead)], self_loop=ids[loops[:2]])
    return dict(indptr=indptr, indices=indices, num_nodes=N), pools


@functools.lru_cache(maxsize=2)
def transition_query(seed=20):
    """(query [TRANSITION_ROOTS], kind of every row as an index into KINDS): kinds and pool members drawn with a fixed seed"""
    _, pools = transition_graph()
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, len(KINDS), TRANSITION_ROOTS)
    q = np.array([pools[KINDS[k]][rng.integers(0, len(pools[KINDS[k]]))] for k in kind], dtype=np.int64)
    return q.astype(np.int32), kind


def in_graph(q, N):
    q = np.asarray(q).astype(np.int64)
    return (q >= 0) & (q < N)


# ------------------------------------------------------------------------------------------------------------ the reference
def reference(g, q, M, m, rng, seed=13, bucket=-1):
    """The oracle's sets of the roots of q that lie in the graph -- a root outside it (SUBGACC_NO_ROOT included) is never looked up,
    draws nothing and leaves an empty row: dict(good [n] bool, nsize [n] (0 for the others), off [n + 1], ids [X] and keys [X] uint64
    in first-visit order, total = the oracle's result itself)"""
    import oracle
    q = np.asarray(q, dtype=np.int32)
    good = in_graph(q, g["num_nodes"])
    o_ns, remap, enc = oracle.gset_sampler(g["indptr"], g["indices"], q[good], num_walks=M, num_steps=m, bucket=bucket, seed=seed, rng=rng)
    nsize = np.zeros(len(q), dtype=np.int32)
    nsize[good] = o_ns
    off = np.concatenate([[0], np.cumsum(nsize)]).astype(np.int64)
    ukeys = lp_keys(enc, M, m)
    return dict(good=good, nsize=nsize, off=off, ids=remap[0], keys=ukeys[remap[1]], oracle=(o_ns, remap, enc))


def as_rows(ref, M, m):
    """reference() as finished rows, in the layout of W.expected_rows (ids ascending inside every row): what _check of the fused-row
    tests compares fused rows, slots and numbering with"""
    o_ns, remap, enc = ref["oracle"]
    nsize, off = ref["nsize"], ref["off"]
    rowid = np.repeat(np.arange(len(nsize)), nsize)
    order = np.lexsort((remap[0], rowid))
    ukeys = lp_keys(enc, M, m)
    assert len(np.unique(ukeys)) == len(ukeys)
    sf = remap[1][order]
    return dict(nsize=nsize, off=off, ids=remap[0][order], sf=sf, keys=ukeys[sf], ukeys=ukeys, visit_sf=remap[1].copy())


def walk_reference(g, q, M, m, rng, seed=13, first_hop_wo=True):
    """oracle.walk_sampler over the roots inside the graph: (walks [n_good, M, m + 1], nsize, off, ids, keys) in STEP-major order"""
    import oracle
    q = np.asarray(q, dtype=np.int32)
    good = in_graph(q, g["num_nodes"])
    walks, ns, ids, counts = oracle.walk_sampler(g["indptr"], g["indices"], q[good], num_walks=M, num_steps=m, seed=seed,
                                                 replacement=bool(first_hop_wo), rng=rng)
    nsize = np.zeros(len(q), dtype=np.int32)
    nsize[good] = ns
    off = np.concatenate([[0], np.cumsum(nsize)]).astype(np.int64)
    return dict(good=good, walks=walks.reshape(-1, M, m + 1), nsize=nsize, off=off, ids=ids, keys=count_keys(counts, M, m))


def recount(walks, M, m, order, bucket=-1):
    """sets_from_walks over the walks of many roots [k, M, m + 1] -> (nsize, ids, keys, totals)"""
    ns, ids, keys, totals = [], [], [], []
    for wk in walks:
        i, c, t = sets_from_walks(wk, M, m, order, bucket)
        ns.append(len(i))
        ids.append(i)
        keys.append(count_keys(c, M, m))
        totals.append(t)
    cat = (lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt))
    return np.array(ns, dtype=np.int32), cat(ids, np.int32), cat(keys, np.uint64), np.array(totals, dtype=np.int64)


# ------------------------------------------------------------------------------------------------------ D. compact_sets cases
def compact_case(n, seed=3):
    """strided sets for subgacc_compact_sets: n rows of stride 400 whose sizes cycle through 0, 63, 64, 65 and -- the last row -- 300
    with 300 distinct keys (more than the 256 slots of a wave's fold table); the other rows draw their keys from a pool of 40, so
    rows share keys.  -> dict(ids [n, stride], keys [n, stride] uint64, nsize, row_off, stride)"""
    rng = np.random.default_rng([n, seed])
    stride = 400
    sizes = np.array([(0, 63, 64, 65)[(i + n) % 4] for i in range(n)], dtype=np.int32)
    sizes[-1] = 300
    pool = rng.integers(1, 2 ** 62, 40, dtype=np.int64).astype(np.uint64)
    ids = np.full((n, stride), POISON, dtype=np.int32)
    keys = np.full((n, stride), np.uint64(POISON & (2 ** 64 - 1)), dtype=np.uint64)
    for i, k in enumerate(sizes):
        ids[i, :k] = rng.permutation(100000)[:k]
        keys[i, :k] = pool[rng.integers(0, len(pool), k)]
    wide = np.unique(rng.integers(1, 2 ** 62, 400, dtype=np.int64).astype(np.uint64))[:300]
    assert len(wide) == 300
    keys[-1, :300] = rng.permutation(wide)
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return dict(ids=ids, keys=keys, nsize=sizes, row_off=row_off, stride=stride)


def compact_expected(c):
    """NumPy restatement of the copy: (packed ids, packed keys, the distinct keys in order of first occurrence in the packed array)"""
    sel = np.arange(c["stride"])[None, :] < c["nsize"][:, None]
    ids, keys = c["ids"][sel], c["keys"][sel]
    _, first = np.unique(keys, return_index=True)
    return ids, keys, keys[np.sort(first)]

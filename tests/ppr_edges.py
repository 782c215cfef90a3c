"""Inputs and host restatements for the edge tests of csrc/ppr.hip and csrc/encode.hip (tests/test_ppr_edges_cpu.py shows on the
host that every case is what it claims, tests/test_gpu_ppr_edges.py runs them on the GPU).  No GPU is needed here.

The push kernel keeps the dicts of one root in an open-addressed table of `cap = 2^log2` slots: a node's first slot is `khash`,
probing steps by one and wraps at `cap`.  It gives a root up (out_count = -1, flags[2] |= 1) on three tests:
    before a pop        np + 1 + ntouched > cap
    after a trip        (ntouched + 256) * 4 > 3 * cap     or     np + 1 + ntouched + 256 > cap
with ntouched the nodes in the table and np <= ntouched those in p, both growing only.  With T the nodes a root touches in all
(the popped nodes and their neighbours, `touched_count`) this gives the two bounds below; between them nothing is claimed."""
import numpy as np
import scipy.sparse as sps

TRIP = 256                       # kPprUnroll * 64 neighbours per trip of the push loop
ALPHA, EPS = 0.5, 1e-4           # the reference's defaults


def khash(ids, log2):
    """the kernel's first slot of a node id: (id * 2654435761 mod 2^32) >> (32 - log2)"""
    return ((np.asarray(ids, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2)


def certainly_accepted(touched, cap):
    """np <= ntouched <= touched: none of the three tests can fire (cap >= 1,024 covers touched < 127 in the 3/4 test)"""
    return cap >= 1024 and 2 * touched + TRIP + 1 <= cap


def certainly_refused(touched, cap):
    """the trip that brings ntouched to `touched` fails the 3/4 test"""
    return 4 * (touched + TRIP) > 3 * cap


def touched_count(indptr, indices, popped_ids):
    """|popped u N(popped)|: with topk >= np the oracle's row is the popped set"""
    popped_ids = np.asarray(popped_ids, dtype=np.int64)
    nb = [indices[indptr[u]:indptr[u + 1]] for u in popped_ids]
    return len(np.union1d(popped_ids, np.concatenate(nb + [np.zeros(0, np.int64)])))


def graph_from_edges(N, src, dst, symmetric=True):
    """(indptr int32, indices int32) of a simple graph with sorted rows; symmetric: every edge in both directions"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if symmetric:
        src, dst = np.r_[src, dst], np.r_[dst, src]
    A = sps.csr_matrix((np.ones(len(src)), (src, dst)), shape=(N, N))
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


def is_simple_symmetric(indptr, indices):
    N = len(indptr) - 1
    rows = np.repeat(np.arange(N), np.diff(indptr))
    key = rows.astype(np.int64) * N + indices
    if len(np.unique(key)) != len(key) or (rows == indices).any():
        return False
    return np.array_equal(np.sort(key), np.sort(indices.astype(np.int64) * N + rows))


def star(d):
    """hub 0 with leaves 1 .. d"""
    return graph_from_edges(d + 1, np.zeros(d, np.int64), np.arange(1, d + 1))


def complete_bipartite(a, b):
    """K(a, b): nodes 0 .. a-1 against a .. a+b-1"""
    return graph_from_edges(a + b, np.repeat(np.arange(a), b), np.tile(np.arange(a, a + b), a))


def directed_graph(N, E, seed):
    """as tests/test_gpu_ppr.py: rows >= N / 2 have no out-edges"""
    rng = np.random.default_rng(seed)
    A = sps.csr_matrix((np.ones(E), (rng.integers(0, N // 2, E), rng.integers(0, N, E))), shape=(N, N))
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


def colliding_ids(K, slots, log2=10, N=200_000, root_slot=None):
    """(root, the first K ids below N whose first slot is one of `slots`): the root is the LAST id of `root_slot`, or the first id
    of the slot half a table away from slots[0]"""
    h = khash(np.arange(N), log2)
    leaves = np.flatnonzero(np.isin(h, np.asarray(slots, dtype=np.uint64)))[:K]
    assert len(leaves) == K, "not enough ids below N hash to these slots"
    if root_slot is None:
        root = int(np.flatnonzero(h == np.uint64((slots[0] + (1 << (log2 - 1))) & ((1 << log2) - 1)))[0])
    else:
        root = int(np.flatnonzero(h == np.uint64(root_slot))[-1])
    assert root not in leaves
    return root, leaves


def colliding_star(K, slots, log2=10, N=200_000, root_slot=None):
    """A symmetric simple graph on N mostly isolated nodes: the root's K neighbours all start probing at `slots`, so one trip
    holds many claimants of one free slot and the chain runs on past slot cap - 1 when slot cap - 1 is used.
    Returns (indptr, indices, root, leaves)."""
    root, leaves = colliding_ids(K, slots, log2, N, root_slot)
    indptr, indices = graph_from_edges(N, np.full(K, root), leaves)
    return indptr, indices, root, leaves


def mixed_graph(log2=10, N=200_000):
    """One graph for a wave that runs accepted and refused roots in turn: the colliding star (300 leaves on slots cap-1, cap-2,
    root on cap-1), stars of 512 and 600 leaves (refused at 2^10 slots) and of 7 leaves on ids the colliding star leaves free.
    Returns (indptr, indices, {name: (hub, leaves)})."""
    cap = 1 << log2
    root, leaves = colliding_ids(300, [cap - 1, cap - 2], log2, N, root_slot=cap - 1)
    free = np.setdiff1d(np.arange(N), np.r_[root, leaves])
    parts, at = {"colliding": (root, leaves)}, 1000
    for name, d in (("star512", 512), ("star600", 600), ("star7", 7)):
        parts[name] = (int(free[at]), free[at + 1: at + 1 + d])
        at += d + 1
    src = np.concatenate([np.full(len(lv), hub) for hub, lv in parts.values()])
    dst = np.concatenate([lv for _, lv in parts.values()])
    indptr, indices = graph_from_edges(N, src, dst)
    return indptr, indices, parts


def repeated_entry_star(d=399, m=4):
    """NOT a simple graph: the hub's row lists each of its d leaves m times.  The lanes that hold the copies of a new leaf all
    claim its slot with the same entry and all read their own key back, so the leaf is counted m times: ntouched reaches
    1 + m * d, which no table up to 2 * num_nodes + 257 slots lets pass once m * d + 257 > 3 / 4 * 2 * (2 * num_nodes + 257)."""
    N = d + 1
    indptr = np.r_[0, m * d, m * d + np.arange(1, d + 1)].astype(np.int32)
    indices = np.r_[np.repeat(np.arange(1, d + 1), m), np.zeros(d, np.int64)].astype(np.int32)
    assert len(indptr) == N + 1 and indptr[-1] == len(indices)
    return indptr, indices


# ------------------------------------------------------------------------------------------- DEG / SPD: a plain restatement
def encode_union(x, adj, mode):
    """utils.py:22-34 as a per-row union of two sorted id lists with a value rule, no sparse algebra.  x: scipy CSR with positive
    values, adj: scipy CSR of ones (symmetric).  Returns (indptr, ids, val, agg or None).
    DEG  ids = X_i u A_i; val(i, j) = log(|X_j u A_j| + 1); agg(i, j) = x(i, j) [j in X_i] + 1 / |A_i| [j in A_i]
    SPD  ids = A_i u X_i u {i}; val = 1 [A] + 0.5 [X and N(i) n N(j) != {}] + 0.3 [X]; val(i, i) = 2.3"""
    N = x.shape[0]
    xr = [x.indices[x.indptr[i]:x.indptr[i + 1]] for i in range(N)]
    xv = [x.data[x.indptr[i]:x.indptr[i + 1]] for i in range(N)]
    ar = [adj.indices[adj.indptr[i]:adj.indptr[i + 1]] for i in range(N)]
    uni = [np.union1d(xr[i], ar[i]) for i in range(N)]
    ulen = np.array([len(u) for u in uni])
    ids, val, agg, lens = [], [], [], []
    for i in range(N):
        u = uni[i] if mode == "DEG" else np.union1d(uni[i], [i])
        in_x, in_a = np.isin(u, xr[i]), np.isin(u, ar[i])
        xval = np.zeros(len(u))
        xval[in_x] = xv[i][np.searchsorted(xr[i], u[in_x])]
        if mode == "DEG":
            v = np.log(ulen[u] + 1)
            inv = 1.0 / len(ar[i]) if len(ar[i]) else 0.0
            agg.append(np.where(in_a, np.where(in_x, xval + inv, inv), xval))
        else:
            two = np.array([in_x[k] and len(np.intersect1d(ar[i], ar[j])) > 0 for k, j in enumerate(u)], dtype=bool)
            v = np.zeros(len(u))
            v[in_a] = 1.0
            v[two] += 0.5
            v[in_x] += 0.3
            v[u == i] = 2.3
        ids.append(u)
        val.append(v)
        lens.append(len(u))
    indptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts + [np.zeros(0, dt)]).astype(dt)
    return indptr, cat(ids, np.int32), cat(val, np.float64), (cat(agg, np.float64) if mode == "DEG" else None)


def _csr_rows(N, rows, vals=None):
    lens = [len(r) for r in rows]
    indptr = np.r_[0, np.cumsum(lens)].astype(np.int64)
    indices = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    data = np.ones(len(indices)) if vals is None else np.concatenate(vals + [np.zeros(0)])
    m = sps.csr_matrix((data, indices, indptr), shape=(N, N))
    m.sort_indices()
    return m


HUBS = {10: 63, 20: 64, 30: 65, 40: 130, 50: 257}       # node: degree, both sides of the 64-lane loops over the neighbours
ISOLATED = 5


def edge_inputs_for_encoders(N=400, seed=0):
    """(X, A) as scipy CSR for the DEG / SPD union kernels.
    A: symmetric, ones; HUBS have exactly the stated degrees; self-loops on node 0 (its smallest id), N // 2 and N - 1 (its
    largest id); node ISOLATED has no entry at all.
    X: positive float64; rows of 0 (node 10, node ISOLATED), 1, 63, 64, 65, 129 and N entries, the others 2..6; own id
       row 0      in A and in X, smallest id of the row          row N-1    in A and in X (the row is [N-1]), largest id
       row N//2   in A only                                      row 1      in X only, smallest id of the row
       row N-2    in X only, largest id of the row               row 2, N-3 in neither, below / above every id of the row"""
    rng = np.random.default_rng(seed)
    mid = N // 2
    special = set(HUBS) | {ISOLATED, 0, 1, 2, mid, N - 3, N - 2, N - 1}
    pool = np.array([v for v in range(60, N - 3) if v not in special])
    src, dst = [], []
    for hub, d in HUBS.items():
        src.append(np.full(d, hub))
        dst.append(rng.choice(pool, d, replace=False))
    e = rng.choice(pool, (2, 300))                          # background edges among the pool
    keep = e[0] != e[1]
    src.append(e[0][keep]), dst.append(e[1][keep])
    for a, bs in ((0, [0, 3, 70, 90]), (mid, [mid, 61, N - 4]), (N - 1, [N - 1, 7, 62]), (1, [3, 80]), (N - 2, [4, 81]),
                  (2, [3, 100]), (N - 3, [8, 101])):
        src.append(np.full(len(bs), a)), dst.append(np.array(bs))
    src, dst = np.concatenate(src), np.concatenate(dst)
    A = sps.csr_matrix((np.ones(2 * len(src)), (np.r_[src, dst], np.r_[dst, src])), shape=(N, N))
    A.sum_duplicates()
    A.data[:] = 1.0
    A.sort_indices()
    assert A.getnnz(axis=1)[ISOLATED] == 0 and all(A.getnnz(axis=1)[h] == d for h, d in HUBS.items())

    others = np.array([v for v in range(N) if v != ISOLATED])      # ISOLATED appears in the full row only
    rows = [np.sort(rng.choice(others[others != i], rng.integers(2, 7), replace=False)) for i in range(N)]

    def pick(i, k, must=(), lo=0, hi=N):
        """k sorted ids of [lo, hi) with `must` among them; half of the rest from A's row i where it has that many"""
        cand = np.setdiff1d(np.arange(lo, hi), np.r_[list(must), ISOLATED, i]).astype(np.int64)
        nb = np.intersect1d(A.indices[A.indptr[i]:A.indptr[i + 1]], cand)
        a = rng.choice(nb, min(len(nb), (k - len(must)) // 2), replace=False)
        b = rng.choice(np.setdiff1d(cand, a), k - len(must) - len(a), replace=False)
        return np.sort(np.r_[list(must), a, b]).astype(np.int64)

    rows[10] = np.zeros(0, np.int64)
    rows[ISOLATED] = np.zeros(0, np.int64)
    rows[N - 1] = np.array([N - 1])
    rows[0] = pick(0, 63, must=[0])
    rows[20] = pick(20, 64)
    rows[30] = pick(30, 65, must=[30])
    rows[40] = pick(40, 129)
    rows[50] = np.arange(N)
    rows[mid] = pick(mid, 4)
    rows[1] = pick(1, 5, must=[1], lo=1)
    rows[N - 2] = pick(N - 2, 5, must=[N - 2], hi=N - 1)
    rows[2] = pick(2, 4, lo=3)
    rows[N - 3] = pick(N - 3, 4, hi=N - 3)
    X = _csr_rows(N, rows, [rng.uniform(0.05, 1.0, len(r)) for r in rows])
    return X, A


def long_row_inputs(kmax, N=8200):
    """(X, A, s): a ring of N nodes; node s = N // 2 has degree 65 and an X row of `kmax` entries, every other X row has 1..3:
    the row that sizes the LDS of the fill kernel (10 * kmax + 20 bytes: 65,530 at 6,551, 65,540 at 6,552)"""
    rng = np.random.default_rng(kmax)
    s = N // 2
    ring = np.arange(N)
    extra = rng.choice(np.setdiff1d(ring, [s - 1, s, s + 1]), 63, replace=False)
    src, dst = np.r_[ring, np.full(63, s)], np.r_[(ring + 1) % N, extra]
    A = sps.csr_matrix((np.ones(2 * len(src)), (np.r_[src, dst], np.r_[dst, src])), shape=(N, N))
    A.sum_duplicates()
    A.data[:] = 1.0
    A.sort_indices()
    assert A.getnnz(axis=1)[s] == 65
    k = rng.integers(1, 4, N)
    rows = [np.unique((i + rng.integers(-40, 41, k[i])) % N) for i in range(N)]
    rows[s] = np.sort(rng.choice(N, kmax, replace=False))
    X = _csr_rows(N, rows, [rng.uniform(0.05, 1.0, len(r)) for r in rows])
    return X, A, s


# ------------------------------------------------------------------------------------------- normalise / encode: hand-built rows
def packed_rows(nnz, n_nodes, sinks, nonsinks, seed=0):
    """(roots, row_off, ids, vals) with `nnz` entries over 7 rows, empty ones first, in the middle and last; roots and columns of
    degree 0 (`sinks`) among them.  The LAST entry is far above the others, its column a sink and its row's root not one, so the
    maximum of every normalisation falls into the last wave of the launch."""
    rng = np.random.default_rng(seed + nnz)
    a = nnz // 3
    lens = np.array([0, a, 0, 0, nnz - 2 * a, a, 0]) if nnz >= 3 else np.array([0, nnz, 0, 0, 0, 0, 0])
    row_off = np.r_[0, np.cumsum(lens)].astype(np.int64)
    roots = rng.choice(nonsinks, len(lens)).astype(np.int32)
    roots[0], roots[2] = sinks[0], sinks[1]                 # empty rows
    if nnz >= 3:
        roots[1] = sinks[2]                                 # a full row whose root has degree 0
    ids = rng.integers(0, n_nodes, nnz).astype(np.int32)
    ids[::5] = rng.choice(sinks, len(ids[::5]))
    vals = rng.uniform(1e-3, 1.0, nnz).astype(np.float32)
    if nnz:
        vals[-1], ids[-1] = np.float32(1e9), sinks[3]
    return roots, row_off, ids, vals

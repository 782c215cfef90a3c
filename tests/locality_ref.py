"""NumPy restatement of the locality order (csrc/locality.hip, include/subgacc.h: subgacc_locality_round; sampler.locality_order):
shared by tests/test_locality_cpu.py and tests/test_gpu_locality.py."""
import numpy as np


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def lp_round(indptr, indices, lab, t, cap=64):
    """one round: labels after round t (int32 [N])"""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    N = indptr.size - 1
    deg = indptr[1:] - indptr[:-1]
    upd = ((mix32(np.arange(N)) & 1).astype(np.int64) == (t & 1)) & (deg > 0)
    U = np.nonzero(upd)[0]
    new = lab.copy()
    if U.size == 0:
        return new
    k = np.minimum(deg[U], cap)
    rep = np.repeat(U, k)
    start = np.repeat(np.cumsum(k) - k, k)
    j = np.arange(rep.size, dtype=np.int64) - start
    d = deg[rep]
    pos = np.where(d <= cap, j, j * d // cap)
    cand = lab[indices[indptr[rep] + pos]].astype(np.int64)
    node = np.concatenate([rep, U])
    cl = np.concatenate([cand, lab[U].astype(np.int64)])
    key, cnt = np.unique(node * N + cl, return_counts=True)
    kn, kl = key // N, key % N
    best = np.lexsort((kl, -cnt, kn))             # per node: highest count first, then the smallest label
    kn, kl = kn[best], kl[best]
    first = np.ones(kn.size, dtype=bool)
    first[1:] = kn[1:] != kn[:-1]
    new[kn[first]] = kl[first].astype(np.int32)
    return new


def locality_labels(indptr, indices, rounds=8, cap=64):
    lab = np.arange(np.asarray(indptr).size - 1, dtype=np.int32)
    for t in range(rounds):
        lab = lp_round(indptr, indices, lab, t, cap)
    return lab


def order_and_rank(labels):
    order = np.argsort(labels, kind="stable").astype(np.int32)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size, dtype=np.int32)
    return order, rank


def locality_score(indptr, indices, rank, window=2048):
    """fraction of the edges whose endpoints' ranks lie within `window` of each other"""
    indptr = np.asarray(indptr, dtype=np.int64)
    src = np.repeat(np.arange(indptr.size - 1), indptr[1:] - indptr[:-1])
    dst = np.asarray(indices, dtype=np.int64)
    return float(np.mean(np.abs(rank[src].astype(np.int64) - rank[dst]) <= window))

"""CPU: randomized sweep of the oracle (oracle/subgacc_oracle.c) against the REFERENCE ITSELF (subg_acc/subg_acc.c), beyond the
46 committed fixtures: random graphs (isolated nodes, star hubs, K2 components), random M / m / bucket / seeds / query shapes.

    gset_sampler  nthread=1 (the only reproducible setting, subg_acc.c:731-732)        subg_acc.c:649-1034
    walk_sampler  nthread 1..8, both first-hop modes                                   subg_acc.c:316-389
    walk_join     over walk_sampler's own output                                       subg_acc.c:509-647
    batch_sampler seeded with seed + getpid() by the reference (:421)                   subg_acc.c:391-507

The reference's outputs of every case are committed as SHA-256 digests (tests/golden/ref_sweep.npz; batch_sampler's with the
seed + getpid() sum they were made with), so the sweep runs wherever the oracle builds.  Where the compiled reference exists
(oracle/_ref, `make -C oracle ref`) each case is also compared with it array by array, and
`PYTHONPATH=. python tests/test_oracle_vs_ref.py` re-makes the digests from it.  Every case has its own seeded stream: a failing
case number reproduces alone."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

import oracle

ref = oracle.ref_module()
SWEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sweep.npz")

CASES = 240


def digest(arrays):
    """SHA-256 over the shapes and int64 values of a case's outputs: equal digests <=> np.array_equal on every array"""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(np.asarray(a), dtype=np.int64)
        h.update(repr(a.shape).encode() + a.tobytes())
    return h.hexdigest()


def check(kind, case, o, r, what):
    """the oracle's outputs `o` against the reference's: `r` itself where it was computed here, and the committed digest"""
    if r is not None:
        for a, b in zip(o, r, strict=True):
            assert np.array_equal(a, b), what
    assert digest(o) == str(stored()[kind][case]), f"{what}: not the reference's output (committed digest)"


@functools.lru_cache(maxsize=None)
def stored():
    with np.load(SWEEP) as z:
        return {k: z[k] for k in z.files}


def rand_graph(rng):
    import scipy.sparse as sps
    N = int(rng.integers(4, 400))
    E = int(rng.integers(1, 6 * N))
    iso = int(rng.integers(0, 4))
    star = int(rng.integers(0, N - 1)) if rng.random() < 0.4 else 0
    k2 = rng.random() < 0.3
    r, c = rng.integers(0, N, E), rng.integers(0, N, E)
    if star:
        r = np.concatenate([r, np.zeros(star, int)])
        c = np.concatenate([c, rng.choice(np.arange(1, N), star, replace=False)])
    tot = N + iso + (2 if k2 else 0)
    if k2:
        r, c = np.concatenate([r, [tot - 2]]), np.concatenate([c, [tot - 1]])
    A = sps.csr_matrix((np.ones(len(r)), (r, c)), shape=(tot, tot))
    A = sps.csr_matrix(A + A.T)          # symmetrised like dataloader.py:122-135: no dead ends
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32)


def rand_query(rng, n_nodes):
    kind = rng.integers(0, 4)
    if kind == 0:
        return np.arange(n_nodes)
    if kind == 1:                                            # repeated, unordered roots
        return rng.integers(0, n_nodes, int(rng.integers(1, 2 * n_nodes)))
    if kind == 2:
        return np.sort(rng.choice(n_nodes, int(rng.integers(1, n_nodes + 1)), replace=False))
    return rng.integers(0, n_nodes, int(rng.integers(1, 9)))  # a handful (fewer roots than threads, below)


def rand_walk_params(rng):
    M = int(rng.choice([1, 2, 3, 5, 8, 16, 20, 31, 32, 64, 100, 200]))
    shift = int(M).bit_length()
    m = int(rng.integers(1, min(6, 63 // shift) + 1))       # m*SHIFT+1 <= 64 (subg_acc.c:905-915)
    return M, m


def mask_isolated(ptr, query, nsize, remap):
    """the reference leaves the id word of an isolated root uninitialised (subg_acc.c:753-761)"""
    remap = remap.copy()
    deg = np.diff(ptr)[query]
    off = np.concatenate([[0], np.cumsum(nsize)])[:-1]
    remap[0, off[deg == 0]] = np.asarray(query)[deg == 0]
    return remap


def gset_case(case):
    """-> (what, the oracle's outputs, the reference's -- None without oracle/_ref)"""
    rng = np.random.default_rng(10_000 + case)
    ptr, idx = rand_graph(rng)
    q = rand_query(rng, len(ptr) - 1)
    M, m = rand_walk_params(rng)
    bucket = int(rng.integers(2, M * m + 2)) if rng.random() < 0.3 else -1
    seed = int(rng.integers(0, 2**31 - 1))
    r = None
    if ref is not None:
        nsize, remap, enc, raw = ref.gset_sampler(ptr, idx, q, num_walks=M, num_steps=m, bucket=bucket, nthread=1,
                                                  seed=seed, debug=1)
        r = [nsize, mask_isolated(ptr, q, nsize, remap), enc, raw]
    o = oracle.gset_sampler(ptr, idx, q, num_walks=M, num_steps=m, bucket=bucket, seed=seed, debug=True)
    return f"case {case}: N={len(ptr) - 1} n={len(q)} M={M} m={m} bucket={bucket} seed={seed}", list(o[:4]), r


def walk_case(case):
    """-> (what, [(kind, the oracle's outputs, the reference's -- None without oracle/_ref)] for "walk" and "walkjoin")"""
    rng = np.random.default_rng(20_000 + case)
    ptr, idx = rand_graph(rng)
    q = rand_query(rng, len(ptr) - 1).astype(np.int32)
    M, m = rand_walk_params(rng)
    T = int(rng.integers(1, 9))
    rep = bool(rng.integers(0, 2))
    seed = int(rng.integers(0, 2**31 - 1))
    r_walk = None
    if ref is not None:
        walks, obj = ref.walk_sampler(ptr, idx, q, num_walks=M, num_steps=m, nthread=T, seed=seed, replacement=rep)
        r_walk = [walks, [len(obj[i, 0]) for i in range(len(q))], np.concatenate([obj[i, 0] for i in range(len(q))]),
                  np.concatenate([obj[i, 1] for i in range(len(q))])]
    o_walk = list(oracle.walk_sampler(ptr, idx, q, num_walks=M, num_steps=m, nthread=T, seed=seed, replacement=rep))
    what = f"case {case}: N={len(ptr) - 1} n={len(q)} M={M} m={m} T={T} rep={rep} seed={seed}"
    # the legacy join over these walks (pairs of sampled roots, (u, u) included).  Distinct roots only: with a root
    # repeated in `walk` the reference adds duplicate keys to a uthash table (HASH_ADD_INT, subg_acc.c:563) --
    # which of them HASH_FIND returns flips with every bucket expansion (expansion re-chains a bucket in reverse),
    # i.e. depends on how many other roots there are.  The goldens' small `dup` case (no expansion: the last row
    # wins) is what the oracle and the HIP path implement; the reference's callers pass unique nodes.
    walks, nsize, ids = (r_walk or o_walk)[:3]
    keys = np.split(ids, np.cumsum(nsize)[:-1])
    first = np.sort(np.unique(q, return_index=True)[1])
    uq, uw, ukeys = q[first], walks[first], [keys[i] for i in first]
    Q = int(rng.integers(1, 40))
    pairs = uq[rng.integers(0, len(uq), (Q, 2))]
    pairs[0] = (uq[0], uq[0])
    r_join = list(ref.walk_join(uw, ukeys, pairs, nthread=1, return_idx=True)) if ref is not None else None
    o_join = list(oracle.walk_join(uw, ukeys, pairs, return_idx=True))
    return what, [("walk", o_walk, r_walk), ("walkjoin", o_join, r_join)]


def batch_case(case):
    """-> (what, the oracle's output for a given seed + getpid() sum, (the reference's output, the sum it started from) or None)"""
    rng = np.random.default_rng(30_000 + case)
    ptr, idx = rand_graph(rng)
    N = len(ptr) - 1
    q = rand_query(rng, N).astype(np.int32)
    M = int(rng.integers(1, 60))
    S = int(rng.integers(1, 10))
    thld = int(rng.integers(1, 4 * N))
    seed = int(rng.integers(0, 2**30))

    def run(seed_eff):
        return [oracle.batch_sampler(ptr, idx, q, num_walks=M, num_steps=S, thld=thld, seed_eff=seed_eff)]
    live = None
    if ref is not None:          # (this process: the sum the reference starts from is known)
        live = [ref.batch_sampler(ptr, idx, q, num_walks=M, num_steps=S, thld=thld, seed=seed)], seed + os.getpid()
    return f"case {case}: N={N} n={len(q)} M={M} S={S} thld={thld} seed={seed}", run, live


@pytest.mark.parametrize("block", range(8))
def test_gset_sampler_random_sweep(block, capfd):
    for case in range(block * CASES // 8, (block + 1) * CASES // 8):
        what, o, r = gset_case(case)
        check("gset", case, o, r, what)
    ctypes.CDLL(None).fflush(None)
    capfd.readouterr()        # the reference printf()s statistics


@pytest.mark.parametrize("block", range(8))
def test_walk_sampler_and_walk_join_random_sweep(block, capfd):
    for case in range(block * CASES // 8, (block + 1) * CASES // 8):
        what, parts = walk_case(case)
        for kind, o, r in parts:
            check(kind, case, o, r, what)
    ctypes.CDLL(None).fflush(None)
    capfd.readouterr()


@pytest.mark.parametrize("block", range(4))
def test_batch_sampler_random_sweep(block):
    for case in range(block * CASES // 4, (block + 1) * CASES // 4):
        what, run, live = batch_case(case)
        if live is not None:
            assert np.array_equal(run(live[1])[0], live[0][0]), what
        check("batch", case, run(int(stored()["batch_seed_eff"][case])), None, what)


if __name__ == "__main__":     # re-make the committed digests from the compiled reference
    assert ref is not None, "needs oracle/_ref (`make -C oracle ref`)"
    digests = {"gset": [], "walk": [], "walkjoin": [], "batch": []}
    seed_eff = []
    for case in range(CASES):
        digests["gset"].append(digest(gset_case(case)[2]))
        for kind, _, r in walk_case(case)[1]:
            digests[kind].append(digest(r))
        r, s = batch_case(case)[2]
        digests["batch"].append(digest(r))
        seed_eff.append(s)
    np.savez_compressed(SWEEP, batch_seed_eff=np.array(seed_eff, np.int64), **{k: np.array(v) for k, v in digests.items()})

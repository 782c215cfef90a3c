"""The packed key row (include/subgacc_packed.h, csrc/packed_rows.hpp) restated in NumPy, and the graphs, shapes and hand-made rows
that sit on the branch points of its three kernels -- the walk's packed store (csrc/walk_rows.hip), sjoin_packpair_kernel and
unpack_packed_rows_kernel (csrc/sjoin_packed.hip).  No GPU here: tests/test_packed_rows_cpu.py round-trips the format and proves
with the oracle that every case reaches the branch it is named for, tests/test_gpu_packed_rows.py drives the kernels.

The restatement follows the header's text, not the kernels' code: fields are cut out of the key one by one and narrowed."""
import functools

import numpy as np

import walk_rows_edges as W

SEED = 13
KESC = 64                    # escape keys of a row that sjoin_packpair_kernel stages out of its first trip (kEsc)


# ------------------------------------------------------------------------------------------------------------ the format
def id_bits(num_nodes):
    """bits of num_nodes - 1, at least 1 (subgacc_hop_records_format)"""
    return max(int(num_nodes - 1).bit_length(), 1)


def fmt(num_nodes, m):
    """(cb, fb)"""
    cb = 32 - id_bits(num_nodes)
    return cb, (cb - 1) // m


def eligible(num_nodes, M, m, idx64=False):
    """the predicate of the header, from the launcher's restatement (W.variant): 32-bit key rows of a two-wave form, fb >= 3"""
    if not 2 <= m <= 4 or W.key_bits(M, m) > 31 or M > W.WALK_THREADS:
        return False
    tup = W.variant(M, m, "keys32", idx64)
    return tup is not None and tup[2] == 128 and fmt(num_nodes, m)[1] >= 3


def fields(keys, M, m):
    """[len, m + 1]: the lead flag and the counts of hops 1 .. m of 32-bit LP keys"""
    s = W.key_shift(M)
    k = np.asarray(keys).astype(np.uint64)
    cols = [(k >> np.uint64(m * s)) & np.uint64(1)] + [(k >> np.uint64((m - c) * s)) & np.uint64((1 << s) - 1) for c in range(1, m + 1)]
    return np.stack(cols, axis=1).astype(np.int64)


def key_of(f, M, m):
    s = W.key_shift(M)
    f = np.asarray(f).astype(np.int64)
    k = f[:, 0] << (m * s)
    for c in range(1, m + 1):
        k |= f[:, c] << ((m - c) * s)
    return k.astype(np.uint32)


def codes(keys, M, m, cb, fb):
    """(code of every key: the cb ones for an escape, is it an escape)"""
    f = fields(keys, M, m)
    code = f[:, 0]
    for c in range(1, m + 1):
        code = (code << fb) | (f[:, c] & ((1 << fb) - 1))
    ones = (1 << cb) - 1
    esc = (f[:, 1:] >= (1 << fb)).any(axis=1) | (code == ones)
    return np.where(esc, ones, code).astype(np.uint32), esc


def pack_row(ids, keys, M, m, cb, fb):
    """(words uint32 [ns], the escape list uint32 [ne]) of one row (ids ascending)"""
    code, esc = codes(keys, M, m, cb, fb)
    words = (np.asarray(ids).astype(np.uint32) << np.uint32(cb)) | code
    return words, np.asarray(keys).astype(np.uint32)[esc]


def unpack_row(words, esc_list, M, m, cb, fb):
    """(ids int32, keys uint32) of a packed row; an escape beyond the list reads as key 0"""
    words = np.asarray(words).astype(np.uint32)
    ones = np.uint32((1 << cb) - 1)
    code = (words & ones).astype(np.int64)
    is_esc = code == int(ones)
    f = np.zeros((len(words), m + 1), np.int64)
    f[:, 0] = (code >> (m * fb)) & 1
    for c in range(1, m + 1):
        f[:, c] = (code >> ((m - c) * fb)) & ((1 << fb) - 1)
    keys = key_of(f, M, m)
    rank = np.cumsum(is_esc) - 1
    lst = np.asarray(esc_list).astype(np.uint32)
    ok = is_esc & (rank < len(lst))
    keys[is_esc] = 0
    keys[ok] = lst[rank[ok]]
    return (words >> np.uint32(cb)).astype(np.int32), keys


# ------------------------------------------------------------------------------------------------------------ walk: shapes and graph
# (m, M): every instantiation of the packed store -- 1,024 slots with five members per lane (2, 3, 4 hops) and eight (3 hops above 640
# members), 512 slots with two waves (3 and 4 hops; 2 hops with int64 offsets) -- and the one-wave neighbour that has none
SHAPES = ((3, 200), (3, 256), (3, 136), (2, 256), (2, 204), (4, 102), (4, 127))
# node ids of the graph of a shape: fb = 3 at three and four hops, 5 at two (fb = 3 at two hops needs 2^24 nodes)
NODES = {2: 1 << 20, 3: 1 << 20, 4: 1 << 19}
RUNS = (3, 4, 5, 127, 128, 129)


def pinned_tree(b, M, m, base, fan=None):
    """a root (id base) with `fan` (default M) children, every child the head of a chain of its own -- level j on the ids
    base + 1 + (j - 1) * fan + i -- but the first 2^fb chains end in ONE node with the highest id of all: a set of
    fan * m + 2 - 2^fb members in which the last member of the sorted row, and only it, escapes (count >= 2^fb) -> the root"""
    fb = fmt(NODES[m], m)[1]
    merge = 1 << fb
    fan = fan or M
    assert merge <= fan <= M and (M // fan) < (1 << fb)
    ids = base + np.arange(fan * m + 2)
    nodes = b.new(len(ids), ids)
    root, lvl, top = nodes[0], nodes[1: 1 + fan * m].reshape(m, fan), nodes[-1]
    b.edges(root, lvl[0])
    for j in range(m - 2):
        b.edges(lvl[j], lvl[j + 1])
    last = lvl[m - 1].copy()
    last[:merge] = top
    b.edges(lvl[m - 2], last)
    return root


@functools.lru_cache(maxsize=None)
def walk_graph(M, m):
    """The graph of one shape: W.degree_ladder (a root of every out-degree 0 .. M + 2, 2M, 4M + 1: isolated, modulo and shuffled first
    hops, first-hop counts on both sides of 2^fb), W.tree (the largest set), runs of exactly 3, 4, 5, 127, 128 and 129 members whose
    root has the highest id, a run of 5 whose root has the lowest, two pinned trees (the whole fan: the escape is the last member of
    the longest row; ~400 members: it falls to the second wave of a trip of four members per lane), a pair of nodes that point at each other (degree 1:
    both members escape) and a root with two leaves that point back (degree 2: all three escape).  No dead ends.
    -> dict(indptr, indices, num_nodes, roots = {name: node ids}, rows = {name: rows of the batch}, degrees, batch)"""
    N = NODES[m]
    b = W._Builder([M, m, 9])
    ladder, degs = W.degree_ladder(b, M)
    named = {"ladder": ladder, "tree": np.array([W.tree(b, M, m)])}
    runs = [ns for ns in RUNS if ns - 1 <= M]
    named["run"] = np.array([W.run(b, ns, 10000 * (k + 1)) for k, ns in enumerate(runs)])
    named["run_low"] = np.array([W.run(b, 5, 0)])
    named["pinned"] = np.array([pinned_tree(b, M, m, 100000), pinned_tree(b, M, m, 200000, fan=min(-(-400 // m), M))])
    a, c = b.new(2)
    b.edges([a, c], [c, a])
    r, x, y = b.new(3)
    b.edges([r, r, x, y], [x, y, r, r])
    named["pair"], named["star"] = np.array([a]), np.array([r])
    indptr, indices, ids = b.finish(N)
    order = ["ladder", "tree", "run", "run_low", "pinned", "pair", "star"]
    roots = {k: ids[named[k]] for k in order}
    batch = np.concatenate([roots[k] for k in order] + [roots["ladder"][[5, 5]], roots["pair"]])      # repeated roots
    where, at = {}, 0
    for k in order:
        where[k] = np.arange(at, at + len(roots[k]))
        at += len(roots[k])
    return dict(indptr=indptr, indices=indices, num_nodes=N, roots=roots, rows=where, degrees=degs, runs=runs,
                batch=batch.astype(np.int32), Q=M * m + 1)


@functools.lru_cache(maxsize=None)
def walk_rows(M, m, rng="philox"):
    """the oracle's rows of walk_graph's batch: dict(nsize, off, ids ascending inside every row, keys uint32)"""
    import oracle
    g = walk_graph(M, m)
    nsize, remap, enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng)
    off = np.concatenate([[0], np.cumsum(nsize)]).astype(np.int64)
    rowid = np.repeat(np.arange(len(nsize)), nsize)
    order = np.lexsort((remap[0], rowid))
    keys = W.lp_keys(enc, M, m)[remap[1][order]]
    assert (keys < 2 ** 31).all()
    return dict(nsize=nsize, off=off, ids=remap[0][order], keys=keys.astype(np.uint32))


def row(exp, i):
    return exp["ids"][exp["off"][i]: exp["off"][i + 1]], exp["keys"][exp["off"][i]: exp["off"][i + 1]]


# ------------------------------------------------------------------------------------------------------------ join: hand-made rows
# (m, M, num_nodes, pitch): the three forms of sjoin_packpair_kernel (join_lanes) at every row width, the pitch that fills four trips
# of 128 lanes exactly, and at three hops over 2^22 nodes cb = 1 + 3 * fb: the code of all ones exists and must escape
JOIN_SHAPES = ((3, 200, 1 << 22, 608), (3, 256, 1 << 20, 800), (3, 136, 1 << 20, 416), (2, 256, 1 << 20, 544), (2, 204, 1 << 20, 416),
               (4, 102, 1 << 19, 416), (4, 127, 1 << 19, 512))
JOIN_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)


def join_lanes(pitch):
    """(lanes per pair, register trips) of subgacc_sjoin_fill_packed's launch: 128 x 4 up to 512 members, 128 x 5 up to 640, 256 x 4 above"""
    return (256, 4) if pitch > 640 else (128, 5 if pitch > 512 else 4)


@functools.lru_cache(maxsize=None)
def join_rows(M, m, num_nodes, pitch):
    """Rows for the join, by name -> dict(ids [n] list, keys [n] list, names): the lengths of JOIN_LENGTHS (those the pitch holds) and
    the longest row of the shape, over a universe of ids so small that any two rows share members; "none": no escape; "all": every
    member escapes; "many": more escapes than the join stages (KESC); "ones": small counts whose code is all ones, where it exists.
    Escapes are about a fifth of the other rows' members, the first and the last member among them."""
    rs = np.random.default_rng([M, m, pitch])
    cb, fb = fmt(num_nodes, m)
    Q = min(M * m + 1, pitch)
    universe = np.sort(rs.choice(num_nodes, int(1.6 * Q), replace=False)).astype(np.int64)
    universe[0], universe[-1] = 0, num_nodes - 1                    # the smallest and the largest id there is
    s = W.key_shift(M)

    def keys_for(n, share):
        f = np.zeros((n, m + 1), np.int64)
        f[:, 0] = rs.integers(0, 2, n)
        f[:, 1:] = rs.integers(0, 1 << fb, (n, m))
        f[:, 1] = np.maximum(f[:, 1], 1)
        big = rs.random(n) < share
        if n and share > 0:
            big[[0, n - 1]] = True
        col = rs.integers(1, m + 1, n)
        f[big, col[big]] = rs.integers(1 << fb, min(M, (1 << s) - 1) + 1, int(big.sum()))
        return key_of(f, M, m)

    lens = [n for n in JOIN_LENGTHS if n <= Q] + [Q]
    names = [f"len{n}" for n in lens] + ["none", "all", "many", "ones"]
    ids, keys = [], []
    for n in lens:
        ids.append(np.sort(rs.choice(universe, n, replace=False)) if n else np.zeros(0, np.int64))
        keys.append(keys_for(n, 0.2))
    n = min(300, Q)
    ids.append(np.sort(rs.choice(universe, n, replace=False)))
    keys.append(keys_for(n, 0.0))
    n = min(100, Q)
    ids.append(np.sort(rs.choice(universe, n, replace=False)))
    keys.append(keys_for(n, 1.0))
    n = min(400, Q)
    ids.append(np.sort(rs.choice(universe, n, replace=False)))
    keys.append(keys_for(n, 0.3))
    n = min(40, Q)
    f = np.full((n, m + 1), (1 << fb) - 1, np.int64)                   # every count 2^fb - 1 ...
    f[:, 0] = np.arange(n) % 2                                       # ... with the flag: the code is 1 + m * fb ones
    ids.append(np.sort(rs.choice(universe, n, replace=False)))
    keys.append(key_of(f, M, m))
    return dict(ids=[np.asarray(i, np.int64) for i in ids], keys=keys, names=names, cb=cb, fb=fb)


def join_pairs(n_rows, count):
    """[2, count] row pairs: every (i, j) once -- (u, u) and both orders of every two rows -- then repeats"""
    i, j = np.divmod(np.arange(count) % (n_rows * n_rows), n_rows)
    return np.stack([i, j]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
# (torch and the library are imported when a GPU test calls these, not when the CPU tests import this module)
def lib_module():
    from surel_plus_amd import _lib
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(n, dtype, init=None):
    """n words of poison (or `init`) between two poisoned guards: (whole buffer, the n words)"""
    import torch
    whole = torch.full((n + 2 * W.GUARD,), W.POISON, dtype=dtype, device="cuda")
    view = whole[W.GUARD: W.GUARD + n]
    if init is not None:
        view.copy_(dev(init).view(dtype))
    return whole, view


def back(whole, n):
    """the n words as NumPy, after the guards in front and behind were seen untouched"""
    h = whole.cpu().numpy()
    assert (h[:W.GUARD] == W.POISON).all() and (h[W.GUARD + n:] == W.POISON).all(), "a guard word was written"
    return h[W.GUARD: W.GUARD + n]


def launch_keys32(csr, q, M, m, rng, pitch=0, work=None, n_work=None, entry=None, check=True):
    """The reference of the packed walk: today's two planes of 32-bit key rows (no table of distinct rows) through the C ABI, into
    poisoned, guarded outputs.  entry: None (subgacc_walk_spg), "sparse" or "list" (a work list).
    -> dict(rc, P, n, ids [n, P], pay [n, P], nsize [n], flags [4])"""
    import torch
    from surel_plus_amd import sampler
    L = lib_module()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n = len(q)
    Pw = pitch if pitch > 0 else M * m + 1
    d_q = dev(np.asarray(q, dtype=np.int32))
    cfg = sampler.make_cfg(csr, M, m, -1, SEED, rng, row_pitch=pitch)
    rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st) if entry != "sparse" else (None, None)
    w_ids, ids = guarded(n * Pw, torch.int32)
    w_pay, pay = guarded(n * Pw, torch.int32)
    w_ns, nsize = guarded(n, torch.int32)
    w_fl, flags = guarded(4, torch.int32, np.zeros(4, np.int32))
    d_wl = dev(np.asarray(work, dtype=np.int32)) if work is not None else None
    d_nw = dev(np.array([n_work], dtype=np.int64)) if work is not None else None
    g = (cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n)
    rows = (ptr(ids), ptr(pay), ptr(nsize), ptr(flags), st)
    if entry == "sparse":
        rc = lib.subgacc_walk_spg_sparse(*g, ptr(d_wl), ptr(d_nw), None, 0, *rows)
    elif entry == "list":
        rc = lib.subgacc_walk_spg_list(*g, ptr(rp), ptr(rs), ptr(d_wl), ptr(d_nw), None, 0, *rows)
    else:
        rc = lib.subgacc_walk_spg(*g, 0, ptr(rp), ptr(rs), None, 0, *rows)
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    return dict(rc=rc, P=Pw, n=n, ids=back(w_ids, n * Pw).reshape(n, Pw), pay=back(w_pay, n * Pw).reshape(n, Pw), nsize=back(w_ns, n),
                flags=back(w_fl, 4))

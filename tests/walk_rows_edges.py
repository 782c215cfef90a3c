"""Graphs and shapes that sit on the branch points of the fused-row walk (csrc/walk_rows.hip: walk_rows_kernel, launch_walk_rows;
csrc/walk.hip: launch_walk), and plain-Python restatements of those branch points.  No GPU here: tests/test_walk_rows_edges_cpu.py
proves with the oracle that every case reaches the branch it is named for, tests/test_gpu_walk_rows_edges.py drives the kernels
through the C ABI.

The restatements (variant, outcome, level1, table_epilogue, key_row_levels, first_hop) follow the launcher and the two epilogues line
by line.  They say WHICH instantiation a launch runs and WHICH branch a row takes, never what the row is: the expected rows are
always the oracle's (expected_rows)."""
import functools

import numpy as np

POISON = -1515870811         # 0xA5A5A5A5: what every output holds before a launch (ids and 31-bit keys are never negative)
GUARD = 64                   # poisoned words in front of and behind every output (a multiple of 4: the rows stay 16-byte aligned)
NO_ROOT = -2 ** 31           # SUBGACC_NO_ROOT
NEIGH_CAP = 1_000_000        # kNeighCap
FINE_ABOVE = 12              # kFineAbove: level 2 from 13 members in one level-1 bucket on
AGAIN_ABOVE = 16             # SG_SORT_AGAIN_ABOVE: level 3 of the two-wave key rows from 17 members in one level-2 part on
WALK_THREADS = 256           # kWalkThreads
SPG_FOLD = 128               # kSpgFold
LDS_BYTES = 160 * 1024       # kLdsBytes
FORMS = ("table", "keys32", "keys64", "tags")


# ------------------------------------------------------------------------------------------------- restatements: the launcher
def table_size_for(q):
    t = 64
    while t < q + q // 4 + 1:
        t <<= 1
    return t


def key_shift(M):
    """subgacc_key_shift: 32 - clz(M)"""
    return int(M).bit_length()


def key_bits(M, m):
    return m * key_shift(M) + 1


def walk_lds_bytes(T, nwords, M, Q, spg, bucket_truncates):
    head = T * 16 + nwords * 4 + (nwords + 1) * 4 + M * 4
    fold = 8 + SPG_FOLD * 16 + 64
    if not spg:
        return head + Q * 2 + 16
    if bucket_truncates:
        return head + Q * 2 + fold + 16
    return head + max(fold, Q * 2) + 16


def kr_red_offset(T, M, stride, NT, wide):
    walk = T * (12 if wide else 8) + M * 4 + 8
    sort = stride * (16 if wide else 8) + (NT + 4) * 4 + 4 * NT * 4
    return (max(walk, sort) + 15) & ~15


def _rows(M, m, form, idx64, records, bucket):
    """launch_walk followed by launch_walk_rows: (the instantiation or None, the outcome's name)"""
    assert form in FORMS
    bits = key_bits(M, m)
    if bits > 64 or (bits == 64 and M == (1 << key_shift(M)) - 1):
        return None, "refused: key width"
    Q = M * m + 1
    stride = bucket if bucket > 0 else Q
    if form == "keys64" and (bucket > 0 or bits <= 31):
        return None, "refused: walk_keyrows64"                    # the entry point's own checks
    if form == "tags" and bucket > 0:
        return None, "refused: walk_tags"
    T = table_size_for(Q)
    if T > 4 * WALK_THREADS:
        return None, "refused: LDS"                               # SUBGACC_ERR_LDS: "use subgacc_walk_sets + subgacc_spg_build"
    lds = walk_lds_bytes(T, (Q + 31) // 32, M, Q, True, stride < Q)
    assert lds <= LDS_BYTES
    declined = {"table": "walk_sets_kernel<SPG>", "keys32": "refused: key rows", "keys64": "refused: key rows",
                "tags": "refused: walk_tags"}[form]
    if lds > 64 * 1024 or M > WALK_THREADS or stride != Q or m < 2 or m > 4 or T not in (512, 1024):
        return None, declined
    rec = 0 if not records else (16 if idx64 else 8)
    keyrows = form in ("keys32", "keys64")
    if keyrows and bits > 31:
        if form != "keys64" or m != 4 or bits > 63 or T != 1024 or (stride + 2) // 2 + 1 > 4 * 128:
            return None, declined
        return (4, 8, 128, rec, False, True, 7 if stride <= 7 * 128 else 0), "walk_rows_kernel"
    if keyrows:
        if (stride + 2) // 2 + 1 > 4 * (64 if T == 512 else 128):
            return None, declined
        if T == 1024:
            return (m, 8, 128, rec, True, True, 5 if stride <= 5 * 128 else 0), "walk_rows_kernel"
        if not idx64 and m == 2:
            return (2, 8, 64, rec, True, True, 0), "walk_rows_kernel"           # ONE wave per root
        return (m, 4, 128, rec, True, True, 0), "walk_rows_kernel"
    if T == 1024 and not idx64 and bits <= 31 and m <= 3:
        return (m, 8, 128, rec, True, False, 0), "walk_rows_kernel"             # 32-bit counts, 128 lanes x 8 slots
    if T == 1024:
        return (m, 4, 256, rec, False, False, 0), "walk_rows_kernel"
    return (m, 4, 128, rec, False, False, 0), "walk_rows_kernel"                # T == 512 ("half")


def variant(M, m, form, idx64=False, records=False, rng="philox", bucket=-1):
    """(MH, SPL, NT, REC, K32, KR, EPLP) of the walk_rows_kernel<idx64, rng, ...> this launch runs, or None where launch_walk_rows
    declines (outcome() names what happens then).  `records`: hop records of the form that goes with the row offsets are given.
    rng picks the RNG template argument and nothing else."""
    assert rng in ("rand_r", "philox")
    return _rows(M, m, form, idx64, records, bucket)[0]


def outcome(M, m, form, idx64=False, records=False, bucket=-1):
    """'walk_rows_kernel', 'walk_sets_kernel<SPG>' (the general kernel takes the rows) or 'refused: ...'"""
    return _rows(M, m, form, idx64, records, bucket)[1]


def _reachable():
    """every (idx64, instantiation) launch_walk_rows can reach in a product build, written out: the forms of rows_form crossed with
    the shapes that can stand in front of them.  These are also all the instantiations a product build of walk_rows.hip holds: the
    launcher no longer names a form that no shape reaches"""
    out = set()
    for idx64 in (False, True):
        recs = (0, 16) if idx64 else (0, 8)
        for rec in recs:
            out.add((idx64, (4, 8, 128, rec, False, True, 7)))                  # 64-bit key rows (EPLP = 0: no served stride above 896)
            out.add((idx64, (2, 8, 128, rec, True, True, 5)))                   # 32-bit key rows, 1,024 slots: m = 2 and 4 never above 640
            out.add((idx64, (3, 8, 128, rec, True, True, 5)))
            out.add((idx64, (3, 8, 128, rec, True, True, 0)))
            out.add((idx64, (4, 8, 128, rec, True, True, 5)))
            if idx64:
                out.add((idx64, (2, 4, 128, rec, True, True, 0)))               # 512 slots, two waves
            else:
                out.add((idx64, (2, 8, 64, rec, True, True, 0)))                # 512 slots, one wave (int32 offsets, 2 hops)
            out.add((idx64, (3, 4, 128, rec, True, True, 0)))
            out.add((idx64, (4, 4, 128, rec, True, True, 0)))
            for m in (2, 3, 4):
                out.add((idx64, (m, 4, 128, rec, False, False, 0)))             # table form, 512 slots
            if idx64:
                for m in (2, 3, 4):
                    out.add((idx64, (m, 4, 256, rec, False, False, 0)))         # table form, 1,024 slots, 64-bit counts
            else:
                out.add((idx64, (4, 4, 256, rec, False, False, 0)))             # (m <= 3 with int32 offsets: the 32-bit-count form)
                out.add((idx64, (2, 8, 128, rec, True, False, 0)))
                out.add((idx64, (3, 8, 128, rec, True, False, 0)))
    return frozenset(out)


REACHABLE = _reachable()

# ------------------------------------------------------------------------------------------------------------ the shape table
# (m, M): the smallest shapes at which each boundary of the launcher and the epilogues exists; SHAPES are served by the fused-row
# kernel, GENERAL and REFUSED are the dispatch neighbours that are not
SHAPES = ((2, 102), (2, 204), (2, 205), (2, 256),
          (3, 68), (3, 136), (3, 137), (3, 213), (3, 214), (3, 227), (3, 228), (3, 256),
          (4, 51), (4, 102), (4, 103), (4, 127), (4, 128), (4, 204))
GENERAL = ((2, 101), (3, 67), (2, 257), (5, 100))       # Q = 203, 202 (256 slots), M = 257, m = 5: walk_sets_kernel<SPG>
REFUSED = (4, 205)                                      # Q = 821: a 2,048-slot table
WORKLIST_SHAPES = ((2, 204), (3, 214), (4, 128))        # a 512-slot, a 1,024-slot and a 64-bit shape

# what stands at each shape: {(m, M): {form: instantiation with int32 offsets and no records}}
SHAPE_TABLE = {
    (2, 102): {"table": (2, 4, 128, 0, False, False, 0), "keys32": (2, 8, 64, 0, True, True, 0)},
    (2, 204): {"table": (2, 4, 128, 0, False, False, 0), "keys32": (2, 8, 64, 0, True, True, 0)},
    (2, 205): {"table": (2, 8, 128, 0, True, False, 0), "keys32": (2, 8, 128, 0, True, True, 5)},
    (2, 256): {"table": (2, 8, 128, 0, True, False, 0), "keys32": (2, 8, 128, 0, True, True, 5)},
    (3, 68): {"table": (3, 4, 128, 0, False, False, 0), "keys32": (3, 4, 128, 0, True, True, 0)},
    (3, 136): {"table": (3, 4, 128, 0, False, False, 0), "keys32": (3, 4, 128, 0, True, True, 0)},
    (3, 137): {"table": (3, 8, 128, 0, True, False, 0), "keys32": (3, 8, 128, 0, True, True, 5)},
    (3, 213): {"table": (3, 8, 128, 0, True, False, 0), "keys32": (3, 8, 128, 0, True, True, 5)},
    (3, 214): {"table": (3, 8, 128, 0, True, False, 0), "keys32": (3, 8, 128, 0, True, True, 0)},
    (3, 227): {"table": (3, 8, 128, 0, True, False, 0), "keys32": (3, 8, 128, 0, True, True, 0)},
    (3, 228): {"table": (3, 8, 128, 0, True, False, 0), "keys32": (3, 8, 128, 0, True, True, 0)},
    (3, 256): {"table": (3, 8, 128, 0, True, False, 0), "keys32": (3, 8, 128, 0, True, True, 0)},
    (4, 51): {"table": (4, 4, 128, 0, False, False, 0), "keys32": (4, 4, 128, 0, True, True, 0)},
    (4, 102): {"table": (4, 4, 128, 0, False, False, 0), "keys32": (4, 4, 128, 0, True, True, 0)},
    (4, 103): {"table": (4, 4, 256, 0, False, False, 0), "keys32": (4, 8, 128, 0, True, True, 5)},
    (4, 127): {"table": (4, 4, 256, 0, False, False, 0), "keys32": (4, 8, 128, 0, True, True, 5)},
    (4, 128): {"table": (4, 4, 256, 0, False, False, 0), "keys64": (4, 8, 128, 0, False, True, 7)},
    (4, 204): {"table": (4, 4, 256, 0, False, False, 0), "keys64": (4, 8, 128, 0, False, True, 7)},
}


def forms_of(M, m):
    """the row forms the shape admits (tags: the batched registration works on 32-bit key rows)"""
    kf = "keys32" if key_bits(M, m) <= 31 else "keys64"
    return ("table", kf) + (("tags",) if kf == "keys32" else ())


def launches(M, m):
    """[(form, idx64, records)] the GPU file runs at a served shape: records = False, True (8 bytes with int32 offsets, 16 bytes with
    int64) or "narrow" (8-byte records whose degree field holds 8 bits: hubs take the escape path)"""
    return [(f, i, r) for f in forms_of(M, m) for i in (False, True) for r in ((False, True, "narrow") if not i else (False, True))]


def pitches(Q):
    """row_pitch values: 0 (the row capacity itself), a multiple of 32 above Q (wide_rows with an untouched tail), and -- where Q
    itself is a multiple of 4 -- Q + 1, so that the one-member-per-store path runs at every shape"""
    wide = (Q + 32) // 32 * 32
    return (0, wide) + ((Q + 1,) if Q % 4 == 0 else ())


def wide_rows(pitch, Q):
    """launch_walk's rule with 16-byte aligned row pointers (GUARD is a multiple of 4)"""
    return (pitch if pitch > 0 else Q) % 4 == 0


# --------------------------------------------------------------------------------------------- restatements: a row's branches
def first_hop(deg, M, cap=True):
    """the first hop of a root of out-degree `deg`: isolated / modulo (walk w takes neighbour w % deg) / shuffled (Fisher-Yates) /
    capped (shuffled over the first 1,000,000 neighbours)"""
    if deg == 0:
        return "isolated"
    if cap and deg > NEIGH_CAP:
        return "capped"
    return "shuffled" if deg > M else "modulo"


def reciprocal_is_exact(deg):
    """floor(w * ceil(2^16 / deg) / 2^16) == w // deg for every w < 256: what the modulo branch relies on"""
    inv = 65535 // deg + 1
    w = np.arange(256)
    return bool(np.array_equal((w * inv) >> 16, w // deg))


def level1(ids, T, NT):
    """(ns, B, bshift, bucket of every member, members of every bucket): level 1 of both epilogues' sorts"""
    ids = np.asarray(ids).astype(np.int64)
    ns = len(ids)
    assert ns >= 1
    logb = 0
    while (1 << logb) < ns and (2 << logb) <= T // 4 and (2 << logb) <= NT:
        logb += 1
    B = 1 << logb
    rng_ = int(ids.max() - ids.min()) + 1
    Ls = 0 if rng_ <= 1 else int(rng_ - 1).bit_length()
    bshift = Ls - logb if Ls > logb else 0
    bk = (ids - ids.min()) >> bshift
    assert bk.max() < B
    return ns, B, bshift, bk, np.bincount(bk, minlength=B)


def _part(ids, bshift, bk, counts, fine):
    """the level-2 index of every member: its bucket's first part + floor(offset in the bucket's window * parts / width)"""
    ids = np.asarray(ids).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(counts)])
    off = (ids - ids.min()) - (bk << bshift)
    kb = counts[bk] * fine
    sub = ((((off << (32 - bshift)) & 0xFFFFFFFF) * kb) >> 32) if bshift else np.zeros_like(off)
    assert (sub < np.maximum(kb, 1)).all()
    return start[bk] * fine + sub


def table_epilogue(ids, T, NT, K32, stride):
    """dict(ns, B, bshift, maxc, level2, staged) of a set in the table-form epilogue (walk_rows.hip, "the set leaves as a finished SpG
    row")"""
    ns, B, bshift, bk, counts = level1(ids, T, NT)
    maxc = int(counts.max())
    W2 = (ns + 2) // 2 + 1
    level2 = maxc > FINE_ABOVE and W2 <= 4 * NT and (not K32 or B + 1 + W2 <= T)
    staged = ns + B + 1 <= T and (not K32 or 12 * stride <= 8 * T)
    maxc2 = int(np.bincount(_part(ids, bshift, bk, counts, 1)).max()) if level2 else 0
    return dict(ns=ns, B=B, bshift=bshift, maxc=maxc, level2=bool(level2), staged=bool(staged), maxc2=maxc2)


def key_row_levels(ids, T, NT):
    """how many levels the key-row epilogue's sort runs for this set (1..3), with dict(ns, B, bshift, maxc, maxc2): one wave (NT = 64)
    has levels 1 and 2; two waves cut a bucket of k members into FINE * k parts and cut again above SG_SORT_AGAIN_ABOVE"""
    ns, B, bshift, bk, counts = level1(ids, T, NT)
    maxc = int(counts.max())
    info = dict(ns=ns, B=B, bshift=bshift, maxc=maxc, maxc2=0, levels=1)
    if maxc <= FINE_ABOVE:
        return info
    fine = 1 if NT == 64 else (2 * 4 * NT - 1) // (ns + 1)
    assert fine >= 1
    info["maxc2"] = int(np.bincount(_part(ids, bshift, bk, counts, fine)).max())
    info["levels"] = 3 if (NT > 64 and info["maxc2"] > AGAIN_ABOVE) else 2
    return info


def staged_edge(M, m, tup):
    """(the largest ns that is staged through LDS, the smallest that is not) of the table form's `ns + B + 1 <= T` at this shape, or None
    where no set of the shape reaches the edge"""
    _, SPL, NT = tup[:3]
    T = SPL * NT
    B = min(T // 4, NT)
    return (T - B - 1, T - B) if M * m + 1 >= T - B else None


# -------------------------------------------------------------------------------------------------------------------- graphs
N_IDS = 1 << 20              # node ids of the edge graphs: wide enough for a level-1 bucket of 16,384 ids (crowded)
RUN = 64                     # members of a run at most (B >= 64 from 33 members on: bshift == 0 in every instantiation)
POOL = 4096                  # the common pool of degree_ladder
HUB_DEG = 300                # out-degree of the pool's hub (a reached node whose degree does not fit 8 bits of a hop record)
SPREAD = 27                  # spread members of the crowded sets (27 + 24 = 51 neighbours: the smallest M of the shape table)
CROWD = (12, 13, 24)         # members packed into one level-1 bucket: level 1 only / level 2 / level 2 itself crowded
BUCKET_IDS = 1 << 14         # ids per level-1 bucket of a crowded set (64 buckets over 2^20 ids)


class _Builder:
    """edges over logical nodes; finish() gives every logical node an id -- the pinned ones theirs, the others a random free one"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.count, self.pinned, self.src, self.dst = 0, {}, [], []

    def new(self, k, ids=None):
        nodes = np.arange(self.count, self.count + k, dtype=np.int64)
        self.count += k
        if ids is not None:
            assert len(ids) == k
            self.pinned.update(zip(nodes.tolist(), np.asarray(ids).tolist()))
        return nodes

    def edges(self, src, dst):
        src, dst = np.broadcast_arrays(np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64))
        self.src.append(src.ravel().copy())
        self.dst.append(dst.ravel().copy())

    def finish(self, N):
        ids = np.full(self.count, -1, dtype=np.int64)
        pn, pi = np.array(list(self.pinned.keys()), dtype=np.int64), np.array(list(self.pinned.values()), dtype=np.int64)
        assert len(np.unique(pi)) == len(pi) and (pi >= 0).all() and (pi < N).all()
        ids[pn] = pi
        free = np.setdiff1d(np.arange(N, dtype=np.int64), pi)
        rest = np.nonzero(ids < 0)[0]
        ids[rest] = self.rng.permutation(free)[: len(rest)]
        src, dst = ids[np.concatenate(self.src)], ids[np.concatenate(self.dst)]
        order = np.argsort(src, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int32)
        return indptr, dst[order].astype(np.int32), ids


def degree_ladder(b, M):
    """one root of out-degree d for every d in 0 .. M + 2, plus 2M and 4M + 1; neighbours are distinct nodes of a common pool whose
    nodes have three out-edges into the pool (no dead ends) -- but pool[0], a hub of HUB_DEG out-edges that every tenth pool node
    points to.  -> (roots, their degrees)"""
    pool = b.new(POOL)
    b.edges(np.repeat(pool[1:], 3), pool[b.rng.integers(0, POOL, 3 * (POOL - 1))])
    b.edges(pool[0], pool[b.rng.permutation(POOL - 1)[:HUB_DEG] + 1])
    b.edges(pool[10::10], pool[0])
    degs = list(range(M + 3)) + [2 * M, 4 * M + 1]
    roots = b.new(len(degs))
    for r, d in zip(roots, degs):
        if d:
            b.edges(r, pool[b.rng.permutation(POOL)[:d]])
    return roots, np.array(degs)


def tree(b, M, m, ns=None, children=None):
    """a root with `children` (default M) children, every child the head of a chain of m - 1 further nodes of its own: every walk
    reaches m nodes no other walk reaches, ns == M * m + 1 exactly -- with more children than M the Fisher-Yates draw picks M of them.
    ns < Q: Q - ns chains end in chain 0's last node instead of their own (one member less each).  -> the root"""
    Q = M * m + 1
    children = children or M
    k = 0 if ns is None else Q - ns
    assert children >= M and 0 <= k <= M - 1 and (k == 0 or children == M) and m >= 2
    root = b.new(1)[0]
    chain = b.new(children * m).reshape(children, m)             # chain[j, d]: the node walk j stands on after hop d + 1
    b.edges(root, chain[:, 0])
    b.edges(chain[:, : m - 2], chain[:, 1: m - 1])
    last = chain[:, m - 1].copy()
    last[1: 1 + k] = chain[0, m - 1]
    b.edges(chain[:, m - 2], last)
    return root


def run(b, ns, base):
    """a root whose set is exactly the ids base .. base + ns - 1: the root (id base, or the last id with base > 0) points to all the
    others, every member to its successor -> the root"""
    nodes = b.new(ns, np.arange(base, base + ns))
    root = nodes[0] if base == 0 else nodes[-1]
    b.edges(root, nodes[nodes != root])
    b.edges(nodes, np.roll(nodes, -1))
    return root


def crowded(b):
    """three roots whose sets are SPREAD members over the whole id range -- at most one to a level-1 bucket of 16,384 ids, ids 64 and
    N - 65 among them -- and 12, 13 or 24 members of ONE bucket that holds nobody else: the first 20 on consecutive ids, the others
    3,000 ids apart.  Spread members point to each other, packed ones to spread ones: every set is closed.  -> the roots"""
    buckets = [x for x in range(1, 63) if x not in (20, 40, 41, 42)][:: 2][: SPREAD - 2]
    assert len(buckets) == SPREAD - 2
    s_ids = [RUN] + [RUN + x * BUCKET_IDS + 5000 for x in buckets] + [N_IDS - RUN - 1]
    zone = RUN + 20 * BUCKET_IDS
    p_ids = [zone + i for i in range(20)] + [zone + 3000 * i for i in range(1, 5)]
    S, P = b.new(SPREAD, s_ids), b.new(24, p_ids)
    roots = b.new(3, [RUN + (40 + i) * BUCKET_IDS + 7 for i in range(3)])
    b.edges(S, np.roll(S, -1))
    b.edges(S, np.roll(S, -7))
    b.edges(P, S[0])
    b.edges(P, S[1])
    for r, k in zip(roots, CROWD):
        b.edges(r, np.concatenate([S, P[:k]]))
    return roots


def self_loop(b):
    """a root whose only edge is its own loop; a root with a loop and one neighbour (which points back); a root whose only neighbour
    has nothing but its own loop -> the three roots"""
    a, c, x, d, y = b.new(5)
    b.edges([a, c, c, x, d, y], [a, c, x, c, y, y])
    return np.array([a, c, d])


@functools.lru_cache(maxsize=None)
def edge_graph(M, m):
    """The directed graph of one shape: degree_ladder(M), tree(M, m) (modulo and shuffled roots, and the trimmed trees on both sides of
    the staging edge where the shape reaches it), run (base 0 and base N - ns), crowded, self_loop -- disjoint, no dead ends (a walk
    never stands on a node without out-edges while it has hops left: both RNG modes run the fused-row kernel on it).
    -> dict(indptr, indices, num_nodes, roots = {name: node ids}, degrees = the ladder's, batch = the roots of the GPU launches)"""
    b = _Builder([M, m])
    Q = M * m + 1
    ladder, degs = degree_ladder(b, M)
    trees = {"tree": tree(b, M, m), "tree_shuffled": tree(b, M, m, children=M + 3)}
    for idx64 in (False, True):                                   # (the int64 table form of a 1,024-slot shape has 256 lanes)
        tup = variant(M, m, "table", idx64)
        e = staged_edge(M, m, tup) if tup else None
        if e and f"tree_{e[0]}" not in trees:
            trees[f"tree_{e[0]}"], trees[f"tree_{e[1]}"] = tree(b, M, m, ns=e[0]), tree(b, M, m, ns=e[1])
    rs = min(M + 1, RUN)
    runs = np.array([run(b, rs, 0), run(b, rs, N_IDS - rs)])
    crowd = crowded(b)
    loops = self_loop(b)
    indptr, indices, ids = b.finish(N_IDS)
    roots = {"ladder": ids[ladder], "run": ids[runs], "crowded": ids[crowd], "self_loop": ids[loops]}
    roots.update({k: ids[[v]] for k, v in trees.items()})
    assert roots["run"].tolist() == [0, N_IDS - 1]                # the first and the last node id are roots
    order = ["ladder"] + sorted(trees) + ["run", "crowded", "self_loop"]
    batch = np.concatenate([roots[k] for k in order] + [roots["ladder"][[5, 5]], roots["run"][:1], roots["tree"]])      # repeated roots
    where, at = {}, 0
    for k in order:
        where[k] = np.arange(at, at + len(roots[k]))
        at += len(roots[k])
    return dict(indptr=indptr, indices=indices, num_nodes=N_IDS, roots=roots, rows=where, degrees=degs,
                batch=batch.astype(np.int32), Q=Q)


@functools.lru_cache(maxsize=None)
def dead_ends(M, m):
    """A small directed graph with dead ends: for every s in 1 .. m - 1 a root whose walks all stop after hop s (chains of s nodes, the
    last without out-edges), a root that is itself the owner of the LAST adjacency entry (the kernel clamps dropped loads to it),
    and 200 nodes of a pool of 600 in which every fifth node has one edge, into a dead end.  The dead ends have the highest ids:
    their rows begin at nnz.  -> as edge_graph"""
    b = _Builder([M, m, 1])
    N = 3000
    dead = b.new(400, np.arange(N - 400, N))                      # never a source
    pool = b.new(600)
    live = pool[np.arange(600) % 5 != 0]
    tgt = np.concatenate([pool, dead[:100]])
    b.edges(np.repeat(live, 3), tgt[b.rng.integers(0, len(tgt), 3 * len(live))])
    b.edges(pool[::5], dead[100:220])                              # every fifth pool node: one edge, into a dead end
    stops, used = [], 220
    for s in range(1, m):
        r = b.new(1)[0]
        heads = b.new(7 * s).reshape(7, s)
        b.edges(r, heads[:, 0])
        b.edges(heads[:, : s - 1], heads[:, 1:])
        b.edges(heads[:, s - 1], dead[used: used + 7])
        used += 7
        stops.append(r)
    owner = b.new(1, [N - 401])[0]                                # the last node with out-edges: its row ends at nnz
    b.edges(owner, np.concatenate([dead[300:303], pool[:2]]))
    indptr, indices, ids = b.finish(N)
    assert indptr[N - 400] == indptr[N] == len(indices) and indptr[N - 401] < indptr[N - 400]
    roots = {"stops": ids[np.array(stops)], "owner": ids[[owner]], "pool": ids[pool[:200]], "dead": ids[dead[:3]]}
    order = ["stops", "owner", "pool", "dead"]
    batch = np.concatenate([roots[k] for k in order])
    where, at = {}, 0
    for k in order:
        where[k] = np.arange(at, at + len(roots[k]))
        at += len(roots[k])
    return dict(indptr=indptr, indices=indices, num_nodes=N, roots=roots, rows=where, batch=batch.astype(np.int32), Q=M * m + 1)


HUB_NODES = 1_000_100


@functools.lru_cache(maxsize=None)
def hub_cap():
    """two roots of out-degree 1,000,000 (node 0) and 1,000,001 (node 1) in a graph of 1,000,100 nodes whose other nodes have one
    out-edge each; a handful of roots"""
    N = HUB_NODES
    others = np.arange(2, N, dtype=np.int64)
    deg = np.ones(N, dtype=np.int64)
    deg[0], deg[1] = NEIGH_CAP, NEIGH_CAP + 1
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    indices = np.concatenate([np.arange(100, 100 + NEIGH_CAP), np.arange(99, 100 + NEIGH_CAP), (others * 7919 + 13) % (N - 2) + 2])
    batch = np.array([0, 1, 5, 1, 0, N - 1], dtype=np.int32)
    return dict(indptr=indptr, indices=indices.astype(np.int32), num_nodes=N, batch=batch, degrees=deg[batch])


def symmetric(g):
    """the same graph with every edge in both directions and no self loops (scipy's A + A.T), as the reference's loader makes them"""
    import scipy.sparse as sps
    N = g["num_nodes"]
    A = sps.csr_matrix((np.ones(len(g["indices"])), g["indices"], g["indptr"]), shape=(N, N))
    A = sps.csr_matrix(A + A.T)
    A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    return dict(g, indptr=A.indptr.astype(np.int32), indices=A.indices.astype(np.int32))


def out_degree(g, nodes):
    return np.diff(g["indptr"])[np.asarray(nodes)]


# ------------------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
@functools.lru_cache(maxsize=None)
def symmetric_edge_graph(M, m):
    """edge_graph(M, m) as the reference's loader would hand it over: every edge in both directions, no self loops (the self-loop
    roots become a node without edges, a pair and a pair; the ladder's pool nodes gain the degrees of hubs)"""
    return symmetric(edge_graph(M, m))


def graph(kind, M, m):
    return {"edge": edge_graph, "dead": dead_ends, "sym": symmetric_edge_graph}[kind](M, m) if kind != "hub" else hub_cap()


@functools.lru_cache(maxsize=None)
def _oracle(kind, M, m, rng, seed, bucket):
    import oracle
    g = graph(kind, M, m)
    return tuple(oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, bucket=bucket, seed=seed, rng=rng))


def lp_keys(enc, M, m):
    """the packed LP key (include/subgacc.h: count of step j in bits [(m - j) * SHIFT, + SHIFT), LEAD = bit m * SHIFT on the root's
    row) of every row of the oracle's enc [c, m + 1], as uint64"""
    s = key_shift(M)
    e = np.asarray(enc).astype(np.uint64)
    key = (e[:, 0] != 0).astype(np.uint64) << np.uint64(m * s)
    for j in range(1, m + 1):
        key |= e[:, j] << np.uint64((m - j) * s)
    return key


def expected_rows(kind, M, m, rng, seed=13, bucket=-1):
    """THE reference, computed once per (graph, shape, rng) and shared: the oracle's sets as finished rows --
    dict(nsize [n], off [n + 1], ids [X] ascending inside every row, keys [X] uint64 the member's LP key, sf [X] its row in enc,
    ukeys [c] the distinct LP keys in the oracle's first-occurrence order)"""
    nsize, remap, enc = _oracle(kind, M, m, rng, seed, bucket)
    off = np.concatenate([[0], np.cumsum(nsize)]).astype(np.int64)
    rowid = np.repeat(np.arange(len(nsize)), nsize)
    order = np.lexsort((remap[0], rowid))
    ukeys = lp_keys(enc, M, m)
    assert len(np.unique(ukeys)) == len(ukeys)
    sf = remap[1][order]
    out = dict(nsize=nsize, off=off, ids=remap[0][order], sf=sf, keys=ukeys[sf], ukeys=ukeys, visit_sf=remap[1].copy())
    for v in out.values():
        v.setflags(write=False)
    return out


def row_of(exp, i):
    return exp["ids"][exp["off"][i]: exp["off"][i + 1]]


def numbering_of(exp, rows):
    """the distinct LP keys of the listed rows in first-occurrence order -- rows in ascending row number, members in first-visit order:
    what the table of distinct rows numbers when only these rows were sampled (all rows: the oracle's own enc)"""
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    sf = np.concatenate([exp["visit_sf"][exp["off"][i]: exp["off"][i + 1]] for i in rows] + [np.zeros(0, np.int32)])
    _, first = np.unique(sf, return_index=True)
    return exp["ukeys"][sf[np.sort(first)]]

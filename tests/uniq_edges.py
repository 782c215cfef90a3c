"""Inputs and host restatements for the edge tests of csrc/uniq.hip and csrc/uniq_table.hpp (tests/test_uniq_edges_cpu.py shows on the
host that every input is what it claims, tests/test_gpu_uniq_edges.py runs them on the GPU).  NumPy only; no GPU is needed here.

Two tables.  The table of distinct LP rows: `cap` slots (a power of two) in HBM, a key's home is mix64(key) & (cap - 1), probing
steps by one, wraps at `cap` and gives up after MAX_PROBES slots (flags[2] |= 1); in front of it every insert block folds its tile of
INS_TILE keys into an LDS table of LDS_SLOTS slots, home (mix64(key) >> 40) & 1023, and gives up after LDS_WINDOW slots -- such a key
goes straight to HBM.  The stamped table of the root-dedup prologue: dedup_slots(n) slots, a root's home is the top bits of
uint32(root) * 2654435761, probing steps by one and wraps."""
import numpy as np

EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)        # kEmptyKey: marks a free slot and is not a key
MAX_PROBES = 128                                 # kMaxProbes
LDS_SLOTS, LDS_WINDOW = 1024, 16                 # kInsLds and the probe window of the fold
INS_TILE, UNIQ_TILE = 2048, 1024                 # kInsTile, kUniqTile
NO_ROOT = -2 ** 31                               # SUBGACC_NO_ROOT
POOL = 1 << 20                                   # the key families are filtered out of arange(1, POOL)
ROLE_BLOCKS = {(2, 2): (0, 1), (3, 4): (0, 2, 1, 2)}      # segment block -> root block: pairs u, v; triplets u, w, v, w


# ------------------------------------------------------------------------------------------------------------- the hashes
def mix64(keys):
    x = np.array(keys, dtype=np.uint64, copy=True).reshape(-1)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def hbm_home(keys, cap):
    return (mix64(keys) & np.uint64(cap - 1)).astype(np.int64)


def lds_home(keys):
    return ((mix64(keys) >> np.uint64(40)) & np.uint64(LDS_SLOTS - 1)).astype(np.int64)


def root_home(roots, c):
    log2 = int(c).bit_length() - 1
    assert 1 << log2 == c
    r = np.asarray(roots, dtype=np.int64).astype(np.uint32).astype(np.uint64)
    return (((r * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - log2)).astype(np.int64)


def dedup_slots(n):
    c = 1024
    while c < 2 * n:
        c <<= 1
    return c


# ------------------------------------------------------------------------------------------------------------- key families
_POOL = {}


def _pool():
    if "keys" not in _POOL:
        _POOL["keys"] = np.arange(1, POOL, dtype=np.uint64)
        _POOL["mix"] = mix64(_POOL["keys"])
    return _POOL["keys"], _POOL["mix"]


def same_hbm_home(k, cap, home):
    """the k smallest keys of the pool whose home in a table of `cap` slots is `home`"""
    keys, mix = _pool()
    hit = keys[(mix & np.uint64(cap - 1)) == np.uint64(home)]
    assert len(hit) >= k
    return hit[:k].copy()


def same_lds_home(k, home, distinct_hbm_cap):
    """k keys of the pool with LDS home `home` whose homes in an HBM table of `distinct_hbm_cap` slots differ pairwise"""
    keys, mix = _pool()
    hit = keys[((mix >> np.uint64(40)) & np.uint64(LDS_SLOTS - 1)) == np.uint64(home)]
    _, first = np.unique(hbm_home(hit, distinct_hbm_cap), return_index=True)
    first.sort()
    assert len(first) >= k
    return hit[first[:k]].copy()


def same_root_home(k, c, home):
    """the k smallest node ids of the pool whose home in a prologue table of c slots is `home`"""
    ids = np.arange(1, POOL, dtype=np.int64)
    hit = ids[root_home(ids, c) == home]
    assert len(hit) >= k
    return hit[:k].copy()


def chain_end(homes, cap):
    """linear probing, one key per entry of `homes` in turn: (slots taken in all, longest probe count)"""
    taken = np.zeros(cap, dtype=bool)
    longest = 0
    for h in homes:
        p = 0
        while taken[(h + p) % cap]:
            p += 1
        taken[(h + p) % cap] = True
        longest = max(longest, p + 1)
    return taken, longest


# ------------------------------------------------------------------------------------------------------------- references
def ref_uniq(keys):
    """-> (sf int32 [n], ukeys uint64 [c], first_pos int64 [c]): the distinct keys numbered by the position of their first occurrence"""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.uint64), np.zeros(0, np.int64)
    u, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(u), dtype=np.int64)
    rank[order] = np.arange(len(u))
    return rank[inv.reshape(-1)].astype(np.int32), u[order], first[order].astype(np.int64)


def key_shift(M):
    return int(M).bit_length()


def ref_unpack(keys, M, m):
    """-> int64 [n, m + 1]: column 0 = M where the LEAD bit (bit m*shift) is set, column j the j-th field from the top"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    shift = key_shift(M)
    out = np.zeros((len(keys), m + 1), dtype=np.int64)
    out[:, 0] = np.where((keys >> np.uint64(m * shift)) & np.uint64(1), M, 0)
    for j in range(1, m + 1):
        out[:, j] = ((keys >> np.uint64((m - j) * shift)) & np.uint64((1 << shift) - 1)).astype(np.int64)
    return out


def ref_unpack_f32(keys, M, m):
    return ref_unpack(keys, M, m).astype(np.float32) / np.float32(M)


def pack_rows(rows, M, m):
    """ref_unpack's inverse: rows [n, m + 1] (column 0 zero or not) -> uint64 keys"""
    rows = np.asarray(rows).astype(np.int64)
    shift = key_shift(M)
    assert m * shift + 1 <= 64 and rows.shape[1] == m + 1
    assert (rows[:, 1:] >= 0).all() and (rows[:, 1:] < (1 << shift)).all()
    keys = (rows[:, 0] != 0).astype(np.uint64) << np.uint64(m * shift)
    for j in range(1, m + 1):
        keys |= rows[:, j].astype(np.uint64) << np.uint64((m - j) * shift)
    return keys


def random_keys(rng, n, M, m, lead):
    """n keys whose fields stay within the shift; lead: None = the LEAD bit at random, else set / clear"""
    shift = key_shift(M)
    rows = rng.integers(0, 1 << shift, size=(n, m + 1))
    rows[:, 0] = rng.integers(0, 2, size=n) if lead is None else int(lead)
    keys = pack_rows(rows, M, m)
    assert not (keys == EMPTY_KEY).any()
    return keys


def narrow(edge):
    """int64 ids -> the int32 roots of the sampler: an id outside [0, 2^31 - 1] becomes -1"""
    v = np.asarray(edge, dtype=np.int64).reshape(-1)
    return np.where((v < 0) | (v > 0x7FFFFFFF), -1, v).astype(np.int32)


def _first_rows(edge):
    r = narrow(edge)
    _, first, inv = np.unique(r, return_index=True, return_inverse=True)
    return r, first[inv.reshape(-1)].astype(np.int64)


def ref_dedup(edge):
    """-> roots int32 [n], own int64 [n], partner int64 [n], row_len_zeroed_mask bool [n], n_distinct (pairs: edge = [u.. | v..])"""
    r, row = _first_rows(edge)
    n = len(r)
    assert n % 2 == 0
    is_first = row == np.arange(n)
    roots = np.where(is_first, r, NO_ROOT).astype(np.int32)
    partner = np.r_[row[n // 2:], row[:n // 2]]
    return roots, row, partner, ~is_first, int(is_first.sum())


def ref_dedup_roles(edge, B, r, s):
    """-> roots int32 [r*B], own int64 [s*B], row_len_zeroed_mask, n_distinct: first occurrences over the WHOLE root list"""
    rt, row = _first_rows(edge)
    n = len(rt)
    assert n == r * B
    is_first = row == np.arange(n)
    roots = np.where(is_first, rt, NO_ROOT).astype(np.int32)
    own = np.concatenate([row[b * B:(b + 1) * B] for b in ROLE_BLOCKS[(r, s)]])
    return roots, own, ~is_first, int(is_first.sum())


# ------------------------------------------------------------------------------------------------------------- the inputs
INSERT_SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 2048 + 5]
KEY_SETS = ["equal", "distinct", "of37"]


def sized_keys(n, kind, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "equal":
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    if kind == "distinct":
        return rng.permutation(np.arange(7, 7 + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    vals = rng.integers(0, 1 << 63, size=37, dtype=np.uint64)
    vals[0], vals[1] = 0, 0xFFFFFFFFFFFFFFFE          # the two ends of the key range are keys like any other
    return vals[rng.integers(0, 37, size=n)]


def lds_crowd(split):
    """40 keys of one LDS home, each twice, among 300 other keys (with repeats): in one insert tile (split False), or laid over
    the edge between tile 0 and tile 1, every one of them once among the last 40 keys of tile 0 and once among the first 40 of
    tile 1 (split True).
    -> (keys, the 40)"""
    rng = np.random.default_rng(40)
    crowd = same_lds_home(40, 517, 4096)
    others = rng.integers(1 << 32, 1 << 62, size=150, dtype=np.uint64)
    others = others[rng.integers(0, 150, size=300)]
    if not split:
        keys = rng.permutation(np.r_[crowd, crowd, others])
        assert len(keys) <= INS_TILE
        return keys, crowd
    left = np.r_[others[rng.integers(0, 300, size=INS_TILE - 40)], crowd[:20], crowd[39:19:-1]]
    right = np.r_[crowd[20:], crowd[19::-1], others]
    return np.r_[left, right], crowd


def chain_keys(k, cap, home, spread):
    """k keys of one HBM home; spread: repeated and laid over several insert tiles with fillers of the SAME keys (nothing else
    enters the table)"""
    keys = same_hbm_home(k, cap, home)
    if not spread:
        return keys
    rng = np.random.default_rng(k)
    n = 2 * INS_TILE + 300
    out = keys[rng.integers(0, k, size=n)]
    out[rng.permutation(n)[:k]] = keys                 # every key at least once
    return out


def first_at(positions, n):
    """n keys whose first occurrences stand exactly at `positions` (0 among them); every other element repeats an earlier key"""
    positions = sorted(positions)
    assert positions[0] == 0 and positions[-1] < n
    rng = np.random.default_rng(n)
    keys = np.empty(n, dtype=np.uint64)
    seen = 0
    nxt = set(positions)
    for e in range(n):
        if e in nxt:
            keys[e] = np.uint64(0xABCD0000 + 977 * seen)
            seen += 1
        else:
            keys[e] = np.uint64(0xABCD0000 + 977 * int(rng.integers(0, seen)))
    return keys


def repeated(c, n, seed=0):
    """n >= c elements over exactly c distinct keys, first occurrences scattered"""
    rng = np.random.default_rng(c * 31 + seed)
    vals = rng.permutation(np.arange(1, c + 1, dtype=np.uint64)) * np.uint64(0x100000001B3)
    keys = vals[rng.integers(0, c, size=n)]
    keys[rng.permutation(n)[:c]] = vals
    return keys


def pair_batch(B, kind, seed=0):
    """int64 [2B] = [u.. | v..]"""
    rng = np.random.default_rng(B * 7 + seed)
    n = 2 * B
    if kind == "one":
        return np.full(n, 4242, dtype=np.int64)
    if kind == "distinct":
        return rng.permutation(np.arange(100, 100 + n, dtype=np.int64) * 3)
    if kind == "random":                                # about half of the endpoints repeat
        return rng.integers(0, max(2, n // 2), size=n).astype(np.int64) * 11
    if kind == "self":                                  # u == v in every other pair
        e = rng.integers(0, 5 * n, size=n).astype(np.int64)
        e[B::2] = e[:B:2]
        return e
    if kind == "ends":                                  # the ids 0 and 2^31 - 1, as first and as repeated endpoints
        e = rng.integers(1, 1000, size=n).astype(np.int64)
        e[rng.permutation(n)[:min(n, 6)]] = np.array([0, 0x7FFFFFFF, 0, 0x7FFFFFFF, 0x7FFFFFFF, 0])[:min(n, 6)]
        return e
    if kind == "outside":                               # -1, -5, 2^31 and 2^40: all root -1, one first occurrence
        e = rng.integers(1, 1000, size=n).astype(np.int64)
        bad = np.array([-5, 1 << 31, -1, 1 << 40, -1, 1 << 40, -5, 1 << 31])
        e[np.sort(rng.permutation(n)[:min(n, 8)])] = bad[:min(n, 8)]
        return e
    raise KeyError(kind)


def triplet_batch(B, seed=0):
    """int64 [3B] = [u.. | v.. | w..]: negatives keep (u, v) of their positive, and some node is u of one triplet and w of another"""
    rng = np.random.default_rng(B * 13 + seed)
    u = rng.integers(0, max(2, B // 2), size=B).astype(np.int64)
    v = rng.integers(0, max(2, B // 2), size=B).astype(np.int64) + 5000
    w = rng.integers(0, 3 * B + 2, size=B).astype(np.int64) + 9000
    w[B // 2] = u[0]
    return np.r_[u, v, w]


def colliding_batch(c, B, seed=0):
    """int64 [2B] for a table of c slots: 40 roots whose home is the LAST slot, each twice, among 2B - 80 others -> (edge, the 40)
    (c = 1,024 takes 2B <= 512, c = 2,048 takes 512 < 2B <= 1,024: dedup_slots)"""
    assert dedup_slots(2 * B) == c
    rng = np.random.default_rng(c + seed)
    crowd = same_root_home(40, c, c - 1)
    others = rng.integers(0, 1 << 20, size=2 * B - 80).astype(np.int64)
    return rng.permutation(np.r_[crowd, crowd, others]), crowd

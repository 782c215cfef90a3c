"""Inputs and host restatements for the edge tests of csrc/keyrows.hip (tests/test_keyrows_edges_cpu.py shows on the host that every
input is what it claims, tests/test_gpu_keyrows_edges.py runs them on the GPU).  NumPy only; no GPU and no torch is needed here.

The pass.  A block owns a range of rows_per_block(n) rows and one dictionary in LDS: DICT entries, a key's home is kr_home(key),
probing steps by one, wraps at DICT and gives up after PROBES slots -- such a key is registered in (or asked from) the HBM table by
the member itself.  The look-up forms preload at most DICT_MAX numbered keys.  The rows that lowered a tag are collected in a bitmap of
one bit per row of the range.  A row is loaded in groups of GROUP members; the translate pass takes TRANSLATE_BLOCK entries per block,
16 bytes at a time.

Key rows: (ids int32 [n*stride], keys int32 [n*stride], nsize int32 [n]); row i is [i*stride, +min(nsize[i], stride)), the slots
behind it hold ID_POISON / KEY_POISON, which no row uses as a key.  A key is the 32-bit pattern, zero-extended in the HBM table."""
import numpy as np

DICT_BITS = 12                                   # kKrDictBits
DICT = 1 << DICT_BITS                            # kKrDict
DICT_MAX = DICT * 3 // 4                         # kKrDictMax
PROBES = 32                                      # kKrProbes
MAX_ROWS = 4096                                  # kKrMaxRows: rows per block at most (the candidate bitmap)
MIN_ROWS = 32                                    # the lower clamp of the rows per block in keyrows_launch
RANGES = 4 * 256 * 4                             # rows per block = n / RANGES before the clamps (keyrows_launch)
WAVES = 8                                        # kKrWaves = kKrThreads / kWave = 512 / 64
GROUP = 8 * 64                                   # kKrUnroll * kWave: the members of a row whose loads are in flight together
TRANSLATE_BLOCK = 512 * 4 * 8                    # kKrThreads * 4 * 8: entries per block of the translate pass
EMPTY_ENTRY = 0xFFFFFFFF                         # kKrEmpty: marks a free dictionary entry and is not a key
KEY_POISON, ID_POISON = 0x7E7E7E7E, -0x01010102  # the slots of a strided row behind nsize[i]
POOL = 1 << 20                                   # the key families are filtered out of arange(1, POOL)
_M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------- the hash
def kr_home(keys):
    """kr_home of keyrows.hip on the 32-bit patterns of `keys`"""
    h = np.asarray(keys).astype(np.int64).astype(np.uint64).reshape(-1) & _M32
    h = (h * np.uint64(0x9E3779B1)) & _M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA77)) & _M32
    return (h >> np.uint64(32 - DICT_BITS)).astype(np.int64)


def rows_per_block(n):
    return min(max(n // RANGES, MIN_ROWS), MAX_ROWS)


_POOL = {}


def same_home(k, home):
    """the k smallest keys of [1, POOL) whose kr_home is `home`"""
    if "keys" not in _POOL:
        _POOL["keys"] = np.arange(1, POOL, dtype=np.uint32)
        _POOL["home"] = kr_home(_POOL["keys"])
    hit = _POOL["keys"][_POOL["home"] == home]
    assert len(hit) >= k
    return hit[:k].copy()


def dict_leftover(keys):
    """a sequential dictionary of DICT entries and PROBES probes, the distinct `keys` in the order given -> how many find no place"""
    taken = np.zeros(DICT, dtype=bool)
    left = 0
    for h in kr_home(keys).tolist():
        for p in range(PROBES):
            s = (h + p) & (DICT - 1)
            if not taken[s]:
                taken[s] = True
                break
        else:
            left += 1
    return left


# ------------------------------------------------------------------------------------------------------------- strided rows
def strided(rows, stride, nsize=None):
    """rows: one array of uint32 keys per row (len <= stride) -> (ids, keys, nsize); `nsize` overrides the lengths (an entry above
    `stride` is read as `stride`: that row must come with `stride` keys)"""
    n = len(rows)
    keys = np.full((n, stride), KEY_POISON, dtype=np.uint32)
    ids = np.full((n, stride), ID_POISON, dtype=np.int32)
    lens = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(rows):
        r = np.asarray(r, dtype=np.uint32)
        assert len(r) <= stride and not (r == KEY_POISON).any() and not (r == EMPTY_ENTRY).any()
        keys[i, :len(r)] = r
        ids[i, :len(r)] = (i * 7919 + np.arange(len(r)) * 31 + 1) & 0x7FFFFFFF
        lens[i] = len(r)
    if nsize is not None:
        nsize = np.asarray(nsize, dtype=np.int32)
        assert np.array_equal(np.minimum(nsize, stride), lens)
        lens = nsize
    return ids.reshape(-1), keys.reshape(-1).view(np.int32), lens


def _live(nsize, stride):
    """-> (e int64: the flat slots of the live members in store order, ns: the clamped lengths)"""
    ns = np.minimum(np.asarray(nsize, dtype=np.int64), stride)
    if stride == 1:
        return np.flatnonzero(ns > 0), ns
    live = np.arange(stride, dtype=np.int64)[None, :] < ns[:, None]
    return np.flatnonzero(live.reshape(-1)), ns


def row_offsets(nsize, stride):
    """-> int64 [n + 1]: the packed place of every row, from the clamped lengths"""
    ns = np.minimum(np.asarray(nsize, dtype=np.int64), stride)
    return np.r_[0, np.cumsum(ns)].astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- references
def ref_register(keys, nsize, stride, root_base=0):
    """-> dict: keys uint64 [c] ascending (zero-extended), f / r int64 [c] (first row, first position in it), coarse / exact uint64 [c]
    (the tags), number int64 [c] (rank by exact tag: the reference's first-occurrence order, subg_acc.c:957-978), ukeys uint64 [c]
    (the keys in number order), first_rows int64 (the distinct f)"""
    e, _ = _live(nsize, stride)
    kv = np.asarray(keys).view(np.uint32)[e].astype(np.uint64)
    u, first = np.unique(kv, return_index=True)          # the first index in store order: the smallest (row, position)
    fe = e[first]
    f, r = fe // stride, fe % stride
    exact = ((root_base + f) * stride + r).astype(np.uint64)
    coarse = ((root_base + f) * stride + stride - 1).astype(np.uint64)
    order = np.argsort(exact, kind="stable")
    number = np.empty(len(u), dtype=np.int64)
    number[order] = np.arange(len(u))
    return {"keys": u, "f": f, "r": r, "coarse": coarse, "exact": exact, "number": number, "ukeys": u[order],
            "first_rows": np.unique(f), "first_slot": int(e[0]) if len(e) else -1}


def _payload(kv, ukeys):
    """number + 1 of every key of kv (uint64) under the numbering `ukeys`; 0 for a key that is not in it"""
    ukeys = np.asarray(ukeys, dtype=np.uint64)
    if len(ukeys) == 0:
        return np.zeros(len(kv), dtype=np.int32)
    order = np.argsort(ukeys, kind="stable")
    su = ukeys[order]
    at = np.minimum(np.searchsorted(su, kv), len(su) - 1)
    return np.where(su[at] == kv, order[at] + 1, 0).astype(np.int32)


def ref_compact(ids, keys, nsize, stride, row_off, ukeys=None):
    """-> (out_indices, out_data int32 [row_off[n]]): row i packed at row_off[i]; the payload is number + 1 under `ukeys`, or
    (ukeys None) the key itself"""
    e, ns = _live(nsize, stride)
    row_off = np.asarray(row_off, dtype=np.int64)
    dst = row_off[e // stride] + e % stride
    total = int(row_off[len(ns)])
    oi, od = np.zeros(total, dtype=np.int32), np.zeros(total, dtype=np.int32)
    kv = np.asarray(keys).view(np.uint32)[e]
    oi[dst] = np.asarray(ids)[e]
    od[dst] = kv.view(np.int32) if ukeys is None else _payload(kv.astype(np.uint64), ukeys)
    assert len(np.unique(dst)) == len(dst) == total
    return oi, od


def ref_translate(data, n_eff, ukeys):
    """data int32 (keys) -> a copy whose first n_eff entries are number + 1 (0: a key that is in no table)"""
    out = np.array(data, dtype=np.int32, copy=True)
    n_eff = max(0, min(len(out), int(n_eff)))
    out[:n_eff] = _payload(out[:n_eff].view(np.uint32).astype(np.uint64), ukeys)
    return out


def range_census(keys, nsize, stride):
    """-> (the most distinct keys any block range shows, the sum of the distinct keys over the ranges): with at most PROBES keys in
    every range no probe chain can be longer than PROBES, so nothing is crowded and every dictionary entry is flushed once -- a
    range lists at most one candidate per distinct key"""
    e, ns = _live(nsize, stride)
    if len(e) == 0:
        return 0, 0
    kv = np.asarray(keys).view(np.uint32)[e].astype(np.uint64)
    block = (e // stride // rows_per_block(len(ns))).astype(np.uint64)
    pairs = np.unique((block << np.uint64(32)) | kv)
    per = np.bincount((pairs >> np.uint64(32)).astype(np.int64))
    return int(per.max()), int(per.sum())


def standin_keys(keys, nsize, stride, lo, hi, listed, filler):
    """the stand-in for the walk of the candidates (chunk of rows lo .. hi): uint64 [(hi - lo)*stride], the live members of the
    `listed` rows (numbers inside the chunk) with their keys, `filler` everywhere else"""
    ns = np.minimum(np.asarray(nsize[lo:hi], dtype=np.int64), stride)
    k = np.asarray(keys).view(np.uint32)[lo * stride:hi * stride].astype(np.uint64).reshape(hi - lo, stride)
    on = np.zeros(hi - lo, dtype=bool)
    on[np.asarray(listed, dtype=np.int64)] = True
    live = (np.arange(stride, dtype=np.int64)[None, :] < ns[:, None]) & on[:, None]
    return np.where(live, k, np.uint64(filler)).reshape(-1)


# ------------------------------------------------------------------------------------------------------------- the inputs
FAMILY = np.array([0, 1, 0x7FFFFFFF, 5, 77, 0x12345, 0x40000000, 3, 900, 0x7FFFFFFE, 2, 0x00FF00FF, 31, 32, 33, 4096, 65535, 65536,
                   0x3FFFFFFF, 1000003], dtype=np.uint32)        # 20 keys: 0, 1 and 2^31 - 1 are keys like any other
SMALL_N = [1, 7, 8, 9, 31, 32, 33, 65]           # around kKrWaves = 8 rows (one per wave) and MIN_ROWS = 32 rows (one block range)
SMALL_STRIDE = 12


def small_store(n, kind="mixed"):
    """n rows at stride 12 over the 20 keys of FAMILY; mixed: empty rows at the front, in the middle and at the end of a range
    (and of the store); empty: no row has a member"""
    rng = np.random.default_rng(n)
    lens = rng.integers(1, SMALL_STRIDE + 1, size=n)
    if kind == "empty":
        lens[:] = 0
    elif n >= 7:
        lens[[0, n // 2, min(MIN_ROWS - 1, n - 1)]] = 0
        if n > MIN_ROWS:
            lens[[MIN_ROWS, n - 1]] = 0
    rows = [FAMILY[rng.integers(0, len(FAMILY), size=l)] for l in lens]
    return strided(rows, SMALL_STRIDE) + (SMALL_STRIDE,)


LONG_STRIDE = 2 * GROUP + 1                      # 1025: two whole load groups and one member
LONG_NS = [1, 63, 64, 65, GROUP - 1, GROUP, GROUP + 1, LONG_STRIDE]      # around a wave's 64 lanes and the group of 512


def long_rows(ns):
    """10 rows of length ns at stride 1025 (row 5 is empty, row 7 claims nsize = stride + 5 and is read as `stride`); first
    appearances stand at the positions 0, 511, 512 and ns - 1 of rows 0 and 2 (where the row is that long) -- row 2 hands its new
    keys out in descending order, so the numbering depends on the position inside the row --, in row 1 (up to four keys of its own) and at the position stride - 1 of row 7"""
    marks = sorted({p for p in (0, GROUP - 1, GROUP, ns - 1) if p < ns})
    rows, fresh = [], 1000
    for i in range(10):
        if i == 5:
            rows.append(np.zeros(0, np.uint32))
            continue
        row = np.full(LONG_STRIDE if i == 7 else ns, 500, dtype=np.uint32)      # 500: everybody's key, first at row 0, position 0
        if i in (0, 2):
            for p in (marks if i == 0 else marks[::-1]):                        # row 2 hands them out in the opposite order
                row[p] = fresh if not (i == 0 and p == 0) else 500
                fresh += 1
        elif i == 7:
            row[ns:] = 3000                                                     # nothing new behind ns, but for the last slot
            row[LONG_STRIDE - 1] = 2000 if ns < LONG_STRIDE else 3000
        else:
            row[:] = 3000 + (np.arange(len(row)) * 7 + i) % 4                   # four keys of the rows in between
        rows.append(row)
    nsize = [len(r) for r in rows]
    nsize[7] = LONG_STRIDE + 5
    return strided(rows, LONG_STRIDE, nsize) + (LONG_STRIDE,)


WIDE_STRIDE = 4
WIDE_N = {33: RANGES * 33 + 5, 64: RANGES * 64}  # n / RANGES = 33 (bits of a range straddle a bitmap word, a short last block), 64


def _planted(n, stride, lens, kv, rows, base):
    """give each of `rows` a key of its own (base + index) at position row % length"""
    for x, p in enumerate(rows):
        if lens[p] == 0:
            lens[p] = stride
        kv[p, p % lens[p]] = base + x
    return lens, kv


def wide_store(rpb):
    """WIDE_N[rpb] rows at stride 4, lengths 0..4, 8 common keys; rows with a key of their own on the first and the last row of a
    range, on either side of a range boundary, on local row 32 and at both ends of the last block -> (..., planted rows)"""
    n, s = WIDE_N[rpb], WIDE_STRIDE
    assert rows_per_block(n) == rpb
    i = np.arange(n, dtype=np.int64)
    lens = (i * 7 // 3) % (s + 1)
    kv = (100 + (i[:, None] + np.arange(s)[None, :] * 3) % 8).astype(np.uint32)
    last = (n - 1) // rpb * rpb
    planted = sorted({0, 32, rpb - 1, rpb, 2 * rpb - 1, 2 * rpb, 1000 * rpb - 1, 1000 * rpb, last - 1, last, n - 1})
    lens, kv = _planted(n, s, lens, kv, planted, 0x30000000)
    live = np.arange(s)[None, :] < lens[:, None]
    keys = np.where(live, kv, np.uint32(KEY_POISON)).astype(np.uint32)
    ids = np.where(live, ((i[:, None] * 5 + np.arange(s)[None, :]) & 0x7FFFFFFF), ID_POISON).astype(np.int32)
    return ids.reshape(-1), keys.reshape(-1).view(np.int32), lens.astype(np.int32), s, np.array(planted)


FULL_N = RANGES * MAX_ROWS                       # the smallest n whose n / RANGES reaches kKrMaxRows: 4,096 rows per block


def full_store():
    """FULL_N rows at stride 1 (every 97th is empty), 24 of 300 keys per range; rows 0, 4095, 4096 and n - 1 -- local rows 0 and
    4095, the first and the last bit of the bitmap -- carry a key of their own -> (keys, nsize, stride, planted rows)"""
    n = FULL_N
    assert rows_per_block(n) == MAX_ROWS and rows_per_block(n - RANGES) == MAX_ROWS - 1
    fam = (np.arange(300, dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(3) | np.uint32(1 << 27)
    assert len(np.unique(fam)) == 300
    i = np.arange(n, dtype=np.int64)
    kv = fam[((i >> 12) * 5 + (i & 4095) % 24) % 300]
    lens = (i % 97 != 5).astype(np.int32)
    planted = np.array([0, MAX_ROWS - 1, MAX_ROWS, n - 1])
    lens[planted] = 1
    kv[planted] = 0x30000000 + np.arange(4, dtype=np.uint32)
    kv[lens == 0] = KEY_POISON
    return kv.view(np.int32), lens, 1, planted


CROWD = 40                                       # PROBES + 8 keys of one home: at most PROBES of them find a dictionary entry
CROWD_HOME = DICT - 2                            # the chains of the two families run over the end of the dictionary


def crowd_keys():
    return same_home(CROWD, CROWD_HOME), same_home(CROWD, CROWD_HOME + 1)


def crowded_store(layout):
    """40 rows at stride 96 (two block ranges).  one_row: row 3 shows all 80 keys of the two families, shuffled, the rows behind it
    repeat some of them; spread: every row of range 0 shows three of them (all 80 by row 26) among repeats of earlier ones"""
    a, b = crowd_keys()
    both = np.r_[a, b]
    rng = np.random.default_rng(len(layout))
    perm = rng.permutation(80)
    rows = []
    for i in range(40):
        if layout == "one_row":
            rows.append(rng.permutation(both) if i == 3 else (both[rng.integers(0, 80, size=i % 9)] if i > 3 else np.array([7, 8])))
        else:
            new = both[perm[(i * 3 + np.arange(3)) % 80]] if i < MIN_ROWS else both[:0]
            rows.append(np.r_[both[rng.integers(0, 80, size=i % 5)], new, both[rng.integers(0, 80, size=2)]])
    return strided(rows, 96) + (96,)


MANY_STRIDE = 256                                # 32 rows x 256 slots hold up to 8,192 members: one block range


def many_keys(c, seed=0):
    """c distinct keys of [1, POOL) in 32 rows at stride 256, every row with new keys among repeats of earlier ones"""
    assert c <= MIN_ROWS * (MANY_STRIDE - 32)
    rng = np.random.default_rng(c + seed)
    fam = rng.permutation(np.arange(1, POOL, dtype=np.uint32))[:c]
    cut = np.linspace(0, c, MIN_ROWS + 1).astype(np.int64)
    rows = []
    for i in range(MIN_ROWS):
        new = fam[cut[i]:cut[i + 1]]
        old = fam[rng.integers(0, max(1, cut[i]), size=MANY_STRIDE - len(new) - (i % 7))] if i else fam[:0]
        rows.append(rng.permutation(np.r_[new, old]))
    return strided(rows, MANY_STRIDE) + (MANY_STRIDE,), fam


def valued_store(kind):
    """the ends of the key range.  low: the keys 0, 1 and 2^31 - 1 alone and mixed with others; high: keys with bit 31 set
    (negative as int32) next to them, 0xFFFFFFFE -- one below the empty entry -- among them"""
    low = np.array([0, 1, 0x7FFFFFFF], dtype=np.uint32)
    high = np.array([0x80000000, 0x80000001, 0xFFFFFFFE, 0xC0000000], dtype=np.uint32)
    rng = np.random.default_rng(len(kind))
    pool = np.r_[low, FAMILY[3:9]] if kind == "low" else np.r_[low, high, FAMILY[3:6]]
    rows = [low[[2]], low[[0]], low[[1, 0, 2]]] + [pool[rng.integers(0, len(pool), size=rng.integers(0, 9))] for _ in range(37)]
    rows.append(pool)
    return strided(rows, 16) + (16,)


TRANSLATE_N = [1, 3, 4, 5, TRANSLATE_BLOCK - 1, TRANSLATE_BLOCK, TRANSLATE_BLOCK + 1, 3 * TRANSLATE_BLOCK + 2]
STRANGER = 0x2BADBAD                             # a key no table of the translate cases holds


def translate_data(n, fam):
    """n payload keys out of fam, the first and the last among them, and (n > 4) the STRANGER"""
    rng = np.random.default_rng(n)
    d = np.asarray(fam, dtype=np.uint32)[rng.integers(0, len(fam), size=n)]
    d[0], d[-1] = fam[0], fam[-1]
    if n > 4:
        d[[2, n - 2]] = STRANGER
    return d.view(np.int32)

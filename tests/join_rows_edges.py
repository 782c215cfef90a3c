"""Inputs that sit on the branch points of the f32 row-form join (subgacc_sjoin_fill_v2 with form = ROWS: csrc/sjoin.hip, sjoin.hpp,
sjoin_f64pair.hpp) and a plain NumPy restatement of what that join writes.  No torch and no GPU here:
tests/test_join_rows_edges_cpu.py shows that the restatement is the reference's join (the goldens, the C merge join, gather_numpy) and
that every case reaches the edge it is named for; tests/test_gpu_join_rows_edges.py drives the kernels through the C ABI and compares
bit for bit.

EdgeRows      rows from explicit id arrays (sorted, unique, int32) with one payload word per member, rendered as the three row layouts
              of include/subgacc.h (packed, strided, headed); every slot that is not a member holds poison.
join_rows_ref the join of a segment list over such rows: seg, xz, idx, segid, flags3 and `live` (the rows a skipped pair leaves alone).
route         WHICH kernel instantiation the library launches for a case: the launchers of csrc/sjoin.hip restated (launch_key_join,
              launch_table_pairs, launch_f64_pairs, launch_segments and the dispatch in subgacc_sjoin_fill_v2).  It never says what a
              row is.
CASES         the named cases, shared by the CPU and the GPU file.

Constants as the code has them: kWave 64, kPairEmit 128 lanes (256 for k = 4 / 64-bit k = 5 with max_len > 512 above 2,048 pairs),
kRegTrips = kF64RegTrips = 4, split = 2 up to 2,048 pairs, 160 KiB of LDS.

Documented limits the cases pin (include/subgacc.h, subgacc_join_desc):
  - a row number outside [0, n_rows) reads as an empty row, flags[3] |= 16;
  - a row longer than its layout's bound -- max_len for packed rows, row_stride for strided rows (row_len above it), row_stride - 1
    for headed rows (the head above it) -- sets flags[3] |= 1 and its pair (mirrored lists: both segments; other lists: the segment
    whose PARTNER row is too long) is not written, the others are; nothing behind the row's slot is read;
  - a pair that is not mirrored sets flags[3] |= 4 and neither of its segments is written;
  - an SFptr outside the table sets flags[3] |= 2 and BOTH halves of that output row become table row 0 (the zero row of Z_SF); out_idx
    still receives the raw pair; without out_xz no table is consulted and the flag stays clear;
  - a partner that is absent is key 0 / SFptr 0 / 0.0: the zero row, table row 0, (0.0 + 1.0) - 1.0."""
import functools
from types import SimpleNamespace

import numpy as np

WAVE = 64
LDS = 160 * 1024
REG_TRIPS = 4
ID_POISON = 0x7F7F7F7F
KIND_CODE = {"sfptr": 0, "f64": 1, "key32": 2, "key64": 3}          # SUBGACC_JOIN_SFPTR / F64 / KEY32 / KEY64
PAYLOAD_DTYPE = {"sfptr": np.int32, "f64": np.float64, "key32": np.uint32, "key64": np.uint64}
# what a slot behind a row's members holds: a key with a count in every field, an SFptr far outside any table, a NaN
PAYLOAD_POISON = {"sfptr": np.int32(0x7E7E7E7E), "f64": np.float64("nan"), "key32": np.uint32(0x7FFFFFFF), "key64": np.uint64(0x7FFFFFFFFFFFFFFF)}


# ------------------------------------------------------------------------------------------------------------------- rows
class EdgeRows:
    """n rows; row r = (ids[r] sorted unique int32, vals[r] one payload word per member)"""

    def __init__(self, name, ids, vals, kind):
        self.name, self.kind = name, kind
        self.ids = [np.ascontiguousarray(i, np.int32) for i in ids]
        self.vals = [np.ascontiguousarray(v, PAYLOAD_DTYPE[kind]) for v in vals]
        self.n = len(self.ids)
        self.len = np.array([len(i) for i in self.ids], np.int64)
        for i, v in zip(self.ids, self.vals):
            assert i.shape == v.shape and i.ndim == 1 and (np.diff(i) > 0).all() and (len(i) == 0 or (i[0] >= 0 and i[-1] < ID_POISON))

    @classmethod
    def from_packed(cls, name, row_off, ids, vals, kind):
        row_off = np.asarray(row_off, np.int64)
        return cls(name, [ids[row_off[r]:row_off[r + 1]] for r in range(len(row_off) - 1)],
                   [vals[row_off[r]:row_off[r + 1]] for r in range(len(row_off) - 1)], kind)

    def row(self, r):
        """row r, or the empty row for a row number outside the store"""
        if 0 <= r < self.n:
            return self.ids[r], self.vals[r]
        return np.zeros(0, np.int32), np.zeros(0, PAYLOAD_DTYPE[self.kind])

    def with_vals(self, name, vals, kind):
        return EdgeRows(name, self.ids, vals, kind)

    # ---- the three layouts of include/subgacc.h
    def packed(self):
        """-> row_off int64 [n+1], ids [X], payload [X]"""
        off = np.zeros(self.n + 1, np.int64)
        np.cumsum(self.len, out=off[1:])
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        return off, cat(self.ids, np.int32), cat(self.vals, PAYLOAD_DTYPE[self.kind])

    def strided(self, stride):
        """-> row_len int32 [n], ids [n*stride], payload [n*stride]: row r = [r*stride, +row_len[r]), poison behind.  A row longer than
        its slot keeps its row_len and the members that fit: the join must flag it and never look behind the slot"""
        ids = np.full((self.n, stride), ID_POISON, np.int32)
        pay = np.full((self.n, stride), PAYLOAD_POISON[self.kind], PAYLOAD_DTYPE[self.kind])
        for r in range(self.n):
            m = min(int(self.len[r]), stride)
            ids[r, :m] = self.ids[r][:m]
            pay[r, :m] = self.vals[r][:m]
        return self.len.astype(np.int32), ids.ravel(), pay.ravel()

    def headed(self, stride):
        """-> ids [n*stride] (slot 0 of a row = its length, members behind it), payload [n*stride] (member t at r*stride + t)"""
        assert stride % 32 == 0
        ids = np.full((self.n, stride), ID_POISON, np.int32)
        pay = np.full((self.n, stride), PAYLOAD_POISON[self.kind], PAYLOAD_DTYPE[self.kind])
        for r in range(self.n):      # (a head above stride - 1: the head stays, the members that fit)
            m = min(int(self.len[r]), stride - 1)
            ids[r, 0] = self.len[r]
            ids[r, 1:1 + m] = self.ids[r][:m]
            pay[r, :m] = self.vals[r][:m]
        return ids.ravel(), pay.ravel()


def decode_packed(row_off, ids, pay):
    return [(ids[row_off[r]:row_off[r + 1]], pay[row_off[r]:row_off[r + 1]]) for r in range(len(row_off) - 1)]


def decode_strided(row_len, ids, pay, stride):
    return [(ids[r * stride: r * stride + row_len[r]], pay[r * stride: r * stride + row_len[r]]) for r in range(len(row_len))]


def decode_headed(ids, pay, stride):
    n = len(ids) // stride
    return [(ids[r * stride + 1: r * stride + 1 + ids[r * stride]], pay[r * stride: r * stride + ids[r * stride]]) for r in range(n)]


# ------------------------------------------------------------------------------------------------------------------- LP keys
def key_shift(M):
    """SHIFT = 32 - clz(M) (subgacc_key_shift)"""
    return int(M).bit_length()


def pack_keys(lead, counts, M, wide):
    """key = sum_j c_j << ((m - j) * SHIFT) | lead << (m * SHIFT); counts [n, m] = c_1 .. c_m"""
    counts = np.asarray(counts, np.uint64)
    m, s = counts.shape[1], key_shift(M)
    assert m * s + 1 <= (63 if wide else 31) and int(counts.max(initial=0)) < (1 << s)
    key = np.asarray(lead, np.uint64) << np.uint64(m * s)
    for j in range(1, m + 1):
        key |= counts[:, j - 1] << np.uint64((m - j) * s)
    return key.astype(np.uint64 if wide else np.uint32)


def unpack_keys(keys, M, hops):
    """float32 [n, hops + 1]: [lead bit, float32(c_1) / float32(M), ..] -- main.py:174's IEEE division, c_1 the highest field"""
    key = np.asarray(keys).astype(np.uint64)
    s = key_shift(M)
    out = np.empty((key.size, hops + 1), np.float32)
    out[:, 0] = ((key >> np.uint64(hops * s)) & np.uint64(1)).astype(np.float32)
    fm = np.float32(M)
    for c in range(1, hops + 1):
        field = (key >> np.uint64((hops - c) * s)) & np.uint64((1 << s) - 1)
        out[:, c] = field.astype(np.float32) / fm
    return out


def random_keys(rng, n, M, hops, wide):
    """keys with a count in every field: each count one of 0, 1, M // 2, M - 1, M or uniform in [0, M], the lead bit on every third"""
    pool = np.array([0, 1, M // 2, M - 1, M], np.int64)
    counts = np.where(rng.random((n, hops)) < 0.5, pool[rng.integers(0, 5, (n, hops))], rng.integers(0, M + 1, (n, hops)))
    return pack_keys(rng.integers(0, 3, n) == 0, counts, M, wide)


# ------------------------------------------------------------------------------------------------------------------- the join
def _partner_of(own, partner, pair_block):
    if partner is not None:
        return np.asarray(partner, np.int64)
    assert pair_block > 0
    j = np.arange(own.size)
    return own[np.where((j // pair_block) & 1, j - pair_block, j + pair_block)]


def join_rows_ref(rows, own, partner, payload_kind, pair_block=0, max_len=None, table=None, val_add=0, slot_id=None, num_walks=0,
                  num_steps=0, want_xz=True):
    """The row form over `rows`: segment j emits one row per member of row own[j], ascending ids, as (value of the member, value of the
    same id in row partner[j] or absent).  partner = None: the own row of j's mirror (pair_block > 0).  max_len: the longest row the
    store's layout admits -- the descriptor's max_len for packed rows, row_stride for strided, row_stride - 1 for headed rows (None: no
    bound).  Table payload: a member's word becomes SFptr+1 = slot_id[word] + 1 or word + val_add BEFORE the join (absent
    stays 0).  -> seg int64 [S+1], xz f32 [R, 2, k], idx i32 [R, 2] (table payload, else None), segid int64 [R], flags3, live bool [R]
    (False: a row of a skipped pair -- the fill leaves it as it was)."""
    assert payload_kind == rows.kind
    own = np.asarray(own, np.int64)
    S, n = own.size, rows.n
    partner = _partner_of(own, partner, pair_block)
    inside = lambda r: (r >= 0) & (r < n)
    rlen = lambda r: np.where(inside(r), rows.len[np.clip(r, 0, max(n - 1, 0))] if n else 0, 0)
    lens, plens = rlen(own), rlen(partner)
    seg = np.zeros(S + 1, np.int64)
    np.cumsum(lens, out=seg[1:])
    flags3 = 16 if not (inside(own).all() and inside(partner).all()) else 0
    skip = np.zeros(S, bool)
    bound = np.iinfo(np.int64).max if max_len is None else max(int(max_len), 1)
    if pair_block > 0:
        assert S % (2 * pair_block) == 0
        j = np.arange(S).reshape(-1, 2, pair_block)[:, 0].ravel()
        j2 = j + pair_block
        broken = (own[j2] != partner[j]) | (partner[j2] != own[j])
        long_ = ~broken & ((lens[j] > bound) | (plens[j] > bound))
        flags3 |= (4 if broken.any() else 0) | (1 if long_.any() else 0)
        skip[j] = skip[j2] = broken | long_
    else:
        skip = plens > bound
        flags3 |= 1 if skip.any() else 0
    # the payload as the kernels see it
    if payload_kind == "sfptr":
        if slot_id is not None:
            vals = [np.asarray(slot_id, np.int32)[v] + np.int32(1) for v in rows.vals]
        else:
            vals = [v + np.int32(val_add) for v in rows.vals]
    else:
        vals = rows.vals
    empty = np.zeros(0, PAYLOAD_DTYPE[payload_kind])
    cache = {}

    def segment(ra, rb):      # one np.searchsorted per distinct (own row, partner row)
        if (ra, rb) not in cache:
            ia, va = (rows.ids[ra], vals[ra]) if 0 <= ra < n else (np.zeros(0, np.int32), empty)
            ib, vb = (rows.ids[rb], vals[rb]) if 0 <= rb < n else (np.zeros(0, np.int32), empty)
            if len(ib):
                pos = np.searchsorted(ib, ia)
                posc = np.minimum(pos, len(ib) - 1)
                hit = (pos < len(ib)) & (ib[posc] == ia)
                got = np.where(hit, vb[posc], vb.dtype.type(0))
            else:
                got = np.zeros_like(va)
            cache[(ra, rb)] = (va, got)
        return cache[(ra, rb)]

    parts = [segment(int(a), int(b)) for a, b in zip(own, partner)]
    A = np.concatenate([p[0] for p in parts]) if parts else empty
    B = np.concatenate([p[1] for p in parts]) if parts else empty
    live = np.repeat(~skip, lens)
    segid = np.repeat(np.arange(S, dtype=np.int64), lens)
    idx = None
    if payload_kind in ("key32", "key64"):
        xz = np.stack([unpack_keys(A, num_walks, num_steps), unpack_keys(B, num_walks, num_steps)], axis=1)
    elif payload_kind == "f64":
        xz = np.stack([A.astype(np.float32), ((B + 1.0) - 1.0).astype(np.float32)], axis=1)[:, :, None]
    else:
        idx = np.stack([A, B], axis=1).astype(np.int32)
        xz = None
        if want_xz:
            T = table.shape[0]
            bad = ((idx < 0) | (idx >= T)).any(axis=1)
            if (bad & live).any():
                flags3 |= 2
            safe = np.where(bad[:, None], 0, idx)
            xz = np.asarray(table, np.float32)[safe]
    return SimpleNamespace(seg=seg, xz=xz, idx=idx, segid=segid, flags3=int(flags3), live=live)


# ------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one call of subgacc_sjoin_fill_v2: rows in one layout, a segment list, a payload and the outputs wanted.
    max_len: the descriptor's (packed rows: the bound; strided / headed float rows: the speculative length; else unused);
    outs: subset of {"xz", "idx", "segid"}; xz_off / table_off: floats past a 16-byte boundary."""

    def __init__(self, name, rows, layout, own, partner, pair_block, stride=0, max_len=0, M=0, hops=0, table=None, slot_id=None,
                 outs=("xz",), xz_off=0, table_off=0, inst=None, base_pairs=0, note=""):
        self.name, self.rows, self.layout, self.stride, self.max_len = name, rows, layout, stride, max_len
        self.own = np.asarray(own, np.int64)
        self.partner = None if partner is None else np.asarray(partner, np.int64)
        self.pair_block, self.M, self.hops, self.table, self.slot_id = pair_block, M, hops, table, slot_id
        self.outs, self.xz_off, self.table_off, self.inst, self.base_pairs, self.note = tuple(outs), xz_off, table_off, inst, base_pairs, note
        self.kind = rows.kind
        self.k = (hops + 1) if self.kind in ("key32", "key64") else (1 if self.kind == "f64" else (table.shape[1] if table is not None else 1))

    @property
    def S(self):
        return self.own.size

    @property
    def ML(self):
        """JoinArgs.max_len (join_args): the caller's bound for packed rows, what a row's slot holds otherwise"""
        if self.layout == "packed":
            return max(self.max_len, 1)
        return self.stride - 1 if self.layout == "headed" else self.stride

    @property
    def val_add(self):
        return 1 if (self.kind == "sfptr" and self.layout == "strided" and self.slot_id is None) else 0

    def ref(self):
        return _ref(self.name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = CASES[name]
    return join_rows_ref(c.rows, c.own, c.partner, c.kind, pair_block=c.pair_block, max_len=c.ML,
                         table=c.table, val_add=c.val_add, slot_id=c.slot_id, num_walks=c.M, num_steps=c.hops, want_xz="xz" in c.outs)


def pair_split(pairs):
    return 2 if pairs * 2 <= 4096 else 1


def route(c):
    """the kernel instantiation subgacc_sjoin_fill_v2 launches for case c, as its launchers decide it"""
    ML, pairs, mirrored = c.ML, c.S // 2, c.pair_block > 0
    b = lambda v: "true" if v else "false"
    if c.kind in ("key32", "key64"):
        wide, k = c.kind == "key64", c.hops + 1
        nt = 256 if (ML > 512 and pair_split(pairs) == 1 and (k == 4 or (wide and k == 5))) else 128
        kv = (5 if k == 5 else 0) if wide else (k if k in (3, 4, 5) else 0)
        assert mirrored and ML * (20 if wide else 12) + 16 + (nt // WAVE) * (WAVE * 2 * k + 4) * 4 <= LDS
        return f"sjoin_keypair_kernel<{kv}, {nt}, {b(wide)}, false>"
    if c.kind == "f64":
        if mirrored and ML * 20 + 16 <= LDS:
            return f"sjoin_f64pair_kernel<{64 if ML <= 128 else 128}>"
        assert c.layout == "packed"
        return f"sjoin_fill_kernel<true, 0, {b(ML * 12 <= LDS)}>"
    xz = "xz" in c.outs
    vec4 = xz and c.k == 4 and c.table_off % 4 == 0 and c.xz_off % 4 == 0
    if mirrored and ML * 16 <= LDS:
        kv = 4 if vec4 else (c.k if xz and c.k in (3, 5) else 0)
        return f"sjoin_keypair_kernel<{kv}, 128, false, true>"
    assert c.layout == "packed"
    return f"sjoin_fill_kernel<false, {4 if vec4 else 0}, {b(ML * 8 <= LDS)}>"


def lanes(c):
    r = route(c)
    if r.startswith("sjoin_keypair_kernel"):
        return int(r.split(",")[1])
    if r.startswith("sjoin_f64pair_kernel"):
        return int(r[r.index("<") + 1:-1])
    return 64


def pair_rows(c):
    """[(ra, rb)] of the mirrored pairs of case c"""
    own = c.own.reshape(-1, 2, c.pair_block)
    return list(zip(own[:, 0].ravel().tolist(), own[:, 1].ravel().tolist()))


def pair_lengths(c):
    """(ns, nt) of every mirrored pair whose rows lie inside the store"""
    n = c.rows.n
    return [tuple(sorted((int(c.rows.len[a]), int(c.rows.len[b])))) for a, b in pair_rows(c) if 0 <= a < n and 0 <= b < n]


# ---- row plans
LENS128 = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 576, 577, 577, 641)      # stride 672; two distinct rows of 577
STRIDE128 = 672
LENS256 = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1089, 1089, 1153)      # stride 1,184; two distinct rows of 1,089
STRIDE256 = 1184
LENS512 = tuple(l for l in LENS128 if l <= 512)
LENS64 = (0, 1, 63, 64, 65, 127, 128)
LENS_SMALL = (0, 1, 2, 63, 64, 65, 129)
PAD_ROWS = 2                 # two one-member rows behind every plan: what a list is filled up with


def plan_ids(lens, seed):
    """rows of the given lengths, ids drawn from [0, 2 * max length): neighbours share about half of the shorter row; behind them
    PAD_ROWS one-member rows (the same id, so that they hit)"""
    rng = np.random.default_rng(seed)
    U = max(2 * max(lens), 64)
    ids = [np.sort(rng.choice(U, L, replace=False)).astype(np.int32) for L in lens]
    return ids + [np.array([5], np.int32)] * PAD_ROWS


def plan_pairs(lens, extra=()):
    """each row with itself, with its neighbour in both orders and with the empty row (row 0) in both orders, then `extra` (pairs of
    LENGTHS)"""
    n, a, b = len(lens), [], []
    assert lens[0] == 0
    for i in range(n):
        a += [i, i, 0]
        b += [i, 0, i]
        if i + 1 < n:
            a += [i, i + 1]
            b += [i + 1, i]
    for la, lb in extra:
        a.append(lens.index(la))
        b.append(lens.index(lb))
    return np.array(a, np.int64), np.array(b, np.int64)


def fill_up(a, b, pairs, n_plan):
    """the pair list filled up to `pairs` with pairs of the one-member rows n_plan, n_plan + 1"""
    pad = pairs - len(a)
    assert pad >= 0
    t = np.arange(pad)
    return np.concatenate([a, n_plan + (t % 2)]), np.concatenate([b, n_plan + ((t // 2) % 2)])


def mirrored(a, b, given):
    return np.concatenate([a, b]), (np.concatenate([b, a]) if given else None), len(a)


def key_vals(ids, M, hops, wide, seed):
    """64-bit keys: every second id that a row shares with the row before it gets that row's key with the other lead bit -- the two
    keys of such a hit agree in their low 32 bits (every 64-bit shape's lead bit lies above bit 31) and differ above"""
    rng = np.random.default_rng(seed)
    vals = [random_keys(rng, len(i), M, hops, wide) for i in ids]
    if wide:
        lead = np.uint64(1) << np.uint64(hops * key_shift(M))
        assert hops * key_shift(M) >= 32
        for r in range(1, len(ids)):
            _, ia, ib = np.intersect1d(ids[r - 1], ids[r], return_indices=True)
            vals[r][ib[::2]] = vals[r - 1][ia[::2]] ^ lead
    return vals


def low_word_twins(c):
    """hits of case c's pairs whose two keys agree in the low 32 bits and differ above"""
    m, n = np.uint64(0xFFFFFFFF), 0
    for a, b in pair_rows(c):
        if a != b and 0 <= a < c.rows.n and 0 <= b < c.rows.n:
            _, ia, ib = np.intersect1d(c.rows.ids[a], c.rows.ids[b], return_indices=True)
            ka, kb = c.rows.vals[a][ia], c.rows.vals[b][ib]
            n += int((((ka & m) == (kb & m)) & (ka != kb)).sum())
    return n


F64_POOL = np.array([1e-3, 0.3, 1e-20, -1e-20, -0.25, 0.5, 5e-324, 1e-310, -1e-310, 1e-40, 3e-39, 1e20, -7.125, 0.0, 2.0 ** -53, 1.0 - 2.0 ** -53])


def f64_vals(ids, seed):
    """scores: half from F64_POOL (values that (v + 1.0) - 1.0 changes, sends to 0 or keeps; negative; subnormal in double and in
    float), half uniform in (0, 1)"""
    rng = np.random.default_rng(seed)
    return [np.where(rng.random(len(i)) < 0.5, F64_POOL[rng.integers(0, len(F64_POOL), len(i))], rng.random(len(i))) for i in ids]


def make_table(T, k, seed):
    """f32 [T, k], row 0 NOT zero: a test sees that absent / out-of-table reads row 0 and writes no literal zeros"""
    return np.random.default_rng(seed).standard_normal((T, k)).astype(np.float32)


TABLE_ROWS = 97
UNIQ_CAP = 256


def sf_vals(ids, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, len(i)).astype(np.int32) for i in ids]


def overlap_rows(seed=3):
    """for the length classes (ns, nt) the six overlap patterns -> ids, [(pattern, ra, rb)]"""
    classes = [(1, 1), (1, 64), (64, 65), (129, 257), (513, 577), (577, 641)]
    ids, pairs = [], []
    rng = np.random.default_rng(seed)
    for ns, nt in classes:
        t = np.sort(rng.choice(np.arange(1000, 3000), nt, replace=False)).astype(np.int32)
        pats = {
            "disjoint": np.sort(rng.choice(np.setdiff1d(np.arange(1000, 3000), t), ns, replace=False)),
            "first-shared": np.concatenate([[t[0]], np.sort(rng.choice(np.setdiff1d(np.arange(t[0] + 1, 3000), t), ns - 1, replace=False))]),
            "last-shared": np.concatenate([np.sort(rng.choice(np.setdiff1d(np.arange(1000, t[-1]), t), ns - 1, replace=False)), [t[-1]]]),
            "below": np.arange(ns) + 10,
            "above": np.arange(ns) + 5000,
            "identical": t.copy(),      # a second row object with T's ids: both rows have nt members
        }
        for pat, s in pats.items():
            ids += [np.asarray(s, np.int32), t]
            pairs.append((f"{pat}-{len(s)}-{nt}", len(ids) - 2, len(ids) - 1))
    return ids, pairs


CASES = {}


def _add(c):
    assert c.name not in CASES, c.name
    c.inst = route(c)
    CASES[c.name] = c
    return c


KEY32_SHAPES = [(200, 3), (200, 2), (100, 4), (200, 1), (7, 7)]          # k = 4, 3, 5, 2 (KV = 0), 8 (KV = 0)
EXTRA128 = ((513, 577), (577, 641), (641, 641))                          # S streamed for 1, 65 and 129 members
EXTRA256 = ((1025, 1089), (1089, 1153), (1153, 1153))


def _build():
    ids128, ids256, ids512 = plan_ids(LENS128, 1), plan_ids(LENS256, 2), plan_ids(LENS512, 3)
    ids64, idsS = plan_ids(LENS64, 4), plan_ids(LENS_SMALL, 5)
    a128, b128 = plan_pairs(LENS128, EXTRA128)
    a256, b256 = plan_pairs(LENS256, EXTRA256)
    a512, b512 = plan_pairs(LENS512)
    a64, b64 = plan_pairs(LENS64)
    aS, bS = plan_pairs(LENS_SMALL)

    # ---------------------------------------------------------------------------------- key rows, 32 bits
    for M, h in KEY32_SHAPES:
        rows = EdgeRows(f"key32-{M}-{h}-plan128", ids128, key_vals(ids128, M, h, False, 10 + h), "key32")
        own, par, pb = mirrored(a128, b128, False)
        _add(Case(f"key32-M{M}-h{h}-strided-plan128", rows, "strided", own, par, pb, stride=STRIDE128, M=M, hops=h, base_pairs=pb))
    for M, h in [(200, 2), (200, 3)]:      # a packed keyed store, any max_len
        rows = CASES[f"key32-M{M}-h{h}-strided-plan128"].rows
        own, par, pb = mirrored(a128, b128, True)
        _add(Case(f"key32-M{M}-h{h}-packed-plan128", rows, "packed", own, par, pb, max_len=641, M=M, hops=h, base_pairs=pb))
    # 256 lanes: k = 4, more than 2,048 pairs, max_len > 512; and the same list at 2,048 pairs (128 lanes, split = 2)
    rows256 = EdgeRows("key32-200-3-plan256", ids256, key_vals(ids256, 200, 3, False, 21), "key32")
    for pairs in (2048, 2049):
        own, par, pb = mirrored(*fill_up(a256, b256, pairs, len(LENS256)), False)
        _add(Case(f"key32-M200-h3-strided-plan256-{pairs}pairs", rows256, "strided", own, par, pb, stride=STRIDE256, M=200, hops=3,
                  base_pairs=len(a256)))
    # both sides of the split for the 128-lane kernels: k = 3, and k = 4 with max_len <= 512
    rows3 = CASES["key32-M200-h2-strided-plan128"].rows
    rows512 = EdgeRows("key32-200-3-plan512", ids512, key_vals(ids512, 200, 3, False, 22), "key32")
    for pairs in (2048, 2049):
        own, par, pb = mirrored(*fill_up(a128, b128, pairs, len(LENS128)), False)
        _add(Case(f"key32-M200-h2-strided-plan128-{pairs}pairs", rows3, "strided", own, par, pb, stride=STRIDE128, M=200, hops=2,
                  base_pairs=len(a128)))
        own, par, pb = mirrored(*fill_up(a512, b512, pairs, len(LENS512)), False)
        _add(Case(f"key32-M200-h3-packed-max512-{pairs}pairs", rows512, "packed", own, par, pb, max_len=512, M=200, hops=3,
                  base_pairs=len(a512)))
    # overlap patterns per length class
    oids, opairs = overlap_rows()
    orows = EdgeRows("key32-200-3-overlap", oids, key_vals(oids, 200, 3, False, 23), "key32")
    oa, ob = np.array([p[1] for p in opairs]), np.array([p[2] for p in opairs])
    own, par, pb = mirrored(oa, ob, False)
    _add(Case("key32-M200-h3-strided-overlap", orows, "strided", own, par, pb, stride=STRIDE128, M=200, hops=3, base_pairs=pb))
    # lists
    rowsS = EdgeRows("key32-200-3-small", idsS, key_vals(idsS, 200, 3, False, 24), "key32")
    nS = len(aS)
    for given in (False, True):
        own, par, pb = mirrored(aS, bS, given)
        _add(Case(f"key32-list-partner-{'given' if given else 'null'}", rowsS, "strided", own, par, pb, stride=160, M=200, hops=3, base_pairs=pb))
    for blocks in (2, 3):      # pb != pairs: `blocks` mirrored blocks of P pairs in one list
        P = nS // blocks
        own = np.concatenate([np.concatenate([aS[t * P:(t + 1) * P], bS[t * P:(t + 1) * P]]) for t in range(blocks)])
        par = np.concatenate([np.concatenate([bS[t * P:(t + 1) * P], aS[t * P:(t + 1) * P]]) for t in range(blocks)])
        _add(Case(f"key32-list-{blocks}-blocks", rowsS, "strided", own, par if blocks == 2 else None, P, stride=160, M=200, hops=3, base_pairs=P))
    own, par, pb = mirrored(aS, bS, True)
    par = par.copy()
    broken = int(np.flatnonzero((rowsS.len[aS] >= 63) & (rowsS.len[bS] >= 63) & (aS != bS))[2])
    par[pb + broken] = (par[pb + broken] + 1) % len(LENS_SMALL)          # the mirror of this pair names another row as its partner
    _add(Case("key32-list-unmirrored-pair", rowsS, "strided", own, par, pb, stride=160, M=200, hops=3, base_pairs=pb, note=broken))
    for given in (False, True):
        a2, b2 = aS.copy(), bS.copy()
        long_ = np.flatnonzero((rowsS.len[aS] >= 63) & (rowsS.len[bS] >= 63) & (aS != bS))
        a2[long_[0]], b2[long_[1]] = rowsS.n, -1               # one row number = n_rows, one = -1, each against a row of >= 63 members
        own, par, pb = mirrored(a2, b2, given)
        _add(Case(f"key32-list-rows-outside-partner-{'given' if given else 'null'}", rowsS, "strided", own, par, pb, stride=160, M=200,
                  hops=3, base_pairs=pb))
    own, par, pb = mirrored(aS, bS, False)
    _add(Case("key32-packed-row-of-max_len+1", rowsS, "packed", own, par, pb, max_len=128, M=200, hops=3, base_pairs=pb))
    # a row longer than its slot, not the last row: strided row_len = row_stride + 1, headed head = row_stride (bound: row_stride - 1)
    for lay, long_len in (("strided", 161), ("headed", 160)):
        lens = (0, 1, 63, long_len, 64, 65, 129)
        lids = plan_ids(lens, 6)
        la, lb = plan_pairs(lens)
        own, par, pb = mirrored(la, lb, lay == "headed")
        _add(Case(f"key32-{lay}-row-longer-than-slot", EdgeRows(f"key32-long-{lay}", lids, key_vals(lids, 200, 3, False, 25), "key32"), lay,
                  own, par, pb, stride=160, M=200, hops=3, outs=("xz", "segid"), base_pairs=pb))
        _add(Case(f"sf-{lay}-row-longer-than-slot", EdgeRows(f"sf-long-{lay}", lids, sf_vals(lids, 1 if lay == "headed" else 0, TABLE_ROWS - 1, 26), "sfptr"),
                  lay, own, par, pb, stride=160, table=make_table(TABLE_ROWS, 3, 27), outs=("xz", "idx"), base_pairs=pb))
        _add(Case(f"f64-{lay}-row-longer-than-slot", EdgeRows(f"f64-long-{lay}", lids, f64_vals(lids, 28), "f64"), lay, own, par, pb,
                  stride=160, outs=("xz", "segid"), base_pairs=pb))
    # output alignment: out_xz at base + 0 .. 3 floats, every width class, with and without out_segid
    for M, h in [(200, 1), (200, 2), (200, 3), (100, 4), (7, 7)]:
        rows = EdgeRows(f"key32-{M}-{h}-small", idsS, key_vals(idsS, M, h, False, 30 + h), "key32")
        own, par, pb = mirrored(aS, bS, False)
        for off in range(4):
            for segid in (False, True):
                _add(Case(f"key32-k{h + 1}-xz+{off}{'-segid' if segid else ''}", rows, "strided", own, par, pb, stride=160, M=M, hops=h,
                          outs=("xz", "segid") if segid else ("xz",), xz_off=off, base_pairs=pb))
    # the quotient: every count 0 .. M in each field, below and at num_walks = 4,096
    for M in (4095, 4096):
        c = np.arange(M + 1)
        keys = pack_keys(c % 2, np.stack([c, M - c], axis=1), M, False)
        cut = list(range(0, M + 1, 480)) + [M + 1]
        qids = [np.arange(cut[i + 1] - cut[i], dtype=np.int32) * 3 for i in range(len(cut) - 1)]
        qrows = EdgeRows(f"key32-{M}-2-quotient", qids, [keys[cut[i]:cut[i + 1]] for i in range(len(cut) - 1)], "key32")
        qa = np.arange(len(qids))
        own, par, pb = mirrored(qa, np.roll(qa, 1), False)
        _add(Case(f"key32-M{M}-h2-quotient", qrows, "strided", own, par, pb, stride=512, M=M, hops=2, base_pairs=pb))

    # ---------------------------------------------------------------------------------- key rows, 64 bits (strided)
    for M, h in [(200, 4), (15, 15), (1000, 5), ((1 << 30) + 3, 2)]:
        rows = EdgeRows(f"key64-{M}-{h}-plan128", ids128, key_vals(ids128, M, h, True, 40 + h), "key64")
        own, par, pb = mirrored(a128, b128, h == 5)
        _add(Case(f"key64-M{M}-h{h}-strided-plan128", rows, "strided", own, par, pb, stride=STRIDE128, M=M, hops=h, base_pairs=pb))
    rows = EdgeRows("key64-200-4-plan256", ids256, key_vals(ids256, 200, 4, True, 45), "key64")
    for pairs in (2048, 2049):
        own, par, pb = mirrored(*fill_up(a256, b256, pairs, len(LENS256)), False)
        _add(Case(f"key64-M200-h4-strided-plan256-{pairs}pairs", rows, "strided", own, par, pb, stride=STRIDE256, M=200, hops=4,
                  base_pairs=len(a256)))
    rows = EdgeRows("key64-200-4-small", idsS, key_vals(idsS, 200, 4, True, 46), "key64")
    own, par, pb = mirrored(aS, bS, False)
    _add(Case("key64-M200-h4-headed-small", rows, "headed", own, par, pb, stride=160, M=200, hops=4, outs=("xz", "segid"), base_pairs=pb))

    # ---------------------------------------------------------------------------------- table payload
    slot_id = np.random.default_rng(50).integers(0, TABLE_ROWS - 1, UNIQ_CAP).astype(np.int32)
    sf_rows = {
        "packed": EdgeRows("sf-packed-plan128", ids128, sf_vals(ids128, 1, TABLE_ROWS, 51), "sfptr"),          # SFptr+1
        "strided": EdgeRows("sf-strided-plan128", ids128, sf_vals(ids128, 0, TABLE_ROWS - 1, 52), "sfptr"),    # slot, table[slot + 1]
        "uniq": EdgeRows("sf-uniq-plan128", ids128, sf_vals(ids128, 0, UNIQ_CAP, 53), "sfptr"),                # slot of the id plane
    }
    sf_rows["headed"] = sf_rows["packed"]          # SFptr+1 as well: the headed rendering of the packed store
    own, par, pb = mirrored(a128, b128, False)
    for k in (1, 3, 4, 5, 8, 16):
        table = make_table(TABLE_ROWS, k, 60 + k)
        for form, rows in sf_rows.items():
            layout = "strided" if form == "uniq" else form
            _add(Case(f"sf-{form}-k{k}-plan128", rows, layout, own, par, pb, stride=0 if layout == "packed" else STRIDE128,
                      max_len=641 if layout == "packed" else 0, table=table, slot_id=slot_id if form == "uniq" else None, base_pairs=pb))
    rowsS = EdgeRows("sf-packed-small", idsS, sf_vals(idsS, 1, TABLE_ROWS, 55), "sfptr")
    rowsU = EdgeRows("sf-uniq-small", idsS, sf_vals(idsS, 0, UNIQ_CAP, 56), "sfptr")
    own, par, pb = mirrored(aS, bS, False)
    for k in (1, 3, 4, 5, 8, 16):
        table = make_table(TABLE_ROWS, k, 70 + k)
        for off in range(4):
            _add(Case(f"sf-packed-k{k}-xz+{off}", rowsS, "packed", own, par, pb, max_len=129, table=table, xz_off=off,
                      outs=("xz", "segid") if off % 2 else ("xz",), base_pairs=pb))
    table4 = make_table(TABLE_ROWS, 4, 74)
    _add(Case("sf-packed-k4-table+1", rowsS, "packed", own, par, pb, max_len=129, table=table4, table_off=1, base_pairs=pb))
    for form, rows in (("packed", rowsS), ("uniq", rowsU)):
        lay = dict(layout="packed", max_len=129) if form == "packed" else dict(layout="strided", stride=160, slot_id=slot_id)
        _add(Case(f"sf-{form}-idx-alone", rows, own=own, partner=par, pair_block=pb, table=None, outs=("idx", "segid"), base_pairs=pb, **lay))
        _add(Case(f"sf-{form}-idx+xz-k3", rows, own=own, partner=par, pair_block=pb, table=make_table(TABLE_ROWS, 3, 73), outs=("xz", "idx"),
                  base_pairs=pb, **lay))
    bad = [v.copy() for v in rowsS.vals]
    bad[4][3], bad[5][10], bad[6][100] = TABLE_ROWS, -5, TABLE_ROWS + 1000          # an SFptr = table_rows, a negative one
    rowsB = rowsS.with_vals("sf-packed-small-bad", bad, "sfptr")
    for k in (3, 4):
        _add(Case(f"sf-packed-k{k}-sfptr-outside-table", rowsB, "packed", own, par, pb, max_len=129, table=make_table(TABLE_ROWS, k, 75),
                  outs=("xz", "idx"), base_pairs=pb))
    _add(Case("sf-packed-sfptr-outside-table-idx-alone", rowsB, "packed", own, par, pb, max_len=129, outs=("idx",), base_pairs=pb))
    for ml in (10240, 10241):      # the pair kernel's last max_len and the one-segment kernel's first, the same short rows
        _add(Case(f"sf-packed-k3-max_len-{ml}", rowsS, "packed", own, par, pb, max_len=ml, table=make_table(TABLE_ROWS, 3, 76), base_pairs=pb))

    # ---------------------------------------------------------------------------------- float payload
    f128 = EdgeRows("f64-plan128", ids128, f64_vals(ids128, 80), "f64")
    f64r = EdgeRows("f64-plan64", ids64, f64_vals(ids64, 81), "f64")
    o128, p128, pb128 = mirrored(a128, b128, False)
    o64, p64, pb64 = mirrored(a64, b64, True)
    _add(Case("f64-packed-max128", f64r, "packed", o64, p64, pb64, max_len=128, outs=("xz", "segid"), base_pairs=pb64))
    _add(Case("f64-packed-max129", f64r, "packed", o64, p64, pb64, max_len=129, base_pairs=pb64))
    _add(Case("f64-strided-128", f64r, "strided", o64, p64, pb64, stride=128, base_pairs=pb64))
    _add(Case("f64-headed-160", f64r, "headed", o64, p64, pb64, stride=160, base_pairs=pb64))
    f127 = EdgeRows("f64-plan64-127", ids64[:6] + ids64[7:], f64_vals(ids64[:6] + ids64[7:], 82), "f64")
    a63, b63 = plan_pairs(LENS64[:6])
    o63, p63, pb63 = mirrored(a63, b63, False)
    _add(Case("f64-headed-128", f127, "headed", o63, p63, pb63, stride=128, outs=("xz", "segid"), base_pairs=pb63))
    _add(Case("f64-packed-plan128", f128, "packed", o128, p128, pb128, max_len=641, outs=("xz", "segid"), base_pairs=pb128))
    for pairs in (2048, 2049):
        own, par, pb = mirrored(*fill_up(a128, b128, pairs, len(LENS128)), False)
        _add(Case(f"f64-packed-plan128-{pairs}pairs", f128, "packed", own, par, pb, max_len=641, base_pairs=len(a128)))
    for spec in (0, 96, 100, 512, 600):      # strided / headed rows: the descriptor's max_len is the speculative length
        _add(Case(f"f64-strided-spec{spec}", f128, "strided", o128, p128, pb128, stride=STRIDE128, max_len=spec, base_pairs=pb128))
        _add(Case(f"f64-headed-spec{spec}", f128, "headed", o128, p128, pb128, stride=STRIDE128, max_len=spec,
                  outs=("xz", "segid") if spec == 100 else ("xz",), base_pairs=pb128))
    for ml in (8191, 8192):
        _add(Case(f"f64-packed-max_len-{ml}", f64r, "packed", o64, p64, pb64, max_len=ml, base_pairs=pb64))

    # ---------------------------------------------------------------------------------- one wave per segment (pair_block = 0, packed)
    seg_lens = (1, 63, 64, 65, 129, 0, 300, 20)
    sids = plan_ids(seg_lens, 90)
    so = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 4, 6], np.int64)          # own rows of 1, 63, 64, 65, 129 (and the empty and a long one)
    sp = np.array([6, 6, 6, 6, 6, 7, 5, 2, 4, 4, 6, 0, 3], np.int64)          # partners WITHOUT their mirrors
    srows = EdgeRows("seg-sf", sids, sf_vals(sids, 1, TABLE_ROWS, 91), "sfptr")
    for k in range(1, 17):
        _add(Case(f"seg-sf-k{k}", srows, "packed", so, sp, 0, max_len=300, table=make_table(TABLE_ROWS, k, 100 + k),
                  outs=("xz", "segid") if k % 2 else ("xz",)))
    _add(Case("seg-sf-k4-xz+1", srows, "packed", so, sp, 0, max_len=300, table=make_table(TABLE_ROWS, 4, 104), xz_off=1))
    _add(Case("seg-sf-k4-idx+xz", srows, "packed", so, sp, 0, max_len=300, table=make_table(TABLE_ROWS, 4, 104), outs=("xz", "idx", "segid")))
    _add(Case("seg-sf-idx-alone", srows, "packed", so, sp, 0, max_len=300, outs=("idx",)))
    _add(Case("seg-sf-partner-of-max_len+1", srows, "packed", so, sp, 0, max_len=299, table=make_table(TABLE_ROWS, 3, 103)))
    bad = [v.copy() for v in srows.vals]
    bad[4][7], bad[6][0] = TABLE_ROWS, -1
    _add(Case("seg-sf-k4-sfptr-outside-table", srows.with_vals("seg-sf-bad", bad, "sfptr"), "packed", so, sp, 0, max_len=300,
              table=make_table(TABLE_ROWS, 4, 104), outs=("xz", "idx")))
    frows = EdgeRows("seg-f64", sids, f64_vals(sids, 92), "f64")
    _add(Case("seg-f64", frows, "packed", so, sp, 0, max_len=300, outs=("xz", "segid")))
    for ml in (20480, 20481):
        _add(Case(f"seg-sf-k3-max_len-{ml}", srows, "packed", so, sp, 0, max_len=ml, table=make_table(TABLE_ROWS, 3, 103)))
        _add(Case(f"seg-sf-k4-max_len-{ml}", srows, "packed", so, sp, 0, max_len=ml, table=make_table(TABLE_ROWS, 4, 104)))
    for ml in (13653, 13654):
        _add(Case(f"seg-f64-max_len-{ml}", frows, "packed", so, sp, 0, max_len=ml))


_build()

# groups the tests iterate
SAME_OUTPUT = [      # (case, case): the same rows and list on both sides of a dispatch boundary -> identical outputs
    ("sf-packed-k3-max_len-10240", "sf-packed-k3-max_len-10241"), ("f64-packed-max_len-8191", "f64-packed-max_len-8192"),
    ("seg-sf-k3-max_len-20480", "seg-sf-k3-max_len-20481"), ("seg-sf-k4-max_len-20480", "seg-sf-k4-max_len-20481"),
    ("seg-f64-max_len-13653", "seg-f64-max_len-13654"), ("f64-packed-max128", "f64-packed-max129"),
    ("f64-packed-max128", "f64-strided-128"), ("f64-packed-max128", "f64-headed-160"),          # the three renderings of one case
    ("key32-M200-h2-strided-plan128", "key32-M200-h2-packed-plan128"), ("key32-M200-h3-strided-plan128", "key32-M200-h3-packed-plan128"),
    ("f64-strided-spec0", "f64-headed-spec0"), ("f64-strided-spec0", "f64-packed-plan128"), ("f64-strided-spec96", "f64-strided-spec600"), ("f64-headed-spec100", "f64-headed-spec512"),
    ("key32-list-partner-null", "key32-list-partner-given"),
    ("sf-packed-k3-plan128", "sf-headed-k3-plan128"), ("sf-packed-k4-plan128", "sf-headed-k4-plan128"),
]
SPLIT_PAIRS = [      # split = 2 and split = 1 lists built from the same base pairs: the same rows for those pairs
    ("key32-M200-h3-strided-plan256-2048pairs", "key32-M200-h3-strided-plan256-2049pairs"),
    ("key32-M200-h2-strided-plan128-2048pairs", "key32-M200-h2-strided-plan128-2049pairs"),
    ("key32-M200-h3-packed-max512-2048pairs", "key32-M200-h3-packed-max512-2049pairs"),
    ("key64-M200-h4-strided-plan256-2048pairs", "key64-M200-h4-strided-plan256-2049pairs"),
    ("f64-packed-plan128-2048pairs", "f64-packed-plan128-2049pairs"),
]

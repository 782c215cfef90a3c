"""Synthetic rows for the segmented sorts of csrc/spg.hip, and NumPy restatements of the sort's branch points.  No GPU here: the
generators and the case tables are shared by tests/test_spg_rows_cpu.py (which proves that every row reaches the branch it is meant
for) and tests/test_gpu_spg_rows.py (which drives the kernels through the C ABI).

The restatements (level1, level2, bcap_build, bcap_finish) follow bucket_sort_regs and the two host rules line by line.  They say
WHICH branch a row takes, never what the sorted row is: the expected output is always expected_order(ids) = np.argsort(ids, "stable")
applied to ids and payload."""
import numpy as np

TOP = 2 ** 31 - 1            # the largest id
WAVE = 64
FINE_ABOVE = 12              # kFineAbove: level 2 runs when a level-1 bucket holds more members
BUCKET_MAX_LEN = 1024        # kBucketMaxLen: the bucket kernel's longest row; finish_rows' largest stride
LDS_BYTES = 160 * 1024       # kLdsBytes
FOLD_SLOTS, FOLD_PROBES = 256, 16        # kFinFold and the probes of finish_row's fold table
POISON = -1515870811         # 0xA5A5A5A5: what every output holds before a launch (ids are never negative)
GUARD = 64                   # poisoned words in front of and behind every output

RUN_LENGTHS = (13, 40, 100, 300)         # the runs of `stairs`, cycled while they fit
WINDOW = 2 ** 22             # a run lies in [base, base + WINDOW): one level-1 bucket of the finest level 1 (512 buckets over 2^31)
BASE_UNIT = 2 ** 25          # run bases are multiples of it: a bucket boundary of every level 1 with 64 or more buckets


# ------------------------------------------------------------------------------------------------------------------ generators
def _shuffled(ids, rng):
    ids = np.asarray(ids, dtype=np.int64)
    assert len(np.unique(ids)) == len(ids) and (len(ids) == 0 or (ids.min() >= 0 and ids.max() <= TOP))
    return ids[rng.permutation(len(ids))].astype(np.int32)


def spread(ns, rng):
    """ids over the whole of [0, 2^31 - 1], with 0 and 2^31 - 1 among them when ns >= 2: the range is cut into ceil(ns / 4) equal
    strata and every stratum gets its share of uniform draws -- random inside a bucket, but no bucket of a level 1 with ns / 4 or
    more buckets can collect more than two strata (8 members)"""
    if ns <= 1:
        return _shuffled(rng.integers(0, TOP + 1, ns), rng)
    strata = -(-ns // 4)
    edges = (np.arange(strata + 1, dtype=np.int64) * 2 ** 31) // strata
    share = np.full(strata, ns // strata)
    share[: ns % strata] += 1
    ids = []
    for s in range(strata):
        lo, hi = int(edges[s]), int(edges[s + 1])
        got = set()
        if s == 0:
            got.add(0)
        if s == strata - 1 and len(got) < share[s]:
            got.add(TOP)
        while len(got) < share[s]:
            got.add(int(rng.integers(lo, hi)))
        ids.extend(got)
    ids = np.array(ids, dtype=np.int64)
    assert ids.min() == 0 and ids.max() == TOP
    return _shuffled(ids, rng)


def consecutive(ns, rng, base=None):
    """base .. base + ns - 1: as many ids as the range is wide (one bucket per id while ns <= bcap)"""
    if base is None:
        base = int(rng.integers(0, TOP + 2 - max(ns, 1)))
    return _shuffled(base + np.arange(ns, dtype=np.int64), rng)


def consecutive_top(ns, rng):
    """the consecutive ids that end at 2^31 - 1"""
    return consecutive(ns, rng, base=TOP + 1 - ns)


def island(ns, rng):
    """0, 2^31 - 1 and ns - 2 consecutive ids in between: level 1 puts all but two members into ONE bucket, and level 2 (its
    sub-buckets are as wide as the bucket's window / its count, at least 4,104 ids) puts all of those into ONE sub-bucket.  The run
    starts 2^21 ids behind a multiple of 2^25, away from every bucket and sub-bucket edge for ns < 1,448"""
    assert ns >= 3
    base = int(rng.integers(1, 63)) * BASE_UNIT + 2 ** 21
    return _shuffled(np.concatenate([[0, TOP], base + np.arange(ns - 2, dtype=np.int64)]), rng)


def stairs_runs(ns):
    """the lengths of the runs of `stairs`: 13, 40, 100, 300, 13, ... while they fit ns - 2; what is left over joins the last"""
    assert ns >= 64
    left, runs = ns - 2, []
    while left >= RUN_LENGTHS[len(runs) % 4]:
        runs.append(RUN_LENGTHS[len(runs) % 4])
        left -= runs[-1]
    runs[-1] += left
    return runs


def stairs(ns, rng):
    """0, 2^31 - 1 and runs of different lengths at far-apart bases (distinct multiples of 2^25: every run has a level-1 bucket of
    its own).  Inside a run of L members the stride differs: L/3 members at strides 1 and 2 from the base, L/6 at stride 3 from
    base + 2^21, the others one by one over [base + 2.5 * 2^20, base + 2^22) -- so one crowded level-1 bucket holds two
    sub-buckets with many members and many with one or two"""
    runs = stairs_runs(ns)
    assert len(runs) <= 62
    bases = (1 + rng.permutation(62)[: len(runs)]).astype(np.int64) * BASE_UNIT
    ids = [np.array([0, TOP], dtype=np.int64)]
    for L, base in zip(runs, bases):
        n1, n2 = L // 3, L // 6
        nw = L - n1 - n2
        clump1 = base + np.cumsum(1 + (np.arange(n1) & 1)) - 1                   # strides 1, 2, 1, 2, ...
        clump2 = base + 2 ** 21 + 3 * np.arange(n2)
        lo, hi = 5 * 2 ** 19, WINDOW
        cell = (hi - lo) // nw
        wide = base + lo + np.arange(nw, dtype=np.int64) * cell + rng.integers(0, cell, nw)
        ids += [clump1, clump2, wide]
    return _shuffled(np.concatenate(ids), rng)


GENERATORS = {"spread": spread, "consecutive": consecutive, "consecutive-top": consecutive_top, "island": island, "stairs": stairs}
MIN_NS = {"spread": 0, "consecutive": 0, "consecutive-top": 0, "island": 3, "stairs": 64}       # below: the generator is undefined
SORT_ONLY = ("spread", "consecutive", "consecutive-top")                                          # what the bitonic kernel gets


def defined(gen, ns):
    return ns >= MIN_NS[gen]


def row(gen, ns, seed=0):
    """the row of generator `gen` with ns members: a function of (gen, ns, seed) alone, the same on the CPU and in the GPU tests"""
    rng = np.random.default_rng([seed, sorted(GENERATORS).index(gen), ns])
    ids = GENERATORS[gen](ns, rng)
    assert ids.dtype == np.int32 and len(ids) == ns
    return ids


def rows(lengths, gens=tuple(GENERATORS), seed=0):
    """[(gen, ns, ids)] of every length crossed with every generator that is defined for it"""
    return [(g, ns, row(g, ns, seed)) for ns in lengths for g in gens if defined(g, ns)]


def expected_order(ids):
    """THE reference: a stable argsort of the row's ids"""
    return np.argsort(ids, kind="stable")


# ---------------------------------------------------------------------------------------------------------------- restatements
def bcap_build(max_len):
    """subgacc_spg_build's bucket bound for rows of up to max_len <= 1,024 members"""
    cap = max_len if max_len > 0 else 1
    bcap = 64
    while bcap < cap and bcap < 1024:
        bcap <<= 1
    return min(bcap, 512)


def bcap_finish(stride):
    """subgacc_finish_rows' bucket bound"""
    bcap = 64
    while bcap < stride and bcap < 256:
        bcap <<= 1
    return bcap


def _level1(ids, bcap):
    ids = np.asarray(ids).astype(np.int64)
    ns = len(ids)
    logb = 0
    while (1 << logb) < ns and (1 << logb) < bcap:
        logb += 1
    rng_ = int(ids.max() - ids.min()) + 1
    Ls = 0 if rng_ <= 1 else int(rng_ - 1).bit_length()
    bk = ((ids - ids.min()) << logb) >> Ls
    assert bk.max() < (1 << logb)
    return logb, Ls, bk


def level1(ids, bcap):
    """(logb, Ls, the members of every level-1 bucket) of bucket_sort_regs for a row of ns >= 1 members"""
    logb, Ls, bk = _level1(ids, bcap)
    return logb, Ls, np.bincount(bk, minlength=1 << logb)


def takes_level2(ids, bcap):
    """the kernel's own condition for level 2"""
    logb, Ls, counts = level1(ids, bcap)
    return counts.max() > FINE_ABOVE and Ls > logb


def level2(ids, bcap):
    """idx2 of every member, as bucket_sort_regs computes it on its level-2 branch (Ls > logb)"""
    logb, Ls, bk = _level1(ids, bcap)
    assert Ls > logb
    ids = np.asarray(ids).astype(np.int64)
    counts = np.bincount(bk, minlength=1 << logb)
    start = np.concatenate([[0], np.cumsum(counts)])
    bshift = Ls - logb
    off = (ids - ids.min()) - (bk << bshift)
    assert (off >= 0).all() and (off < (1 << bshift)).all()
    scaled = (off << (32 - bshift)) & 0xFFFFFFFF                                  # a uint32 in the kernel
    idx2 = start[bk] + ((scaled * counts[bk]) >> 32)                              # __umulhi
    assert (idx2 < start[bk + 1]).all()
    return idx2, bk


# ------------------------------------------------------------------------------------------------------------- the case tables
# subgacc_spg_build, bucket kernel: both sides of every members-per-lane edge (E in 1..8, 10, 13, 16 by ceil(ns / 64))
BUILD_NS = (0, 1, 2, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512, 513, 640, 641, 832, 833, 1023, 1024)
BUILD_MAX_LEN = (1, 64, 65, 512, 513, 1024)          # bcap 64, 64, 128, 512, 512 (clamped from 1,024), 512
UNDERSTATED_BUCKET = (100, (0, 1, 64, 100, 101, 1000))                            # max_len, row lengths
UNDERSTATED_BITONIC = (1025, (0, 64, 1025, 2048, 2049, 5000))
BITONIC_MAX_LEN = (1025, 5000, 8192, 8193, 16384)
BITONIC_REFUSED = 16385                              # P = 32,768: 256 KiB of LDS

# subgacc_finish_rows: every EMAX instantiation (4, 7, 10, 16 by ceil(stride / 64)) and both sides of each of its edges
FINISH_STRIDES = (64, 256, 257, 448, 449, 640, 641, 1024)
FINISH_REFUSED = 1025
E_EDGES = (128, 129, 256, 257, 448, 449, 640, 641, 832, 833)


def build_lengths(max_len):
    return tuple(ns for ns in BUILD_NS if ns <= max_len)


def pow2_at_least(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def bitonic_lengths(max_len):
    """short rows, the first rows of the bitonic kernel, and rows of P - 1 and P members (P: the power of two the launch sorts in)"""
    P = pow2_at_least(max_len)
    return tuple(sorted({0, 1, 64, 1025, 2047, 2048, P - 1, P}))


def finish_lengths(stride):
    return tuple(sorted({0, 1, stride} | {e for e in E_EDGES if e <= stride}))


def emax_of(stride):
    """the finish_rows_kernel<EMAX> a stride launches"""
    e = -(-stride // WAVE)
    return 4 if e <= 4 else 7 if e <= 7 else 10 if e <= 10 else 16


def finish_members_per_lane(stride, ns):
    """the finish_row<E> a row of ns members runs in finish_rows_kernel<emax_of(stride)> (0: the row is left alone)"""
    e, emax = -(-ns // WAVE), emax_of(stride)
    if e == 0:
        return 0
    ladder = {4: (2, 4), 7: (2, 4, 7), 10: (4, 7, 10), 16: (4, 7, 10, 13, 16)}[emax]
    return next(E for E in ladder if e <= E)


def build_members_per_lane(ns):
    e = -(-ns // WAVE)
    return 0 if e == 0 else next(E for E in (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16) if e <= E)


# ------------------------------------------------------------------------------------------- staging rows of subgacc_finish_rows
KEY_POISON = np.uint64(0xDEADBEEFDEADBEEF)  # the staging keys behind a row's members (never read)
_KEYS = np.unique(np.random.default_rng(77).integers(1, 2 ** 62, 1500, dtype=np.uint64))
assert len(_KEYS) == 1500
_KEYS = _KEYS[np.random.default_rng(78).permutation(1500)]
POOL_WALK, POOL_256, POOL_OWN = _KEYS[:48], _KEYS[48:348], _KEYS[348:]        # shared by all rows of a call: 48, 300 and 1,152 keys
KEY_KINDS = ("walk", "256", "own")


def row_keys(kind, ns, rng):
    """walk: two to four dozen distinct keys of a pool of 48 (a walk's own shape); 256: exactly 256 distinct keys, as many as the
    fold table has slots (rows of 256 members and more); own: every member its own key -- at 1,024 members most of them meet a
    fold table whose 16 probed slots are taken and go to the table of distinct rows one by one"""
    if kind == "own":
        return rng.permutation(POOL_OWN)[:ns]
    pool, d = (POOL_WALK, min(ns, int(rng.integers(24, 49)))) if kind == "walk" else (POOL_256, 256)
    assert ns >= d
    distinct = rng.permutation(pool)[:d]
    return rng.permutation(np.concatenate([distinct, distinct[rng.integers(0, d, ns - d)]])) if ns else distinct


def finish_case(stride, seed=0):
    """staging rows: every length of finish_lengths(stride) x every id generator x every kind of keys"""
    cases = [(g, ns, ids, kind) for g, ns, ids in rows(finish_lengths(stride), seed=seed) for kind in KEY_KINDS
             if kind != "256" or ns >= 256]
    rng = np.random.default_rng([seed, stride])
    n = len(cases)
    ids = np.full((n, stride), POISON, dtype=np.int32)
    keys = np.full((n, stride), KEY_POISON, dtype=np.uint64)
    nsize = np.zeros(n, dtype=np.int32)
    for i, (_, ns, members, kind) in enumerate(cases):
        ids[i, :ns], keys[i, :ns], nsize[i] = members, row_keys(kind, ns, rng), ns
    return cases, ids, keys, nsize

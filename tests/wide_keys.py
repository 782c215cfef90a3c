"""Inputs and NumPy restatements for the columns of 64-bit key rows (csrc/keycols64.hip: subgacc_keyrows_columns64) -- shared by
test_wide_keys_cpu.py, which shows on the host that the restatements are what they claim, and the GPU tests of the entry point and
of the step.  No device, no library."""
import numpy as np

DICT_BITS = 12              # kWcDictBits: a block's LDS set holds 4,096 keys
PROBES = 32                 # kWcProbes
MIN_SLOTS = 1024            # the HBM set's slots at least
MAX_T = 8192                # the largest table_rows (16,384 slots x 8 B = 128 KiB of LDS in the finish kernel)
POISON64 = 0x7FFFFFFFFFFFFFFF       # what stands behind a row's members: never read
POISON32 = -7               # what out_cols holds before a call: kept at every position >= nsize[i]
MASK64 = (1 << 64) - 1


def shift_of(M):
    """subgacc_key_shift: 32 - clz(M)"""
    return int(M).bit_length()


def key_bits(M, hops):
    return hops * shift_of(M) + 1


def pack(counts, lead, M):
    """the LP key of a member: count_j << ((m-j)*SHIFT), bit m*SHIFT on the root's own member (subg_acc.c:936-955)"""
    s, k = shift_of(M), 0
    for v in counts:
        assert 0 <= int(v) <= M
        k = (k << s) | int(v)
    return k | (int(bool(lead)) << (len(counts) * s))


def lp_keys(count, seed, M, hops, extra=()):
    """`count` distinct valid LP keys of (M, hops) as sorted uint64, `extra` among them; a quarter carry the lead bit"""
    rng = np.random.default_rng(seed)
    keys = set(int(k) for k in extra)
    assert len(keys) <= count
    while len(keys) < count:
        k = pack(rng.integers(0, M + 1, hops), rng.integers(0, 4) == 0, M)
        if k:
            keys.add(k)
    return np.array(sorted(keys), dtype=np.uint64)


def edge_keys(M, hops):
    """pairs that differ only in the lead bit, only in the top count, only in the low 32-bit word's lowest count, and the largest
    valid key -- for (200, 4) the lead is bit 32, for (30000, 4) bit 60: a truncation to 32 bits merges some of them"""
    s = shift_of(M)
    base = [M // 2] * hops
    top = [M // 2 + 1] + base[1:]
    low = base[:-1] + [M // 2 + 1]
    keys = [pack(base, 0, M), pack(base, 1, M), pack(top, 0, M), pack(low, 0, M), pack([M] * hops, 1, M), pack([0] * (hops - 1) + [1], 0, M),
            pack([0] * hops, 1, M), pack([1] + [0] * (hops - 1), 0, M)]
    assert len(set(keys)) == len(keys) and max(keys) < 1 << (hops * s + 1)
    return keys


def mix(keys):
    """wc_mix of keycols64.hip on a uint64 array (array arithmetic wraps modulo 2^64)"""
    h = np.asarray(keys, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(32)
    h *= np.uint64(0xD6E8FEB86659FD93)
    h ^= h >> np.uint64(32)
    return h


def mix_int(key):
    """the same on one Python int"""
    h = (int(key) * 0x9E3779B97F4A7C15) & MASK64
    h ^= h >> 32
    h = (h * 0xD6E8FEB86659FD93) & MASK64
    return h ^ (h >> 32)


def lds_home(keys):
    """a key's first slot in the block's LDS set: the top 12 bits of its mix"""
    return (mix(keys) >> np.uint64(64 - DICT_BITS)).astype(np.int64)


def same_home_keys(count, seed, M, hops):
    """`count` distinct valid keys whose LDS home is one slot (more than PROBES of them cannot all stand in the block's set)"""
    rng = np.random.default_rng(seed)
    s = shift_of(M)
    found, home = [], None
    while len(found) < count:
        c = rng.integers(0, M + 1, (200000, hops)).astype(np.uint64)
        k = np.zeros(len(c), dtype=np.uint64)
        for j in range(hops):
            k = (k << np.uint64(s)) | c[:, j]
        k = np.unique(k[k != 0])
        h = lds_home(k)
        if home is None:
            home = int(np.bincount(h, minlength=1 << DICT_BITS).argmax())
        found = sorted(set(found) | set(int(x) for x in k[h == home]))
    return np.array(found[:count], dtype=np.uint64), home


def set_slots(T):
    """keycols64_set_slots: a power of two >= 2 T, >= 1,024"""
    cap = MIN_SLOTS
    while cap < 2 * T:
        cap *= 2
    return cap


def rows_per_block(n):
    return min(max(n // (4 * 256 * 4), 32), 4096)


def feature_rows(keys, M, hops):
    """subgacc_unpack_lp(out_f32) of 64-bit keys: float32 divisions by float32(M)"""
    s = shift_of(M)
    k = np.asarray(keys, dtype=np.uint64)
    cols = [np.where((k >> np.uint64(hops * s)) & np.uint64(1), np.float32(M), np.float32(0))]
    cols += [((k >> np.uint64((hops - j) * s)) & np.uint64((1 << s) - 1)).astype(np.float32) for j in range(1, hops + 1)]
    return (np.stack(cols, 1).astype(np.float32) / np.float32(M)).astype(np.float32).reshape(len(k), hops + 1)


def members(keys, lens):
    """the distinct keys in front of the rows' lengths (keys [n, stride] uint64; a length beyond the stride is clamped)"""
    n, stride = keys.shape
    mask = np.arange(stride)[None, :] < np.minimum(lens, stride)[:, None]
    return np.unique(keys[mask])


def columns(keys, lens, T, M, hops):
    """what subgacc_keyrows_columns64 writes for rows whose distinct keys fit its set:
    (count, ukeys64 [T-1], ukeys [T-1], feat [T, hops+1], cols [n, stride] with POISON32 where nothing is written, overflow)"""
    n, stride = keys.shape
    present = members(keys, lens)
    assert len(present) <= set_slots(T), "the set itself would overflow: which keys it keeps depends on the schedule"
    c = min(len(present), T - 1)
    kept = present[:c]
    ukeys64 = np.zeros(T - 1, dtype=np.uint64)
    ukeys64[:c] = kept
    ukeys = np.zeros(T - 1, dtype=np.int32)
    ukeys[:c] = np.arange(1, c + 1)
    feat = np.zeros((T, hops + 1), dtype=np.float32)
    feat[1: c + 1] = feature_rows(kept, M, hops)
    cols = np.full((n, stride), POISON32, dtype=np.int32)
    mask = np.arange(stride)[None, :] < np.minimum(lens, stride)[:, None]
    pos = np.searchsorted(kept, keys[mask])
    hit = (pos < c) & (kept[np.minimum(pos, max(c - 1, 0))] == keys[mask]) if c else np.zeros(int(mask.sum()), dtype=bool)
    cols[mask] = np.where(hit, pos + 1, 0).astype(np.int32)
    return c, ukeys64, ukeys, feat, cols, len(present) > T - 1


def strided(lens, keyset, seed, stride):
    """rows of the given lengths (clamped to the stride when laid out), keys drawn from `keyset`, every key of the set standing
    somewhere while there is room; POISON64 behind the members -> keys [n, stride] uint64"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    keys = np.full((n, stride), POISON64, dtype=np.uint64)
    at = 0
    for i, L in enumerate(np.minimum(lens, stride)):
        k = keyset[rng.integers(0, len(keyset), L)] if len(keyset) else np.zeros(0, dtype=np.uint64)
        take = min(int(L), len(keyset) - at)
        k[:take] = keyset[at: at + take]
        at += take
        keys[i, :L] = k
    return keys, at

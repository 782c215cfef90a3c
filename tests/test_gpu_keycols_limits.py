"""GPU (MI355X): the columns of a step's LP keys (subgacc_keyrows_columns) and the count form over key rows (subgacc_sjoin_key_counts)
at the limits of their LDS dictionary, their HBM set, their sort and their search -- the capacity mechanisms of csrc/keycols.hip that
a few hundred keys never engage.  The reference is NumPy on the host: np.unique of the members in front of each row's length,
Rows.counts, _feature_rows and subgacc_unpack_lp.  Everything is compared bit for bit; every output and the workspace keep their
guard words (_columns and _key_counts check them).  Each case asserts on the host, before any launch, that its rows reach the
mechanism it is about."""
import numpy as np
import pytest
import torch

from gpu_helpers import sp  # noqa: F401
from test_gpu_step_stage import (GUARD, HOPS, M, POISON, SHIFT, STRIDE, Rows, _columns, _feature_rows, _key_counts, _lp_keys,
                                 _workspace)

pytestmark = pytest.mark.gpu

DICT = 4096                 # kKcDict: keys of a block's LDS set
MIN_SLOTS = 1024            # the HBM set's slots at least
LDS_BYTES = 160 * 1024      # kLdsBytes: what a workgroup may ask for


def _slots(T):
    """keycols_set_slots: a power of two >= 2 T, >= 1,024"""
    cap = MIN_SLOTS
    while cap < 2 * T:
        cap *= 2
    return cap


def _rows_per_block(n):
    """the scan's choice in subgacc_keyrows_columns"""
    return min(max(n // (4 * 256 * 4), 32), 4096)


def _members(rows, first=0, last=None):
    """the distinct keys in front of the lengths of rows [first, last)"""
    last = rows.n if last is None else min(last, rows.n)
    mask = np.arange(rows.stride)[None, :] < rows.len[first:last, None]
    return np.unique(rows.keys[first:last][mask])


def _block_keys(rows):
    rpb = _rows_per_block(rows.n)
    return [_members(rows, f, f + rpb) for f in range(0, rows.n, rpb)]


def _unpack(keys, M=M, hops=HOPS):
    """subgacc_unpack_lp(out_f32, zero row first) of `keys`: [len(keys) + 1, hops + 1]"""
    from surel_plus_amd import _lib
    ref = torch.full((len(keys) + 1, hops + 1), -7.0, dtype=torch.float32, device="cuda")
    k64 = torch.from_numpy(keys.astype(np.int64)).cuda()
    _lib.check(_lib.lib().subgacc_unpack_lp(_lib.ptr(k64), len(keys), None, M, hops, None, None, _lib.ptr(ref), 1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return ref.cpu().numpy()


def _check_columns(res, kept, T, M=M, hops=HOPS, shift=SHIFT):
    """ukeys = `kept` and zeros behind; feat = row 0 zero, the unpacked kept keys (both references), zero rows behind"""
    ukeys, count, feat, flags = res
    c = len(kept)
    print(f"columns pass: T = {T}, count = {int(count)}, flags = {flags.cpu().tolist()}")
    assert int(count) == c
    got = ukeys.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:c], kept) and not got[c:].any()
    f = feat.cpu().numpy()
    assert f.shape == (T, hops + 1)
    assert np.array_equal(f[: c + 1].view(np.uint32), _unpack(kept, M, hops).view(np.uint32))
    assert np.array_equal(f[1: c + 1].view(np.uint32), _feature_rows(kept, M, hops, shift).view(np.uint32))
    assert not f[0].any() and not f[c + 1:].any()


def _check_counts(sp, rows, ukeys, count, kept, T, missing, forms=(False, True), **shape):
    """the count kernel against Rows.counts(kept, T): counts, lengths, flags[3] & 2 exactly when a key of the rows is not listed"""
    want, want_len, miss = rows.counts(kept, T)
    assert bool(miss) == missing
    for partner in forms:
        out, olen, fl = _key_counts(sp, rows, ukeys, count, T, partner=partner, **shape)
        print(f"count kernel: T = {T}, n_keys = {int(count)}, partner list {partner}, flags = {fl.tolist()}")
        assert bool(int(fl[3]) & 2) == missing and not fl[:3].any() and not int(fl[3]) & ~2
        assert np.array_equal(out, want) and np.array_equal(olen, want_len)
        assert np.array_equal(out.sum(1), want.sum(1))
        if not missing:
            assert np.array_equal(out.sum(1), 2.0 * want_len)
    return want, want_len


def _dev_keys(keys, count):
    """a hand-built sorted key list with guard words behind it, and its count, on the device"""
    u = torch.full((len(keys) + GUARD,), -7, dtype=torch.int32, device="cuda")
    u[: len(keys)] = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).cuda()
    return u, torch.tensor([count], dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------------------------- 1, 2. the block's LDS dictionary overflows
WIDE = 4608                 # a row of case 2 alone holds more keys than the dictionary


def _crowded_rows(n):
    """6,000 distinct keys in n rows of which every block's range holds more than the LDS dictionary does"""
    keyset = _lp_keys(6000, 21)
    if n <= 32:
        return Rows(keyset, seed=n, lens=[0, 1, 255, 257] + [STRIDE] * (n - 4))
    # rows 0, 8, 16, ... fill their stride with keys that differ: rows 32 and 64 are a block's whole range
    lens = [WIDE if i % 8 == 0 else (0, 1, 31, 255, 257, 544, 1000)[i % 7] for i in range(n)]
    a = [0, 8, 32, n - 1, 1, 2, 5, 6, 9, 31, 33 % n, 16]
    b = [0, 32, n - 1, n - 1, 2, 5, 6, 8, 9, 32, 24, 17]
    return Rows(keyset, seed=n, lens=lens, stride=WIDE, pairs=(a, b), distinct=True, id_space=3 * WIDE)


@pytest.mark.parametrize("n", [32, 33, 65], ids=["one-block", "two-blocks", "three-blocks"])
def test_lds_dictionary_overflow(sp, n):
    """more distinct keys in every block's range than its 4,096-slot dictionary holds: keys go to the HBM set by themselves (the
    !kc_note branch), from one block and -- the same keys, concurrently, with the end-of-range flush of the others -- from two and
    three; then the count kernel with T = 6,001 (rows of up to 4,608 members: the searched row's loads past its register trips)"""
    rows = _crowded_rows(n)
    T = 8192
    present = _members(rows)
    blocks = _block_keys(rows)
    assert _rows_per_block(n) == 32 and len(blocks) == (n + 31) // 32
    assert all(len(b) > DICT for b in blocks), [len(b) for b in blocks]
    assert len(present) == 6000 and np.array_equal(present, rows.present()) and _slots(T) == 16384
    assert all(len(np.intersect1d(blocks[0], b)) > DICT for b in blocks)            # largely the same keys
    res = _columns(sp, rows, T)                         # (_columns: guards intact, the workspace zeroed)
    assert int(res[1]) == 6000 and not res[3].any()
    _check_columns(res, present, T)
    _check_counts(sp, rows, res[0], res[1], present, 6001, missing=False)


# ------------------------------------------------------------------------------------------------- 3. the largest set, a full sort
@pytest.fixture(scope="module")
def big_rows():
    """32 rows that fill STRIDE with 16,383 and with 16,384 distinct keys, laid over the rows in ascending order (key i is member
    i % STRIDE of row i // STRIDE); a dozen pairs: Rows.counts is a Python loop"""
    keyset = _lp_keys(16384, 31)
    a = [0, 1, 2, 3, 24, 24, 25, 31, 12, 30, 23, 5]
    b = [0, 2, 3, 3, 24, 25, 26, 30, 24, 31, 24, 6]
    return {c: Rows(keyset[:c], seed=c, lens=[STRIDE] * 32, pairs=(a, b)) for c in (16383, 16384)}


def test_largest_set_exactly_full_columns(sp, big_rows):
    """table_rows = 16,384: 32,768 slots, 128 KiB of LDS, the bitonic sort over an array that is half keys; count == T - 1, no flag"""
    rows, T = big_rows[16383], 16384
    present = _members(rows)
    assert len(present) == T - 1 and _slots(T) == 32768 and _slots(T) * 4 == 128 * 1024
    res = _columns(sp, rows, T)
    assert int(res[1]) == T - 1 and not res[3].any()
    _check_columns(res, present, T)


def test_largest_set_one_key_too_many(sp, big_rows):
    """one key more than columns in a set that is not full: flags[2] & 1, exactly the smallest T - 1 keys kept"""
    rows, T = big_rows[16384], 16384
    present = _members(rows)
    assert len(present) == T and len(present) < _slots(T)
    res = _columns(sp, rows, T)
    fl = res[3].cpu().numpy()
    assert int(fl[2]) & 1 and not fl[[0, 1, 3]].any() and int(res[1]) == T - 1
    _check_columns(res, present[: T - 1], T)


def test_count_kernel_at_its_lds_limit(sp, big_rows):
    """the largest table_rows the count kernel's LDS check admits for rows of STRIDE members (8 row_stride + 12 T + 16 bytes), one
    more refused; the first T - 1 sorted keys listed: the members whose keys lie beyond are not counted, flags[3] & 2"""
    rows = big_rows[16383]
    T = (LDS_BYTES - 16 - 8 * rows.stride) // 12
    assert 8 * rows.stride + 12 * T + 16 <= LDS_BYTES < 8 * rows.stride + 12 * (T + 1) + 16 and 13000 < T < 16384
    present = _members(rows)
    kept = present[: T - 1]
    assert len(present) > T - 1 and (T - 2) // STRIDE in rows.a and (rows.a > T // STRIDE).any()    # rows on both sides of the cut
    ukeys, count = _dev_keys(kept, T - 1)
    with pytest.raises(ValueError, match="LDS"):                 # SUBGACC_ERR_LDS
        _key_counts(sp, rows, ukeys, count, T + 1)
    want, _ = _check_counts(sp, rows, ukeys, count, kept, T, missing=True)
    assert want[:, T - 1].any()                                  # the last column is used


# --------------------------------------------------------------------------------------------------------- 4. the HBM set is full
@pytest.mark.parametrize("T", [2, 300])
def test_hbm_set_full(sp, T):
    """1,500 distinct keys for 1,024 slots: every slot probed, flags[2] & 1, the key dropped.  WHICH keys are dropped depends on the
    schedule: only what does not is asserted -- a sorted subset of the keys present, its feature rows, zeros behind, guards, the
    workspace zeroed -- and the count kernel on the keys that were kept"""
    rows = Rows(_lp_keys(1500, 41), seed=41)
    present = _members(rows)
    assert len(present) == 1500 > _slots(T) == MIN_SLOTS
    res = _columns(sp, rows, T)                         # (guards intact, the workspace zeroed)
    ukeys, count, feat, flags = res
    fl = flags.cpu().numpy()
    assert int(fl[2]) & 1 and not fl[[0, 1, 3]].any() and int(count) == T - 1
    kept = ukeys.cpu().numpy().view(np.uint32)[: T - 1]
    print(f"hbm-set-full T={T}: count {int(count)}, flags {fl.tolist()}, kept {kept[:4].tolist()}.. of present {present[:4].tolist()}..")
    assert (kept[1:] > kept[:-1]).all() and np.isin(kept, present).all()
    _check_columns(res, kept, T)                        # feat: exactly the kept keys unpacked, row 0 and the rows behind zero
    _check_counts(sp, rows, ukeys, count, kept, T, missing=True)


def test_more_keys_than_columns_from_two_blocks(sp):
    """900 distinct keys fit the set (1,024 slots) but not the 299 columns, and each of two blocks brings keys the other lacks:
    exactly the smallest 299 are kept"""
    T = 300
    lens = [(0, 1, 31, 64)[i % 4] for i in range(32)] + [1, 0, 100, 31]        # 768 + 132 members: every key stands exactly once
    rows = Rows(_lp_keys(900, 43)[np.random.default_rng(43).permutation(900)], seed=43, lens=lens)
    present = _members(rows)
    b0, b1 = _block_keys(rows)
    assert len(present) == 900 and T - 1 < 900 < _slots(T) == MIN_SLOTS and _rows_per_block(rows.n) == 32
    assert len(np.setdiff1d(b0, b1)) and len(np.setdiff1d(b1, b0))
    assert len(np.setdiff1d(present[: T - 1], b1)) and len(np.setdiff1d(present[: T - 1], b0))     # the kept keys come from both
    res = _columns(sp, rows, T)
    fl = res[3].cpu().numpy()
    assert int(fl[2]) & 1 and not fl[[0, 1, 3]].any() and int(res[1]) == T - 1
    _check_columns(res, present[: T - 1], T)
    _check_counts(sp, rows, res[0], res[1], present[: T - 1], T, missing=True, forms=(False,))


# ------------------------------------------------------------------------------------------------------------ 5. workspace reuse
def test_workspace_reused_after_an_overflow(sp):
    """one workspace for an overflowing call (set full), a clean 700-key call and a call with other keys, as StepBuffers reuses
    col_ws: the later results are exact, no earlier key appears in them, the flags are each call's own"""
    from surel_plus_amd import _lib
    pool = _lp_keys(2450, 51)
    pool = pool[np.random.default_rng(51).permutation(len(pool))]
    k1, k2, k3 = np.sort(pool[:1500]), np.sort(pool[1500:2200]), np.sort(pool[2200:])
    assert not len(np.intersect1d(k1, k2)) and not len(np.intersect1d(k1, k3)) and not len(np.intersect1d(k2, k3))
    ws = _workspace(_lib.lib().subgacc_keyrows_columns_workspace_bytes(701))
    r1, r2, r3 = Rows(k1, seed=1), Rows(k2, seed=2), Rows(k3, seed=3)
    assert len(_members(r1)) == 1500 > _slots(300) and len(_members(r2)) == 700 and len(_members(r3)) == 250
    res = _columns(sp, r1, 300, ws=ws)                  # (after every call: the whole workspace zero, its guard intact)
    assert int(res[3][2]) & 1 and int(res[1]) == 299
    res = _columns(sp, r2, 701, ws=ws)
    assert not res[3].any()
    _check_columns(res, k2, 701)
    assert not np.isin(res[0].cpu().numpy().view(np.uint32), k1).any()
    res = _columns(sp, r3, 300, ws=ws)
    assert not res[3].any()
    _check_columns(res, k3, 300)
    got = res[0].cpu().numpy().view(np.uint32)[:250]
    assert not np.isin(got, k1).any() and not np.isin(got, k2).any()


# ------------------------------------------------------------------------------------------------ 6. kc_column's halving search
@pytest.mark.parametrize("c,T", [(c, c + 1) for c in (2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)] + [(257, 400)])
def test_search_boundaries(sp, c, T):
    """key counts at 2, 3 and powers of two with their neighbours, a hand-built sorted list: its smallest and largest key stand in
    the rows, and so do three keys that are NOT listed -- below the list, above it, between two listed keys"""
    full = _lp_keys(c + 3, 60 + c)
    mid = 1 + (c + 1) // 2
    absent = full[[0, mid, c + 2]]
    listed = np.delete(full, [0, mid, c + 2])
    assert len(listed) == c and absent[0] < listed[0] and absent[2] > listed[-1] and listed[mid - 2] < absent[1] < listed[mid - 1]
    rows = Rows(full, seed=c)
    present = _members(rows)
    assert np.isin(absent, present).all() and np.isin(listed[[0, -1]], present).all() and len(present) == c + 3
    ukeys, count = _dev_keys(listed, c)
    want, want_len = _check_counts(sp, rows, ukeys, count, listed, T, missing=True)
    assert (want.sum(1) <= 2.0 * want_len).all() and (want.sum(1) < 2.0 * want_len).any()
    assert want[:, 1].any() and want[:, c].any() and not want[:, c + 1:].any()      # the list's first and last key are found


# --------------------------------------------------------------------------------------------------------- 7. degenerate counts
def test_no_rows(sp):
    """n = 0: only the finish kernel runs; count 0, ukeys and feat zero, no flag"""
    rows = Rows(np.zeros(0, dtype=np.uint32), seed=0, lens=[])
    assert rows.n == 0
    T = 40
    res = _columns(sp, rows, T)
    assert not res[3].any()
    _check_columns(res, np.zeros(0, dtype=np.uint32), T)


def test_key_count_is_clamped(sp):
    """*n_keys of 0 and -5: no key is found, column 0 holds the absent-partner counts alone; T + 100: the same as T - 1, the
    guard words behind ukeys are not keys"""
    rows = Rows(_lp_keys(15, 71), seed=71)
    T = 16
    present = _members(rows)
    assert len(present) == T - 1
    ukeys, count, _, flags = _columns(sp, rows, T)
    assert int(count) == T - 1 and not flags.any()
    none = np.zeros(0, dtype=np.uint32)
    for v in (0, -5):
        cnt = torch.tensor([v], dtype=torch.int64, device="cuda")
        want, want_len = _check_counts(sp, rows, ukeys, cnt, none, T, missing=True)
        assert not want[:, 1:].any() and want[:, 0].any() and (want[:, 0] <= want_len).all()
    _check_counts(sp, rows, ukeys, count, present, T, missing=False)
    cnt = torch.tensor([T + 100], dtype=torch.int64, device="cuda")
    assert ukeys.untyped_storage().nbytes() // 4 == T - 1 + GUARD                  # the guard words stand behind the keys
    _check_counts(sp, rows, ukeys, cnt, present, T, missing=False)


# ------------------------------------------------------------------------------------------------- 8. key shapes up to 31 bits
@pytest.mark.parametrize("Mx,hops", [(1023, 3), (7, 10), (200, 2)], ids=["M1023-3hops", "M7-10hops", "M200-2hops"])
def test_key_shapes(sp, Mx, hops):
    """keys of num_steps * SHIFT + 1 = 31 bits (and of 17): lead bit set and clear with every count at M, the largest and the
    smallest valid key; sorted unsigned; feature rows of num_steps + 1 columns, divisions by a float(M) that is no power of two"""
    from surel_plus_amd import _lib
    shift = _lib.lib().subgacc_key_shift(Mx, hops)
    assert shift == int(Mx).bit_length() and hops * shift + 1 == (17 if Mx == 200 else 31)
    counts_at_m = 0
    for _ in range(hops):
        counts_at_m = (counts_at_m << shift) | Mx
    lead = 1 << (hops * shift)
    edge = [lead | counts_at_m, counts_at_m, 1, lead, Mx << ((hops - 1) * shift)]    # largest, lead clear, smallest, lead alone
    assert max(edge) < 2 ** 31 and (hops * shift + 1 < 31 or max(edge) >= 2 ** 30)
    keyset = np.unique(np.concatenate([_lp_keys(300, 80 + hops, Mx, hops, shift), np.array(edge, dtype=np.uint32)]))
    rows = Rows(keyset, seed=Mx)
    present = _members(rows)
    c = len(present)
    assert np.array_equal(present, keyset) and np.isin(edge, present).all() and present[-1] == edge[0] and present[0] == 1
    T = c + 6
    res = _columns(sp, rows, T, M=Mx, hops=hops)        # (the guard behind T * (hops + 1) floats is checked there)
    assert int(res[1]) == c and not res[3].any()
    _check_columns(res, present, T, Mx, hops, shift)
    f = res[2].cpu().numpy()
    assert (f[c] == 1.0).all() and f[1, -1] == np.float32(1) / np.float32(Mx) and not f[1, :-1].any()
    _check_counts(sp, rows, res[0], res[1], present, T, missing=False, forms=(False,), M=Mx, hops=hops)


# ------------------------------------------------------------------------------------- 9. rows_per_block > 32 and a ragged tail
def test_33_rows_per_block_and_a_ragged_tail(sp):
    """n = 33 * 4,096 + 7 rows of stride 32: rows_per_block = 33 (a wave takes a fifth row of its block), 4,097 blocks, the last
    of 7 rows; keys that stand only in the very last row, and only in the last row of a middle block"""
    n, stride, T = 33 * 4096 + 7, 32, 4096
    rpb = _rows_per_block(n)
    assert rpb == 33 and n % rpb == 7 and -(-n // rpb) == 4097
    rng = np.random.default_rng(9)
    pool = _lp_keys(2010, 91)
    pool = pool[rng.permutation(len(pool))]
    main, last_only, mid_only = pool[:2000], pool[2000:2005], pool[2005:]
    lens = np.array([0, 1, 31, 32])[rng.integers(0, 4, n)]
    keys = main[rng.integers(0, len(main), (n, stride))].astype(np.uint32)
    mid_row = 2000 * rpb + rpb - 1
    lens[n - 1], lens[mid_row] = 31, 32
    keys[n - 1, 26:31] = last_only
    keys[mid_row, 27:32] = mid_only
    keys[np.arange(stride)[None, :] >= lens[:, None]] = POISON
    rows = Rows.of(keys, lens)
    present = _members(rows)
    assert len(present) == 2010 and np.array_equal(present, np.sort(pool))
    mask = np.arange(stride)[None, :] < lens[:, None]
    row_of = np.nonzero(mask)[0]
    assert set(row_of[np.isin(keys[mask], last_only)]) == {n - 1} and set(row_of[np.isin(keys[mask], mid_only)]) == {mid_row}
    res = _columns(sp, rows, T)
    assert int(res[1]) == 2010 and not res[3].any()
    _check_columns(res, present, T)

"""GPU (MI355X): the three row entry points of csrc/spg.hip -- subgacc_spg_build (bucket kernel and bitonic fallback),
subgacc_finish_rows and subgacc_rows_to_headed -- driven through the C ABI with synthetic rows (tests/spg_rows.py) that sit on the
kernels' own branch points: every members-per-lane instantiation from both sides of its edge, id ranges of one id and of 2^31,
level 2 with all of a crowded bucket in one sub-bucket and with sub-buckets of different counts, the 1,024 / 1,025 boundary between
the kernels, the bitonic kernel above 64 KiB of LDS, the refusals, the slot_id translation, finish_row's fold table past its 256
slots and 16 probes, the full table of distinct rows, the cut of a headed row.  tests/test_spg_rows_cpu.py shows on the host that
every row reaches the branch it is here for.

The reference is np.argsort(ids, kind="stable") per row, applied to ids and payload; every comparison is bit for bit.  Every output
is poisoned before the launch and stands between two poisoned guards that must come back untouched.  The rows of one call are the
concatenation of all cases of a parametrisation: each test is a handful of launches."""
import numpy as np
import pytest
import torch

import spg_rows as R
from gpu_helpers import sp  # noqa: F401
from spg_rows import GUARD, POISON

pytestmark = pytest.mark.gpu

EMPTY_KEY = np.uint64(2 ** 64 - 1)          # kEmptyKey of csrc/uniq_table.hpp
KEY_POISON = R.KEY_POISON


# --------------------------------------------------------------------------------------------------------------------- plumbing
def _lib():
    from surel_plus_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype, init=None):
    """n words of poison (or `init`) between two poisoned guards: (whole buffer, the n words)"""
    whole = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device="cuda")
    view = whole[GUARD: GUARD + n]
    if init is not None:
        view.copy_(_dev(init).view(dtype))
    return whole, view


def _back(whole, n):
    """the n words as NumPy, after the guards in front and behind were seen untouched"""
    h = whole.cpu().numpy()
    assert (h[:GUARD] == POISON).all() and (h[GUARD + n:] == POISON).all(), "a guard word was written"
    return h[GUARD: GUARD + n]


def _pack(rows):
    """rows [(gen, ns, ids)] -> row_off [n + 1], ids [total]"""
    lens = np.array([ns for _, ns, _ in rows], dtype=np.int64)
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([i for _, _, i in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return row_off, ids


def _payload(total, seed):
    """random int32 SFptr values, -1 and 2^31 - 2 among them: the kernel stores sf + 1"""
    sf = np.random.default_rng(seed).integers(-1, 2 ** 31 - 1, total).astype(np.int32)
    sf[: min(total, 2)] = np.array([-1, 2 ** 31 - 2], dtype=np.int32)[: min(total, 2)]
    return sf


def _spg_build(rows, max_len, sf, table=None, cap=0):
    """one call of subgacc_spg_build: (return code, out_indices, out_data, flags), guards checked"""
    L = _lib()
    row_off, ids = _pack(rows)
    total = len(ids)
    d_off, d_ids, d_sf = _dev(row_off), _dev(ids), _dev(sf)
    w_idx, o_idx = _guarded(total, torch.int32)
    w_dat, o_dat = _guarded(total, torch.int32)
    w_fl, fl = _guarded(4, torch.int32, np.zeros(4, np.int32))
    rc = L.lib().subgacc_spg_build(L.ptr(d_off), len(rows), L.ptr(d_ids), L.ptr(d_sf), L.ptr(table), cap, max_len, L.ptr(o_idx),
                                   L.ptr(o_dat), L.ptr(fl), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, _back(w_idx, total), _back(w_dat, total), _back(w_fl, 4)


def _expect_sorted(rows, data, limit):
    """the NumPy sort of every row of at most `limit` members; poison over the span of every longer one"""
    row_off, ids = _pack(rows)
    want_idx = np.full(len(ids), POISON, dtype=np.int32)
    want_dat = np.full(len(ids), POISON, dtype=np.int32)
    for r, (_, ns, _) in enumerate(rows):
        if ns > limit:
            continue
        b, e = row_off[r], row_off[r + 1]
        order = R.expected_order(ids[b:e])
        want_idx[b:e], want_dat[b:e] = ids[b:e][order], data[b:e][order]
    return want_idx, want_dat


def _check_build(rows, max_len, what, limit=None, flags=(0, 0, 0, 0), seed=0):
    _, ids = _pack(rows)
    sf = _payload(len(ids), seed + max_len)
    rc, idx, dat, fl = _spg_build(rows, max_len, sf)
    print(f"spg_build {what}: max_len = {max_len}, rows = {len(rows)}, members = {len(ids)}, rc = {rc}, flags = {fl.tolist()}")
    assert rc == 0
    want_idx, want_dat = _expect_sorted(rows, (sf.astype(np.int64) + 1).astype(np.int32), max_len if limit is None else limit)
    assert fl.tolist() == list(flags)
    assert np.array_equal(idx, want_idx) and np.array_equal(dat, want_dat)
    return idx


def _bucket_rows(max_len):
    rows = R.rows(R.build_lengths(max_len))
    if max_len == 1024:                                  # 8 k + 1 rows: the tail of the XCD mapping holds ONE row
        extra = R.rows((833, 1024, 65, 449, 2, 641, 1, 193), ("spread", "consecutive"), seed=1)
        rows += extra[: (1 - len(rows)) % 8]
        assert len(rows) % 8 == 1
    return rows


# ------------------------------------------------------------------------------------------ 1. subgacc_spg_build, bucket kernel
@pytest.mark.parametrize("max_len", R.BUILD_MAX_LEN)
def test_bucket_kernel_every_lane_count_and_id_range(sp, max_len):
    """every row length of BUILD_NS that fits max_len, crossed with spread / consecutive (random base and up to 2^31 - 1) /
    island / stairs ids, in one launch: E = 1..8, 10, 13, 16 members per lane from both sides of every edge; bcap 64, 128, 512 and
    the clamp; level 1 alone, one bucket per id, level 2 with one sub-bucket and with many"""
    rows = _bucket_rows(max_len)
    assert max_len <= R.BUCKET_MAX_LEN and all(ns <= max_len for _, ns, _ in rows)
    assert {ns for _, ns, _ in rows} == set(R.build_lengths(max_len))
    bcap = R.bcap_build(max_len)
    crowded = [g for g, ns, ids in rows if ns and R.takes_level2(ids, bcap)]
    print(f"bcap = {bcap}, level-2 rows = {len(crowded)} of {len(rows)}, E = {sorted({R.build_members_per_lane(ns) for _, ns, _ in rows})}")
    assert max_len < 64 or {"island", "stairs"} <= set(crowded)
    _check_build(rows, max_len, "bucket kernel")


@pytest.mark.parametrize("n", [0, 1, 7, 9])
def test_bucket_kernel_row_counts(sp, n):
    """0 rows (OK, nothing touched), 1, 7 and 9: fewer rows than XCDs, and a grid of 16 blocks of which 7 have no row"""
    pool = [r for r in R.rows((1024, 513, 64, 321, 1), seed=2) if r[1]]
    rows = pool[::2][:n]
    assert len(rows) == n
    idx = _check_build(rows, 1024, f"{n} rows", seed=n)
    assert n or len(idx) == 0


def test_bucket_kernel_slot_id_translation(sp):
    """sf holds slots of a hand-built table of distinct rows whose id column (byte offset 16 * capacity) is a known permutation:
    the payload is perm[sf] + 1 in sorted order, from the bucket kernel and from the bitonic kernel"""
    L = _lib()
    cap = 4096
    nbytes = L.lib().subgacc_uniq_table_bytes(cap)
    assert nbytes == 20 * cap
    rng = np.random.default_rng(5)
    perm = rng.permutation(cap).astype(np.int32)
    assert not np.array_equal(perm, np.arange(cap)) and np.array_equal(np.sort(perm), np.arange(cap))
    table = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    table[16 * cap:].view(torch.int32).copy_(_dev(perm))
    for max_len, rows in ((1024, R.rows((0, 1, 2, 64, 65, 257, 513, 1024), seed=3)),
                          (1025, R.rows((0, 1, 64, 1025, 2048), R.SORT_ONLY, seed=3))):
        _, ids = _pack(rows)
        sf = rng.integers(0, cap, len(ids)).astype(np.int32)
        sf[:2] = (0, cap - 1)
        rc, idx, dat, fl = _spg_build(rows, max_len, sf, table, cap)
        print(f"spg_build with a table: max_len = {max_len}, rows = {len(rows)}, rc = {rc}, flags = {fl.tolist()}")
        assert rc == 0 and not fl.any()
        want_idx, want_dat = _expect_sorted(rows, perm[sf] + 1, R.pow2_at_least(max_len))
        assert np.array_equal(idx, want_idx) and np.array_equal(dat, want_dat)
        assert not np.array_equal(dat, _expect_sorted(rows, sf + 1, R.pow2_at_least(max_len))[1])      # not the slots themselves


# ----------------------------------------------------------------------------------------- 2. subgacc_spg_build, bitonic kernel
def _bitonic_rows(max_len):
    lengths = R.bitonic_lengths(max_len)
    if max_len <= 8192:
        return R.rows(lengths, R.SORT_ONLY)
    P = R.pow2_at_least(max_len)                         # 128 KiB of LDS per row: a dozen rows
    both = R.rows((1025, 2048, P - 1, P), ("consecutive", "consecutive-top"))
    return R.rows(lengths, ("spread",)) + [both[i] for i in (0, 3, 4, 7)]


@pytest.mark.parametrize("max_len", R.BITONIC_MAX_LEN)
def test_bitonic_kernel(sp, max_len):
    """the first max_len past the bucket kernel (P = 2,048), 64 KiB of LDS exactly (5,000 and 8,192) and 128 KiB (8,193 and
    16,384: the hipFuncSetAttribute branch); rows of 1,025, 2,047, 2,048, P - 1 and P members beside rows of 0, 1 and 64"""
    rows = _bitonic_rows(max_len)
    P = R.pow2_at_least(max_len)
    assert max_len > R.BUCKET_MAX_LEN and 8 * P <= R.LDS_BYTES and {ns for _, ns, _ in rows} == set(R.bitonic_lengths(max_len))
    assert max_len <= 8192 or len(rows) == 12
    print(f"P = {P}, LDS = {8 * P // 1024} KiB")
    _check_build(rows, max_len, "bitonic kernel", limit=P)


def test_bitonic_kernel_refuses_what_lds_cannot_hold(sp):
    """max_len = 16,385 asks for P = 32,768 (256 KiB): SUBGACC_ERR_LDS, nothing launched, nothing written"""
    L = _lib()
    rows = R.rows((1, 64, 1025), R.SORT_ONLY)
    _, ids = _pack(rows)
    sf = _payload(len(ids), 9)
    rc, idx, dat, fl = _spg_build(rows, R.BITONIC_REFUSED, sf)
    print(f"spg_build refused: max_len = {R.BITONIC_REFUSED}, rc = {rc}, flags = {fl.tolist()}")
    assert rc == L.ERR_LDS and not fl.any() and (idx == POISON).all() and (dat == POISON).all()
    with pytest.raises(ValueError, match="LDS"):
        L.check(rc)


# ------------------------------------------------------------------------------------------------------ 3. under-stated max_len
def test_bucket_kernel_refuses_rows_longer_than_max_len(sp):
    """max_len = 100 with rows of 100, 101 and 1,000 members: flags[3] & 1 and no other flag, the rows of up to 100 sorted, the
    span of every longer row still poison"""
    max_len, lengths = R.UNDERSTATED_BUCKET
    rows = R.rows(lengths)
    assert {100, 101, 1000} <= {ns for _, ns, _ in rows} and R.bcap_build(max_len) == 128
    _check_build(rows, max_len, "under-stated, bucket kernel", flags=(0, 0, 0, 1))


def test_bitonic_kernel_refuses_rows_longer_than_its_power_of_two(sp):
    """max_len = 1,025 (P = 2,048) with rows of 2,048, 2,049 and 5,000 members: the rows of up to P sorted, the others left alone"""
    max_len, lengths = R.UNDERSTATED_BITONIC
    rows = R.rows(lengths, R.SORT_ONLY)
    assert {2048, 2049, 5000} <= {ns for _, ns, _ in rows} and R.pow2_at_least(max_len) == 2048
    _check_build(rows, max_len, "under-stated, bitonic kernel", limit=2048, flags=(0, 0, 0, 1))


# ------------------------------------------------------------------------------------------------------- 4. subgacc_finish_rows
def _finish_rows(ids, keys, nsize, stride, root_base, cap):
    """one call of subgacc_finish_rows on a freshly reset table: (rc, row_ids, row_slot, flags, table keys, mintag, id)"""
    L = _lib()
    n = len(nsize)
    nbytes = L.lib().subgacc_uniq_table_bytes(cap)
    assert nbytes == 20 * cap
    table = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(L.lib().subgacc_uniq_reset(L.ptr(table), cap, L.stream_ptr()))
    w_ids, row_ids = _guarded(n * stride, torch.int32, ids.reshape(-1))
    w_slot, row_slot = _guarded(n * stride, torch.int32)
    w_fl, fl = _guarded(4, torch.int32, np.zeros(4, np.int32))
    d_keys, d_ns = _dev(keys.reshape(-1).view(np.int64)), _dev(nsize)
    rc = L.lib().subgacc_finish_rows(L.ptr(row_ids), L.ptr(d_keys), L.ptr(d_ns), n, stride, root_base, L.ptr(table), cap,
                                     L.ptr(row_slot), L.ptr(fl), L.stream_ptr())
    torch.cuda.synchronize()
    t = table.cpu().numpy()
    assert (t[nbytes:] == 0xA5).all(), "bytes behind the table were written"
    tk, tm = t[: 8 * cap].view(np.uint64), t[8 * cap: 16 * cap].view(np.uint64)
    return (rc, _back(w_ids, n * stride).reshape(n, stride), _back(w_slot, n * stride).reshape(n, stride), _back(w_fl, 4), tk, tm,
            t[16 * cap: 20 * cap].view(np.int32))


def _check_sorted_rows(ids, nsize, got_ids, got_slot):
    """the ids of every row sorted, slots [ns, stride) of row_ids and row_slot untouched; -> the stable order of every row"""
    orders = []
    for i, ns in enumerate(nsize):
        order = R.expected_order(ids[i, :ns])
        orders.append(order)
        assert np.array_equal(got_ids[i, :ns], ids[i, :ns][order]), i
        assert np.array_equal(got_ids[i, ns:], ids[i, ns:]) and (got_slot[i, ns:] == POISON).all(), i
    return orders


@pytest.mark.parametrize("root_base", [0, 12345])
@pytest.mark.parametrize("stride", R.FINISH_STRIDES)
def test_finish_rows(sp, stride, root_base):
    """finish_rows_kernel<4 | 7 | 10 | 16> from both sides of every stride edge, every finish_row<E> of each from both sides of its
    row-length edge, all id generators, three kinds of keys: ids sorted in place, every member's slot holds its key, the occupied
    slots are exactly the distinct keys, every slot's tag is the smallest (root_base + i) * stride + r of its key, no flag"""
    cases, ids, keys, nsize = R.finish_case(stride)
    n, cap = len(cases), 4096
    assert {ns for _, ns, _, _ in cases} == set(R.finish_lengths(stride)) and {k for *_, k in cases} <= set(R.KEY_KINDS)
    assert stride < 256 or {k for *_, k in cases} == set(R.KEY_KINDS)
    rc, got_ids, got_slot, fl, tk, tm, tid = _finish_rows(ids, keys, nsize, stride, root_base, cap)
    print(f"finish_rows: stride = {stride} (EMAX {R.emax_of(stride)}, bcap {R.bcap_finish(stride)}), root_base = {root_base}, "
          f"rows = {n}, E = {sorted({R.finish_members_per_lane(stride, int(v)) for v in nsize})}, rc = {rc}, flags = {fl.tolist()}")
    assert rc == 0 and not fl.any()
    orders = _check_sorted_rows(ids, nsize, got_ids, got_slot)
    member = np.arange(stride)[None, :] < nsize[:, None]
    for i, ns in enumerate(nsize):
        slot = got_slot[i, :ns]
        assert (slot >= 0).all() and (slot < cap).all() and np.array_equal(tk[slot], keys[i, :ns][orders[i]]), i
    all_keys = keys[member]
    tags = ((root_base + np.arange(n, dtype=np.int64))[:, None] * stride + np.arange(stride)[None, :])[member].astype(np.uint64)
    uniq, inv = np.unique(all_keys, return_inverse=True)
    want_tag = np.full(len(uniq), np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(want_tag, inv, tags)
    occupied = np.nonzero(tk != EMPTY_KEY)[0]
    assert len(occupied) == len(uniq) and np.array_equal(np.sort(tk[occupied]), uniq)
    assert np.array_equal(tm[occupied], want_tag[np.searchsorted(uniq, tk[occupied])])
    free = tk == EMPTY_KEY
    assert (tm[free] == EMPTY_KEY).all() and (tid == -1).all()                   # what subgacc_uniq_reset left


def test_finish_rows_refuses_a_stride_of_1025(sp):
    L = _lib()
    stride = R.FINISH_REFUSED
    ids = np.full((2, stride), POISON, dtype=np.int32)
    keys = np.full((2, stride), KEY_POISON, dtype=np.uint64)
    nsize = np.array([64, 1025], dtype=np.int32)
    for i, ns in enumerate(nsize):
        ids[i, :ns], keys[i, :ns] = R.row("spread", int(ns)), R.POOL_OWN[0]
    rc, got_ids, got_slot, fl, tk, _, _ = _finish_rows(ids, keys, nsize, stride, 0, 64)
    print(f"finish_rows refused: stride = {stride}, rc = {rc}, flags = {fl.tolist()}")
    assert rc == L.ERR_LDS and not fl.any() and np.array_equal(got_ids, ids) and (got_slot == POISON).all()
    assert (tk == EMPTY_KEY).all()
    with pytest.raises(ValueError, match="finish_rows"):
        L.check(rc)


def test_finish_rows_full_table(sp):
    """a table of 64 slots and a row with 200 distinct keys: flags[2] & 1 and no other flag; every row_slot >= 0 names a slot that
    holds the member's key, the others are -1 (the table is full: 64 members have a slot), the ids are sorted all the same"""
    stride, ns, cap = 256, 200, 64
    ids = np.full((1, stride), POISON, dtype=np.int32)
    keys = np.full((1, stride), KEY_POISON, dtype=np.uint64)
    ids[0, :ns], keys[0, :ns] = R.row("stairs", ns), R.POOL_OWN[:ns]
    nsize = np.array([ns], dtype=np.int32)
    rc, got_ids, got_slot, fl, tk, tm, _ = _finish_rows(ids, keys, nsize, stride, 3, cap)
    slot = got_slot[0, :ns]
    print(f"finish_rows full table: capacity = {cap}, distinct keys = {ns}, rc = {rc}, flags = {fl.tolist()}, "
          f"members with a slot = {int((slot >= 0).sum())}")
    assert rc == 0 and fl.tolist() == [0, 0, 1, 0]
    order = _check_sorted_rows(ids, nsize, got_ids, got_slot)[0]
    want_key = keys[0, :ns][order]
    has = slot >= 0
    assert (slot[~has] == -1).all() and (slot[has] < cap).all() and np.array_equal(tk[slot[has]], want_key[has])
    assert has.sum() == cap and (tk != EMPTY_KEY).all() and len(np.unique(tk)) == cap
    assert np.array_equal(tm[slot[has]], (3 * stride + order[has]).astype(np.uint64))        # order: sorted position -> staging r


# ---------------------------------------------------------------------------------------------------- 5. subgacc_rows_to_headed
def _headed(lengths, stride, pbytes, seed, with_flags):
    L = _lib()
    ptype, ttype = (np.int32, torch.int32) if pbytes == 4 else (np.int64, torch.int64)
    rng = np.random.default_rng([seed, stride, pbytes])
    lens = np.array(lengths, dtype=np.int64)
    n, total = len(lens), int(lens.sum())
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, 2 ** 31, total).astype(np.int32)
    pay = rng.integers(np.iinfo(ptype).min, np.iinfo(ptype).max, total, dtype=ptype, endpoint=True)
    w_ids, o_ids = _guarded(n * stride, torch.int32)
    w_pay, o_pay = _guarded(n * stride, ttype)
    w_fl, fl = _guarded(4, torch.int32, np.zeros(4, np.int32))
    d_off, d_ids, d_pay = _dev(row_off), _dev(ids), _dev(pay)
    rc = L.lib().subgacc_rows_to_headed(L.ptr(d_off), n, L.ptr(d_ids), L.ptr(d_pay), pbytes, stride, L.ptr(o_ids), L.ptr(o_pay),
                                        L.ptr(fl) if with_flags else None, L.stream_ptr())
    torch.cuda.synchronize()
    want_ids = np.full((n, stride), POISON, dtype=np.int32)
    want_pay = np.full((n, stride), POISON, dtype=ptype)
    for r in range(n):
        k = min(int(lens[r]), stride - 1)                                        # cut to stride - 1 where the row is too long
        want_ids[r, 0] = k
        want_ids[r, 1: 1 + k] = ids[row_off[r]: row_off[r] + k]
        want_pay[r, :k] = pay[row_off[r]: row_off[r] + k]
    got_ids, got_pay, got_fl = _back(w_ids, n * stride), _back(w_pay, n * stride), _back(w_fl, 4)
    assert rc == 0
    assert np.array_equal(got_ids.reshape(n, stride), want_ids) and np.array_equal(got_pay.reshape(n, stride), want_pay)
    return got_fl, bool((lens > stride - 1).any())


@pytest.mark.parametrize("pbytes", [4, 8])
@pytest.mark.parametrize("stride", [2, 32, 96])
def test_rows_to_headed(sp, stride, pbytes):
    """rows of 0, 1, 63, 64, 65, stride - 1, stride and stride + 70 members in calls of 1, 5 and 8 rows (a workgroup takes four):
    slot 0 holds the length, cut to stride - 1 where the row is too long; members and payloads bit-equal, the slots behind the row's
    end still poison; flags[3] & 1 exactly when a row was cut; with flags = NULL the same rows, cut the same way"""
    every = [0, 1, 63, 64, 65, stride - 1, stride, stride + 70]
    fits = sorted({k for k in every if k <= stride - 1})
    calls = [[stride - 1], [stride], [stride + 70],                              # 1 row: the longest that fits, two that are cut
             (fits * 5)[:5], [stride + 70, 0, 65, stride, 1],                    # 5 rows: none cut, two or three cut
             [every[i] for i in (6, 2, 0, 7, 4, 1, 5, 3)]]                       # 8 rows: every length
    assert [len(c) for c in calls] == [1, 1, 1, 5, 5, 8] and {k for c in calls for k in c} == set(every)
    for c, lengths in enumerate(calls):
        fl, cut = _headed(lengths, stride, pbytes, c, True)
        print(f"rows_to_headed: stride = {stride}, payload = {pbytes} bytes, rows = {lengths}, cut = {cut}, flags = {fl.tolist()}")
        assert fl.tolist() == [0, 0, 0, int(cut)]
        fl, _ = _headed(lengths, stride, pbytes, c, False)
        assert not fl.any()                                                      # the flags it was not given
    assert [bool(max(c) > stride - 1) for c in calls] == [False, True, True, False, True, True]

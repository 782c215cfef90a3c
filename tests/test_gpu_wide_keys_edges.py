"""GPU (MI355X): subgacc_keyrows_columns64 alone (csrc/keycols64.hip) -- the columns of 64-bit key rows and the rows as 32-bit
surrogate keys, over synthetic int64 rows between poisoned rims.  Every case is called twice on one workspace; every output is
compared bit for bit with the NumPy restatement of tests/wide_keys.py (shown against the oracle in test_wide_keys_cpu.py), the
workspace is left zeroed, every guard is intact, and out_cols keeps its poison at every position behind a row's members.  Keys of
(200, 4) have 33 bits, keys of (30000, 4) have 61: a truncation to 32 bits anywhere merges keys of every set below."""
import numpy as np
import pytest
import torch

import wide_keys as W
from gpu_helpers import sp  # noqa: F401
from test_gpu_step_stage import GUARD, LENS, Rows, _guarded, _key_counts, _workspace

pytestmark = pytest.mark.gpu

HOPS = 4
STRIDE = 544                # the stride of M = 128, 4 hops: 513 members rounded up to whole 128-byte lines
SHAPES = [pytest.param(200, id="33-bits"), pytest.param(30000, id="61-bits")]
TRIP_LENS = (0, 1, 63, 64, 65, 255, 256, 257, STRIDE, STRIDE + 56)      # a trip is 4 x 64 members; the last nsize is beyond the stride


def _columns64(keys, lens, T, M, ws=None):
    """the entry point twice over the same rows and workspace -> (count, ukeys64, ukeys, feat, cols [n, stride], flags) as NumPy"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    n, stride = keys.shape
    kd = _guarded(n * stride, torch.int64, W.POISON64)
    kd[: n * stride] = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).reshape(-1)).cuda()
    nsize = _guarded(n, torch.int32, 1 << 20)
    nsize[:n] = torch.from_numpy(np.asarray(lens, dtype=np.int32)).cuda()
    nbytes = L.subgacc_keyrows_columns64_workspace_bytes(T)
    assert nbytes == W.set_slots(T) * 8
    ws = _workspace(nbytes) if ws is None else ws
    assert ws.numel() - GUARD >= nbytes
    nbytes = ws.numel() - GUARD
    runs = []
    for _ in range(2):
        u64, u, count = _guarded(T - 1, torch.int64, -7), _guarded(T - 1, torch.int32, -7), _guarded(1, torch.int64, -7)
        feat = _guarded(T * (HOPS + 1), torch.float32, -7.0)
        cols = _guarded(n * stride, torch.int32, W.POISON32)
        flags = torch.zeros(4, dtype=torch.int32, device="cuda")
        _lib.check(L.subgacc_keyrows_columns64(_lib.ptr(kd), _lib.ptr(nsize), n, stride, M, HOPS, T, _lib.ptr(u64), _lib.ptr(u),
                                               _lib.ptr(count), _lib.ptr(feat), _lib.ptr(cols), _lib.ptr(flags), _lib.ptr(ws), nbytes,
                                               _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((u64[T - 1:] == -7).all()) and bool((u[T - 1:] == -7).all()) and bool((count[1:] == -7).all())
        assert bool((feat[T * (HOPS + 1):] == -7.0).all()) and bool((cols[n * stride:] == W.POISON32).all())
        assert bool((ws[:nbytes] == 0).all()) and bool((ws[nbytes:] == 0x5A).all())       # left zeroed, its guard alone
        runs.append((int(count[0]), u64[: T - 1].cpu().numpy().view(np.uint64), u[: T - 1].cpu().numpy(),
                     feat[: T * (HOPS + 1)].view(T, HOPS + 1).cpu().numpy(), cols[: n * stride].view(n, stride).cpu().numpy(),
                     flags.cpu().numpy()))
        runs[-1] += ((u[: T - 1], count[:1], cols[: n * stride]),)                          # (on the device, for the count kernel)
    a, b = runs
    assert a[0] == b[0] and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[1:6], b[1:6]))
    return b


def _check(res, keys, lens, T, M):
    """every output against W.columns, bit for bit; flags[2] & 1 exactly on an overflow, no other flag"""
    count, u64, u, feat, cols, flags = res[:6]
    c, want64, want, wfeat, wcols, over = W.columns(keys, np.asarray(lens), T, M, HOPS)
    print(f"columns64: n = {keys.shape[0]}, T = {T}, count = {count} (want {c}), flags = {flags.tolist()}, overflow {over}")
    assert count == c and flags.tolist() == [0, 0, 1 if over else 0, 0]
    assert np.array_equal(u64, want64) and np.array_equal(u, want)
    assert np.array_equal(feat.view(np.uint32), wfeat.view(np.uint32))
    assert np.array_equal(cols, wcols)                  # the surrogates, and the poison behind every row's members
    return c, over


def _rows(lens, keyset, seed, stride=STRIDE):
    keys, at = W.strided(lens, keyset, seed, stride)
    assert at == len(keyset), "every key of the set stands somewhere"
    return keys


# ------------------------------------------------------------------------------------------------ 1. key counts, widths, row lengths
@pytest.mark.parametrize("M", SHAPES)
@pytest.mark.parametrize("nkeys,T", [pytest.param(1, 2, id="one-key"), pytest.param(1, 40, id="one-key-wide"),
                                     pytest.param(15, 16, id="T-1-keys"), pytest.param(16, 16, id="T-keys"),
                                     pytest.param(700, 1030, id="700-keys-T1030")])
def test_columns_and_surrogates_equal_their_restatement(sp, M, nkeys, T):
    """row lengths 0, 1, 63, 64, 65, 255, 256, 257, a row that fills the stride and an nsize beyond it; one key (every LDS atomic of a
    block on one address), exactly T - 1 keys, and T keys: an overflow by one -- flags[2] & 1, count == T - 1, the smallest T - 1
    kept, surrogate 0 for the dropped key's members and for nobody else.  The sets hold pairs that differ only in the lead bit (bit 32
    resp. 60), only in the top count, only in the low word, and the largest valid key."""
    edge = W.edge_keys(M, HOPS) if nkeys >= 8 else ()
    keyset = W.lp_keys(nkeys, 100 + nkeys, M, HOPS, extra=edge)
    keys = _rows(TRIP_LENS, keyset, nkeys)
    present = W.members(keys, np.array(TRIP_LENS))
    assert np.array_equal(present, keyset) and (not edge or np.isin(np.array(edge, dtype=np.uint64), present).all())
    if edge:
        assert len(np.unique(present & np.uint64(0xFFFFFFFF))) < len(present)           # a 32-bit compare would merge keys
    res = _columns64(keys, TRIP_LENS, T, M)
    c, over = _check(res, keys, TRIP_LENS, T, M)
    assert over == (nkeys > T - 1) and c == min(nkeys, T - 1)
    cols = res[4]
    mask = np.arange(STRIDE)[None, :] < np.minimum(TRIP_LENS, STRIDE)[:, None]
    if over:
        dropped = keys == present[-1]
        assert dropped[mask].any() and np.array_equal((cols == 0) & mask, dropped & mask)
    else:
        assert (cols[mask] >= 1).all() and np.array_equal(res[1][cols[mask] - 1], keys[mask])


# ------------------------------------------------------------------------------------------------ 2. a crowded home in the LDS set
@pytest.mark.parametrize("M", SHAPES)
def test_forty_keys_of_one_home_against_the_32_probes(sp, M):
    """40 keys whose first slot in the block's LDS set is the same: the probes run out and keys go to the HBM set by themselves"""
    crowd, home = W.same_home_keys(40, 9, M, HOPS)
    assert len(crowd) == 40 > W.PROBES and (W.lds_home(crowd) == home).all()
    lens = [40, 0, 7, 256]
    keys = _rows(lens, crowd, 3)
    res = _columns64(keys, lens, 64, M)
    c, over = _check(res, keys, lens, 64, M)
    assert c == 40 and not over


# ------------------------------------------------------------------------------------------------ 3. the spill, the largest table
@pytest.mark.parametrize("M", SHAPES)
def test_5000_keys_in_one_blocks_range_with_the_largest_table(sp, M):
    """5,000 distinct keys in the 32 rows of one block: more than its 4,096-slot LDS set holds, the rest goes to the HBM set key by
    key; T = 8,192 is the largest table the call accepts (16,384 slots, 128 KiB sorted in LDS)"""
    T = W.MAX_T
    keyset = W.lp_keys(5000, 77, M, HOPS, extra=W.edge_keys(M, HOPS))
    lens = [STRIDE] * 30 + [1, 0]
    assert len(lens) == 32 == W.rows_per_block(len(lens)) and W.set_slots(T) * 8 == 128 * 1024
    keys = _rows(lens, keyset, 5)
    assert len(W.members(keys, np.array(lens))) == 5000 > 1 << W.DICT_BITS
    res = _columns64(keys, lens, T, M)
    c, over = _check(res, keys, lens, T, M)
    assert c == 5000 and not over


# ------------------------------------------------------------------------------------------------ 4. row counts
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 65])
def test_row_counts_around_a_blocks_smallest_range(sp, n):
    """a block's smallest range is 32 rows: 1, 31, 32 rows are one block, 33 two, 65 three; keys that stand in the last row alone;
    n = 0 runs the finish kernel alone -- count 0, zero lists, a zero table"""
    M, T = 30000, 300
    pool = W.lp_keys(250, 11 + n, M, HOPS, extra=W.edge_keys(M, HOPS))
    rng = np.random.default_rng(n)
    lens = [int(x) for x in rng.choice([0, 1, 5, 63, 64, 65], n)]
    if n:
        lens[-1] = 64
    room = int(np.sum(lens))
    main, last = pool[: max(min(room - 10, 240), 0)], pool[240:]
    keys, at = W.strided(lens, main, n, 96)
    if n:
        assert at == len(main)
        keys[n - 1, 54:64] = last                      # ten keys that only the very last row shows
    res = _columns64(keys, lens, T, M)
    c, over = _check(res, keys, lens, T, M)
    assert not over and c == (len(main) + 10 if n else 0)
    if n == 0:
        assert not res[1].any() and not res[2].any() and not res[3].any() and res[4].size == 0


def test_workspace_reused_after_an_overflowing_call(sp):
    """one workspace for a call whose keys overflow the columns and then a clean call with other keys, as StepBuffers reuses col_ws"""
    from surel_plus_amd import _lib
    M = 200
    pool = W.lp_keys(900, 21, M, HOPS)
    k1, k2 = pool[::2], pool[1::2]
    ws = _workspace(_lib.lib().subgacc_keyrows_columns64_workspace_bytes(460))
    lens = [STRIDE, 0, 200]
    r1, r2 = _rows(lens, k1, 1), _rows(lens, k2, 2)
    c, over = _check(_columns64(r1, lens, 300, M, ws=ws), r1, lens, 300, M)
    assert over and c == 299
    res = _columns64(r2, lens, 460, M, ws=ws)
    c, over = _check(res, r2, lens, 460, M)
    assert not over and c == 450 and not np.isin(res[1][:450], k1).any()


# ------------------------------------------------------------------------------------------------ 5. the count kernel over the surrogates
class _Surrogates:
    """the Rows layout with the surrogate plane as its payload: what _key_counts hands to subgacc_sjoin_key_counts as KEY32 rows"""

    def __init__(self, rows, cols):
        ids, _, nsize = rows.device()
        self.n, self.stride, self.a, self.b, self._dev = rows.n, rows.stride, rows.a, rows.b, (ids, cols, nsize)

    def device(self):
        return self._dev


@pytest.mark.parametrize("M", SHAPES)
@pytest.mark.parametrize("nkeys,T", [pytest.param(299, 300, id="299-keys"), pytest.param(40, 40, id="one-key-too-many")])
def test_the_count_kernel_over_the_surrogates_counts_the_64_bit_keys_ranks(sp, M, nkeys, T):
    """the Rows layout of LENS (a row with itself, with its neighbour, disjoint ids, full overlap, empty rows) whose members carry the
    64-bit key of rank r where Rows put r + 1: subgacc_sjoin_key_counts over (cols, out_ukeys, out_count) as KEY32 rows equals
    Rows.counts on those ranks, with and without a partner list; with one key too many the dropped key's members are not counted"""
    keys64 = W.lp_keys(nkeys, 31 + nkeys, M, HOPS, extra=W.edge_keys(M, HOPS))
    rows = Rows(np.arange(1, nkeys + 1, dtype=np.uint32), seed=nkeys)
    assert len(LENS) < rows.n and rows.stride == STRIDE
    mask = np.arange(rows.stride)[None, :] < rows.len[:, None]
    wide = np.full((rows.n, rows.stride), W.POISON64, dtype=np.uint64)
    wide[mask] = keys64[rows.keys[mask].astype(np.int64) - 1]
    res = _columns64(wide, rows.len, T, M)
    c, over = _check(res, wide, rows.len, T, M)
    assert c == min(nkeys, T - 1) and over == (nkeys > T - 1)
    want_cols = np.where(rows.keys[mask] <= c, rows.keys[mask], 0)
    assert np.array_equal(res[4][mask], want_cols.astype(np.int32))
    ukeys, count, cols = res[6]
    want, want_len, missing = rows.counts(np.arange(1, c + 1, dtype=np.uint32), T)
    assert missing == over
    for partner in (False, True):
        out, olen, fl = _key_counts(sp, _Surrogates(rows, cols), ukeys, count, T, partner=partner, M=M, hops=HOPS)
        print(f"count kernel over surrogates: T = {T}, partner list {partner}, flags = {fl.tolist()}")
        assert fl.tolist() == [0, 0, 0, 2 if over else 0]
        assert np.array_equal(out, want) and np.array_equal(olen, want_len)
        if not over:
            assert np.array_equal(out.sum(1), 2.0 * want_len)

"""GPU (MI355X): csrc/uniq.hip and csrc/uniq_table.hpp through their C entry points, on inputs built to stand at their limits
(inputs and references: tests/uniq_edges.py, shown to be what they claim by tests/test_uniq_edges_cpu.py).

The table of distinct LP rows -- subgacc_uniq_reset / _insert / _number / _translate as sampler.dedup_lp_rows calls them: every size
around the block, kUniqTile and kInsTile; the keys 0 and 2^64 - 2; more distinct keys in a tile than the LDS fold table has slots and
40 keys of one LDS home against its window of 16; chains of kMaxProbes and kMaxProbes + 1 keys of one home, wrapping past the last
slot; a table that is exactly full and one key more; chunked inserts in the wrong order with tag_base; the direct ranking against the
scan numbering on both sides of small_limit, with first occurrences on the tile edges of the scan; max_unique below the count;
translate under a device-side element count.  subgacc_unpack_lp at every key width up to bit 63, and its two refusals.  The three
step prologues: every span choice, ids at and beyond the ends of int32, roots that collide and wrap in the stamped table, five steps
on one workspace, and the step stamp across its wrap from 0xFFFFFFFF to 1.

Rules of this file.  Every output lies between two poisoned rims that must come back untouched.  Every comparison is bit for bit.
Every case runs twice and must give the same bits.

Pinned behaviour that the code, not the reference, defines:
  * subgacc_uniq_number with n = 0 (slot = NULL) and more than small_limit distinct keys numbers nothing: out_count is the count, the
    ids stay -1 and out_ukeys is untouched (the scan path has no elements to scan); at most small_limit keys are ranked as usual.
  * a key that an over-full table drops (flags[2]) has out_slot 0: every out_slot is a slot of the table.
  * the work list of the dedup prologues is compared as a set: its order is the order of arrival."""
import ctypes as C

import numpy as np
import pytest
import torch

import uniq_edges as E

pytestmark = pytest.mark.gpu

RIM = 256                                   # elements on either side of every output
POISON = {torch.uint8: 0x5A, torch.int16: 0x5A5A, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}
FLAGS0 = [7, 9, 0, 11]                      # flags[0], [1], [3] must come back as they went in
ERR_KEYWIDTH = -3


@pytest.fixture(scope="module", autouse=True)
def L():
    import os
    from surel_plus_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libsubgacc_hip.so must be built (no fallback)"
    assert _lib.lib().subgacc_device_count() >= 1, "no gfx950 device"
    return _lib


def _L():
    from surel_plus_amd import _lib
    return _lib


class Rimmed:
    """n elements of `dtype` on the device, poisoned, between two poisoned rims"""

    def __init__(self, n, dtype, init=None):
        self.n, self.poison = int(n), POISON[dtype]
        self.whole = torch.full((self.n + 2 * RIM,), self.poison, dtype=dtype, device="cuda")
        self.t = self.whole[RIM:RIM + self.n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).view(dtype).cuda())

    def ptr(self, offset=0):
        return C.c_void_p(self.whole.data_ptr() + (RIM + offset) * self.whole.element_size())

    def host(self):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        assert (w[:RIM] == self.poison).all(), "the rim in front of an output was written"
        assert (w[RIM + self.n:] == self.poison).all(), "the rim behind an output was written"
        return w[RIM:RIM + self.n].copy()


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _table(raw, cap):
    """the table's bytes -> (keys uint64 [cap], mintag uint64 [cap], id int32 [cap])"""
    return raw[:8 * cap].view(np.uint64), raw[8 * cap:16 * cap].view(np.uint64), raw[16 * cap:20 * cap].view(np.int32)


def _same(a, b, names):
    for k in names:
        assert np.array_equal(a[k], b[k]), f"two runs of one case differ in {k}"


# ------------------------------------------------------------------------------------------------------------- insert, number, translate
def _uniq(keys, cap, small_limit=0, chunks=None, max_unique=None, add=0, n_dev=None, null_number=False):
    """reset, insert (one call per chunk (start, end), in the order given), number, translate -- as sampler.dedup_lp_rows calls them.
    null_number: number with slot = NULL and n = 0 (and no translate)."""
    lib = _L().lib()
    st = _L().stream_ptr()
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    c = len(np.unique(keys))
    max_unique = c + 8 if max_unique is None else max_unique
    d_keys = _dev(keys)
    nbytes = lib.subgacc_uniq_table_bytes(cap)
    assert nbytes == 20 * cap
    table = Rimmed(nbytes, torch.uint8)
    slot = Rimmed(n, torch.int32)
    flags = Rimmed(4, torch.int32, np.array(FLAGS0, dtype=np.int32))
    ukeys = Rimmed(max_unique, torch.int64)
    count = Rimmed(1, torch.int64)
    nn = 0 if null_number else n
    ws = Rimmed(lib.subgacc_uniq_number_workspace_bytes(cap, nn), torch.uint8)
    rcs = [lib.subgacc_uniq_reset(table.ptr(), cap, st)]
    for a, b in ([(0, n)] if chunks is None else chunks):
        rcs.append(lib.subgacc_uniq_insert(table.ptr(), cap, C.c_void_p(d_keys.data_ptr() + 8 * a), b - a, a, slot.ptr(a), flags.ptr(), st))
    res = {"n": n, "cap": cap, "slot": slot.host(), "table_in": table.host()}
    rcs.append(lib.subgacc_uniq_number(table.ptr(), cap, C.c_void_p(0) if null_number else slot.ptr(), nn,
                                       ukeys.ptr() if max_unique else C.c_void_p(0), max_unique, count.ptr(), small_limit, ws.ptr(),
                                       ws.n, st))
    if not null_number:
        d_n = None if n_dev is None else _dev(np.array([n_dev], dtype=np.int64))
        rcs.append(lib.subgacc_uniq_translate(table.ptr(), cap, slot.ptr(), n, C.c_void_p(d_n.data_ptr()) if d_n is not None else C.c_void_p(0),
                                              add, st))
    ws.host()
    res.update(rcs=rcs, sf=slot.host(), table=table.host(), flags=flags.host(), ukeys=ukeys.host().view(np.uint64), count=count.host()[0])
    return res


def _check_uniq(res, keys, add=0, n_dev=None, max_unique=None, numbered=True):
    keys = np.asarray(keys, dtype=np.uint64)
    n, cap = len(keys), res["cap"]
    sf, ukeys, first = E.ref_uniq(keys)
    c = len(ukeys)
    assert all(rc == 0 for rc in res["rcs"]), res["rcs"]
    assert res["flags"].tolist() == FLAGS0, "flags[0], [1], [3] are not this call's, flags[2] = 0: every key found a slot"
    assert res["count"] == c
    # the table, byte for byte: the occupied slots are exactly the distinct keys, each with its first position, ids a permutation of 0..c
    for name in ("table_in", "table"):
        tk, tt, tid = _table(res[name], cap)
        occ = tk != E.EMPTY_KEY
        assert occ.sum() == c and np.array_equal(np.sort(tk[occ]), np.sort(ukeys))
        order = np.argsort(tk[occ])
        want_first = first[np.argsort(ukeys)]
        assert np.array_equal(tt[occ][order], want_first.astype(np.uint64)), "mintag is not the key's first position"
        assert (tt[~occ] == E.EMPTY_KEY).all() and (tid[~occ] == -1).all()
        if name == "table_in" or not numbered:
            assert (tid == -1).all()
        else:
            assert np.array_equal(np.sort(tid[occ]), np.arange(c))
            assert np.array_equal(tid[occ][order], np.argsort(np.argsort(want_first)))     # id = rank of the first position
    # every member's slot holds its key
    tk = _table(res["table_in"], cap)[0]
    assert ((res["slot"] >= 0) & (res["slot"] < cap)).all() and np.array_equal(tk[res["slot"]], keys)
    mu = c + 8 if max_unique is None else max_unique
    w = min(c, mu) if numbered else 0
    assert np.array_equal(res["ukeys"][:w], ukeys[:w])
    assert (res["ukeys"][w:] == np.uint64(POISON[torch.int64])).all(), "out_ukeys was written beyond min(count, max_unique)"
    if numbered:
        lim = n if n_dev is None else max(0, min(n, n_dev))
        assert np.array_equal(res["sf"][:lim], sf[:lim] + add)
        assert np.array_equal(res["sf"][lim:], res["slot"][lim:]), "elements at and past min(n, *n_dev) keep their slots"
    else:
        assert np.array_equal(res["sf"], res["slot"])


def _twice(keys, cap, check=True, **kw):
    a, b = _uniq(keys, cap, **kw), _uniq(keys, cap, **kw)
    # (untranslated, `sf` still holds the slots, and which key of a chain gets which slot is the order of arrival)
    _same(a, b, ("ukeys", "count", "flags") if kw.get("null_number") else ("sf", "ukeys", "count", "flags"))
    if check:
        _check_uniq(a, keys, add=kw.get("add", 0), n_dev=kw.get("n_dev"), max_unique=kw.get("max_unique"),
                    numbered=not kw.get("null_number", False))
    return a


@pytest.mark.parametrize("kind", E.KEY_SETS)
@pytest.mark.parametrize("n", E.INSERT_SIZES)
def test_sizes_around_the_block_and_both_tiles(n, kind):
    keys = E.sized_keys(n, kind)
    for small_limit in (0, 16):             # direct ranking; the scan numbering wherever there are more than 16 distinct keys
        _twice(keys, 16384, small_limit=small_limit)


def test_extreme_keys():
    keys = np.array([2 ** 64 - 2, 0, 5, 0, 2 ** 64 - 2, 2 ** 63, 1, 2 ** 63, 2 ** 64 - 2], dtype=np.uint64)
    for small_limit in (0, 2):
        res = _twice(keys, 64, small_limit=small_limit)
        assert res["ukeys"][:5].tolist() == [2 ** 64 - 2, 0, 5, 2 ** 63, 1]


def test_more_distinct_keys_in_a_tile_than_lds_slots():
    keys = E.sized_keys(E.INS_TILE, "distinct", seed=1)
    assert len(np.unique(E.lds_home(keys))) <= E.LDS_SLOTS < len(keys)
    for small_limit in (0, 16):
        _twice(keys, 8192, small_limit=small_limit)


@pytest.mark.parametrize("split", [False, True])
def test_forty_keys_of_one_lds_home(split):
    keys, crowd = E.lds_crowd(split)        # at most 16 of the 40 fit the window: 24 and more go straight to HBM
    for small_limit in (0, 16):
        _twice(keys, 4096, small_limit=small_limit)


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("home", [3, 255])
def test_chain_of_max_probes_is_accepted(home, spread):
    keys = E.chain_keys(E.MAX_PROBES, 256, home, spread)
    for small_limit in (0, 16):
        res = _twice(keys, 256, small_limit=small_limit)
        occ = np.flatnonzero(_table(res["table"], 256)[0] != E.EMPTY_KEY)
        assert np.array_equal(np.sort((occ - home) % 256), np.arange(128)), "one unbroken chain from the home slot, wrapping at the end"


def _flagged(keys, cap):
    res = _uniq(keys, cap)
    assert all(rc == 0 for rc in res["rcs"])
    assert res["flags"].tolist() == [FLAGS0[0], FLAGS0[1], 1, FLAGS0[3]]
    assert ((res["slot"] >= 0) & (res["slot"] < cap)).all(), "a dropped key's slot must still be a slot of the table"
    return res


@pytest.mark.parametrize("home", [3, 255])
def test_chain_of_max_probes_plus_one_is_flagged(home):
    _flagged(E.chain_keys(E.MAX_PROBES + 1, 256, home, spread=True), 256)


def test_table_exactly_full_and_one_key_more():
    keys = E.sized_keys(65, "distinct", seed=2)
    full = np.r_[keys[:64], keys[:64][::-1]]
    for small_limit in (0, 16):
        res = _twice(full, 64, small_limit=small_limit)
        assert (_table(res["table"], 64)[0] != E.EMPTY_KEY).all()
    _flagged(np.r_[keys, keys], 64)


@pytest.mark.parametrize("n,n1", [(3000, 1500), (2 * 2048 + 77, 2048 + 1), (700, 255)])
def test_chunks_in_the_wrong_order_with_tag_base(n, n1):
    rng = np.random.default_rng(n1)
    vals = rng.integers(0, 1 << 62, size=90, dtype=np.uint64)
    keys = np.r_[vals[rng.integers(0, 50, size=n1)], vals[rng.integers(25, 90, size=n - n1)]]
    first = E.ref_uniq(keys)[2]
    assert (first < n1).any() and (first >= n1).any() and np.isin(keys[:n1], keys[n1:]).any()
    for small_limit in (0, 16):
        _twice(keys, 1024, small_limit=small_limit, chunks=[(n1, n), (0, n1)])


@pytest.mark.parametrize("c", [1, 255, 256, 257, 600])
def test_both_sides_of_small_limit(c):
    keys = E.repeated(c, 2 * c + 3)
    out = [_twice(keys, 1024, small_limit=sl) for sl in (c, c - 1, c + 1)]       # c - 1: the scan numbering (0 at c = 1: the default)
    _same(out[0], out[1], ("sf", "ukeys", "count"))
    _same(out[0], out[2], ("sf", "ukeys", "count"))


def test_first_occurrences_on_the_scan_tile_edges():
    n = 4 * E.UNIQ_TILE + 100
    keys = E.first_at((0, 5, 1023, 1024, 1500, 2047, 2048, 2049, n - 1), n)
    a = _twice(keys, 64, small_limit=3)         # 9 > 3: the scan numbering, tile 3 without a first occurrence
    b = _twice(keys, 64, small_limit=9)
    _same(a, b, ("sf", "ukeys", "count"))


def test_small_limit_defaults_and_clamp():
    _twice(E.repeated(200, 500), 256, small_limit=10 ** 6)          # clamped to the capacity
    # 0 means 8,192: with nothing to scan (n = 0, slot = NULL) 8,192 keys are ranked and 8,193 are only counted
    for c in (8192, 8193):
        keys = E.sized_keys(c, "distinct", seed=3)
        res = _twice(keys, 16384, small_limit=0, null_number=True, check=False)
        _check_uniq(res, keys, numbered=c <= 8192, n_dev=0)         # nothing was translated
        if c <= 8192:
            assert np.array_equal(res["ukeys"][:c], E.ref_uniq(keys)[1])


@pytest.mark.parametrize("small_limit", [0, 16])
def test_max_unique_below_the_count(small_limit):
    keys = E.repeated(300, 2500)
    for mu in (0, 299, 300):
        _twice(keys, 1024, small_limit=small_limit, max_unique=mu)


def test_number_without_elements():
    keys = E.repeated(600, 1300)
    _twice(keys, 1024, small_limit=16, null_number=True)            # 600 > 16 and nothing to scan: counted, not numbered
    res = _twice(keys, 1024, small_limit=600, null_number=True, check=False)
    _check_uniq(res, keys, numbered=True, n_dev=0)                   # ranked from the table alone; nothing translated


@pytest.mark.parametrize("add", [0, 1])
def test_translate_under_a_device_side_count(add):
    keys = E.repeated(77, 1000)
    for n_dev in (None, 0, 999, 1000, 1005):
        _twice(keys, 256, add=add, n_dev=n_dev)


# ------------------------------------------------------------------------------------------------------------- subgacc_unpack_lp
UNPACK = [(1, 1), (255, 7), (256, 7), (126, 9), (200, 3), (32767, 4)]


def _unpack(keys, M, m, n_dev, outs, zero_row):
    lib = _L().lib()
    n, ncol = len(keys), m + 1
    d_keys = _dev(keys)
    d_n = None if n_dev is None else _dev(np.array([n_dev], dtype=np.int64))
    o16 = Rimmed(n * ncol, torch.int16) if "i16" in outs else None
    o32 = Rimmed(n * ncol, torch.int32) if "i32" in outs else None
    f32 = Rimmed((n + (1 if zero_row else 0)) * ncol, torch.int32) if "f32" in outs else None
    null = C.c_void_p(0)
    rc = lib.subgacc_unpack_lp(C.c_void_p(d_keys.data_ptr()) if n else null, n, C.c_void_p(d_n.data_ptr()) if d_n is not None else null, M, m,
                               o16.ptr() if o16 else null, o32.ptr() if o32 else null, f32.ptr() if f32 else null, zero_row,
                               _L().stream_ptr())
    return rc, {k: (o.host() if o else None) for k, o in (("i16", o16), ("i32", o32), ("f32", f32))}


def _check_unpack(keys, M, m, n_dev, outs, zero_row):
    (rc, got), (rc2, got2) = _unpack(keys, M, m, n_dev, outs, zero_row), _unpack(keys, M, m, n_dev, outs, zero_row)
    assert rc == 0 and rc2 == 0
    n = len(keys)
    rows = E.ref_unpack(keys, M, m)
    frows = E.ref_unpack_f32(keys, M, m)
    lim = n if n_dev is None else max(0, min(n, n_dev))
    rows[lim:], frows[lim:] = 0, 0                          # rows past the device-side count are zero
    if zero_row:
        frows = np.r_[np.zeros((1, m + 1), np.float32), frows]
    for k, want in (("i16", rows.astype(np.int16)), ("i32", rows.astype(np.int32)), ("f32", frows.view(np.int32))):
        if k in outs:
            assert np.array_equal(got[k], want.reshape(-1)), f"{k} of (M, m) = ({M}, {m}), n = {n}, n_dev = {n_dev}"
            assert np.array_equal(got[k], got2[k])
        else:
            assert got[k] is None


@pytest.mark.parametrize("M,m", UNPACK)
def test_unpack_lp(M, m):
    rng = np.random.default_rng(M + m)
    for n in (0, 1, m, 255, 256, 257):
        keys = np.r_[E.random_keys(rng, n // 2, M, m, 1), E.random_keys(rng, n - n // 2, M, m, 0)]
        rng.shuffle(keys)
        if n > 1:
            keys[0] = E.pack_rows(np.array([[1] + [(1 << E.key_shift(M)) - 1] * (m - 1) + [0]]), M, m)[0]    # every field but the last full
        _check_unpack(keys, M, m, None, ("i16", "i32", "f32"), 1)
        for outs in (("i16",), ("i32",), ("f32",)):
            _check_unpack(keys, M, m, None, outs, 1)
        _check_unpack(keys, M, m, None, ("f32",), 0)
        for n_dev in (0, n - 1, n + 3):
            _check_unpack(keys, M, m, n_dev, ("i16", "i32", "f32"), 1)
            _check_unpack(keys, M, m, n_dev, ("f32", "i32"), 0)


@pytest.mark.parametrize("M,m", [(127, 9), (200, 8)])
def test_unpack_lp_refuses_what_cannot_be_a_key(M, m):
    keys = np.arange(1, 258, dtype=np.uint64)
    for zero_row in (0, 1):
        rc, got = _unpack(keys, M, m, None, ("i16", "i32", "f32"), zero_row)
        assert rc == ERR_KEYWIDTH
        assert (got["i16"] == POISON[torch.int16]).all() and (got["i32"] == POISON[torch.int32]).all()
        assert (got["f32"] == POISON[torch.int32]).all()


# ------------------------------------------------------------------------------------------------------------- the prologues
def _workspace(n):
    ws = Rimmed(_L().lib().subgacc_step_dedup_workspace_bytes(n), torch.uint8)
    ws.t.zero_()
    return ws


def _stamp(ws, value=None):
    word = ws.t[:8].view(torch.int64)
    if value is not None:
        word.fill_(value)
    return int(word.item())


def _prologue(kind, edge, cap, n_zero, ws=None, roles=None):
    """kind: "plain" | "dedup" | "roles" (roles = (B, r, s)); cap = 0: uniq_table = NULL"""
    lib, st = _L().lib(), _L().stream_ptr()
    edge = np.asarray(edge, dtype=np.int64)
    n = len(edge)
    d_edge = _dev(edge)
    null = C.c_void_p(0)
    table = Rimmed(20 * cap, torch.uint8) if cap else None
    zero = Rimmed(n_zero, torch.int64)
    roots = Rimmed(n, torch.int32)
    own = Rimmed(roles[2] * roles[0] if roles else n, torch.int64)
    partner, worklist, row_len, nd = Rimmed(n, torch.int64), Rimmed(n, torch.int32), Rimmed(n, torch.int32), Rimmed(1, torch.int64)
    tp, zp = (table.ptr() if cap else null), (zero.ptr() if n_zero else null)
    if kind == "plain":
        rc = lib.subgacc_step_prologue(tp, cap, zp, n_zero, C.c_void_p(d_edge.data_ptr()), roots.ptr(), n, st)
    else:
        ws = _workspace(n) if ws is None else ws
        if kind == "dedup":
            rc = lib.subgacc_step_prologue_dedup(tp, cap, zp, n_zero, C.c_void_p(d_edge.data_ptr()), roots.ptr(), own.ptr(), partner.ptr(),
                                                 worklist.ptr(), row_len.ptr(), n, ws.ptr(), ws.n, nd.ptr(), st)
        else:
            B, r, s = roles
            rc = lib.subgacc_step_prologue_dedup_roles(tp, cap, zp, n_zero, C.c_void_p(d_edge.data_ptr()), roots.ptr(), own.ptr(),
                                                       worklist.ptr(), row_len.ptr(), n, B, r, s, ws.ptr(), ws.n, nd.ptr(), st)
        ws.host()
    return {"rc": rc, "table": table.host() if cap else None, "zero": zero.host(), "roots": roots.host(), "own": own.host(),
            "partner": partner.host(), "worklist": worklist.host(), "row_len": row_len.host(), "nd": nd.host()[0], "cap": cap}


def _check_prologue(res, kind, edge, roles=None):
    n = len(edge)
    assert res["rc"] == 0
    assert (res["zero"] == 0).all(), "the n_zero status words"
    if res["cap"]:                                            # the LP table is reset
        tk, tt, tid = _table(res["table"], res["cap"])
        assert (tk == E.EMPTY_KEY).all() and (tt == E.EMPTY_KEY).all() and (tid == -1).all()
    p32, p64 = POISON[torch.int32], POISON[torch.int64]
    if kind == "plain":
        assert np.array_equal(res["roots"], E.narrow(edge))
        for k, p in (("own", p64), ("partner", p64), ("worklist", p32), ("row_len", p32)):
            assert (res[k] == p).all()
        return
    if kind == "dedup":
        roots, own, partner, zeroed, nd = E.ref_dedup(edge)
        assert np.array_equal(res["partner"], partner)
    else:
        roots, own, zeroed, nd = E.ref_dedup_roles(edge, *roles)
        assert (res["partner"] == p64).all()
    assert np.array_equal(res["roots"], roots) and np.array_equal(res["own"], own) and res["nd"] == nd
    assert (res["row_len"][zeroed] == 0).all() and (res["row_len"][~zeroed] == p32).all(), "row_len: 0 at the repeats and only there"
    assert np.array_equal(np.sort(res["worklist"][:nd]), np.flatnonzero(~zeroed)), "the work list is the set of first occurrences"
    assert (res["worklist"][nd:] == p32).all(), "the work list was written beyond n_distinct"


def _prologue_twice(kind, edge, cap, n_zero, roles=None):
    a, b = _prologue(kind, edge, cap, n_zero, roles=roles), _prologue(kind, edge, cap, n_zero, roles=roles)
    for k in ("zero", "roots", "own", "partner", "row_len", "nd"):
        assert np.array_equal(a[k], b[k]), f"two runs of one case differ in {k}"
    assert np.array_equal(np.sort(a["worklist"][:a["nd"]]), np.sort(b["worklist"][:b["nd"]]))
    _check_prologue(a, kind, edge, roles)
    return a


def _spans(n):
    """(capacity, n_zero): the launch is sized by n, by the capacity, by n_zero; and without a table"""
    lo = 1 << max(0, (n - 1).bit_length() - 1)              # the largest power of two below n (1 at n = 2)
    hi = 1 << (n.bit_length() + 1)
    return [(lo, 5), (hi, 5), (hi, hi + 7), (lo, n + 300), (0, 3), (0, 0)]


@pytest.mark.parametrize("batch", ["one", "distinct", "random", "self", "ends", "outside"])
@pytest.mark.parametrize("B", [1, 127, 128, 129, 1000])
def test_pair_prologues(B, batch):
    edge = E.pair_batch(B, batch)
    for cap, n_zero in _spans(2 * B) if batch == "random" else _spans(2 * B)[:2]:
        a = _prologue_twice("dedup", edge, cap, n_zero)
        b = _prologue_twice("roles", edge, cap, n_zero, roles=(B, 2, 2))
        for k in ("roots", "own", "row_len", "nd"):
            assert np.array_equal(a[k], b[k]), "(r, s) = (2, 2) is the pair form"
        _prologue_twice("plain", edge, cap, n_zero)


def test_plain_prologue_with_nothing_but_status_words_or_a_table():
    for cap, n_zero in ((0, 300), (512, 0), (0, 0)):
        res = _prologue("plain", np.zeros(0, np.int64), cap, n_zero)
        _check_prologue(res, "plain", np.zeros(0, np.int64))


@pytest.mark.parametrize("B", [1, 85, 86, 341])
def test_triplet_prologue(B):
    edge = E.triplet_batch(B)
    for cap, n_zero in _spans(3 * B):
        _prologue_twice("roles", edge, cap, n_zero, roles=(B, 3, 4))
        _prologue_twice("plain", edge, cap, n_zero)


@pytest.mark.parametrize("c,B", [(1024, 140), (2048, 300)])
def test_roots_that_collide_and_wrap(c, B):
    edge, crowd = E.colliding_batch(c, B)
    _prologue_twice("dedup", edge, 64, 5)
    _prologue_twice("roles", edge, 64, 5, roles=(B, 2, 2))
    _prologue_twice("dedup", edge[::-1].copy(), 64, 5)


def _step(kind, edge, ws):
    n = len(edge)
    roles = None if kind == "dedup" else ((n // 3, 3, 4) if kind == "triplets" else (n // 2, 2, 2))
    k = "dedup" if kind == "dedup" else "roles"
    _check_prologue(_prologue(k, edge, 256, 9, ws=ws, roles=roles), k, edge, roles)


@pytest.mark.parametrize("kind", ["dedup", "roles", "triplets"])
def test_five_steps_on_one_workspace(kind):
    n = 600
    e1 = E.colliding_batch(2048, 300)[0] if kind != "triplets" else E.triplet_batch(200)
    rng = np.random.default_rng(9)
    batches = [e1, rng.integers(0, 150, size=n).astype(np.int64), e1[::-1].copy(), np.full(n, int(e1[0]), dtype=np.int64),
               np.r_[e1[n // 2:], e1[:n // 2]]]
    for rep in range(2):
        ws = _workspace(n)
        for i, e in enumerate(batches):
            _step(kind, e, ws)                                  # batch 3 is batch 1 reversed: every root's row changes, its slot does not
            assert _stamp(ws) == i + 1


@pytest.mark.parametrize("kind", ["dedup", "roles", "triplets"])
def test_the_stamp_wraps(kind):
    """stamps 1, 2, then 0xFFFFFFFF, 1, 2: the step after 0xFFFFFFFF must not lose against the stamps of the era that ends"""
    n = 600
    rng = np.random.default_rng(17)
    e1 = E.colliding_batch(2048, 300)[0] if kind != "triplets" else E.triplet_batch(200)
    e2 = rng.integers(0, 150, size=n).astype(np.int64)
    e3 = rng.integers(0, 400, size=n).astype(np.int64) * 7
    batches = [e1, e2, e3, e3[::-1].copy(), np.roll(e1, 1)]
    stamps = [1, 2, 0xFFFFFFFF, 1, 2]
    for rep in range(2):
        ws = _workspace(n)
        for i, (e, want) in enumerate(zip(batches, stamps)):
            if i == 2:
                assert _stamp(ws, 0xFFFFFFFE) == 0xFFFFFFFE
            print(f"run {rep + 1}, step {i + 1} of 5: stamp {_stamp(ws):#x} -> {want:#x}")
            _step(kind, e, ws)
            assert _stamp(ws) == want, f"step {i + 1}"

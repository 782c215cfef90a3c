"""CPU: the inputs of tests/test_gpu_keyrows_edges.py are what they claim to be (tests/keyrows_edges.py).  kr_home equals a scalar
restatement in Python integers; the key families share their home, are distinct and lie below 2^31; the references equal plain
sequential loops; every crowded input leaves keys out of the modelled dictionary in the order given (and, with more keys of one home
than probes, in any order); every store stands on the edge it is named for.  And the four subgacc_keyrows_* entry points refuse what
they must before anything is launched (no GPU is needed for that)."""
import ctypes as C

import numpy as np
import pytest

import keyrows_edges as K


def _home(k):
    h = k * 0x9E3779B1 % 2 ** 32
    h ^= h >> 15
    h = h * 0x85EBCA77 % 2 ** 32
    return h >> 20


def test_kr_home_is_the_hash_it_restates():
    ks = [0, 1, 2, 12345, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 0x7E7E7E7E, 0x9E3779B1]
    assert K.kr_home(np.array(ks, dtype=np.uint32)).tolist() == [_home(k) for k in ks]
    assert K.kr_home(np.array(ks, dtype=np.uint32).view(np.int32)).tolist() == [_home(k) for k in ks]     # the pattern, not the sign
    rng = np.random.default_rng(1)
    ks = rng.integers(0, 2 ** 32, size=2000, dtype=np.uint64)
    assert K.kr_home(ks).tolist() == [_home(int(k)) for k in ks]
    assert K.DICT == 4096 and K.DICT_MAX == 3072 and K.GROUP == 512 and K.TRANSLATE_BLOCK == 16384
    assert [K.rows_per_block(n) for n in (0, 1, 65, 4096 * 33 - 1, 4096 * 33, 4096 * 33 + 5, 4096 * 64, 4096 * 4095, 4096 * 4096,
                                          4096 * 5000)] == [32, 32, 32, 32, 33, 33, 64, 4095, 4096, 4096]


@pytest.mark.parametrize("home", [0, 1, 2047, K.CROWD_HOME, K.CROWD_HOME + 1])
def test_same_home(home):
    keys = K.same_home(K.CROWD, home)
    assert len(np.unique(keys)) == K.CROWD and (K.kr_home(keys) == home).all()
    assert keys.min() >= 1 and keys.max() < 2 ** 31 and not (keys == K.KEY_POISON).any()
    # one home and PROBES slots: whatever the order, at most PROBES of them find an entry
    for order in (keys, keys[::-1]):
        assert K.dict_leftover(order) == K.CROWD - K.PROBES
    assert K.dict_leftover(keys[:K.PROBES]) == 0 and K.dict_leftover(keys[:K.PROBES + 1]) == 1


def test_the_two_crowds_overlap_and_wrap():
    a, b = K.crowd_keys()
    assert not np.isin(a, b).any() and K.CROWD_HOME + K.PROBES > K.DICT          # the chains run on at entry 0
    # 80 keys for the PROBES + 1 entries the two homes can reach
    for order in (np.r_[a, b], np.r_[b, a], np.random.default_rng(0).permutation(np.r_[a, b])):
        assert K.dict_leftover(order) == 2 * K.CROWD - (K.PROBES + 1)


def _loop_register(keys, nsize, stride, root_base):
    ku = np.asarray(keys).view(np.uint32)
    first = {}
    for i in range(len(nsize)):
        for r in range(min(int(nsize[i]), stride)):
            first.setdefault(int(ku[i * stride + r]), (i, r))
    return first


def _loop_compact(ids, keys, nsize, stride, number):
    ku = np.asarray(keys).view(np.uint32)
    oi, od = [], []
    for i in range(len(nsize)):
        for r in range(min(int(nsize[i]), stride)):
            k = int(ku[i * stride + r])
            oi.append(int(ids[i * stride + r]))
            od.append(number.get(k, -1) + 1 if number is not None else (k - 2 ** 32 if k >= 2 ** 31 else k))
    return np.array(oi, dtype=np.int32), np.array(od, dtype=np.int32)


def _small_cases():
    out = [K.small_store(n, kind) for n in K.SMALL_N for kind in ("mixed", "empty")]
    out += [K.long_rows(ns) for ns in (1, 65, K.GROUP, K.LONG_STRIDE)]
    out += [K.crowded_store("one_row"), K.crowded_store("spread"), K.valued_store("low"), K.valued_store("high"), K.many_keys(300)[0]]
    return out


def test_references_against_sequential_loops():
    for ids, keys, nsize, stride in _small_cases():
        for root_base in (0, 2 ** 33 // stride):
            ref = K.ref_register(keys, nsize, stride, root_base)
            first = _loop_register(keys, nsize, stride, root_base)
            assert ref["keys"].tolist() == sorted(first)
            assert [(int(f), int(r)) for f, r in zip(ref["f"], ref["r"])] == [first[k] for k in sorted(first)]
            assert ref["coarse"].tolist() == [(root_base + first[k][0]) * stride + stride - 1 for k in sorted(first)]
            assert ref["exact"].tolist() == [(root_base + first[k][0]) * stride + first[k][1] for k in sorted(first)]
            assert ref["ukeys"].tolist() == list(first)                         # a dict keeps the order of first appearance
            assert ref["ukeys"][ref["number"]].tolist() == ref["keys"].tolist()
            assert ref["first_rows"].tolist() == sorted({f for f, _ in first.values()})
            assert ref["first_slot"] == (min(f * stride + r for f, r in first.values()) if first else -1)
        number = {k: x for x, k in enumerate(first)}
        off = K.row_offsets(nsize, stride)
        assert off[-1] == np.minimum(nsize, stride).sum() and (np.diff(off) == np.minimum(nsize, stride)).all()
        for ukeys, num in ((ref["ukeys"], number), (None, None), (ref["ukeys"][:3], {k: x for k, x in number.items() if x < 3})):
            oi, od = K.ref_compact(ids, keys, nsize, stride, off, ukeys)
            li, ld = _loop_compact(ids, keys, nsize, stride, num)
            assert np.array_equal(oi, li) and np.array_equal(od, ld) and oi.dtype == od.dtype == np.int32
        # translate: the packed keys under the numbering; beyond n_eff nothing changes; a stranger gives 0
        data = K.ref_compact(ids, keys, nsize, stride, off)[1]
        want = K.ref_compact(ids, keys, nsize, stride, off, ref["ukeys"])[1]
        for n_eff in (0, len(data) - 1, len(data), len(data) + 7):
            got = K.ref_translate(data, n_eff, ref["ukeys"])
            lim = max(0, min(len(data), n_eff))
            assert np.array_equal(got[:lim], want[:lim]) and np.array_equal(got[lim:], data[lim:])
        assert K.ref_translate(np.array([K.STRANGER], np.int32), 1, ref["ukeys"]).tolist() == [0] or K.STRANGER in first


def test_poison_is_nobodys_key_and_sits_behind_every_row():
    for ids, keys, nsize, stride in _small_cases():
        ku, ns = keys.view(np.uint32).reshape(-1, stride), np.minimum(nsize, stride)
        dead = np.arange(stride)[None, :] >= ns[:, None]
        assert (ku[dead] == K.KEY_POISON).all() and not (ku[~dead] == K.KEY_POISON).any() and not (ku[~dead] == K.EMPTY_ENTRY).any()
        assert (ids.reshape(-1, stride)[dead] == K.ID_POISON).all() and not (ids.reshape(-1, stride)[~dead] == K.ID_POISON).any()


@pytest.mark.parametrize("n", K.SMALL_N)
def test_small_stores(n):
    ids, keys, nsize, stride = K.small_store(n)
    assert len(nsize) == n and K.rows_per_block(n) == K.MIN_ROWS
    assert K.range_census(keys, nsize, stride)[0] <= len(K.FAMILY) <= K.PROBES                # nothing can be crowded
    if n >= 7:
        assert nsize[0] == 0 and nsize[n // 2] == 0 and nsize[min(31, n - 1)] == 0 and (nsize > 0).any()
    if n > K.MIN_ROWS:
        assert nsize[K.MIN_ROWS] == 0 and nsize[n - 1] == 0
    assert K.small_store(n, "empty")[2].sum() == 0
    assert K.range_census(*K.small_store(n, "empty")[1:]) == (0, 0)


@pytest.mark.parametrize("ns", K.LONG_NS)
def test_long_rows(ns):
    ids, keys, nsize, stride = K.long_rows(ns)
    assert stride == 2 * K.GROUP + 1 and nsize[7] == stride + 5 and nsize[5] == 0 and (np.delete(nsize, [5, 7]) == ns).all()
    ref = K.ref_register(keys, nsize, stride)
    for row in (0, 2):
        got = set(ref["r"][ref["f"] == row].tolist())
        assert got == {p for p in (0, K.GROUP - 1, K.GROUP, ns - 1) if p < ns}, (row, got)
    if ns < stride:
        assert (stride - 1) in ref["r"][ref["f"] == 7]          # seen only if nsize[7] > stride is read as stride
    assert K.range_census(keys, nsize, stride)[0] <= K.PROBES
    if ns > 1:                                                   # the numbering is not the order of the key values
        assert not np.array_equal(ref["ukeys"], np.sort(ref["ukeys"]))


@pytest.mark.parametrize("rpb", [33, 64])
def test_wide_stores(rpb):
    ids, keys, nsize, stride, planted = K.wide_store(rpb)
    n = len(nsize)
    assert n == K.WIDE_N[rpb] and K.rows_per_block(n) == rpb and (n % rpb != 0) == (rpb == 33)
    ref = K.ref_register(keys, nsize, stride)
    assert np.isin(planted, ref["first_rows"]).all()
    local = planted % rpb
    assert {0, rpb - 1} <= set(local.tolist()) and (rpb != 33 or 32 in local)          # local row 32: the second bitmap word
    assert (planted // rpb).max() == (n - 1) // rpb and n - 1 in planted
    most, total = K.range_census(keys, nsize, stride)
    assert most <= K.PROBES and total < n // 2                  # a pass that lists every row breaks the bound on n_cand
    assert set(np.unique(nsize).tolist()) == {0, 1, 2, 3, 4}


def test_full_store():
    keys, nsize, stride, planted = K.full_store()
    n = len(nsize)
    assert n == 4096 * 4096 and stride == 1 and K.rows_per_block(n) == K.MAX_ROWS
    assert (planted % K.MAX_ROWS).tolist() == [0, K.MAX_ROWS - 1, 0, K.MAX_ROWS - 1]
    ref = K.ref_register(keys, nsize, stride)
    assert np.isin(planted, ref["first_rows"]).all() and 200 < len(ref["keys"]) <= 304
    most, total = K.range_census(keys, nsize, stride)
    assert most <= K.PROBES and total < n // 100
    assert (nsize == 0).sum() > n // 100 and not (keys.view(np.uint32)[nsize > 0] == K.KEY_POISON).any()


@pytest.mark.parametrize("layout", ["one_row", "spread"])
def test_crowded_stores(layout):
    ids, keys, nsize, stride = K.crowded_store(layout)
    a, b = K.crowd_keys()
    ref = K.ref_register(keys, nsize, stride)
    assert np.isin(np.r_[a, b], ref["keys"]).all() and len(nsize) == 40
    first = ref["f"][np.isin(ref["keys"], np.r_[a, b].astype(np.uint64))]
    assert (first < K.MIN_ROWS).all()                           # all 80 meet in the dictionary of range 0
    assert (len(np.unique(first)) == 1) == (layout == "one_row")
    assert K.dict_leftover(ref["ukeys"]) >= 2 * K.CROWD - (K.PROBES + 1)
    assert np.isin(np.r_[a, b], keys.view(np.uint32).reshape(40, stride)[K.MIN_ROWS:]).any()   # and some again in range 1


@pytest.mark.parametrize("c,least", [(3000, 1), (3072, 1), (3073, 1), (4096, 100), (5000, 500)])
def test_many_keys_overflow_the_dictionary(c, least):
    (ids, keys, nsize, stride), fam = K.many_keys(c)
    ref = K.ref_register(keys, nsize, stride)
    assert len(ref["keys"]) == c == len(np.unique(fam)) and len(nsize) == K.MIN_ROWS and fam.max() < 2 ** 20
    assert len(ref["first_rows"]) == K.MIN_ROWS                 # every row is some key's first
    for order in (ref["ukeys"], ref["keys"], ref["keys"][::-1]):
        left = K.dict_leftover(order)
        print(f"{c} keys: {left} find no dictionary entry")
        assert left >= least


@pytest.mark.parametrize("kind", ["low", "high"])
def test_valued_stores(kind):
    ids, keys, nsize, stride = K.valued_store(kind)
    ref = K.ref_register(keys, nsize, stride)
    assert {0, 1, 2 ** 31 - 1} <= set(ref["keys"].tolist()) and ref["ukeys"][:3].tolist() == [2 ** 31 - 1, 0, 1]
    assert ((ref["keys"] >= 2 ** 31).any()) == (kind == "high") and ref["keys"].max() < 2 ** 32 - 1
    if kind == "high":
        assert {2 ** 31, 2 ** 32 - 2} <= set(ref["keys"].tolist()) and (keys < 0).any()


@pytest.mark.parametrize("n", K.TRANSLATE_N)
def test_translate_data(n):
    fam = K.FAMILY
    d = K.translate_data(n, fam)
    assert len(d) == n and d.dtype == np.int32 and ((d == K.STRANGER).sum() == 2) == (n > 4) and K.STRANGER not in fam
    got = K.ref_translate(d, n, fam)
    assert ((got == 0) == (d == K.STRANGER)).all() and (n == 1 or got[0] == 1) and got[-1] == len(fam)


# ------------------------------------------------------------------------------------------------------------- what the entry points refuse
@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_keyrows_entry_points_refuse_before_launching(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)               # any non-null pointer: nothing is read through it before the refusal
    assert [L.subgacc_keyrows_cand_capacity(n) for n in (-5, 0, 1, 4096)] == [16, 16, 17, 4112]

    def reg(keys=here, nsize=here, n=4, stride=8, root_base=0, table=here, cap=1024, cand=here, ccap=20, ncand=here, flags=here):
        return L.subgacc_keyrows_register(keys, nsize, n, stride, root_base, table, cap, cand, ccap, ncand, flags, None)

    def cmp(ids=here, keys=here, nsize=here, off=here, n=4, stride=8, root_base=0, table=here, cap=1024, ukeys=None, nuk=None, mu=0,
            oi=here, od=here, cand=here, ccap=20, ncand=here, flags=here):
        return L.subgacc_keyrows_compact(ids, keys, nsize, off, n, stride, root_base, table, cap, ukeys, nuk, mu, oi, od, cand, ccap,
                                         ncand, flags, None)

    def look(**kw):
        return cmp(**{**dict(ukeys=here, nuk=here, mu=8, cand=None, ccap=0, ncand=None), **kw})

    def tr(data=here, n=4, n_dev=None, table=here, cap=1024, ukeys=here, nuk=here, mu=8):
        return L.subgacc_keyrows_translate(data, n, n_dev, table, cap, ukeys, nuk, mu, None)

    ok = [
        lambda: reg(keys=None, nsize=None, n=0, cand=None, ccap=0, ncand=None, flags=None),
        lambda: cmp(ids=None, keys=None, nsize=None, off=None, n=0, oi=None, od=None, cand=None, ccap=0, ncand=None, flags=None),
        lambda: look(ids=None, keys=None, nsize=None, off=None, n=0, oi=None, od=None, flags=None),
        lambda: tr(data=None, n=0),
    ]
    for i, call in enumerate(ok):
        assert call() == 0, (i, L.subgacc_last_error())
    bad = [
        (lambda: reg(n=-1), b"bad sizes"),
        (lambda: reg(stride=0), b"bad sizes"),
        (lambda: reg(stride=-8), b"bad sizes"),
        (lambda: reg(root_base=-1), b"bad sizes"),
        (lambda: reg(cap=1000), b"power-of-two table"),
        (lambda: reg(cap=0), b"power-of-two table"),
        (lambda: reg(cap=1 << 31), b"power-of-two table"),
        (lambda: reg(table=None), b"power-of-two table"),
        (lambda: reg(n=0, cap=1000), b"power-of-two table"),
        (lambda: reg(keys=None), b"null argument"),
        (lambda: reg(nsize=None), b"null argument"),
        (lambda: reg(flags=None), b"null argument"),
        (lambda: reg(cand=None), b"list their candidates"),
        (lambda: reg(ncand=None), b"list their candidates"),
        (lambda: reg(ccap=19), b"list their candidates"),
        (lambda: reg(n=4096, ccap=4096), b"list their candidates"),
        (lambda: cmp(n=-1), b"bad sizes"),
        (lambda: cmp(cap=48), b"power-of-two table"),
        (lambda: cmp(ccap=19), b"list their candidates"),
        (lambda: cmp(cand=None), b"list their candidates"),
        (lambda: cmp(ids=None), b"copying forms"),
        (lambda: cmp(off=None), b"copying forms"),
        (lambda: cmp(oi=None), b"copying forms"),
        (lambda: cmp(od=None), b"copying forms"),
        (lambda: cmp(keys=None), b"null argument"),
        (lambda: look(nuk=None), b"look-up form"),
        (lambda: look(mu=-1), b"look-up form"),
        (lambda: look(ids=None), b"copying forms"),
        (lambda: look(od=None), b"copying forms"),
        (lambda: look(stride=0), b"bad sizes"),
        (lambda: look(flags=None), b"null argument"),
        (lambda: tr(n=-1), b"keyrows_translate: bad arguments"),
        (lambda: tr(table=None), b"keyrows_translate: bad arguments"),
        (lambda: tr(cap=1000), b"keyrows_translate: bad arguments"),
        (lambda: tr(ukeys=None), b"keyrows_translate: bad arguments"),
        (lambda: tr(nuk=None), b"keyrows_translate: bad arguments"),
        (lambda: tr(mu=-1), b"keyrows_translate: bad arguments"),
        (lambda: tr(n=0, ukeys=None), b"keyrows_translate: bad arguments"),
        (lambda: tr(data=None), b"null payload"),
    ]
    for i, (call, text) in enumerate(bad):
        rc = call()
        assert rc == _lib.ERR_BADARG and text in L.subgacc_last_error(), (i, rc, L.subgacc_last_error())

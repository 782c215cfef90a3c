"""GPU (MI355X): csrc/keyrows.hip through its four C entry points, on synthetic key rows built to stand at its limits (inputs and
references: tests/keyrows_edges.py, shown to be what they claim by tests/test_keyrows_edges_cpu.py).  No graph, no walk.

The pipeline, as sampler.py runs it: subgacc_uniq_reset; subgacc_keyrows_register (or, a job of several chunks,
subgacc_keyrows_compact without ukeys, which registers and copies with the key as payload); a stand-in for subgacc_walk_tags -- exact
tags for the rows listed in `cand` ONLY, through subgacc_uniq_insert over the chunk's slots, every slot that is not a live member of a
listed row holding the key of the store's very first member, whose tag no later slot can lower --; subgacc_uniq_number from the
table alone; then subgacc_keyrows_compact with the numbered keys, or subgacc_keyrows_translate over the packed keys.  Because only the
listed rows get exact tags, a first row that `cand` misses spoils the numbering.

Cases: row counts around the eight waves and the 32 rows of a block range, with empty rows at every end; row lengths around the load
group of 512 and nsize > stride; 33 and 64 rows per block (a short last block, bits that straddle a bitmap word); the full range of
4,096 rows per block; 40 keys of one dictionary home against 32 probes, with a second family on the next home; more distinct keys
in a range than the dictionary has entries; 3,072 / 3,073 / 5,000 numbered keys against the preload cap and max_ukeys below the
count; the keys 0, 1, 2^31 - 1 and keys with bit 31 set; tags beyond 2^32 and chunks in the wrong order; an HBM table that is too
small; the translate pass around its 16-byte step and its 16,384-entry block, at every alignment, under a device-side count.

Rules of this file.  Every output lies between two poisoned rims that must come back untouched.  Every comparison is bit for bit.
Every case runs twice, reset included, and must give the same bits -- but for the order of `cand` and its superfluous members.

Pinned behaviour that the code, not the reference, defines:
  * 0xFFFFFFFF marks an empty dictionary entry and is NOT a key (key rows need num_steps*SHIFT + 1 <= 31 bits); it is never fed here.
  * a key with bit 31 set is zero-extended everywhere (table, ukeys, dictionary) and round-trips; as a payload it is a negative int32.
  * `cand` is compared as a set: a superset of the first rows, each row once; which other rows it lists is the order of arrival.
  * a key that is in no table translates to 0.
  * after flags[2] |= 1 (more distinct keys than the HBM table holds) the contents are void; only flags and rims are checked."""
import ctypes as C

import numpy as np
import pytest
import torch

import keyrows_edges as K
from test_gpu_uniq_edges import FLAGS0, POISON, Rimmed, _dev, _same, _table

pytestmark = pytest.mark.gpu

EMPTY64 = np.uint64(0xFFFFFFFFFFFFFFFF)
RANK_LIMIT = 16384                          # the small_limit of the sampler's table-only ranking
NULL = C.c_void_p(0)


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


def _at(t, elements):
    return C.c_void_p(t.data_ptr() + elements * t.element_size())


_REFS = {}


def _ref(name, store):
    """the reference of a named store, computed once and left unchanged"""
    if name not in _REFS:
        ids, keys, nsize, stride = store
        _REFS[name] = (K.ref_register(keys, nsize, stride), K.range_census(keys, nsize, stride))
    return _REFS[name]


# ------------------------------------------------------------------------------------------------------------- the pipeline
def _run(store, ref, mode, cap=1024, root_base=0, chunks=None, max_unique=None, n_dev=None):
    """mode: "register" (register, stand-in, number), "lookup" (... and compact with ukeys), "copy" (per chunk: compact without
    ukeys, stand-in; number; translate).  chunks: (lo, hi) row ranges in the order given, each registered with root_base + lo."""
    lib, st = _L().lib(), _L().stream_ptr()
    ids, keys, nsize, stride = store
    n = len(nsize)
    chunks = [(0, n)] if chunks is None else chunks
    c = len(ref["keys"])
    mu = c + 8 if max_unique is None else max_unique
    d_keys, d_ns = _dev(keys), _dev(nsize)
    off = K.row_offsets(nsize, stride)
    total = int(off[-1])
    table = Rimmed(lib.subgacc_uniq_table_bytes(cap), torch.uint8)
    flags = Rimmed(4, torch.int32, np.array(FLAGS0, dtype=np.int32))
    res = {"rcs": [lib.subgacc_uniq_reset(table.ptr(), cap, st)], "cap": cap, "chunks": []}
    if mode != "register":
        d_ids, d_off = _dev(ids), _dev(off)
        out_i, out_d = Rimmed(total, torch.int32), Rimmed(total, torch.int32)
    g0 = ref["first_slot"]
    filler = int(np.asarray(keys).view(np.uint32)[g0]) if g0 >= 0 else 0
    for lo, hi in chunks:
        cn = hi - lo
        ccap = lib.subgacc_keyrows_cand_capacity(cn)
        assert ccap >= cn
        cand, ncand = Rimmed(ccap, torch.int32), Rimmed(1, torch.int64, np.zeros(1, np.int64))
        if mode == "copy":
            rc = lib.subgacc_keyrows_compact(_at(d_ids, lo * stride), _at(d_keys, lo * stride), _at(d_ns, lo), _at(d_off, lo), cn, stride,
                                             root_base + lo, table.ptr(), cap, NULL, NULL, 0, out_i.ptr(), out_d.ptr(), cand.ptr(), ccap,
                                             ncand.ptr(), flags.ptr(), st)
        else:
            rc = lib.subgacc_keyrows_register(_at(d_keys, lo * stride), _at(d_ns, lo), cn, stride, root_base + lo, table.ptr(), cap,
                                              cand.ptr(), ccap, ncand.ptr(), flags.ptr(), st)
        res["rcs"].append(rc)
        nc, listed = int(ncand.host()[0]), cand.host()
        if len(chunks) == 1:
            res["table_reg"] = table.host()
        # ---- cand: checked here, before anything is built from it
        assert 0 <= nc <= cn, f"*n_cand = {nc} for {cn} rows"
        assert (listed[nc:] == POISON[torch.int32]).all(), "cand was written beyond *n_cand"
        listed = listed[:nc]
        assert ((listed >= 0) & (listed < cn)).all(), "cand names a row outside [0, n)"
        assert len(np.unique(listed)) == nc, "cand names a row twice"
        res["chunks"].append((lo, hi, np.sort(listed)))
        # ---- the stand-in for subgacc_walk_tags: exact tags tag_base + e for the listed rows only
        e0 = max(0, g0 - lo * stride)       # no slot in front of the store's first member: there the filler's tag would be too low
        if g0 >= 0 and e0 < cn * stride:
            d_a = _dev(K.standin_keys(keys, nsize, stride, lo, hi, listed, filler)[e0:])
            res["rcs"].append(lib.subgacc_uniq_insert(table.ptr(), cap, C.c_void_p(d_a.data_ptr()), cn * stride - e0,
                                                      (root_base + lo) * stride + e0, NULL, flags.ptr(), st))
            torch.cuda.synchronize()
    ukeys, count = Rimmed(mu, torch.int64), Rimmed(1, torch.int64)
    ws = Rimmed(lib.subgacc_uniq_number_workspace_bytes(cap, 0), torch.uint8)
    res["rcs"].append(lib.subgacc_uniq_number(table.ptr(), cap, NULL, 0, ukeys.ptr() if mu else NULL, mu, count.ptr(), RANK_LIMIT, ws.ptr(),
                                              ws.n, st))
    if mode == "lookup":
        ccap = lib.subgacc_keyrows_cand_capacity(n)
        cand, ncand = Rimmed(ccap, torch.int32), Rimmed(1, torch.int64, np.zeros(1, np.int64))
        res["table_num"] = table.host()
        res["rcs"].append(lib.subgacc_keyrows_compact(C.c_void_p(d_ids.data_ptr()), C.c_void_p(d_keys.data_ptr()), C.c_void_p(d_ns.data_ptr()),
                                                      C.c_void_p(d_off.data_ptr()), n, stride, root_base, table.ptr(), cap, ukeys.ptr(),
                                                      count.ptr(), mu, out_i.ptr(), out_d.ptr(), cand.ptr(), ccap, ncand.ptr(), flags.ptr(),
                                                      st))
        assert ncand.host()[0] == 0 and (cand.host() == POISON[torch.int32]).all(), "the look-up form lists no candidates"
        assert np.array_equal(table.host(), res["table_num"]), "the look-up form only reads the table"
    elif mode == "copy":
        d_n = None if n_dev is None else _dev(np.array([n_dev], dtype=np.int64))
        res["out_d_keys"] = out_d.host()
        res["rcs"].append(lib.subgacc_keyrows_translate(out_d.ptr(), total, C.c_void_p(d_n.data_ptr()) if d_n is not None else NULL,
                                                        table.ptr(), cap, ukeys.ptr(), count.ptr(), mu, st))
    ws.host()
    res.update(table=table.host(), flags=flags.host(), ukeys=ukeys.host().view(np.uint64), count=int(count.host()[0]), mu=mu)
    if mode != "register":
        res.update(out_i=out_i.host(), out_d=out_d.host())
    return res


def _check_table(raw, cap, ref, tags, numbered):
    tk, tt, tid = _table(raw, cap)
    occ = tk != EMPTY64
    assert occ.sum() == len(ref["keys"]), "the occupied slots are the distinct keys, each once"
    order = np.argsort(tk[occ])
    assert np.array_equal(tk[occ][order], ref["keys"])
    assert np.array_equal(tt[occ][order], ref[tags]), f"mintag is not the {tags} tag"
    assert (tt[~occ] == EMPTY64).all() and (tid[~occ] == -1).all()
    if numbered:
        assert np.array_equal(tid[occ][order], ref["number"]), "id is not the rank of the exact tag"
    else:
        assert (tid == -1).all()


def _check(res, store, ref, census, mode, root_base=0, n_dev=None):
    ids, keys, nsize, stride = store
    c = len(ref["keys"])
    if root_base:
        ref = dict(ref, coarse=ref["coarse"] + np.uint64(root_base * stride), exact=ref["exact"] + np.uint64(root_base * stride))
    assert all(rc == 0 for rc in res["rcs"]), res["rcs"]
    assert res["flags"].tolist() == FLAGS0, "flags[0], [1], [3] are not this pass's, flags[2] = 0: every key found a slot"
    if "table_reg" in res:                  # one chunk: the table as the registering pass left it
        _check_table(res["table_reg"], res["cap"], ref, "coarse", False)
    for lo, hi, listed in res["chunks"]:
        first = ref["first_rows"][(ref["first_rows"] >= lo) & (ref["first_rows"] < hi)] - lo
        missing = np.setdiff1d(first, listed)
        assert len(missing) == 0, f"cand misses the first rows {missing[:8] + lo} of chunk {lo}..{hi}"
    if len(res["chunks"]) == 1 and census[0] <= K.PROBES:
        # at most kKrProbes distinct keys in every block range: nothing is crowded, a range lists at most one row per dictionary entry
        nc = len(res["chunks"][0][2])
        print(f"n_cand = {nc}, first rows = {len(ref['first_rows'])}, sum of distinct keys over the ranges = {census[1]}, n = {len(nsize)}")
        assert nc <= census[1], "more candidates than dictionary entries were flushed"
    assert res["count"] == c
    w = min(c, res["mu"])
    assert np.array_equal(res["ukeys"][:w], ref["ukeys"][:w]), "the numbering is not the order of first appearance"
    assert (res["ukeys"][w:] == np.uint64(POISON[torch.int64])).all()
    _check_table(res["table"], res["cap"], ref, "exact", True)
    if mode == "register":
        return
    off = K.row_offsets(nsize, stride)
    want_i, want_keys = K.ref_compact(ids, keys, nsize, stride, off)
    assert np.array_equal(res["out_i"], want_i)
    if mode == "lookup":
        assert np.array_equal(res["out_d"], K.ref_compact(ids, keys, nsize, stride, off, ref["ukeys"])[1])
    else:
        assert np.array_equal(res["out_d_keys"], want_keys), "register-and-copy keeps the key as payload"
        n_eff = len(want_keys) if n_dev is None else n_dev
        assert np.array_equal(res["out_d"], K.ref_translate(want_keys, n_eff, ref["ukeys"]))


SAME = {"register": ("ukeys", "count", "flags"), "lookup": ("ukeys", "count", "flags", "out_i", "out_d"),
        "copy": ("ukeys", "count", "flags", "out_i", "out_d", "out_d_keys")}


def _twice(name, store, mode, **kw):
    ref, census = _ref(name, store)
    a, b = _run(store, ref, mode, **kw), _run(store, ref, mode, **kw)
    _same(a, b, SAME[mode])
    _check(a, store, ref, census, mode, root_base=kw.get("root_base", 0), n_dev=kw.get("n_dev"))
    return a


MODES = ["register", "lookup", "copy"]


# ------------------------------------------------------------------------------------------------------------- ranges, waves, row lengths
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", K.SMALL_N)
def test_row_counts_around_the_waves_and_the_range(n, mode):
    _twice(f"small{n}", K.small_store(n), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 9, 33])
def test_a_store_of_empty_rows(n, mode):
    store = K.small_store(n, "empty")
    res = _twice(f"empty{n}", store, mode)
    assert res["count"] == 0 and len(res["chunks"][0][2]) == 0
    if mode != "register":
        assert len(res["out_i"]) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns", K.LONG_NS)
def test_row_lengths_around_the_load_group(ns, mode):
    _twice(f"long{ns}", K.long_rows(ns), mode, n_dev=None if ns != K.GROUP else 3 * K.GROUP)


# ------------------------------------------------------------------------------------------------------------- more than 32 rows per block
@pytest.mark.parametrize("mode", ["register", "copy"])
@pytest.mark.parametrize("rpb", [33, 64])
def test_rows_per_block_above_the_minimum(rpb, mode):
    ids, keys, nsize, stride, planted = K.wide_store(rpb)
    res = _twice(f"wide{rpb}", (ids, keys, nsize, stride), mode)
    assert np.isin(planted, res["chunks"][0][2]).all()


def test_the_full_range_of_4096_rows_per_block():
    """the only shape that reaches kKrMaxRows: 4,096 x 4,096 rows at stride 1, register only (wall time: see the printed figure)"""
    import time
    t0 = time.time()
    keys, nsize, stride, planted = K.full_store()
    res = _twice("full", (None, keys, nsize, stride), "register")
    assert np.isin(planted, res["chunks"][0][2]).all()
    print(f"full range: {time.time() - t0:.1f} s for two runs, input and reference included")


# ------------------------------------------------------------------------------------------------------------- crowded dictionaries
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["one_row", "spread"])
def test_forty_keys_of_one_home_and_forty_of_the_next(layout, mode):
    _twice("crowd_" + layout, K.crowded_store(layout), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", [K.DICT, 5000])
def test_more_distinct_keys_in_a_range_than_dictionary_entries(c, mode):
    _twice(f"many{c}", K.many_keys(c)[0], mode, cap=16384)


@pytest.mark.parametrize("mode", ["lookup", "copy"])
@pytest.mark.parametrize("c", [K.DICT_MAX, K.DICT_MAX + 1])
def test_numbered_keys_around_the_preload_cap(c, mode):
    _twice(f"many{c}", K.many_keys(c)[0], mode, cap=16384)


@pytest.mark.parametrize("mode", ["lookup", "copy"])
def test_max_ukeys_below_the_count(mode):
    """100 of 3,000 numbered keys reach the caller: the others are known to the HBM table alone"""
    res = _twice("many3000", K.many_keys(3000)[0], mode, cap=8192, max_unique=100)
    assert res["count"] == 3000 and res["mu"] == 100


# ------------------------------------------------------------------------------------------------------------- key values, root_base, chunks
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["low", "high"])
def test_the_ends_of_the_key_range(kind, mode):
    res = _twice("valued_" + kind, K.valued_store(kind), mode)
    if kind == "high":
        assert {2 ** 31, 2 ** 32 - 2} <= set(res["ukeys"][:res["count"]].tolist()), "a key with bit 31 set is zero-extended"
        if mode == "copy":
            assert (res["out_d_keys"] < 0).any() and (res["out_d"] > 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_tags_beyond_32_bits(mode):
    for name, store in (("small65", K.small_store(65)), ("long513", K.long_rows(K.GROUP + 1)), ("crowd_spread", K.crowded_store("spread"))):
        base = 2 ** 33 // store[3]
        assert base * store[3] >= 2 ** 32
        _twice(name, store, mode, root_base=base)


@pytest.mark.parametrize("mode", MODES)
def test_chunks_in_the_wrong_order(mode):
    for name, store, cut in (("small65", K.small_store(65), 3), ("crowd_spread", K.crowded_store("spread"), 7),
                             ("valued_high", K.valued_store("high"), 2), ("long513", K.long_rows(K.GROUP + 1), 2)):
        n = len(store[2])
        ref = _ref(name, store)[0]
        assert ((ref["f"] < cut).any() and (ref["f"] >= cut).any())
        _twice(name, store, mode, chunks=[(cut, n), (0, cut)])
        _twice(name, store, mode, chunks=[(cut, n), (0, cut)], root_base=2 ** 33 // store[3])


# ------------------------------------------------------------------------------------------------------------- an HBM table too small
@pytest.mark.parametrize("mode", MODES)
def test_hbm_table_too_small(mode):
    """300 distinct keys for 256 slots: flags[2] |= 1, every call returns, nothing outside the outputs is written (the rims are
    checked when an output is read back); the contents are void and are not compared"""
    store = K.many_keys(300)[0]
    ref = _ref("many300", store)[0]
    res = _run(store, ref, mode, cap=256)
    assert all(rc == 0 for rc in res["rcs"]), res["rcs"]
    assert res["flags"].tolist() == [FLAGS0[0], FLAGS0[1], 1, FLAGS0[3]]
    assert res["count"] <= 256


# ------------------------------------------------------------------------------------------------------------- translate
def _numbered_table(fam, cap, mu):
    """a table that holds `fam`, numbered in the order given"""
    lib, st = _L().lib(), _L().stream_ptr()
    fam64 = np.asarray(fam, dtype=np.uint32).astype(np.uint64)
    table = Rimmed(lib.subgacc_uniq_table_bytes(cap), torch.uint8)
    flags = Rimmed(4, torch.int32, np.array(FLAGS0, dtype=np.int32))
    ukeys, count = Rimmed(mu, torch.int64), Rimmed(1, torch.int64)
    ws = Rimmed(lib.subgacc_uniq_number_workspace_bytes(cap, 0), torch.uint8)
    d_f = _dev(fam64)
    rcs = [lib.subgacc_uniq_reset(table.ptr(), cap, st),
           lib.subgacc_uniq_insert(table.ptr(), cap, C.c_void_p(d_f.data_ptr()), len(fam64), 0, NULL, flags.ptr(), st),
           lib.subgacc_uniq_number(table.ptr(), cap, NULL, 0, ukeys.ptr(), mu, count.ptr(), RANK_LIMIT, ws.ptr(), ws.n, st)]
    assert rcs == [0, 0, 0] and flags.host().tolist() == FLAGS0 and count.host()[0] == len(fam64)
    assert np.array_equal(ukeys.host().view(np.uint64)[:min(mu, len(fam64))], fam64[:mu])
    return table, ukeys, count


def _translate(tab, cap, mu, fam, data, shift, n_dev):
    """`data` stands `shift` words behind a 16-byte boundary, in a buffer 8 words longer than it: what lies around it must stay"""
    lib, st = _L().lib(), _L().stream_ptr()
    table, ukeys, count = tab
    n = len(data)
    whole = np.full(n + 8, POISON[torch.int32], dtype=np.int32)
    whole[shift:shift + n] = data
    buf = Rimmed(n + 8, torch.int32, whole)
    assert buf.t.data_ptr() % 16 == 0
    before = table.host()
    d_n = None if n_dev is None else _dev(np.array([n_dev], dtype=np.int64))
    rc = lib.subgacc_keyrows_translate(buf.ptr(shift), n, C.c_void_p(d_n.data_ptr()) if d_n is not None else NULL, table.ptr(), cap,
                                       ukeys.ptr(), count.ptr(), mu, st)
    assert rc == 0
    got = buf.host()
    assert np.array_equal(table.host(), before), "translate only reads the table"
    want = whole.copy()
    want[shift:shift + n] = K.ref_translate(data, n if n_dev is None else n_dev, np.asarray(fam, dtype=np.uint32).astype(np.uint64))
    assert np.array_equal(got, want), f"n = {n}, {shift} words behind a 16-byte boundary, n_dev = {n_dev}"
    return got


TRANSLATE_TABLES = {"dictionary": (lambda: K.FAMILY, 64, 64),                           # every key is preloaded
                    "beyond_the_cap": (lambda: K.many_keys(5000)[1], 16384, 5008),      # 1,928 keys and more are asked from HBM
                    "max_ukeys": (lambda: K.many_keys(3000)[1], 8192, 100)}             # 2,900 keys never reach the dictionary


@pytest.mark.parametrize("n", K.TRANSLATE_N)
@pytest.mark.parametrize("which", list(TRANSLATE_TABLES))
def test_translate_sizes_alignments_and_counts(which, n):
    make, cap, mu = TRANSLATE_TABLES[which]
    fam = make()
    tab = _numbered_table(fam, cap, mu)
    data = K.translate_data(n, fam)
    for shift in (0, 1, 2, 3):
        for n_dev in ((None, 0, n - 1, n, n + 7) if which == "dictionary" or shift == 1 else (None,)):
            a = _translate(tab, cap, mu, fam, data, shift, n_dev)
            b = _translate(tab, cap, mu, fam, data, shift, n_dev)
            assert np.array_equal(a, b)

"""CPU: the inputs of tests/test_gpu_uniq_edges.py are what they claim to be (tests/uniq_edges.py).  Every key family has the homes,
the sizes and the distinctness it is named for and none holds kEmptyKey; chains that start in the last slot run on at slot 0; the
crowded LDS home sends at least 24 of its 40 keys straight to HBM in any arrival order; ref_uniq equals a loop over a dict and the
(sf, enc) of oracle.gset_sampler; ref_dedup and ref_dedup_roles equal plain loops."""
import numpy as np
import pytest

import uniq_edges as E
from oracle import oracle as orc


def _loop_uniq(keys):
    seen, sf = {}, []
    for k in keys.tolist():
        sf.append(seen.setdefault(k, len(seen)))
    return np.array(sf, dtype=np.int32), np.array(list(seen), dtype=np.uint64)


def test_mix64_is_the_finaliser_it_restates():
    # MurmurHash3's fmix64 on values worked out by hand-free means: plain Python integers
    def fmix(x):
        x ^= x >> 33
        x = x * 0xFF51AFD7ED558CCD % 2 ** 64
        x ^= x >> 33
        x = x * 0xC4CEB9FE1A85EC53 % 2 ** 64
        return x ^ x >> 33
    ks = [0, 1, 2, 12345, 2 ** 63, 2 ** 64 - 2, 0x0123456789ABCDEF]
    assert E.mix64(ks).tolist() == [fmix(k) for k in ks]
    assert E.hbm_home(ks, 256).tolist() == [fmix(k) & 255 for k in ks]
    assert E.lds_home(ks).tolist() == [(fmix(k) >> 40) & 1023 for k in ks]
    ids = [0, 1, 77, 2 ** 31 - 1, -1]
    assert E.root_home(ids, 1024).tolist() == [((i % 2 ** 32) * 2654435761 % 2 ** 32) >> 22 for i in ids]
    assert [E.dedup_slots(n) for n in (0, 2, 512, 513, 1024, 1025, 2000)] == [1024, 1024, 1024, 2048, 2048, 4096, 4096]


def test_family_sizes():
    keys, mix = E._pool()
    hb = np.bincount(E.hbm_home(keys, 256), minlength=256)
    ld = np.bincount(E.lds_home(keys), minlength=1024)
    rt = np.bincount(E.root_home(keys.astype(np.int64), 1024), minlength=1024)
    print(f"keys below 2^20 per HBM home of 256: {hb.min()} .. {hb.max()}; per LDS home: {ld.min()} .. {ld.max()}; "
          f"ids per home of a 1,024-slot prologue table: {rt.min()} .. {rt.max()}, home 1023: {rt[1023]}")
    assert hb.min() >= 3934 and ld.min() >= 924 and rt[1023] == 1023


@pytest.mark.parametrize("cap,home,k", [(256, 3, 128), (256, 3, 129), (256, 255, 128), (256, 255, 129)])
def test_hbm_chain_families(cap, home, k):
    keys = E.same_hbm_home(k, cap, home)
    assert len(np.unique(keys)) == k and (E.hbm_home(keys, cap) == home).all() and not (keys == E.EMPTY_KEY).any()
    taken, longest = E.chain_end(E.hbm_home(keys, cap), cap)
    assert longest == k                                        # the k-th key probes k slots: 128 is accepted, 129 is not
    assert (k <= E.MAX_PROBES) == (k == 128)
    if home == cap - 1:
        assert taken[0] and taken[cap - 1] and k > 1            # the chain is longer than the last slot: it wraps to slot 0
    spread = E.chain_keys(k, cap, home, spread=True)
    assert set(spread.tolist()) == set(keys.tolist()) and len(spread) > 2 * E.INS_TILE       # several tiles, repeated, nothing else
    for t in range(3):
        assert len(np.unique(spread[t * E.INS_TILE:(t + 1) * E.INS_TILE])) > 1


@pytest.mark.parametrize("split", [False, True])
def test_lds_crowd(split):
    keys, crowd = E.lds_crowd(split)
    assert len(np.unique(crowd)) == 40 and (E.lds_home(crowd) == 517).all()
    assert len(np.unique(E.hbm_home(crowd, 4096))) == 40        # no chain in the HBM table: the LDS window alone is on trial
    assert not (keys == E.EMPTY_KEY).any()
    # one home, a window of 16 slots: at most 16 of the 40 find room in the fold table of a tile, in ANY arrival order
    assert 40 - E.LDS_WINDOW >= 24
    tiles = [keys[i:i + E.INS_TILE] for i in range(0, len(keys), E.INS_TILE)]
    assert len(tiles) == (2 if split else 1)
    for t in tiles:
        assert np.isin(crowd, t).all()
    if split:
        assert np.isin(keys[E.INS_TILE - 40:E.INS_TILE], crowd).all() and np.isin(keys[E.INS_TILE:E.INS_TILE + 40], crowd).all()
    else:
        for k in crowd:
            assert (keys == k).sum() == 2
        assert len(keys) == 380


def test_sized_keys():
    for n in E.INSERT_SIZES:
        for kind in E.KEY_SETS:
            keys = E.sized_keys(n, kind)
            assert keys.dtype == np.uint64 and len(keys) == n and not (keys == E.EMPTY_KEY).any()
            c = len(np.unique(keys))
            assert c == {"equal": min(n, 1), "distinct": n, "of37": min(c, 37)}[kind]
            if kind == "of37" and n >= 1023:
                assert c == 37 and 0 in keys and np.uint64(2 ** 64 - 2) in keys


@pytest.mark.parametrize("positions,n", [((0, 5, 1023, 1024, 1500, 2047, 2048, 2049, 4195), 4196), ((0,), 1), ((0, 1), 2)])
def test_first_at(positions, n):
    keys = E.first_at(positions, n)
    sf, ukeys, first = E.ref_uniq(keys)
    assert first.tolist() == list(positions)
    if n > 4096:
        assert not ((first >= 3 * E.UNIQ_TILE) & (first < 4 * E.UNIQ_TILE)).any()       # one whole scan tile without a first occurrence


@pytest.mark.parametrize("c", [1, 255, 256, 257, 600])
def test_repeated(c):
    keys = E.repeated(c, 2 * c + 3)
    assert len(keys) == 2 * c + 3 and len(np.unique(keys)) == c and not (keys == E.EMPTY_KEY).any()


def test_ref_uniq_against_a_dict():
    rng = np.random.default_rng(5)
    cases = [rng.integers(0, 50, size=1000, dtype=np.uint64), rng.integers(0, 2 ** 63, size=777, dtype=np.uint64) * np.uint64(2),
             np.array([2 ** 64 - 2, 0, 2 ** 64 - 2, 0, 5], dtype=np.uint64), np.zeros(0, np.uint64),
             E.lds_crowd(True)[0], E.chain_keys(129, 256, 255, True), E.first_at((0, 1023, 1024, 2047, 2048, 2999), 3000)]
    cases += [E.sized_keys(n, kind) for n in (1, 257, 2049) for kind in E.KEY_SETS]
    for keys in cases:
        sf, ukeys, first = E.ref_uniq(keys)
        lsf, lukeys = _loop_uniq(keys)
        assert np.array_equal(sf, lsf) and np.array_equal(ukeys, lukeys)
        assert np.array_equal(keys[first], ukeys) and (np.diff(first) > 0).all()
        assert sf.dtype == np.int32 and ukeys.dtype == np.uint64


def test_ref_uniq_and_ref_unpack_against_the_oracle_sampler():
    rng = np.random.default_rng(3)
    N, M, m = 300, 20, 3
    src, dst = rng.integers(0, N, size=1500), rng.integers(0, N, size=1500)
    keep = src != dst
    src, dst = np.r_[src[keep], dst[keep]], np.r_[dst[keep], src[keep]]
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    indptr = np.r_[0, np.cumsum(np.bincount(src, minlength=N))].astype(np.int64)
    for name in ("rand_r", "philox"):
        nsize, remap, enc, raw = orc.gset_sampler(indptr, dst.astype(np.int32), np.arange(N), num_walks=M, num_steps=m, rng=name,
                                                  debug=True)
        keys = E.pack_rows(raw, M, m)
        sf, ukeys, first = E.ref_uniq(keys)
        print(f"{name}: {len(keys)} members, {len(ukeys)} distinct LP rows")
        assert len(ukeys) > 50
        assert np.array_equal(E.ref_unpack(keys, M, m), raw.astype(np.int64))
        assert np.array_equal(sf, remap[1])
        assert np.array_equal(E.ref_unpack(ukeys, M, m), enc.astype(np.int64))


@pytest.mark.parametrize("M,m,bits,ok", [(1, 1, 2, True), (255, 7, 57, True), (256, 7, 64, True), (126, 9, 64, True), (200, 3, 25, True),
                                         (32767, 4, 61, True), (127, 9, 64, False), (200, 8, 65, False)])
def test_unpack_cases(M, m, bits, ok):
    shift = E.key_shift(M)
    assert m * shift + 1 == bits
    assert ok == (bits <= 64 and not (bits == 64 and M == (1 << shift) - 1))       # subgacc_key_shift's two refusals
    if not ok:
        return
    rng = np.random.default_rng(M)
    for lead in (0, 1, None):
        keys = E.random_keys(rng, 257, M, m, lead)
        rows = E.ref_unpack(keys, M, m)
        assert np.array_equal(E.pack_rows(rows, M, m), keys)
        assert set(np.unique(rows[:, 0]).tolist()) <= {0, M} and (lead is None or (rows[:, 0] == lead * M).all())
        assert rows[:, 1:].max() < (1 << shift) and rows.max() <= 32767            # the int16 output holds every field
        if bits == 64 and lead:
            assert (keys >> np.uint64(63)).all()                                     # key bit 63 is in use
        f = E.ref_unpack_f32(keys, M, m)
        assert f.dtype == np.float32 and np.array_equal(f, rows.astype(np.float32) / np.float32(M))


def _loop_first(edge):
    seen, row = {}, []
    for j, v in enumerate(np.asarray(edge).tolist()):
        v = -1 if (v < 0 or v > 2 ** 31 - 1) else v
        row.append(seen.setdefault(v, j))
    return row, seen


def _batches():
    out = [E.pair_batch(B, kind) for B in (1, 127, 128, 129, 1000) for kind in ("one", "distinct", "random", "self", "ends", "outside")]
    return out + [E.colliding_batch(1024, 140)[0], E.colliding_batch(2048, 300)[0]]


def test_ref_dedup_against_a_loop():
    for edge in _batches():
        n = len(edge)
        roots, own, partner, zeroed, nd = E.ref_dedup(edge)
        row, seen = _loop_first(edge)
        assert own.tolist() == row and nd == len(seen)
        assert partner.tolist() == [row[(j + n // 2) % n] for j in range(n)]
        for j in range(n):
            first = row[j] == j
            want = (-1 if (edge[j] < 0 or edge[j] > 2 ** 31 - 1) else int(edge[j])) if first else E.NO_ROOT
            assert roots[j] == want and zeroed[j] == (not first)
        assert roots.dtype == np.int32 and own.dtype == np.int64 and partner.dtype == np.int64


def test_batches_are_what_they_are_named_for():
    for B in (1, 127, 128, 129, 1000):
        assert E.ref_dedup(E.pair_batch(B, "one"))[4] == 1
        assert E.ref_dedup(E.pair_batch(B, "distinct"))[4] == 2 * B
        e = E.pair_batch(B, "self")
        assert (e[:B:2] == e[B::2]).all()
        if B > 1:
            assert 1 < E.ref_dedup(E.pair_batch(B, "random"))[4] < 2 * B
        if B >= 127:
            e = E.pair_batch(B, "ends")
            assert (e == 0).sum() == 3 and (e == 2 ** 31 - 1).sum() == 3
            assert {0, 2 ** 31 - 1} <= set(E.ref_dedup(e)[0].tolist())
            e = E.pair_batch(B, "outside")
            assert {-1, -5, 2 ** 31, 2 ** 40} <= set(e.tolist())
            roots = E.ref_dedup(e)[0]
            assert (roots == -1).sum() == 1 and (E.narrow(e) == -1).sum() == 8
            assert np.flatnonzero(roots == -1)[0] == np.flatnonzero(E.narrow(e) == -1)[0]


@pytest.mark.parametrize("c,B", [(1024, 140), (2048, 300)])
def test_colliding_batch_wraps(c, B):
    edge, crowd = E.colliding_batch(c, B)
    assert len(edge) == 2 * B and E.dedup_slots(len(edge)) == c
    assert len(np.unique(crowd)) == 40 and (E.root_home(crowd, c) == c - 1).all() and crowd.max() < 2 ** 20
    for k in crowd:
        assert (edge == k).sum() >= 2
    taken, longest = E.chain_end(E.root_home(np.unique(edge), c), c)
    assert taken[c - 1] and taken[:39].all() and longest >= 40          # forty roots of the last slot: the chain runs on at slot 0


@pytest.mark.parametrize("B", [1, 85, 86, 341])
def test_ref_dedup_roles_against_a_loop(B):
    edge = E.triplet_batch(B)
    roots, own, zeroed, nd = E.ref_dedup_roles(edge, B, 3, 4)
    row, seen = _loop_first(edge)
    u, v, w = row[:B], row[B:2 * B], row[2 * B:]
    assert own.tolist() == u + w + v + w and nd == len(seen)
    assert [j for j in range(3 * B) if not zeroed[j]] == sorted(seen.values())
    if B > 1:
        assert edge[2 * B + B // 2] == edge[0] and own[B + B // 2] == 0           # u of triplet 0 is w of triplet B/2: walked once
    pairs = E.pair_batch(max(B, 2), "random")
    r2, own2, z2, nd2 = E.ref_dedup_roles(pairs, len(pairs) // 2, 2, 2)
    p = E.ref_dedup(pairs)
    assert np.array_equal(r2, p[0]) and np.array_equal(own2, p[1]) and np.array_equal(z2, p[3]) and nd2 == p[4]

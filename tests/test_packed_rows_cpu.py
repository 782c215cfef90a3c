"""CPU: the packed key row (include/subgacc_packed.h) -- its format round-trips, its eligibility predicate in C's and Python's
restatement, and the proof that the cases of tests/test_gpu_packed_rows.py reach the branches they are named for (the graphs and
hand-made rows of tests/packed_rows.py, the rows themselves from the oracle)."""
import itertools

import numpy as np
import pytest

import packed_rows as P
import walk_rows_edges as W


# ------------------------------------------------------------------------------------------------------------------ the format
@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("fb", [3, 4, 6])
def test_every_key_round_trips(m, fb):
    """counts in {0, 1, 2^fb - 2, 2^fb - 1, 2^fb, M} in every field, with and without the flag: small members carry their key in the
    code, the others -- and the code of all ones -- escape; pack then unpack gives every key back"""
    M = 100 if m == 4 else 200                      # (4 hops: 32-bit keys end at M = 127)
    cb = 1 + m * fb                                 # the narrowest word with this fb: the code of all ones exists
    for cb_ in (cb, cb + (m - 1)):                  # ... and the widest: it does not
        assert (cb_ - 1) // m == fb
        vals = [0, 1, (1 << fb) - 2, (1 << fb) - 1, 1 << fb, M]
        f = np.array([(flag,) + c for flag in (0, 1) for c in itertools.product(vals, repeat=m)], np.int64)
        keys = P.key_of(f, M, m)
        assert np.array_equal(P.fields(keys, M, m), f)
        code, esc = P.codes(keys, M, m, cb_, fb)
        big = (f[:, 1:] >= (1 << fb)).any(axis=1)
        ones = (f[:, 0] == 1) & (f[:, 1:] == (1 << fb) - 1).all(axis=1) & (cb_ == 1 + m * fb)
        assert np.array_equal(esc, big | ones) and ones.sum() == (1 if cb_ == cb else 0)
        assert (code[esc] == (1 << cb_) - 1).all() and (code[~esc] < (1 << cb_) - 1).all()
        cap = 1 << (32 - cb_)                            # ids a word of this cb holds: rows of that many members at most
        for at in range(0, len(keys), cap):
            k, e = keys[at: at + cap], esc[at: at + cap]
            ids = np.arange(len(k)) * (3 if 3 * len(k) < cap else 1) + (cap - 1 - (len(k) - 1) * (3 if 3 * len(k) < cap else 1))
            assert ids.min() >= 0 and ids.max() == cap - 1           # (the largest id of the width is among them)
            words, lst = P.pack_row(ids, k, M, m, cb_, fb)
            assert (np.diff(words.astype(np.int64)) > 0).all(), "the words ascend as unsigned numbers"
            assert np.array_equal(lst, k[e])
            got_ids, got_keys = P.unpack_row(words, lst, M, m, cb_, fb)
            assert np.array_equal(got_ids, ids) and np.array_equal(got_keys, k)
            # a list cut short: the escapes beyond it read as key 0, the others are untouched
            got_ids, got_keys = P.unpack_row(words, lst[:3], M, m, cb_, fb)
            want = k.copy()
            want[np.nonzero(e)[0][3:]] = 0
            assert np.array_equal(got_ids, ids) and np.array_equal(got_keys, want)


# ---------------------------------------------------------------------------------------------------------------- the predicate
def _c_format(num_nodes, M, m, idx64):
    import ctypes as C
    from surel_plus_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    cb, fb = C.c_int32(-1), C.c_int32(-1)
    rc = L.subgacc_packed_rows_format(C.c_int64(num_nodes), C.c_int32(M), C.c_int32(m), C.c_int32(int(idx64)), C.byref(cb), C.byref(fb))
    return rc, cb.value, fb.value


def test_eligibility_at_the_id_width_edges():
    """3 hops: 2^22 - 1 and 2^22 nodes have 22-bit ids (cb = 10, fb = 3: packed), 2^22 + 1 has 23 (fb = 2: not); the 2- and 4-hop
    equivalents of fb = 3 | 2; C (when the library is built), Python and the test's own restatement agree everywhere"""
    import os
    from surel_plus_amd import _lib, sampler
    cases = [(3, 200, (1 << 22) - 1, True, (10, 3)), (3, 200, 1 << 22, True, (10, 3)), (3, 200, (1 << 22) + 1, False, (9, 2)),
             # 2 hops: fb = (cb - 1) // 2 is 3 down to cb = 7 (2^25 nodes) and 2 at cb = 6
             (2, 256, 1 << 25, True, (7, 3)), (2, 256, (1 << 25) + 1, False, (6, 2)),
             # 4 hops: fb = 3 down to cb = 13 (2^19 nodes), 2 at cb = 12
             (4, 127, 1 << 19, True, (13, 3)), (4, 127, (1 << 19) + 1, False, (12, 2))]
    built = os.path.exists(_lib.LIB_PATH)
    for m, M, N, want, cf in cases:
        assert P.fmt(N, m) == cf
        assert P.eligible(N, M, m) == want, (m, M, N)
        assert (sampler.packed_rows_form(N, M, m) is not None) == want and (not want or sampler.packed_rows_form(N, M, m) == cf)
        if built:
            assert _c_format(N, M, m, False) == (int(want), *cf), (m, M, N)
    # what else says no: the one-wave form (2 hops, 512 slots, int32 offsets), 64-bit keys, shapes without key rows
    for m, M, idx64, want in ((2, 204, False, False), (2, 204, True, True), (2, 205, False, True), (4, 128, False, False),
                              (3, 67, False, False), (5, 100, False, False), (3, 257, False, False), (1, 200, False, False)):
        assert P.eligible(1 << 16, M, m, idx64) == want, (m, M, idx64)
        assert (sampler.packed_rows_form(1 << 16, M, m, idx64) is not None) == want, (m, M, idx64)
        if built:
            assert _c_format(1 << 16, M, m, idx64)[0] == int(want), (m, M, idx64)


def test_every_gpu_shape_is_eligible_and_names_its_instantiation():
    seen = set()
    for m, M in P.SHAPES:
        N = P.NODES[m]
        for idx64 in (False, True):
            tup = W.variant(M, m, "keys32", idx64)
            assert tup is not None and tup[4] and tup[5]
            assert P.eligible(N, M, m, idx64) == (tup[2] == 128)
            if tup[2] == 128:
                seen.add((idx64,) + tup[:3] + tup[6:])
    # (idx64, MH, SPL, NT, EPLP): every two-wave form of the 32-bit key rows
    want = {(i, mh, 8, 128, 5) for i in (False, True) for mh in (2, 3, 4)} | {(i, 3, 8, 128, 0) for i in (False, True)} | \
        {(i, mh, 4, 128, 0) for i in (False, True) for mh in (3, 4)} | {(True, 2, 4, 128, 0)}
    assert seen == want
    assert not P.eligible(P.NODES[2], 204, 2, False)        # the one-wave neighbour: refused by the entry point


# ------------------------------------------------------------------------------------------- the walk's cases reach their branches
def _packed(exp, i, M, m, cb, fb):
    ids, keys = P.row(exp, i)
    code, esc = P.codes(keys, M, m, cb, fb)
    return ids, keys, esc


@pytest.mark.parametrize("m,M", P.SHAPES)
def test_walk_graph_reaches_every_branch_of_the_packed_store(m, M):
    g = P.walk_graph(M, m)
    exp = P.walk_rows(M, m)
    cb, fb = P.fmt(g["num_nodes"], m)
    assert fb == (3 if m > 2 else 5)
    rows, degs = g["rows"], g["degrees"]
    ns = exp["nsize"]
    esc_of = {i: _packed(exp, i, M, m, cb, fb)[2] for i in range(len(ns))}
    ne = np.array([esc_of[i].sum() for i in range(len(ns))])
    # every row round-trips through the format
    for i in range(len(ns)):
        ids, keys, _ = _packed(exp, i, M, m, cb, fb)
        words, lst = P.pack_row(ids, keys, M, m, cb, fb)
        back = P.unpack_row(words, lst, M, m, cb, fb)
        assert np.array_equal(back[0], ids) and np.array_equal(back[1], keys)
    ladder = rows["ladder"]
    # the isolated root: one member, every count M -- an escape
    iso = ladder[degs == 0][0]
    assert ns[iso] == 1 and ne[iso] == 1
    # rows without any escape, and rows with some
    assert ((ne == 0) & (ns > 1)).any() and ((ne > 0) & (ne < ns)).any()
    # degree 1 and degree 2 with every member an escape: the pair and the star
    for name, n_members in (("pair", 2), ("star", 3)):
        i = rows[name][0]
        assert ns[i] == n_members and ne[i] == n_members, name
    # first-hop counts on both sides of 2^fb: the modulo first hop gives every neighbour floor or ceil of M / degree walks
    lo_deg = -(-M // (1 << fb))                    # the smallest degree with a first-hop count below 2^fb somewhere
    hit = []
    for d in (lo_deg - 1, lo_deg, lo_deg + 1):
        if d < 1:
            continue
        i = ladder[degs == d][0]
        ids, keys, esc = _packed(exp, i, M, m, cb, fb)
        first = P.fields(keys, M, m)[:, 1]
        nb = g["indices"][g["indptr"][g["batch"][i]]: g["indptr"][g["batch"][i] + 1]]
        c1 = first[np.isin(ids, nb)]
        assert len(c1) == d and set(c1.tolist()) <= {M // d, -(-M // d)}
        assert esc[np.isin(ids, nb)][c1 >= (1 << fb)].all()          # (a later hop may add to a neighbour's key, never take away)
        hit.append(sorted(set(c1.tolist())))
    if (m, M) == (3, 200):
        assert lo_deg == 25 and hit == [[8, 9], [8], [7, 8]]          # degrees 24 | 25 | 26 at M = 200
    # the runs: sets of exactly 3, 4, 5 (127, 128, 129 where M holds them) members
    assert ns[rows["run"]].tolist() == g["runs"] and ns[rows["run_low"]].tolist() == [5]
    if M >= 128:
        assert {127, 128, 129} <= set(ns.tolist())
    assert {1, 3, 4, 5} <= set(ns.tolist())
    # escapes in the scalar tail (the last ns % 4 members of a row on 16-byte boundaries)
    tail = [i for i in range(len(ns)) if ns[i] % 4 and esc_of[i][ns[i] - ns[i] % 4:].any()]
    assert tail, "no escape in a scalar tail"
    # the pinned tree: the last member alone escapes; with four members per lane it stands in the tail / the last trip
    for i, fan in zip(rows["pinned"], (M, min(-(-400 // m), M))):
        assert ns[i] == fan * m + 2 - (1 << fb) and ne[i] == 1 and esc_of[i][-1]
    assert 256 <= ns[rows["pinned"][1]] - 1 < 512
    # escapes that the second wave finds, and escapes behind the first trip: one member per lane (the default pitch) and four
    pos = {i: np.nonzero(esc_of[i])[0] for i in range(len(ns))}
    for per in (1, 4):
        assert any(((p // per) % 128 >= 64).any() for p in pos.values()), ("second wave", per)
        if per == 1 or M * m + 2 - (1 << fb) > 512:
            assert any((p >= per * 128).any() for p in pos.values()), ("later trip", per)
        assert any(len(p) >= 2 and (np.diff(p // per) == 0).any() for p in pos.values()) or per == 1, ("two escapes of one lane", per)
    # both kinds of first hop and the largest set
    assert (degs > M).any() and ns.max() == M * m + 1


# ---------------------------------------------------------------------------------------- the join's rows reach their branches
@pytest.mark.parametrize("m,M,N,pitch", P.JOIN_SHAPES)
def test_join_rows_reach_every_branch_of_the_packed_join(m, M, N, pitch):
    r = P.join_rows(M, m, N, pitch)
    cb, fb, names = r["cb"], r["fb"], r["names"]
    assert fb >= 3 and pitch % 32 == 0 and M * m + 1 <= pitch + 31
    nt_lanes, trips = P.join_lanes(pitch)
    assert pitch <= trips * nt_lanes                                 # the register trips hold every row
    esc = [P.codes(k, M, m, cb, fb)[1] for k in r["keys"]]
    lens = [len(i) for i in r["ids"]]
    for n in P.JOIN_LENGTHS:
        assert n in lens or n > pitch
    assert max(lens) == min(M * m + 1, pitch)
    at = {n: i for i, n in enumerate(names)}
    assert not esc[at["none"]].any() and esc[at["all"]].all() and esc[at["many"]].sum() > P.KESC
    if cb == 1 + m * fb:       # small counts whose code is all ones
        f = P.fields(r["keys"][at["ones"]], M, m)
        assert (f[:, 1:] < (1 << fb)).all() and esc[at["ones"]].any() and not esc[at["ones"]].all()
    # every kind of hit over all pairs (i, j): the S member an escape, the T member an escape, both, neither
    kinds = set()
    for i in range(len(lens)):
        for j in range(len(lens)):
            s, t = (i, j) if lens[i] <= lens[j] else (j, i)            # S = the shorter row (equal lengths: the first)
            _, si, ti = np.intersect1d(r["ids"][s], r["ids"][t], return_indices=True)
            kinds |= set(zip(esc[s][si].tolist(), esc[t][ti].tolist()))
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}
    # S longer than T and T longer than S happen by the order of a pair; an empty row stands on either side
    assert lens[0] == 0 and len(set(lens)) > 4
    # escapes in later chunks and later trips of a row (the chunk bases and the ballots of every trip)
    assert any((np.nonzero(e)[0] >= nt_lanes).any() for e in esc) and any((np.nonzero(e)[0] % nt_lanes >= 64).any() for e in esc)
    # every ordered pair fits one mirrored block; the split form (<= 1,024 pairs) and the whole form both run
    assert P.join_pairs(len(lens), len(lens) ** 2).shape == (2, len(lens) ** 2) and len(lens) ** 2 <= 1024

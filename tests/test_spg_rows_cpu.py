"""CPU: the synthetic rows of tests/spg_rows.py reach the branches of csrc/spg.hip's sorts that tests/test_gpu_spg_rows.py means them
for -- shown through the NumPy restatements of the bucket function, the level-2 index and the two host rules, for every
(row length, bucket bound) the GPU tests use.  No row is sorted here."""
import numpy as np
import pytest

import spg_rows as R


def _build_cases():
    """(max_len, bcap, gen, ns, ids) of every row the bucket kernel of subgacc_spg_build is given"""
    out = []
    for max_len in R.BUILD_MAX_LEN + (R.UNDERSTATED_BUCKET[0],):
        lengths = R.build_lengths(max_len) if max_len != R.UNDERSTATED_BUCKET[0] else R.UNDERSTATED_BUCKET[1]
        out += [(max_len, R.bcap_build(max_len), g, ns, ids) for g, ns, ids in R.rows(lengths) if ns <= max_len]
    return out


def _finish_cases():
    out = []
    for stride in R.FINISH_STRIDES:
        out += [(stride, R.bcap_finish(stride), g, ns, ids) for g, ns, ids in R.rows(R.finish_lengths(stride))]
    return out


BUILD, FINISH = _build_cases(), _finish_cases()
SORTED = [c for c in BUILD + FINISH if c[3] >= 1]


def test_host_rules():
    assert [R.bcap_build(m) for m in R.BUILD_MAX_LEN] == [64, 64, 128, 512, 512, 512]
    assert {R.bcap_build(m) for m in R.BUILD_MAX_LEN} == {64, 128, 512} and R.bcap_build(0) == 64 and R.bcap_build(257) == 512
    assert [R.bcap_finish(s) for s in R.FINISH_STRIDES] == [64, 256, 256, 256, 256, 256, 256, 256] and R.bcap_finish(65) == 128
    assert [R.emax_of(s) for s in R.FINISH_STRIDES] == [4, 4, 7, 7, 10, 10, 16, 16]
    assert 8 * R.pow2_at_least(max(R.BITONIC_MAX_LEN)) <= R.LDS_BYTES < 8 * R.pow2_at_least(R.BITONIC_REFUSED)
    assert {8 * R.pow2_at_least(m) > 64 * 1024 for m in R.BITONIC_MAX_LEN} == {False, True}       # both sides of the attribute call
    assert R.FINISH_REFUSED == R.BUCKET_MAX_LEN + 1 and max(R.FINISH_STRIDES) == max(R.BUILD_NS) == R.BUCKET_MAX_LEN


def test_every_pair_is_generated():
    """every (length, generator) pair is there; the only pairs left out are island below 3 members and stairs below 64"""
    left_out = {(g, ns) for ns in R.BUILD_NS for g in R.GENERATORS if not R.defined(g, ns)}
    assert left_out == {("island", 0), ("island", 1), ("island", 2), ("stairs", 0), ("stairs", 1), ("stairs", 2), ("stairs", 63)}
    got = {(g, ns) for m, _, g, ns, _ in BUILD if m == 1024}
    assert got == {(g, ns) for ns in R.BUILD_NS for g in R.GENERATORS} - left_out
    for stride in R.FINISH_STRIDES:
        got = {(g, ns) for s, _, g, ns, _ in FINISH if s == stride}
        assert got == {(g, ns) for ns in R.finish_lengths(stride) for g in R.GENERATORS if R.defined(g, ns)}
        assert {0, 1, stride} <= set(R.finish_lengths(stride)) and max(R.finish_lengths(stride)) == stride


def test_members_per_lane_are_all_reached():
    """every E of the bucket kernel, and every finish_row<E> of every finish_rows_kernel<EMAX>, from both sides of its edge"""
    assert {R.build_members_per_lane(ns) for ns in R.BUILD_NS} == {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16}
    for ns in R.BUILD_NS:
        if ns % 64 == 0 and ns and ns + 1 in R.BUILD_NS:
            assert R.build_members_per_lane(ns) < R.build_members_per_lane(ns + 1)
    want = {4: {0, 2, 4}, 7: {0, 2, 4, 7}, 10: {0, 4, 7, 10}, 16: {0, 4, 7, 10, 13, 16}}
    for emax in want:
        got = {R.finish_members_per_lane(s, ns) for s in R.FINISH_STRIDES if R.emax_of(s) == emax for ns in R.finish_lengths(s)}
        assert got == want[emax], (emax, got)


def test_rows_are_distinct_ids_in_range():
    for _, _, g, ns, ids in BUILD + FINISH:
        assert ids.dtype == np.int32 and len(ids) == ns == len(np.unique(ids)) and (ns == 0 or ids.min() >= 0)
        if g in ("spread", "island", "stairs") and ns >= 2:
            assert ids.min() == 0 and ids.max() == R.TOP
        if g == "consecutive-top" and ns:
            assert ids.max() == R.TOP and ids.min() == R.TOP + 1 - ns
        if g.startswith("consecutive") and ns:
            assert ids.max() - ids.min() == ns - 1
        if ns > 2:
            assert not np.array_equal(ids, np.sort(ids))                                        # shuffled
    for max_len in R.BITONIC_MAX_LEN:
        for g, ns, ids in R.rows(R.bitonic_lengths(max_len), R.SORT_ONLY):
            assert len(np.unique(ids)) == ns and (ns == 0 or (ids.min() >= 0 and ids.max() <= R.TOP))
            assert ns <= R.pow2_at_least(max_len)


def test_the_id_range_edges_are_reached():
    """Ls = 31 (a range of 2^31), Ls = 0 and logb = 0 (one member), Ls = logb and Ls > logb"""
    seen = {(R.level1(ids, bcap)[:2]) for _, bcap, _, ns, ids in SORTED}
    assert (0, 0) in seen and any(Ls == 31 for _, Ls in seen) and any(Ls == logb and Ls for logb, Ls in seen)
    assert {0, 1, 6, 7, 8, 9} <= {logb for logb, _ in seen}
    for _, bcap, g, ns, ids in SORTED:
        logb, Ls, counts = R.level1(ids, bcap)
        assert counts.sum() == ns and (1 << logb) <= max(bcap, 1) and (ns == 1 or (1 << logb) >= min(ns, bcap))
        if g in ("spread", "island", "stairs") and ns >= 2:
            assert Ls == 31


@pytest.mark.parametrize("gen", ["island", "stairs"])
def test_crowded_rows_take_level_2(gen):
    n = 0
    for _, bcap, g, ns, ids in SORTED:
        if g != gen or ns < 64:
            continue
        n += 1
        logb, Ls, counts = R.level1(ids, bcap)
        assert counts.max() > R.FINE_ABOVE and Ls > logb and R.takes_level2(ids, bcap), (g, ns, bcap)
        idx2, bk = R.level2(ids, bcap)
        if gen == "island":
            b = int(np.argmax(counts))
            assert counts[b] == ns - 2 and len(set(idx2[bk == b])) == 1, (ns, bcap)             # the worst case: ONE sub-bucket
        else:
            assert {int(v) & 1 for v in idx2} == {0, 1}                                          # both halves of a counter word
            best = 0
            for b in np.nonzero(counts > R.FINE_ABOVE)[0]:
                sub = np.bincount(idx2[bk == b])
                sub = sub[sub > 0]
                if len(sub) >= 3 and len(set(sub)) >= 2:
                    best += 1
            assert best >= 1, (ns, bcap)
            sub_all = np.bincount(idx2)
            assert (sub_all > 0).sum() >= 3 and len(set(sub_all[sub_all > 0])) >= 2
    assert n >= 20


def test_consecutive_rows_have_a_bucket_per_id():
    n = 0
    for _, bcap, g, ns, ids in SORTED:
        if g.startswith("consecutive") and ns <= bcap:
            logb, Ls, counts = R.level1(ids, bcap)
            assert Ls <= logb and counts.max() == 1 and not R.takes_level2(ids, bcap)
            n += 1
    assert n >= 20


def test_spread_rows_stop_at_level_1():
    n = 0
    for _, bcap, g, ns, ids in SORTED:
        if g == "spread":
            assert R.level1(ids, bcap)[2].max() <= R.FINE_ABOVE and not R.takes_level2(ids, bcap), (ns, bcap)
            n += 1
    assert n >= 50


def test_stairs_runs():
    assert R.stairs_runs(64) == [13, 49] and R.stairs_runs(1024)[:5] == [13, 40, 100, 300, 13] and sum(R.stairs_runs(833)) == 831
    assert all(min(R.stairs_runs(ns)) > R.FINE_ABOVE for ns in R.BUILD_NS if ns >= 64)


def test_finish_rows_past_the_fold_table():
    """on the host: a row of 1,024 members with a key each cannot fold them in 256 slots, so at least 768 go to the table one by
    one; a row of exactly 256 distinct keys fills the fold table or spills"""
    cases, _, keys, nsize = R.finish_case(1024)
    own = [i for i, (_, ns, _, kind) in enumerate(cases) if kind == "own" and ns == 1024]
    assert len(own) == 5 and all(len(np.unique(keys[i])) == 1024 > R.FOLD_SLOTS for i in own)
    full = [i for i, (_, ns, _, kind) in enumerate(cases) if kind == "256"]
    assert full and all(len(np.unique(keys[i, :nsize[i]])) == R.FOLD_SLOTS for i in full)
    walk = [i for i, (_, ns, _, kind) in enumerate(cases) if kind == "walk" and ns >= 128]
    assert walk and all(24 <= len(np.unique(keys[i, :nsize[i]])) <= 48 for i in walk)

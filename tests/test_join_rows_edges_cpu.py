"""CPU: tests/join_rows_edges.py is what it claims.  (1) join_rows_ref reproduces the reference's own join outputs (the goldens) bit for
bit and equals the C merge join (oracle.sjoin) and oracle.gather_numpy on every synthetic case whose payload those take; its key
unpacking equals the sampler's count rows divided in float32.  (2) Every case reaches the edge it is named for -- asserted on the
inputs, so a case list that silently stopped reaching an edge fails here.  (3) The three layouts of one EdgeRows decode to the same
rows.  The kernels themselves: tests/test_gpu_join_rows_edges.py."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
import join_rows_edges as J
from join_rows_edges import CASES

ALL = sorted(CASES)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------------- 1. the restatement is the reference
@pytest.mark.parametrize("name", ["sjoin_int.npz", "sjoin_int_emptyrows.npz", "sjoin_float.npz"])
def test_ref_reproduces_the_goldens(name):
    """xz_ptr1 / ind_ptr1 (segment pointers) and xz_ptr0 / ind_ptr0 (segment ids) of the real reference's gather(), bit for bit"""
    g = np.load(os.path.join(GOLDEN, name))
    f64 = g["z_data"].dtype.kind == "f"
    kind = "f64" if f64 else "sfptr"
    rows = J.EdgeRows.from_packed(name, g["z_indptr"], g["z_indices"], g["z_data"].astype(J.PAYLOAD_DTYPE[kind]), kind)
    own, partner = oracle.pair_segments(g["edge"])
    for given in (True, False):
        r = J.join_rows_ref(rows, own, partner if given else None, kind, pair_block=g["edge"].shape[1], table=None if f64 else g["encode"])
        assert r.flags3 == 0 and r.live.all()
        for xz, ind, want in ((g["xz_ptr1"], g["ind_ptr1"], r.seg), (g["xz_ptr0"], g["ind_ptr0"], r.segid)):
            assert xz.dtype == np.float32 and xz.shape == r.xz.shape and np.array_equal(_bits(xz), _bits(r.xz))
            assert np.array_equal(ind, want)


def _mapped(c):
    """the packed store of case c with the payload as the kernels see it (SFptr+1)"""
    off, ids, pay = c.rows.packed()
    if c.kind == "sfptr":
        pay = (c.slot_id[pay] + 1).astype(np.int32) if c.slot_id is not None else pay + np.int32(c.val_add)
    return off, ids, pay


ORACLE_CASES = [n for n in ALL if CASES[n].kind in ("sfptr", "f64") and CASES[n].ref().flags3 & ~2 == 0]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_ref_equals_the_c_merge_join(name):
    """oracle.sjoin over the same rows and list: seg, and the index pairs (table payload) or the float pairs (float payload)"""
    c, r = CASES[name], CASES[name].ref()
    off, ids, pay = _mapped(c)
    partner = J._partner_of(c.own, c.partner, c.pair_block)
    seg, pairs = oracle.sjoin(off, ids, pay, c.own, partner)
    assert np.array_equal(seg, r.seg)
    if c.kind == "f64":
        assert np.array_equal(_bits(pairs), _bits(r.xz[:, :, 0]))
    else:
        assert np.array_equal(pairs, r.idx)
        if r.xz is not None and not r.flags3:
            assert np.array_equal(_bits(c.table[pairs]), _bits(r.xz))


@pytest.mark.parametrize("name", [n for n in ORACLE_CASES if CASES[n].pair_block == CASES[n].S // 2 and CASES[n].S <= 400 and
                                  not CASES[n].ref().flags3])
def test_ref_equals_gather_numpy(name):
    """gather-shaped lists (one mirrored block) of up to 200 pairs; an SFptr outside the table is not gather_numpy's to index"""
    c, r = CASES[name], CASES[name].ref()
    edge = c.own.reshape(2, -1)
    xz, seg = oracle.gather_numpy(edge, _mapped(c), ptr=True, encode=c.table)
    assert np.array_equal(seg, r.seg)
    if r.xz is not None:
        assert np.array_equal(_bits(xz.astype(np.float32)), _bits(r.xz))
    _, segid = oracle.gather_numpy(edge, _mapped(c), ptr=False, encode=c.table)
    assert np.array_equal(segid, r.segid)


def _graph(N, E, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, N, E), rng.integers(0, N, E)
    keep = u != v
    e = np.unique(np.concatenate([np.stack([u[keep], v[keep]], 1), np.stack([v[keep], u[keep]], 1)]), axis=0)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=N), out=indptr[1:])
    return indptr, e[:, 1].astype(np.int32)


@pytest.mark.parametrize("M,hops", [(200, 3), (200, 4), (100, 2), (4095, 2), (4096, 2)])
def test_key_unpacking_equals_the_count_rows_divided(M, hops):
    """keys packed from oracle.gset_sampler's own count rows (col 0 = M on a root's own row): unpack_keys gives count / M in float32"""
    indptr, indices = _graph(50, 200, 7)
    _, _, enc = oracle.gset_sampler(indptr, indices, np.arange(20), num_walks=M, num_steps=hops)
    enc = enc.astype(np.int64)
    assert enc.shape[1] == hops + 1 and set(np.unique(enc[:, 0])) == {0, M} and enc[:, 1:].max() > M // 4
    wide = hops * J.key_shift(M) + 1 > 31
    keys = J.pack_keys(enc[:, 0] != 0, enc[:, 1:], M, wide)
    assert keys.dtype == (np.uint64 if wide else np.uint32) and wide == (hops == 4)
    want = enc.astype(np.float32) / np.float32(M)
    assert np.array_equal(_bits(J.unpack_keys(keys, M, hops)), _bits(want))


def test_documented_flags_of_the_restatement():
    """empty row for a row number outside the store (16), a skipped pair for an unmirrored (4) or too-long (1) one, both halves table
    row 0 for an SFptr outside the table (2) -- and only with out_xz"""
    for given in ("given", "null"):
        c = CASES[f"key32-list-rows-outside-partner-{given}"]
        r = c.ref()
        assert r.flags3 == 16 and r.live.all() and set(c.own.tolist()) >= {-1, c.rows.n}
        out = np.flatnonzero((c.own < 0) | (c.own >= c.rows.n))
        assert len(out) == 2 and (np.diff(r.seg)[out] == 0).all()
        mir = (out + c.pair_block) % c.S                      # the mirrors: their partner is absent everywhere
        for j in mir:
            assert (r.xz[r.seg[j]:r.seg[j + 1], 1] == 0).all() and r.seg[j + 1] > r.seg[j]
    c = CASES["key32-list-unmirrored-pair"]
    r = c.ref()
    dead = np.flatnonzero(~np.isin(np.arange(c.S), r.segid[r.live]) & (np.diff(r.seg) > 0))
    assert r.flags3 == 4 and sorted(dead.tolist()) == [c.note, c.pair_block + c.note]
    for name in ("key32-packed-row-of-max_len+1", "seg-sf-partner-of-max_len+1"):
        c, r = CASES[name], CASES[name].ref()
        assert r.flags3 == 1 and 0 < (~r.live).sum() < r.live.size and int(c.rows.len.max()) == c.max_len + 1
    for kind in ("key32", "sf", "f64"):          # strided row_len = row_stride + 1, headed head = row_stride: flagged, the pair skipped
        for lay in ("strided", "headed"):
            c = CASES[f"{kind}-{lay}-row-longer-than-slot"]
            r = c.ref()
            long_row = int(np.argmax(c.rows.len))
            assert c.rows.len[long_row] == c.ML + 1 == (161 if lay == "strided" else 160) and long_row != c.rows.n - 1
            dead = set(r.segid[~r.live].tolist())
            touch = {j for j in range(c.S) if long_row in (c.own[j], J._partner_of(c.own, c.partner, c.pair_block)[j])}
            assert r.flags3 == 1 and dead == {j for j in touch if r.seg[j + 1] > r.seg[j]} and len(dead) >= 6 and r.live.sum() > 500
    for name in ("sf-packed-k3-sfptr-outside-table", "sf-packed-k4-sfptr-outside-table", "seg-sf-k4-sfptr-outside-table"):
        c, r = CASES[name], CASES[name].ref()
        bad = ((r.idx < 0) | (r.idx >= c.table.shape[0])).any(1)
        assert r.flags3 == 2 and bad.sum() >= 3 and (r.idx < 0).any() and (r.idx == c.table.shape[0]).any()
        assert (r.xz[bad] == c.table[0]).all() and c.table[0].any()
        one = bad & ~((r.idx < 0) | (r.idx >= c.table.shape[0])).all(1)       # only one half outside: both halves row 0 all the same
        assert one.any()
    assert CASES["sf-packed-sfptr-outside-table-idx-alone"].ref().flags3 == 0


# ------------------------------------------------------------------------------------------------- 2. premises of the cases
INSTANTIATIONS = {      # every instantiation launch_key_join, launch_table_pairs, launch_f64_pairs and launch_segments can pick
    "sjoin_keypair_kernel<4, 256, false, false>", "sjoin_keypair_kernel<4, 128, false, false>", "sjoin_keypair_kernel<3, 128, false, false>",
    "sjoin_keypair_kernel<5, 128, false, false>", "sjoin_keypair_kernel<0, 128, false, false>", "sjoin_keypair_kernel<5, 256, true, false>",
    "sjoin_keypair_kernel<5, 128, true, false>", "sjoin_keypair_kernel<0, 128, true, false>", "sjoin_keypair_kernel<4, 128, false, true>",
    "sjoin_keypair_kernel<3, 128, false, true>", "sjoin_keypair_kernel<5, 128, false, true>", "sjoin_keypair_kernel<0, 128, false, true>",
    "sjoin_f64pair_kernel<64>", "sjoin_f64pair_kernel<128>", "sjoin_fill_kernel<false, 0, true>", "sjoin_fill_kernel<false, 4, true>",
    "sjoin_fill_kernel<false, 0, false>", "sjoin_fill_kernel<false, 4, false>", "sjoin_fill_kernel<true, 0, true>",
    "sjoin_fill_kernel<true, 0, false>"}

EXPECT = {      # the cases named for a dispatch decision, and what it must be
    "key32-M200-h3-strided-plan256-2049pairs": "sjoin_keypair_kernel<4, 256, false, false>",
    "key32-M200-h3-strided-plan256-2048pairs": "sjoin_keypair_kernel<4, 128, false, false>",
    "key32-M200-h3-packed-max512-2049pairs": "sjoin_keypair_kernel<4, 128, false, false>",
    "key32-M200-h2-strided-plan128-2049pairs": "sjoin_keypair_kernel<3, 128, false, false>",
    "key32-M100-h4-strided-plan128": "sjoin_keypair_kernel<5, 128, false, false>",
    "key32-M200-h1-strided-plan128": "sjoin_keypair_kernel<0, 128, false, false>",
    "key32-M7-h7-strided-plan128": "sjoin_keypair_kernel<0, 128, false, false>",
    "key64-M200-h4-strided-plan256-2049pairs": "sjoin_keypair_kernel<5, 256, true, false>",
    "key64-M200-h4-strided-plan256-2048pairs": "sjoin_keypair_kernel<5, 128, true, false>",
    "key64-M15-h15-strided-plan128": "sjoin_keypair_kernel<0, 128, true, false>",
    "key64-M1000-h5-strided-plan128": "sjoin_keypair_kernel<0, 128, true, false>",
    "sf-packed-k4-xz+0": "sjoin_keypair_kernel<4, 128, false, true>", "sf-packed-k4-xz+1": "sjoin_keypair_kernel<0, 128, false, true>",
    "sf-packed-k4-table+1": "sjoin_keypair_kernel<0, 128, false, true>", "sf-packed-idx-alone": "sjoin_keypair_kernel<0, 128, false, true>",
    "sf-packed-k3-max_len-10240": "sjoin_keypair_kernel<3, 128, false, true>", "sf-packed-k3-max_len-10241": "sjoin_fill_kernel<false, 0, true>",
    "f64-packed-max128": "sjoin_f64pair_kernel<64>", "f64-packed-max129": "sjoin_f64pair_kernel<128>",
    "f64-strided-128": "sjoin_f64pair_kernel<64>", "f64-headed-128": "sjoin_f64pair_kernel<64>",
    "f64-packed-max_len-8191": "sjoin_f64pair_kernel<128>", "f64-packed-max_len-8192": "sjoin_fill_kernel<true, 0, true>",
    "seg-sf-k4": "sjoin_fill_kernel<false, 4, true>", "seg-sf-k4-xz+1": "sjoin_fill_kernel<false, 0, true>",
    "seg-sf-k3-max_len-20480": "sjoin_fill_kernel<false, 0, true>", "seg-sf-k3-max_len-20481": "sjoin_fill_kernel<false, 0, false>",
    "seg-sf-k4-max_len-20480": "sjoin_fill_kernel<false, 4, true>", "seg-sf-k4-max_len-20481": "sjoin_fill_kernel<false, 4, false>",
    "seg-f64-max_len-13653": "sjoin_fill_kernel<true, 0, true>", "seg-f64-max_len-13654": "sjoin_fill_kernel<true, 0, false>",
}


def test_every_instantiation_is_reached_and_the_named_ones_are_what_they_say():
    assert {c.inst for c in CASES.values()} == INSTANTIATIONS
    for name, inst in EXPECT.items():
        assert J.route(CASES[name]) == inst == CASES[name].inst, name


PLANS = [n for n in ALL if "plan128" in n or "plan256" in n]


@pytest.mark.parametrize("name", PLANS)
def test_plan_cases_reach_every_trip_span_and_deal(name):
    """a length plan's list: rows at every trip edge of its lane count, S streamed for 1, 65 and 129 members (both rows of
    the pair exceed 4 * NT), chunksS % NW takes every residue, (u, u) pairs, both orders (swap) and equal lengths, the empty row"""
    c = CASES[name]
    NT = J.lanes(c)
    NW = NT // J.WAVE
    pl = J.pair_lengths(c)
    ns = np.array([p[0] for p in pl])
    have = set(c.rows.len.tolist())
    big = "plan256" in name
    top = 4 * (256 if big else 128)
    assert {0, 1, 63, 64, 65, top - 1, top, top + 1} <= have
    if NT == (256 if big else 128):      # the plan's own lane count (a 256-lane plan at 2,048 pairs runs 128 lanes: more of S streams)
        assert {n - J.REG_TRIPS * NT for n in ns.tolist() if n > J.REG_TRIPS * NT} >= {1, 65, 129}
        for e in range(1, J.REG_TRIPS + 1):
            assert {e * NT - 1, e * NT, e * NT + 1} <= have
    else:
        assert (ns > J.REG_TRIPS * NT).any()
    assert {int(-(-n // J.WAVE)) % NW for n in ns.tolist()} == set(range(NW))
    pr = J.pair_rows(c)
    L = c.rows.len
    assert any(a == b for a, b in pr) and any(L[a] > L[b] for a, b in pr) and any(L[a] < L[b] for a, b in pr)
    assert any(a != b and L[a] == L[b] > 64 for a, b in pr)          # na == nb for two distinct rows
    assert any(L[a] == 0 and L[b] > 0 for a, b in pr) and any(L[b] == 0 and L[a] > 0 for a, b in pr) and (0, 0) in pr
    # T staged through its speculative trip, three register trips and the tail loop (r >= 4 * NT)
    assert max(p[1] for p in pl) > J.REG_TRIPS * NT


@pytest.mark.parametrize("name", [n for n in ALL if n.endswith("pairs")])
def test_split_cases_have_2048_and_2049_pairs(name):
    c = CASES[name]
    pairs = int(name.rsplit("-", 1)[1][:-5])
    assert c.S == 2 * pairs and c.pair_block == pairs and J.pair_split(pairs) == (2 if pairs == 2048 else 1)
    # filled up with pairs of one-member rows: the output stays small
    assert c.ref().seg[-1] < 400_000 and (c.rows.len[c.own[c.base_pairs:pairs]] == 1).all()


def test_split_twins_share_their_base_pairs():
    for a, b in J.SPLIT_PAIRS:
        ca, cb = CASES[a], CASES[b]
        P = ca.base_pairs
        assert P == cb.base_pairs and ca.rows is cb.rows and cb.S == ca.S + 2
        assert np.array_equal(ca.own[:P], cb.own[:P]) and np.array_equal(ca.own[ca.pair_block:][:P], cb.own[cb.pair_block:][:P])


def test_overlap_patterns():
    """per length class: disjoint, identical ids, only the first id shared, only the last, S all below / all above T -- the search meets
    an id below every member of T, above every member, equal to the first and equal to the last; T of one member skips the loop"""
    ids, pairs = J.overlap_rows()
    c = CASES["key32-M200-h3-strided-overlap"]
    seen = set()
    for label, ra, rb in pairs:
        pat = label.rsplit("-", 2)[0]
        s, t = c.rows.ids[ra], c.rows.ids[rb]
        both = np.intersect1d(s, t)
        seen.add(pat)
        if pat == "disjoint":
            assert len(both) == 0 and (len(s) == 1 or (s[0] < t[-1] and t[0] < s[-1]))
        elif pat == "identical":
            assert np.array_equal(s, t) and ra != rb
        elif pat == "first-shared":
            assert both.tolist() == [t[0]] and s[0] == t[0]
        elif pat == "last-shared":
            assert both.tolist() == [t[-1]] and s[-1] == t[-1]
        elif pat == "below":
            assert s[-1] < t[0]
        else:
            assert pat == "above" and s[0] > t[-1]
    assert seen == {"disjoint", "identical", "first-shared", "last-shared", "below", "above"}
    lens = {(len(c.rows.ids[ra]), len(c.rows.ids[rb])) for _, ra, rb in pairs}
    assert {(1, 1), (1, 64), (64, 65), (513, 577), (577, 641)} <= lens          # a T of one member; S in registers; S streamed


def test_lists():
    for blocks in (2, 3):
        c = CASES[f"key32-list-{blocks}-blocks"]
        assert c.S == 2 * blocks * c.pair_block and c.pair_block != c.S // 2 and c.ref().flags3 == 0
    assert CASES["key32-list-3-blocks"].partner is None and CASES["key32-list-2-blocks"].partner is not None
    assert CASES["key32-list-partner-null"].partner is None and CASES["key32-list-partner-given"].partner is not None


def test_alignment_cases_cover_every_offset_and_width():
    """out_xz at base + 0, 1, 2, 3 floats (0, 4, 8, 12 bytes past a 16-byte boundary; the GPU file asserts the pointers) for k = 2, 3,
    4, 5, 8 with and without out_segid; the table payload for k = 1 too: a one-member row of two floats behind a head of three
    (total < head); k = 3, 5 also meet mis != 0 in an aligned buffer, at odd row offsets"""
    for k in (2, 3, 4, 5, 8):
        for off in range(4):
            for tail in ("", "-segid"):
                c = CASES[f"key32-k{k}-xz+{off}{tail}"]
                assert c.xz_off == off and c.k == k and ("segid" in c.outs) == bool(tail)
                assert 1 in c.rows.len[c.own].tolist()
    for k in (1, 3, 4, 5, 8, 16):
        for off in range(4):
            assert CASES[f"sf-packed-k{k}-xz+{off}"].xz_off == off and CASES[f"sf-packed-k{k}-xz+{off}"].k == k
    c = CASES["sf-packed-k1-xz+1"]
    seg = c.ref().seg
    one = np.flatnonzero(np.diff(seg) == 1)
    assert any((seg[j] * 2 + 1) % 4 == 1 for j in one)          # a one-row span of 2 floats whose head would be 3
    for k in (3, 5):
        seg = CASES[f"key32-k{k}-xz+0"].ref().seg
        assert ((seg[:-1] * 2 * k) % 4 != 0).any()


@pytest.mark.parametrize("M", [4095, 4096])
def test_quotient_cases_hold_every_count(M):
    c = CASES[f"key32-M{M}-h2-quotient"]
    keys = np.concatenate(c.rows.vals)
    s = J.key_shift(M)
    assert sorted((keys >> np.uint32(s)) & np.uint32((1 << s) - 1)) == list(range(M + 1))
    assert sorted(keys & np.uint32((1 << s) - 1)) == list(range(M + 1))
    assert (M >= 4096) == (c.M >= 4096)


def test_key64_premises():
    """a key with bit 62 set; a hit whose two keys agree in the low 32 bits and differ above; k = 16, the widest row"""
    c = CASES[f"key64-M{(1 << 30) + 3}-h2-strided-plan128"]
    assert any(((v >> np.uint64(62)) & np.uint64(1)).any() for v in c.rows.vals) and c.hops * J.key_shift(c.M) == 62
    assert CASES["key64-M15-h15-strided-plan128"].k == 16
    for name, c in CASES.items():          # built in (key_vals), counted here per case
        if c.kind == "key64":
            assert J.low_word_twins(c) >= (20 if "plan" in name else 3), name


def test_float_premises():
    """some partner value v has (v + 1.0) - 1.0 != v, some has it = 0, some is negative, some is subnormal (in double, and in float)"""
    for name in ("f64-packed-max128", "f64-packed-plan128", "seg-f64"):
        c, r = CASES[name], CASES[name].ref()
        partner = J._partner_of(c.own, c.partner, c.pair_block)
        got = []
        for a, b in zip(c.own.tolist(), partner.tolist()):
            _, _, ib = np.intersect1d(c.rows.ids[a], c.rows.ids[b], return_indices=True)
            got.append(c.rows.vals[b][ib])
        v = np.concatenate(got)
        w = (v + 1.0) - 1.0
        assert ((w != v) & (w != 0)).any() and ((w == 0) & (v != 0)).any() and (w == v).any() and (v < 0).any()
        assert ((v != 0) & (np.abs(v) < 2.2250738585072014e-308)).any()
        own = np.concatenate([c.rows.vals[a] for a in c.own.tolist()])
        f = own.astype(np.float32)
        assert ((f != 0) & (np.abs(f) < np.float32(1.1754944e-38))).any() and ((f == 0) & (own != 0)).any()
        assert (r.xz[:, 1, 0] == 0).any() and (r.xz[:, 1, 0] != 0).any()


def test_spec_len_cases():
    """strided / headed float rows: spec = min(descriptor's max_len or min(slot, 128), slot) against rows shorter, equal and longer;
    spec not a multiple of NT; spec > 4 * NT"""
    for lay in ("strided", "headed"):
        for spec in (0, 96, 100, 512, 600):
            c = CASES[f"f64-{lay}-spec{spec}"]
            eff = spec if spec else min(c.ML, 128)
            L = c.rows.len
            assert c.max_len == spec and J.lanes(c) == 128 and (L < eff).any() and (L > eff).any()
        assert 128 in CASES[f"f64-{lay}-spec0"].rows.len and 512 in CASES[f"f64-{lay}-spec512"].rows.len
    assert 100 % 128 and 600 > 4 * 128


def test_one_segment_cases():
    """segments (a, b) without their mirrors; every k from 1 to 16 (the magic division f / k2) with own rows of 1, 63, 64, 65, 129"""
    for k in range(1, 17):
        c = CASES[f"seg-sf-k{k}"]
        partner = c.partner
        assert c.pair_block == 0 and c.k == k and {1, 63, 64, 65, 129} <= set(c.rows.len[c.own].tolist())
        have = set(zip(c.own.tolist(), partner.tolist()))
        assert any((b, a) not in have for a, b in have)
        k2 = 2 * k
        magic = ((1 << 20) + k2 - 1) // k2
        f = np.arange(64 * k2)
        assert 64 * k2 <= 2048 and np.array_equal((f * magic) >> 20, f // k2)


def test_same_output_twins_differ_only_in_the_route():
    for a, b in J.SAME_OUTPUT:
        ra, rb = CASES[a].ref(), CASES[b].ref()
        assert np.array_equal(ra.seg, rb.seg) and ra.flags3 == rb.flags3 == 0
        assert np.array_equal(_bits(ra.xz), _bits(rb.xz))
        assert (CASES[a].inst, CASES[a].layout, CASES[a].max_len, CASES[a].partner is None) != \
               (CASES[b].inst, CASES[b].layout, CASES[b].max_len, CASES[b].partner is None)


# ------------------------------------------------------------------------------------------------- 3. the layouts
@pytest.mark.parametrize("name", ["key32-M200-h3-strided-plan128", "key64-M200-h4-headed-small", "sf-packed-k3-plan128", "f64-packed-plan128"])
def test_three_layouts_decode_to_the_same_rows(name):
    rows = CASES[name].rows
    stride = -(-(int(rows.len.max()) + 1) // 32) * 32
    views = [J.decode_packed(*rows.packed()), J.decode_strided(*rows.strided(stride), stride), J.decode_strided(*rows.strided(stride + 5), stride + 5),
             J.decode_headed(*rows.headed(stride), stride)]
    for view in views:
        assert len(view) == rows.n
        for r, (i, v) in enumerate(view):
            assert np.array_equal(i, rows.ids[r]) and np.array_equal(v.view(np.uint8), rows.vals[r].view(np.uint8))
    # poison everywhere else: as ids it is above every member, as payload it is no value any row holds
    _, ids, pay = rows.strided(stride)
    mask = np.arange(stride)[None, :] >= rows.len[:, None]
    assert (ids.reshape(rows.n, stride)[mask] == J.ID_POISON).all()
    p = pay.reshape(rows.n, stride)[mask]
    assert np.isnan(p).all() if rows.kind == "f64" else (p == J.PAYLOAD_POISON[rows.kind]).all()
    assert not any((v == J.PAYLOAD_POISON[rows.kind]).any() for v in rows.vals)

"""GPU (MI355X): the f32 row-form join -- subgacc_sjoin_fill_v2 with form = ROWS, the kernels of csrc/sjoin.hip -- called directly
through _lib.join_desc / _lib.join_fill at every trip, span, split and dispatch edge, against the NumPy restatement of
tests/join_rows_edges.py (which tests/test_join_rows_edges_cpu.py pins to the reference's goldens and to the C merge join).  This fill is
the oracle of test_gpu_half_rows.py, test_gpu_half64_rows.py and test_gpu_packed_rows.py; here it is compared itself.

Every case (join_rows_edges.CASES; the parametrize id carries the kernel instantiation <KV, NT, K64, TAB> / <NT> / <F64, KV, STAGE> that
route() says the launchers pick, to be ticked off against launch_key_join, launch_table_pairs, launch_f64_pairs, launch_segments):
  - seg comes from subgacc_sjoin_sizes / subgacc_sjoin_sizes_rows and equals the restatement's;
  - out_xz, out_idx and out_segid each sit between poisoned rims, with poisoned rows behind row R; the WHOLE buffer is compared, so
    the rims, the rows behind R and the segments of skipped pairs must keep their fill value;
  - the status words are [0, 0, 0, flags3 of the restatement];
  - the case runs twice and gives the same bits;
  - every comparison is bit for bit (int32 views): there are no tolerances in this file.

Documented limits pinned here (include/subgacc.h): a row number outside the store reads as an empty row (flags[3] |= 16); a packed row
longer than max_len (|= 1) and a pair that is not mirrored (|= 4) leave their segments unwritten; an SFptr outside the table (|= 2)
makes BOTH halves of the output row table row 0, out_idx keeps the raw pair, and without out_xz no table is consulted; a T without
members reads slot 0 of its LDS array and uses nothing of it (the pairs with the empty row).  row_stride is the bound of strided rows
and row_stride - 1 of headed rows as max_len is of packed ones: a row_len / head above it sets flags[3] |= 1 and skips the pair."""
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import sp  # noqa: F401
import join_rows_edges as J
from join_rows_edges import CASES

pytestmark = pytest.mark.gpu

RIM = 64                      # words of poison in front of and behind every output (a multiple of 4: the base stays 16-byte aligned)
BEHIND = 40                   # rows of poison behind row R
POISON = 0x7C7C7C7C


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


_STORES = {}


def _store(c):
    """the descriptor's store fields for case c, and the tensors the size pass takes; uploaded once per (rows, layout, stride)"""
    key = (id(c.rows), c.layout, c.stride)
    if key not in _STORES:
        if c.layout == "packed":
            off, ids, pay = c.rows.packed()
            t = dict(row_off=_dev(off), ids=_dev(ids), payload=_dev(pay))
        elif c.layout == "strided":
            lens, ids, pay = c.rows.strided(c.stride)
            t = dict(row_len=_dev(lens), ids=_dev(ids), payload=_dev(pay), row_stride=c.stride)
            t["sizes_len"] = t["row_len"]
        else:
            ids, pay = c.rows.headed(c.stride)
            t = dict(ids=_dev(ids), payload=_dev(pay), row_stride=c.stride, sizes_len=_dev(c.rows.len.astype(np.int32)))
        for v in t.values():      # empty stores still need a pointer
            assert not hasattr(v, "numel") or v.numel() > 0
        _STORES[key] = t
    return _STORES[key]


def _poisoned(words, dtype):
    """a poisoned buffer of RIM + 4 + words + RIM elements on a 16-byte boundary (the 4: room for an output base moved by 0 .. 3 floats)"""
    buf = torch.empty(RIM + 4 + words + RIM, dtype=dtype, device="cuda")
    buf.view(torch.int32).fill_(POISON)
    assert buf.data_ptr() % 16 == 0
    return buf


def _mismatch(got, exp, what, name):
    bad = np.flatnonzero(got != exp)
    return f"{name}: {what}: {bad.size} of {got.size} words differ, first at word {bad[:8].tolist()} (got {got[bad[:4]].tolist()}, want {exp[bad[:4]].tolist()})"


def _run_once(c, r):
    from surel_plus_amd import _lib
    L = _lib.lib()
    st = _store(c)
    own, par = _dev(c.own), (None if c.partner is None else _dev(c.partner))
    S, k, R = c.S, c.k, int(r.seg[-1])
    seg = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device="cuda")
    if c.layout == "packed":
        _lib.check(L.subgacc_sjoin_sizes(_lib.ptr(st["row_off"]), c.rows.n, _lib.ptr(own), _lib.ptr(par), S, _lib.ptr(seg), _lib.ptr(flags),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    else:
        _lib.check(L.subgacc_sjoin_sizes_rows(_lib.ptr(st["sizes_len"]), c.rows.n, _lib.ptr(own), _lib.ptr(par), S, _lib.ptr(seg),
                                              _lib.ptr(flags), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    # the size pass first: the outputs below are sized by R, so the fill runs only over the segment pointers the restatement has too
    assert np.array_equal(seg.cpu().numpy(), r.seg), f"{c.name}: seg differs from the restatement's"
    fields = {n: v for n, v in st.items() if n != "sizes_len"}
    fields.update(n_rows=c.rows.n, max_len=c.max_len, own=own, partner=par, S=S, seg=seg, pair_block=c.pair_block, flags=flags)
    if c.kind in ("key32", "key64"):
        fields.update(num_walks=c.M, num_steps=c.hops)
    if c.kind == "sfptr":
        if c.table is not None:
            tbuf = torch.zeros(c.table.size + 8, dtype=torch.float32, device="cuda")
            table = tbuf[c.table_off: c.table_off + c.table.size]
            table.copy_(torch.from_numpy(c.table.ravel()))
            assert table.data_ptr() % 16 == 4 * c.table_off
            fields.update(table=table, table_rows=c.table.shape[0], k=k)
        if c.slot_id is not None:      # a numbered table of distinct rows: 16 bytes per slot, then the id plane the join reads
            cap = c.slot_id.size
            raw = np.concatenate([np.full(cap * 16, 0x7E, np.uint8), c.slot_id.astype(np.int32).view(np.uint8)])
            fields.update(uniq_table=_dev(raw), uniq_capacity=cap)
            assert L.subgacc_uniq_table_bytes(cap) == raw.size
    out, want = {}, {}
    w = 2 * k
    if "xz" in c.outs:
        buf = _poisoned(R * w + BEHIND * w, torch.float32)
        view = buf[RIM + c.xz_off:]
        assert view.data_ptr() % 16 == 4 * c.xz_off          # this output base is 0, 4, 8, 12 bytes past a 16-byte boundary
        exp = np.full(buf.numel(), POISON, np.int32)
        rows = exp[RIM + c.xz_off: RIM + c.xz_off + R * w].reshape(R, w)
        rows[r.live] = np.ascontiguousarray(r.xz.reshape(R, w)).view(np.int32)[r.live]
        fields["out_xz"], out["xz"], want["xz"] = view, buf, exp
    if "idx" in c.outs:
        buf = _poisoned(R * 2 + BEHIND * 2, torch.int32)
        exp = np.full(buf.numel(), POISON, np.int32)
        rows = exp[RIM: RIM + R * 2].reshape(R, 2)
        rows[r.live] = r.idx[r.live]
        fields["out_idx"], out["idx"], want["idx"] = buf[RIM:], buf, exp
    if "segid" in c.outs:
        buf = _poisoned(R + BEHIND, torch.int64)
        exp = np.full(buf.numel(), (POISON << 32) | POISON, np.int64)
        exp[RIM: RIM + R][r.live] = r.segid[r.live]
        fields["out_segid"], out["segid"], want["segid"] = buf[RIM:], buf, exp.view(np.int32)
    _lib.join_fill(_lib.JOIN_ROWS, J.KIND_CODE[c.kind], **fields)
    torch.cuda.synchronize()
    got = {n: b.cpu().numpy().view(np.int32) for n, b in out.items()}
    for n in got:
        assert np.array_equal(got[n], want[n]), _mismatch(got[n], want[n], f"out_{n}", c.name)
    assert flags.cpu().tolist() == [0, 0, 0, r.flags3], f"{c.name}: flags {flags.cpu().tolist()}, flags[3] should be {r.flags3}"
    return got


@functools.lru_cache(maxsize=None)
def _run(name):
    """case `name` twice: every output against the restatement both times (so: the same bits); -> the first run's buffers"""
    c = CASES[name]
    assert J.route(c) == c.inst
    r = c.ref()
    first = _run_once(c, r)
    again = _run_once(c, r)
    assert all(np.array_equal(first[n], again[n]) for n in first)
    return first


def _cases(*prefixes, skip=()):
    return [pytest.param(n, id=f"{n}|{CASES[n].inst}") for n in sorted(CASES)
            if n.startswith(prefixes) and not any(s in n for s in skip)]


# --------------------------------------------------------------------------------------------------------- key rows, 32 bits
@pytest.mark.parametrize("name", _cases("key32-M"))
def test_key32_rows(sp, name):
    """sjoin_keypair_kernel<KV, NT, false, false>, KV = 4, 3, 5 and 0 (k = 2, k = 8), strided rows and a packed keyed store.
    plan128: rows of 0, 1, 63 .. 65, 127 .. 129, 255 .. 257, 383 .. 385, 511 .. 513, 576, 577, 641 members (stride 672), each with itself
    ((u, u): `same`), with its neighbour in both orders (`swap`; na == nb for the two distinct rows of 577 / 1,089 members) and with the empty row (T or S without
    members: LDS slot 0 read and unused), plus (513, 577), (577, 641), (641, 641): S beyond kRegTrips * 128 members is streamed for 1, 65
    and 129 members, T staged from the speculative trip, three register trips and the tail loop.  plan256 at 2,049 pairs: <4, 256, ..>,
    the same plan around 1,023 .. 1,025, 1,089, 1,153 (stride 1,184); at 2,048 pairs the same rows run 128 lanes with split = 2.
    2,048 / 2,049 pairs for k = 3 and for k = 4 with max_len <= 512: S's spans dealt by u % split and (c / NW) % split, T's from
    (wave + rot) % NW + part * NW, every residue of chunksS % NW.  overlap: disjoint, identical, only the first / last id shared, S below /
    above T per length class (the halving search: an id below every member, above every member, equal to the first, to the last, a T
    of one member).  quotient: every count 0 .. M in both fields at num_walks = 4,095 (two fmas) and 4,096 (IEEE division)."""
    _run(name)


@pytest.mark.parametrize("name", _cases("key32-list", "key32-packed-row", "key32-strided-row", "key32-headed-row"))
def test_key32_lists(sp, name):
    """sjoin_keypair_kernel<4, 128, false, false>: `partner` given and NULL; 2 and 3 mirrored blocks in one list (pb != pairs); one pair
    that is not mirrored (flags[3] |= 4, its two segments keep their fill, the others are joined); one row number = n_rows and one
    = -1 (empty rows, flags[3] |= 16 from the size pass); a packed row of max_len + 1 members, a strided row_len of row_stride + 1 and a
    headed row whose head is row_stride (one above its bound), none of them the last row: flags[3] |= 1, the pairs of that row keep
    their fill, the others are joined, nothing behind the row's slot is read"""
    _run(name)


@pytest.mark.parametrize("name", _cases("key32-k"))
def test_key32_output_alignment(sp, name):
    """emit_key_span: out_xz at base + 0, 1, 2, 3 floats for k = 2, 3, 4, 5, 8 (KV = 0, 3, 4, 5, 0), with and without out_segid: a head
    of 0 - 3 floats from lanes 63, 62, 61, aligned 16-byte body words in (KV + 1) / 2 rounds, a tail of 0 - 3 floats from lanes 60, 59,
    58; spans of 1, 2, 63, 64 and 65 rows; the rims on both sides stay untouched"""
    _run(name)


# --------------------------------------------------------------------------------------------------------- key rows, 64 bits
@pytest.mark.parametrize("name", _cases("key64-"))
def test_key64_rows(sp, name):
    """sjoin_keypair_kernel<5, 128, true>, <5, 256, true> (more than 2,048 pairs, rows around 1,024) and <0, 128, true> for k = 16 (the
    widest row), k = 6 and k = 3 with num_walks = 2^30 + 3: the lead bit is bit 62 and every count is divided, not multiplied; keys
    that agree in their low 32 bits and differ above; strided rows and one headed store"""
    _run(name)


# --------------------------------------------------------------------------------------------------------- table payload
@pytest.mark.parametrize("name", _cases("sf-"))
def test_table_rows(sp, name):
    """sjoin_keypair_kernel<KV, 128, false, true>, KV = 4 (float4 table rows: table and out_xz 16-byte aligned), 3, 5, 0; k = 1, 3, 4, 5,
    8, 16 over plan128.  packed and headed rows hold SFptr+1 (val_add = 0), strided rows a slot with table[slot + 1] (val_add = 1) or
    a slot of a numbered table's id plane (uniq_table).  k = 4 with out_xz or table off by 4 bytes: KV = 0.  out_xz at base + 0 .. 3
    floats; k = 1: a one-row span of two floats behind a head of three (total < head).  out_idx alone (the !out_xz path, k read as 1)
    and with out_xz.  An SFptr = table_rows and a negative one: flags[3] |= 2, both halves table row 0, out_idx the raw pair; alone,
    out_idx raises no flag.  A strided / headed row longer than its slot (flags[3] |= 1).  max_len 10,240 (pair kernel) and 10,241 (sjoin_fill_kernel<false, 0, true>) over the same short rows"""
    _run(name)


# --------------------------------------------------------------------------------------------------------- float payload
@pytest.mark.parametrize("name", _cases("f64-"))
def test_float_rows(sp, name):
    """sjoin_f64pair_kernel<64> (max_len <= 128) and <128>: packed, strided and headed rows of 0, 1, 63 .. 65, 127, 128 members, and in
    the 128-lane form plan128 with the pairs that stream S beyond kF64RegTrips * 128; 2,048 / 2,049 pairs.  Strided / headed rows: the
    first spec_len members asked for before the length is known, spec_len = the descriptor's max_len = 0 (min(slot, 128)), 96, 100
    (no multiple of NT), 512, 600 (> 4 * NT) against rows shorter, equal and longer.  Values: float(own) with double subnormals and
    float subnormals, (partner or 0.0) + 1.0 - 1.0 in double that changes v, sends it to 0, keeps it, negative ones.  out_segid.
    A strided / headed row longer than its slot: too_long(), flags[3] |= 1, the pair skipped.
    max_len 8,191 (pair kernel) and 8,192 (sjoin_fill_kernel<true, 0, true>)"""
    _run(name)


# --------------------------------------------------------------------------------------------------------- one wave per segment
@pytest.mark.parametrize("name", _cases("seg-"))
def test_one_segment_kernel(sp, name):
    """sjoin_fill_kernel<F64, KV, STAGE>, pair_block = 0 over packed rows: segments (a, b) without their mirrors; every k from 1 to 16
    (the magic division f / k2 for f < 64 * k2) with own rows of 1, 63, 64, 65, 129 members, an empty own row, an empty partner; KV = 4
    (k = 4, aligned) and KV = 0 (out_xz off by 4 bytes); the float payload; out_idx alone and with out_xz; a partner row of max_len + 1
    members (flags[3] |= 1, that segment keeps its fill); an SFptr outside the table; STAGE = false beyond max_len 20,480 (int) and
    13,653 (float), the same short rows on both sides"""
    _run(name)


# --------------------------------------------------------------------------------------------------------- cross-checks
@pytest.mark.parametrize("a,b", J.SAME_OUTPUT, ids=[f"{a}=={b}" for a, b in J.SAME_OUTPUT])
def test_same_rows_on_both_sides_of_a_boundary(sp, a, b):
    """the same rows and list through two routes -- either side of a max_len dispatch boundary, the packed / strided / headed rendering
    of one store, `partner` given or NULL, another speculative length: identical out_xz"""
    assert CASES[a].inst != CASES[b].inst or CASES[a].layout != CASES[b].layout or CASES[a].max_len != CASES[b].max_len or \
        (CASES[a].partner is None) != (CASES[b].partner is None)
    xa, xb = _run(a)["xz"], _run(b)["xz"]
    n = int(CASES[a].ref().seg[-1]) * 2 * CASES[a].k
    assert np.array_equal(xa[RIM: RIM + n], xb[RIM: RIM + n])


@pytest.mark.parametrize("a,b", J.SPLIT_PAIRS, ids=[a.rsplit("-", 1)[0] for a, _ in J.SPLIT_PAIRS])
def test_split_2_and_split_1_give_the_same_rows(sp, a, b):
    """lists of 2,048 (split = 2) and 2,049 pairs (split = 1; k = 4 / 64-bit k = 5 with max_len > 512: 256 lanes) built from the same
    base pairs: the same rows for those pairs, segment by segment"""
    ca, cb = CASES[a], CASES[b]
    w = 2 * ca.k
    xa, xb = _run(a)["xz"][RIM:], _run(b)["xz"][RIM:]
    sa, sb = ca.ref().seg, cb.ref().seg
    for block, (oa, ob) in enumerate(((0, 0), (ca.pair_block, cb.pair_block))):
        P = ca.base_pairs
        la, lb = sa[oa] * w, sb[ob] * w
        n = (sa[oa + P] - sa[oa]) * w
        assert n == (sb[ob + P] - sb[ob]) * w and n > 0
        assert np.array_equal(xa[la: la + n], xb[lb: lb + n]), f"block {block}"

"""GPU (MI355X): subgacc_sjoin_fill_half_ids (include/subgacc_half_ids.h; csrc/sjoin_half.hip: sjoin_half_ids_kernel) called directly
through _lib.join_desc over the synthetic packed and strided rows of tests/join_rows_edges.py.  The reference is subgacc_sjoin_fill_v2
with out_segid over the same descriptor: its rows after torch's .to(dtype), its segment ids as they stand.  Both outputs lie between
poisoned rims with poisoned rows behind row R, out_rows on a 16-byte boundary and out_segid 0 or 8 bytes past one; the WHOLE buffers are
compared, so rims, the rows behind R and the rows of a skipped pair must keep their poison.  Every case runs twice; all comparisons
are bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import join_rows_edges as J
import test_gpu_join_rows_edges as G
from gpu_helpers import sp  # noqa: F401

pytestmark = pytest.mark.gpu

RIM, BEHIND = 64, 40
P16 = 0x7C7C
P64 = (G.POISON << 32) | G.POISON
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
KEY_SHAPES = {2: (200, 1), 3: (200, 2), 4: (200, 3), 5: (100, 4)}          # k -> (num_walks, hops)
# the lane trips of 128 and 256 lanes, and the 512 prefetched members
LENS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
STRIDE = 544


def _fill(c, dtype, seg_off, want_flag=0):
    """the size pass, then the f32 fill with out_segid and the 16-bit fill with ids over the same descriptor -> the two poisoned
    buffers of the 16-bit call as NumPy words, after they have been compared with the reference's"""
    from surel_plus_amd import _lib
    L, st = _lib.lib(), G._store(c)
    own, par = G._dev(c.own), (None if c.partner is None else G._dev(c.partner))
    S, k = c.S, c.k
    seg = torch.full((S + 1,), -1, dtype=torch.int64, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device="cuda")
    if c.layout == "packed":
        _lib.check(L.subgacc_sjoin_sizes(_lib.ptr(st["row_off"]), c.rows.n, _lib.ptr(own), _lib.ptr(par), S, _lib.ptr(seg), _lib.ptr(flags),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    else:
        _lib.check(L.subgacc_sjoin_sizes_rows(_lib.ptr(st["sizes_len"]), c.rows.n, _lib.ptr(own), _lib.ptr(par), S, _lib.ptr(seg),
                                              _lib.ptr(flags), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    R, w = int(seg[-1].item()), 2 * k
    fields = {n: v for n, v in st.items() if n != "sizes_len"}
    fields.update(n_rows=c.rows.n, max_len=c.max_len, own=own, partner=par, S=S, seg=seg, pair_block=c.pair_block)
    if c.kind == "key32":
        fields.update(num_walks=c.M, num_steps=c.hops)
    else:
        fields.update(table=G._dev(c.table), table_rows=c.table.shape[0], k=k)
    # the reference: poisoned f32 rows and ids; a row that keeps its poisoned id belongs to a skipped pair
    rflags, hflags = flags.clone(), flags.clone()
    rxz = torch.empty((R + BEHIND) * w, dtype=torch.float32, device="cuda")
    rxz.view(torch.int32).fill_(G.POISON)
    rsid = torch.full((R + BEHIND,), P64, dtype=torch.int64, device="cuda")
    _lib.join_fill(_lib.JOIN_ROWS, J.KIND_CODE[c.kind], out_xz=rxz, out_segid=rsid, flags=rflags, **fields)
    torch.cuda.synchronize()
    live = rsid[:R] != P64
    lens = (seg[1:] - seg[:-1])
    assert torch.equal(rsid[:R][live], torch.repeat_interleave(torch.arange(S, device="cuda"), lens)[live])
    want_rows = torch.full((R + BEHIND, w), P16, dtype=torch.int16, device="cuda")
    want_rows[:R][live] = rxz[: R * w].view(R, w)[live].to(dtype).view(torch.int16)
    # the call under test
    buf = torch.full((RIM + (R + BEHIND) * w + RIM,), P16, dtype=torch.int16, device="cuda")
    sbuf = torch.full((RIM + seg_off + R + BEHIND + RIM,), P64, dtype=torch.int64, device="cuda")
    out, sid = buf[RIM:], sbuf[RIM + seg_off:]
    assert out.data_ptr() % 16 == 0 and sid.data_ptr() % 16 == 8 * (seg_off % 2)
    d = _lib.join_desc(_lib.JOIN_ROWS, J.KIND_CODE[c.kind], flags=hflags, **fields)
    code = {torch.float16: _lib.HALF_F16, torch.bfloat16: _lib.HALF_BF16}[dtype]
    _lib.check(L.subgacc_sjoin_fill_half_ids(C.byref(d), code, _lib.ptr(out), _lib.ptr(sid), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((buf[:RIM] == P16).all()) and bool((buf[RIM + (R + BEHIND) * w:] == P16).all()), f"{c.name}: rims of out_rows"
    assert torch.equal(buf[RIM: RIM + (R + BEHIND) * w].view(R + BEHIND, w), want_rows), f"{c.name}: out_rows"
    assert bool((sbuf[: RIM + seg_off] == P64).all()) and bool((sbuf[RIM + seg_off + R + BEHIND:] == P64).all()), f"{c.name}: rims of out_segid"
    assert torch.equal(sid[: R + BEHIND], rsid), f"{c.name}: out_segid"
    assert torch.equal(hflags, rflags) and hflags[:3].tolist() == [0, 0, 0], f"{c.name}: flags {hflags.tolist()} / {rflags.tolist()}"
    assert int(hflags[3].item()) == want_flag, f"{c.name}: flags[3] = {int(hflags[3].item())}, expected {want_flag}"
    if want_flag & 5:
        assert not bool(live.all()) and bool(live.any())          # the skipped pair's rows kept their poison, the others were written
    else:
        assert bool(live.all()) and R > 0
    return buf.cpu().numpy(), sbuf.cpu().numpy()


def _twice(c, dtype, seg_off=1, want_flag=0):
    a, b = _fill(c, dtype, seg_off, want_flag), _fill(c, dtype, seg_off, want_flag)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


_IDS = J.plan_ids(LENS, 7)
_A, _B = J.plan_pairs(LENS)
_ROWS = {}
_KEEP = []          # every EdgeRows a case was made of: test_gpu_join_rows_edges._store keys its uploads by id(rows)


def _plan_rows(kind, k):
    """the plan's rows with 32-bit keys of the shape of k, or with SFptr+1 into a table of TABLE_ROWS rows"""
    if (kind, k) not in _ROWS:
        if kind == "key32":
            M, h = KEY_SHAPES[k]
            _ROWS[kind, k] = J.EdgeRows(f"ids-key32-k{k}", _IDS, J.key_vals(_IDS, M, h, False, 100 + k), "key32")
        else:
            _ROWS[kind, k] = J.EdgeRows(f"ids-sf-k{k}", _IDS, J.sf_vals(_IDS, 1, J.TABLE_ROWS, 110 + k), "sfptr")
    return _ROWS[kind, k]


def _case(name, kind, layout, k, own, par, pb, rows=None, max_len=513, stride=STRIDE):
    M, h = KEY_SHAPES[k] if kind == "key32" else (0, 0)
    table = None if kind == "key32" else J.make_table(J.TABLE_ROWS, k, 120 + k)
    rows = rows if rows is not None else _plan_rows(kind, k)
    _KEEP.append(rows)
    return J.Case(name, rows, layout, own, par, pb, stride=stride if layout == "strided" else 0, max_len=max_len if layout == "packed" else 0,
                  M=M, hops=h, table=table)


STORES = [pytest.param("key32", "strided", id="key32-strided"), pytest.param("key32", "packed", id="key32-packed"),
          pytest.param("sfptr", "packed", id="sfptr-packed")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairs", [0, 2048, 2049], ids=["plan", "2048-pairs-256-lanes", "2049-pairs-128-lanes"])
@pytest.mark.parametrize("k", [2, 3, 4, 5])
@pytest.mark.parametrize("kind,layout", STORES)
def test_rows_and_ids_equal_the_f32_fill(sp, kind, layout, k, pairs, dtype):
    """rows of 0, 1, 63 .. 65, 127 .. 129, 255 .. 257 and 511 .. 513 members, each with itself, with its neighbour in both orders and with
    the empty row in both orders; the list as it stands (256 lanes), filled up to 2,048 pairs (256 lanes) and to 2,049 (128 lanes)"""
    a, b = (_A, _B) if not pairs else J.fill_up(_A, _B, pairs, len(LENS))
    own, par, pb = J.mirrored(a, b, k % 2 == 0)
    assert not pairs or (J.pair_split(pb) == (2 if pairs == 2048 else 1) and pb == pairs)
    _twice(_case(f"{kind}-{layout}-k{k}-{pairs}", kind, layout, k, own, par, pb), dtype, seg_off=k % 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blocks,given", [(1, False), (1, True), (2, True), (2, False), (3, False)],
                         ids=["one-block-partner-null", "one-block-partner-given", "two-blocks-partner-given", "the-triplet-list", "three-blocks"])
def test_lists_of_one_two_and_three_mirrored_blocks(sp, blocks, given, dtype):
    """`partner` given and NULL; two blocks of pair_block = P with the second block's own rows shared with the first's -- the
    triplet list [U|w ; W|u ; V|w ; W|v] -- and three blocks"""
    P = len(_A) // 3
    if blocks == 2 and not given:          # u, v, w: W stands in both blocks
        u, v, wv = _A[:P], _A[P:2 * P], _B[:P]
        own, par = np.concatenate([u, wv, v, wv]), None
    else:
        own = np.concatenate([np.concatenate([_A[t * P:(t + 1) * P], _B[t * P:(t + 1) * P]]) for t in range(blocks)])
        par = np.concatenate([np.concatenate([_B[t * P:(t + 1) * P], _A[t * P:(t + 1) * P]]) for t in range(blocks)]) if given else None
    for k, kind, layout in ((3, "key32", "strided"), (4, "key32", "packed"), (5, "sfptr", "packed")):
        _twice(_case(f"blocks-{blocks}-{given}-k{k}", kind, layout, k, own, par, P), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_disjoint_nested_and_identical_rows(sp, dtype):
    oids, opairs = J.overlap_rows()
    big = oids[opairs[-1][2]]                                   # nested: every second, every third member of a row of 641, and its head
    nested = [big[::2], big[::3], big[:64], big[-1:]]
    ids = oids + nested + [big]
    a = np.array([p[1] for p in opairs] + list(range(len(oids), len(oids) + len(nested))))
    b = np.array([p[2] for p in opairs] + [len(ids) - 1] * len(nested))
    own, par, pb = J.mirrored(a, b, False)
    for k in (2, 3, 4, 5):
        M, h = KEY_SHAPES[k]
        rows = J.EdgeRows(f"overlap-k{k}", ids, J.key_vals(ids, M, h, False, 130 + k), "key32")
        _twice(_case(f"overlap-key32-k{k}", "key32", "strided", k, own, par, pb, rows=rows, stride=672), dtype)
    rows = J.EdgeRows("overlap-sf", ids, J.sf_vals(ids, 1, J.TABLE_ROWS, 140), "sfptr")
    _twice(_case("overlap-sf-k3", "sfptr", "packed", 3, own, par, pb, rows=rows, max_len=641), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_documented_limits_leave_their_pairs_as_poison(sp, dtype):
    """a packed row above max_len (flags[3] & 1) and a list that is not mirrored (& 4): the pair's rows AND ids stay poison; a row
    number outside the store (& 16): an empty row; an SFptr outside the table (& 2): the table's row 0 twice"""
    lens = J.LENS_SMALL
    ids = J.plan_ids(lens, 5)
    a, b = J.plan_pairs(lens)
    keys = J.EdgeRows("limits-key32", ids, J.key_vals(ids, 200, 3, False, 150), "key32")
    own, par, pb = J.mirrored(a, b, False)
    _twice(_case("row-of-max_len+1", "key32", "packed", 4, own, par, pb, rows=keys, max_len=128), dtype, want_flag=1)
    own, par, pb = J.mirrored(a, b, True)
    par = par.copy()
    broken = int(np.flatnonzero((keys.len[a] >= 63) & (keys.len[b] >= 63) & (a != b))[2])
    par[pb + broken] = (par[pb + broken] + 1) % len(lens)
    _twice(_case("unmirrored-pair", "key32", "strided", 4, own, par, pb, rows=keys, stride=160), dtype, want_flag=4)
    for given in (False, True):
        a2, b2 = a.copy(), b.copy()
        long_ = np.flatnonzero((keys.len[a] >= 63) & (keys.len[b] >= 63) & (a != b))
        a2[long_[0]], b2[long_[1]] = keys.n, -1
        own, par, pb = J.mirrored(a2, b2, given)
        _twice(_case(f"rows-outside-{given}", "key32", "strided", 4, own, par, pb, rows=keys, stride=160), dtype, want_flag=16)
    sf = J.sf_vals(ids, 1, J.TABLE_ROWS, 151)
    sf[4][3], sf[5][10], sf[6][100] = J.TABLE_ROWS, -5, J.TABLE_ROWS + 1000
    own, par, pb = J.mirrored(a, b, False)
    for k in (3, 4):
        _twice(_case(f"sfptr-outside-k{k}", "sfptr", "packed", k, own, par, pb, rows=J.EdgeRows(f"limits-sf-{k}", ids, sf, "sfptr"), max_len=129),
               dtype, want_flag=2)

"""GPU (MI355X): the LP encoder's LSTM first stage on the on-demand step -- the index form over strided key rows
(subgacc_sjoin_key_index) against a NumPy restatement, sample_and_index against the row form of the same step and against gather_index
over the all-nodes store, one result whatever the route, too many distinct LP rows, and sample_and_lstm_stage against the float64
reference form.  Pairs, pointers, lengths and table rows are compared bit for bit; the model stage with the bounds
tests/test_gpu_lstm_aggr.py uses for the same recurrent kernel (forward 2e-5 of the reference's largest entry, every parameter gradient
5e-4 of that gradient's largest entry)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import sp, sym_graph  # noqa: F401
from test_gpu_horder import M, World
from test_gpu_lstm_aggr import _nets, _reference_style_lstm
from test_gpu_step_stage import HOPS, LENS, Rows, _columns, _lp_keys

pytestmark = pytest.mark.gpu

GUARD = 64                  # poisoned rows behind the R rows of out_idx
POISON = -0x5A5A5A5A


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------- the kernel alone
def _want_pairs(rows, ukeys, a, b):
    """NumPy restatement of the index form: own = [a | b], partner = [b | a]; row seg[j] + t = (column of member t's key, column of the
    key of the partner row's member with the same id or 0); a key outside `ukeys` reads as column 0"""
    col = {int(k): i + 1 for i, k in enumerate(ukeys)}
    own, par = np.concatenate([a, b]), np.concatenate([b, a])
    out = []
    for ra, rb in zip(own, par):
        pos = {int(v): t for t, v in enumerate(rows.ids[rb, : rows.len[rb]])}
        for t in range(rows.len[ra]):
            hit = pos.get(int(rows.ids[ra, t]))
            out.append((col.get(int(rows.keys[ra, t]), 0), 0 if hit is None else col.get(int(rows.keys[rb, hit]), 0)))
    lens = rows.len[own]
    return np.array(out, dtype=np.int32).reshape(-1, 2), lens, np.concatenate([[0], np.cumsum(lens.astype(np.int64))])


def _key_index(rows, ukeys, count, T, a, b, partner=False, want_len=True):
    """subgacc_sjoin_sizes_rows, then subgacc_sjoin_key_index over `rows` -> (out_idx [R, 2], out_len [S], seg [S+1], flags), every
    output with a poisoned guard behind it that must come back untouched"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    ids, keys, nsize = rows.device()
    own = torch.from_numpy(np.concatenate([a, b])).cuda()
    par = torch.from_numpy(np.concatenate([b, a])).cuda() if partner else None
    S = own.numel()
    seg = torch.full((S + 1 + GUARD,), -7, dtype=torch.int64, device="cuda")
    olen = torch.full((S + GUARD,), -7, dtype=torch.int32, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device="cuda")
    _lib.check(L.subgacc_sjoin_sizes_rows(_lib.ptr(nsize), rows.n, _lib.ptr(own), _lib.ptr(par), S, _lib.ptr(seg), _lib.ptr(flags),
                                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    R = int(seg[S])
    assert R == int(rows.len[np.concatenate([a, b])].sum())        # the guard below stands where the restatement says the rows end
    out = torch.full((R + GUARD, 2), POISON, dtype=torch.int32, device="cuda")
    d = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY32, row_len=nsize, n_rows=rows.n, row_stride=rows.stride, ids=ids, payload=keys,
                       own=own, partner=par, S=S, pair_block=S // 2, table_rows=T, num_walks=M, num_steps=HOPS, flags=flags)
    _lib.check(L.subgacc_sjoin_key_index(C.byref(d), _lib.ptr(ukeys), _lib.ptr(count), _lib.ptr(seg), _lib.ptr(out),
                                         _lib.ptr(olen) if want_len else None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out[R:] == POISON).all()) and bool((seg[S + 1:] == -7).all()) and bool((olen[S:] == -7).all())
    if not want_len:
        assert bool((olen == -7).all())
    return out[:R].cpu().numpy(), olen[:S].cpu().numpy(), seg[: S + 1].cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("nkeys,T", [pytest.param(1, 2, id="one-key"), pytest.param(15, 16, id="T-1-keys"),
                                     pytest.param(299, 300, id="299-keys"), pytest.param(700, 1030, id="700-keys-T1030")])
def test_index_pairs_equal_their_numpy_restatement(sp, nkeys, T):
    """row lengths 0, 1, NT-1, NT, NT+1, 2 NT-1, 2 NT, 2 NT+1 and a row that fills row_stride; every row with itself and with its
    neighbour, disjoint ids, full overlap (rows of equal length: either may be staged), empty rows; with and without the partner list,
    with and without out_len; the list turned round (b, a) gives the same rows"""
    assert LENS == (0, 1, 255, 256, 257, 511, 512, 513, 544)
    rows = Rows(_lp_keys(nkeys, 11 + nkeys), seed=nkeys)
    assert rows.stride == 544
    present = rows.present()
    ukeys, count, feat, flags = _columns(sp, rows, T)
    assert int(count) == nkeys and not flags.any()
    want, want_len, want_seg = _want_pairs(rows, present, rows.a, rows.b)
    assert want.shape[0] == want_seg[-1] and want[:, 0].min() >= 1 and want.max() <= nkeys
    assert (want[:, 1] == 0).any() and (want[:, 1] > 0).any()
    for partner in (False, True):
        out, olen, seg, fl = _key_index(rows, ukeys, count, T, rows.a, rows.b, partner=partner)
        assert not fl.any()
        assert np.array_equal(seg, want_seg) and np.array_equal(olen, want_len) and np.array_equal(out, want)
    out, _, _, _ = _key_index(rows, ukeys, count, T, rows.a, rows.b, want_len=False)        # out_len is optional
    assert np.array_equal(out, want)
    # (b, a): segment j of this list is segment j +- P of the other -- the same rows, whichever row of a pair is S and which T
    P = len(rows.a)
    out_r, olen_r, seg_r, fl = _key_index(rows, ukeys, count, T, rows.b, rows.a)
    assert not fl.any() and np.array_equal(olen_r, np.concatenate([want_len[P:], want_len[:P]]))
    half = int(want_seg[P])
    assert np.array_equal(out_r, np.concatenate([want[half:], want[:half]]))
    # out_feat[out_idx[r]] is the row of the row form: own key unpacked, partner key unpacked or the zero row
    f = feat.cpu().numpy()
    assert not f[0].any()
    own = np.concatenate([rows.a, rows.b])
    keys_in_order = np.concatenate([rows.keys[r, : rows.len[r]] for r in own])
    assert np.array_equal(present[want[:, 0] - 1], keys_in_order)


def test_a_key_that_is_not_in_the_list(sp):
    """ukeys / n_keys without one key that the rows carry: column 0 in exactly the slots that carry it, flags[3] & 2, guards untouched"""
    nkeys, T = 40, 64
    rows = Rows(_lp_keys(nkeys, 3), seed=5)
    present = rows.present()
    gone = present[nkeys // 2]
    kept = np.delete(present, nkeys // 2)
    ukeys = torch.zeros(T - 1, dtype=torch.int32, device="cuda")
    ukeys[: nkeys - 1] = torch.from_numpy(kept.view(np.int32)).cuda()
    count = torch.tensor([nkeys - 1], dtype=torch.int64, device="cuda")
    want, want_len, want_seg = _want_pairs(rows, kept, rows.a, rows.b)
    full, _, _ = _want_pairs(rows, present, rows.a, rows.b)
    col = nkeys // 2 + 1                                    # the column the key has in the full list
    assert (full[:, 0] == col).any() and (full[:, 1] == col).any()
    out, olen, seg, fl = _key_index(rows, ukeys, count, T, rows.a, rows.b)
    assert int(fl[3]) & 2 and not int(fl[3]) & ~2
    assert np.array_equal(out, want) and np.array_equal(olen, want_len) and np.array_equal(seg, want_seg)
    assert np.array_equal(out[:, 0] == 0, full[:, 0] == col)
    assert np.array_equal(out[:, 1] == 0, (full[:, 1] == col) | (full[:, 1] == 0))
    assert gone not in kept


# ------------------------------------------------------------------------------------------------------ the step against the row form
@pytest.mark.parametrize("hops", [2, 3])
def test_the_step_equals_the_row_form_and_the_store(sp, world, hops):
    """table[pairs] is the xz of sample_and_gather over the same seed, bit for bit, indptr its indptr; the same against
    encode[gather_index(edge, store)] over the all-nodes store.  The batch holds (u, u) pairs, repeated endpoints, the isolated root,
    the hubs and every star centre."""
    csr = world.csr
    kw = dict(num_walks=M, num_steps=hops, seed=5)
    e = world.pairs(64, 1)
    en = e.cpu().numpy()
    assert (en[0] == en[1]).any() and len(np.unique(en)) < en.size
    xz, ind, _ = sp.sample_and_gather(csr, e, **kw)
    pairs, indptr, table, sets = sp.sample_and_index(csr, e, **kw)
    R = int(ind[-1])
    assert pairs.dtype == torch.int32 and pairs.shape == (R, 2) and indptr.dtype == torch.int64 and table.shape[1] == hops + 1
    assert torch.equal(indptr, ind)
    assert int(pairs[:, 0].min()) >= 1 and int(pairs.max()) == table.shape[0] - 1 and not bool(table[0].any())
    assert torch.equal(_bits(table[pairs.long()]), _bits(xz))
    z, enc, lens = world.store(hops)
    p_store, ind_store = sp.gather_index(e, z)
    assert torch.equal(ind_store, indptr)
    assert torch.equal(_bits(enc.cuda().float()[p_store.long()]), _bits(table[pairs.long()]))
    # with table_rows: the same pairs, the rows past the batch's distinct LP rows zero
    c = table.shape[0] - 1
    p2, i2, t2, _ = sp.sample_and_index(csr, e, table_rows=c + 40, **kw)
    assert torch.equal(p2, pairs) and torch.equal(i2, indptr) and torch.equal(t2[: c + 1], table) and not bool(t2[c + 1:].any())


# ------------------------------------------------------------------------------------------------------ one result whatever the route
def _result(got):
    pairs, indptr, table = got[:3]
    return pairs[: int(indptr[-1])], indptr, table


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y)
               for x, y in zip(_result(a), _result(b)))


def test_one_result_whatever_the_route(sp, world):
    csr, B, T = world.csr, 64, 512
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    want1 = sp.sample_and_index(csr, e1, table_rows=T, **kw)
    want2 = sp.sample_and_index(csr, e2, table_rows=T, **kw)
    assert not _same(want1, want2)
    assert _same(sp.sample_and_index(csr, e1, table_rows=T, **kw), want1)                       # two runs
    assert _same(sp.sample_and_index(csr, e1, table_rows=T, dedup_roots=True, **kw), want1)
    order = sp.locality_order(csr)
    assert _same(sp.sample_and_index(csr, e1, table_rows=T, order=order, **kw), want1)
    for dedup, ordr in ((False, None), (True, None), (False, order), (True, order)):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=dedup, order=ordr, stage="index", table_rows=T)
        assert bufs.out is None and bufs.segid is None and bufs.counts is None
        assert bufs.pairs.shape == (2 * B * (M * HOPS + 1), 2) and bufs.pairs.dtype == torch.int32
        for e, want in ((e1, want1), (e2, want2), (e1, want1)):             # a second step on the same buffers gives ITS batch
            got = sp.sample_and_index(csr, e, buffers=bufs, dedup_roots=dedup, order=ordr, **kw)
            assert got[0].data_ptr() == bufs.pairs.data_ptr() and got[0].shape == bufs.pairs.shape
            assert got[1].data_ptr() == bufs.seg.data_ptr() and got[2].data_ptr() == bufs.feat.data_ptr()
            assert bufs.sets is got[3]
            got[3].prefetch().resolve()
            assert _same(got, want)


# ------------------------------------------------------------------------------------------------------ too many distinct rows
def test_more_distinct_rows_than_table_rows(sp, world):
    """table_rows = 8 for a batch with hundreds of distinct LP rows: sets.resolve() raises and names table_rows; every pair stays
    inside the table, and the rows of the pair buffer past indptr[-1] keep the poison written before the step"""
    from surel_plus_amd import _lib
    csr, B, T = world.csr, 64, 8
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e = world.pairs(B, 1)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="index", table_rows=T)
    bufs.pairs.fill_(POISON)
    pairs, indptr, table, sets = sp.sample_and_index(csr, e, buffers=bufs, **kw)
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        sets.resolve()
    R = int(indptr[-1])
    assert 0 < R < pairs.shape[0] and table.shape == (T, HOPS + 1)
    assert torch.equal(indptr, sp.sample_and_gather(csr, e, **kw)[1])
    assert int(pairs[:R].min()) >= 0 and int(pairs[:R].max()) <= T - 1
    assert bool((pairs[R:] == POISON).all())
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        sp.sample_and_index(csr, e, table_rows=T, **kw)
    x = sp.sample_and_lstm_stage(csr, e, *_nets(torch.float32, k=HOPS + 1), buffers=bufs, **kw)
    assert x.shape == (2, B, 16)
    with pytest.raises(_lib.SubgAccError, match="table_rows"):      # the stage returns the tensor alone: the step is checked here
        bufs.sets.resolve()


# ------------------------------------------------------------------------------------------------------------------ the stage
# The stage tests' step: 40 pairs on a 600-node graph, 3 hops.  The walks: the 16 of tests/test_gpu_lstm_aggr.py's scale have no key-rows
# form (the fused-row kernel writes key rows from a 512-slot table on: M * hops + 1 >= 205), and the step refuses such a shape before any
# device work -- so M = 68, the smallest M that has 32-bit key rows at 3 hops.  Longer segments than M = 16 would give: the bounds stay.
SM, SHOPS, SB = 68, 3, 40


class Small:
    def __init__(self, sp):
        ptr_, idx = sym_graph(600, 2400, seed=3, hubs=1)
        self.csr = sp.DeviceCSR(ptr_, idx)
        e = np.random.default_rng(4).integers(0, 600, (2, SB))
        e[:, 0] = (7, 7)                    # a (u, u) pair
        e[:, 1] = e[:, 2]                   # a repeated pair
        e[0, 3] = e[0, 4]                   # a repeated endpoint
        self.e = torch.from_numpy(e).cuda()
        self.kw = dict(num_walks=SM, num_steps=SHOPS, seed=5)


@pytest.fixture(scope="module")
def small(sp):
    return Small(sp)


@pytest.mark.parametrize("H,H2,bias", [pytest.param(16, 16, True, id="16-16"), pytest.param(24, 32, False, id="24-32-nobias")])
def test_stage_trains_like_the_float64_reference_form(sp, small, H, H2, bias):
    """sample_and_lstm_stage against to_dense_batch -> nn.LSTM -> last position in float64 on the (xz, indptr) of sample_and_gather
    for the same seed: forward within 2e-5 of the reference's largest entry, every parameter gradient within 5e-4 of that gradient's
    largest entry; every parameter has a gradient"""
    fa, f64 = _nets(torch.float32, H, H2, bias, SHOPS + 1), _nets(torch.float64, H, H2, bias, SHOPS + 1)
    fused = sp.sample_and_lstm_stage(small.csr, small.e, *fa, **small.kw)
    assert fused.shape == (2, SB, H2) and fused.dtype == torch.float32
    xz, ind, _ = sp.sample_and_gather(small.csr, small.e, **small.kw)
    assert int((ind[1:] - ind[:-1]).max()) > int((ind[1:] - ind[:-1]).min())          # the padding is exercised
    truth = _reference_style_lstm(xz.double(), ind, *f64).view(2, -1, H2)
    scale = float(truth.detach().abs().max())
    err = float((fused.detach().double() - truth.detach()).abs().max())
    print(f"forward: max error {err:.3e}, bound {2e-5 * scale:.3e}")
    assert err <= 2e-5 * scale
    torch.manual_seed(2)
    w = torch.randn(2, SB, H2, device="cuda")
    (fused * w).sum().backward()
    (truth * w.double()).sum().backward()
    named = lambda mods: [(n, p) for mod in mods for n, p in mod.named_parameters()]      # noqa: E731
    assert len(named(fa)) == (8 if bias else 6)
    for (n, pa), (_, pc) in zip(named(fa), named(f64)):
        assert pa.grad is not None, n
        gs = float(pc.grad.abs().max())
        gerr = float((pa.grad.double() - pc.grad).abs().max())
        print(f"grad {n}: max error {gerr:.3e}, bound {5e-4 * max(gs, 1e-6):.3e}")
        assert gerr <= 5e-4 * max(gs, 1e-6), n
    with torch.no_grad():
        nog = sp.sample_and_lstm_stage(small.csr, small.e, *_nets(torch.float32, H, H2, bias, SHOPS + 1), **small.kw)
    assert torch.equal(nog, fused.detach())                 # with or without the state for the backward: the same bits


def _run(sp, small, e, w, **route):
    """(output, gradients) of the stage with fresh nets of one seed"""
    nets = _nets(torch.float32, 16, 16, True, SHOPS + 1)
    out = sp.sample_and_lstm_stage(small.csr, e, *nets, **small.kw, **route)
    (out * w).sum().backward()
    return out.detach().clone(), [p.grad.clone() for mod in nets for p in mod.parameters()]


def test_the_stage_gives_the_same_bits_whatever_the_route(sp, small):
    """two runs; buffers / no buffers / dedup_roots / order= (the same table_rows throughout: the GEMMs behind the kernel keep their
    shape); a permuted batch gives the permuted output"""
    csr, e, T = small.csr, small.e, 256
    torch.manual_seed(3)
    w = torch.randn(2, SB, 16, device="cuda")
    out, grads = _run(sp, small, e, w, table_rows=T)
    assert bool(out.abs().sum() > 0) and all(bool(g.abs().sum() > 0) for g in grads)
    order = sp.locality_order(csr)
    routes = [dict(table_rows=T), dict(table_rows=T, dedup_roots=True), dict(table_rows=T, order=order)]
    for dedup, ordr in ((False, None), (True, None), (False, order), (True, order)):
        bufs = sp.StepBuffers(csr, SB, num_walks=SM, num_steps=SHOPS, dedup_roots=dedup, order=ordr, stage="index", table_rows=T)
        routes += [dict(buffers=bufs, dedup_roots=dedup, order=ordr)] * 2               # and the buffers used again
    for route in routes:
        o, g = _run(sp, small, e, w, **route)
        assert torch.equal(o, out), route
        assert all(torch.equal(x, y) for x, y in zip(g, grads)), route
    perm = torch.from_numpy(np.random.default_rng(6).permutation(SB)).cuda()
    o, _ = _run(sp, small, e[:, perm], w, table_rows=T)
    assert torch.equal(o, out[:, perm])


def test_a_backward_behind_the_buffers_next_step_is_refused(sp, small):
    csr, e = small.csr, small.e
    bufs = sp.StepBuffers(csr, SB, num_walks=SM, num_steps=SHOPS, stage="index", table_rows=256)
    nets = _nets(torch.float32, 16, 16, True, SHOPS + 1)
    first = sp.sample_and_lstm_stage(csr, e, *nets, buffers=bufs, **small.kw)
    second = sp.sample_and_lstm_stage(csr, e.flip(1), *nets, buffers=bufs, **small.kw)
    with pytest.raises(RuntimeError, match="step 1 .* step 2"):
        first.sum().backward()
    second.sum().backward()                 # the step the buffers hold still trains
    assert all(p.grad is not None for mod in nets for p in mod.parameters())

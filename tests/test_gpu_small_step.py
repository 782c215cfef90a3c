"""GPU (MI355X): the row-form on-demand step at the small walk shapes -- StepBuffers / sample_and_gather / sample_and_hgather with
small_rows=True: the key rows of the one-wave kernel (subgacc_walk_keyrows_small) under the KEY32 row join, and in 16 bits with
segment ids (subgacc_sjoin_fill_half_ids).  Every reference is code this route does not run: the same step without the keyword (the
general kernel's table form, subgacc_unpack_lp and the SFPTR join), the f32 step followed by torch's .to(dtype), or the oracle.
Everything is compared bit for bit."""
import functools

import numpy as np
import pytest
import torch

import walk_rows_edges as W
import walk_small_edges as S
from gpu_helpers import _oracle_spg, sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 13
# one shape per table size and hop count that can differ: k = 2, 3, 4, 5
SHAPES = ((50, 1), (203, 1), (25, 2), (101, 2), (67, 3), (12, 4), (50, 4))
ONE_PER_K = ((203, 1), (101, 2), (67, 3), (50, 4))
BATCHES = (3, 64, 2049)          # pairs: both sides of pair_split and of the 256-lane rule (2,048 pairs)
DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]


@functools.lru_cache(maxsize=2)
def _csr(M, m):
    from surel_plus_amd.sampler import DeviceCSR
    g = S.graph("edge", M, m)
    return DeviceCSR(g["indptr"], g["indices"])


def _roots(M, m):
    """the roots of the shape's edge graph, and one of them without out-edges"""
    g = S.graph("edge", M, m)
    roots = np.unique(g["batch"]).astype(np.int64)
    lone = roots[W.out_degree(g, roots) == 0]
    assert len(lone) and len(roots) > 8
    return roots, int(lone[0])


def _pairs(M, m, B, seed=1):
    """[2, B] pairs of the graph's roots with a pair (u, u), a root of degree 0 and a repeated endpoint"""
    roots, lone = _roots(M, m)
    e = roots[np.random.default_rng(seed).integers(0, len(roots), (2, B))]
    a, b, c = (int(r) for r in roots[roots != lone][:3])
    e[:, 0], e[:, 1], e[:, 2] = (a, a), (lone, b), (b, c)
    return torch.from_numpy(e).cuda()


def _triplets(M, m, B, seed=2):
    """[3, B] triplets with u == v, u == w, a root of degree 0 and a repeated node"""
    roots, lone = _roots(M, m)
    h = roots[np.random.default_rng(seed).integers(0, len(roots), (3, B))]
    a, b, c = (int(r) for r in roots[roots != lone][:3])
    h[:, 0], h[:, 1], h[:, 2] = (a, a, b), (b, c, b), (lone, c, a)
    return torch.from_numpy(h).cuda()


def _step(sp, csr, e, bufs, **kw):
    """one buffered step, resolved -> (xz [R, 2, k], indptr or ids, sets, R)"""
    xz, ind, sets = sp.sample_and_gather(csr, e, buffers=bufs, **kw)
    sets.resolve()
    seg = ind if bufs.ptr else ind.seg_pointers
    R = int(seg[-1].item())
    return xz[:R].clone(), (ind.clone() if bufs.ptr else ind[:R].clone()), sets, R


def _members(bufs):
    """the ids of every row's members, row after row"""
    ns = bufs.nsize.cpu().numpy()
    ids = bufs.ids.cpu().numpy().reshape(bufs.n, bufs.stride)
    return ns, ids[np.arange(bufs.stride)[None, :] < ns[:, None]]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------ 1. against the table-form route
@pytest.mark.parametrize("rng", ["philox", "rand_r"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("M,m", SHAPES)
def test_the_step_equals_the_table_form_step(sp, M, m, B, rng):
    csr, e = _csr(M, m), _pairs(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, rng=rng)
    old = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, rng=rng)
    new = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, rng=rng, small_rows=True)
    assert not old.small and not old.keyrows and old.table is not None
    assert new.small and new.keyrows and not new.key64 and new.table is None and new.feat is None and new.slot.dtype == torch.int32
    for _ in range(2):                                  # and the buffers used again
        rxz, rind, rsets, R = _step(sp, csr, e, old, **kw)
        xz, ind, sets, R2 = _step(sp, csr, e, new, small_rows=True, **kw)
        assert R == R2 > 0 and torch.equal(ind, rind) and torch.equal(xz.view(torch.int32), rxz.view(torch.int32))
        assert sets.keyrows and sets.small_rows and not sets.key64
    (ns, ids), (rns, rids) = _members(new), _members(old)
    assert np.array_equal(ns, rns) and np.array_equal(ids, rids) and int(ns.min()) == 1
    assert new.walk_order == "batch"


def test_the_step_equals_the_oracle(sp):
    """(100, 2), mag's and DBLP-coauthor's shape, on a graph of 600 nodes: the oracle's sets of the 2B endpoints, joined in NumPy"""
    import oracle
    M, m, B = 100, 2, 40
    ptr_h, idx_h = sym_graph(600, 2400, seed=3, hubs=1)
    csr = sp.DeviceCSR(ptr_h, idx_h)
    e = np.random.default_rng(4).integers(0, 600, (2, B))
    e[:, 0], e[:, 1], e[0, 3] = (7, 7), e[:, 2], e[0, 4]
    spg, enc = _oracle_spg(ptr_h, idx_h, e.reshape(-1), M, m, 5, "philox")
    zsf = oracle.enc_table(enc).astype(np.float32) / np.float32(M)
    oxz, oind = oracle.gather_numpy(np.arange(2 * B).reshape(2, B), spg, ptr=True, encode=zsf)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True)
    xz, ind, _, R = _step(sp, csr, torch.from_numpy(e).cuda(), bufs, num_walks=M, num_steps=m, seed=5, small_rows=True)
    assert np.array_equal(ind.cpu().numpy(), oind) and np.array_equal(xz.cpu().numpy().view(np.int32), oxz.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ 2. root dedup
@pytest.mark.parametrize("M,m", [(100, 2), (50, 1), (50, 4)])
def test_root_dedup_on_an_evaluation_batch(sp, M, m):
    """one source against 63 targets (utils.py:92-95), two of them the same node and one the source itself"""
    csr, B = _csr(M, m), 64
    roots, lone = _roots(M, m)
    t = roots[np.random.default_rng(3).permutation(len(roots))[:B]]
    t[1], t[2], t[3] = t[0], lone, roots[5]
    e = torch.from_numpy(np.stack([np.full(B, roots[5]), t])).cuda()
    distinct = len(np.unique(e.cpu().numpy()))
    kw = dict(num_walks=M, num_steps=m, seed=SEED)
    with pytest.raises(ValueError, match="fused-row walk kernel"):          # without the keyword: refused as ever
        sp.StepBuffers(csr, B, num_walks=M, num_steps=m, dedup_roots=True)
    plain = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True)
    dd = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, dedup_roots=True)
    rxz, rind, _, R = _step(sp, csr, e, plain, small_rows=True, **kw)
    for _ in range(2):
        xz, ind, sets, R2 = _step(sp, csr, e, dd, small_rows=True, dedup_roots=True, **kw)
        assert R2 == R and torch.equal(ind, rind) and torch.equal(xz.view(torch.int32), rxz.view(torch.int32))
        assert sets.n_distinct == distinct < 2 * B
    assert int((dd.nsize > 0).sum().item()) == distinct


# ------------------------------------------------------------------------------------------------------------- 3. the walk's order
@pytest.mark.parametrize("M,m", [(100, 2), (203, 1)])
def test_order_and_sort_roots_change_nothing(sp, M, m, monkeypatch):
    from surel_plus_amd import spjoin
    csr, B = _csr(M, m), 64
    e = _pairs(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, small_rows=True)
    rxz, rind, _, R = _step(sp, csr, e, sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, sort_roots=False), **kw)
    order = sp.locality_order(csr)
    for dedup in (False, True):
        ranked = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, order=order, dedup_roots=dedup)
        xz, ind, sets, _ = _step(sp, csr, e, ranked, dedup_roots=dedup, order=order, **kw)
        assert ranked.walk_order == sets.walk_order == "rank"
        assert torch.equal(ind, rind) and torch.equal(xz.view(torch.int32), rxz.view(torch.int32))
    monkeypatch.setattr(spjoin, "SORT_ROOTS_MIN", 2 * B)        # the batch is as large as the threshold: the rows are taken by root id
    by_id = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True)
    xz, ind, sets, _ = _step(sp, csr, e, by_id, **kw)
    assert by_id.walk_order == sets.walk_order == "id"
    assert torch.equal(ind, rind) and torch.equal(xz.view(torch.int32), rxz.view(torch.int32))


# ----------------------------------------------------------------------------------------------------- 4. segment ids, many batches
@pytest.mark.parametrize("B", [3, 2049])
@pytest.mark.parametrize("M,m", ONE_PER_K)
def test_segment_ids_equal_the_table_form_steps(sp, M, m, B):
    csr, e = _csr(M, m), _pairs(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, ptr=False)
    old = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, ptr=False)
    rxz, rids, _, R = _step(sp, csr, e, old, **kw)
    new = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, ptr=False, small_rows=True)
    xz, ids, _, R2 = _step(sp, csr, e, new, small_rows=True, **kw)
    assert R == R2 and ids.dtype == torch.int64 and torch.equal(ids, rids) and torch.equal(xz.view(torch.int32), rxz.view(torch.int32))
    raw = sp.sample_and_gather(csr, e, buffers=new, small_rows=True, **kw)[1]
    assert raw.seg_pointers.data_ptr() == new.seg.data_ptr() and torch.equal(new.seg, old.seg)
    want = torch.repeat_interleave(torch.arange(2 * B, device="cuda"), new.seg[1:] - new.seg[:-1])
    assert torch.equal(ids, want)


@pytest.mark.parametrize("M,m", [(100, 2), (50, 1)])
def test_many_batches_per_step(sp, M, m):
    """batch=: [nb, 2, b] pairs in one step equal split_batches of the table-form step"""
    csr, nb, b = _csr(M, m), 4, 16
    e = _pairs(M, m, nb * b).view(2, nb, b).permute(1, 0, 2).contiguous()
    kw = dict(num_walks=M, num_steps=m, seed=SEED)
    old = sp.StepBuffers(csr, nb * b, num_walks=M, num_steps=m, batch=b)
    new = sp.StepBuffers(csr, nb * b, num_walks=M, num_steps=m, batch=b, small_rows=True)
    rxz, rind, rsets = sp.sample_and_gather(csr, e, buffers=old, **kw)
    xz, ind, sets = sp.sample_and_gather(csr, e, buffers=new, small_rows=True, **kw)
    rsets.resolve(), sets.resolve()
    assert torch.equal(ind, rind)
    want, got = sp.split_batches(rxz, rind, b), sp.split_batches(xz, ind, b)
    assert len(want) == len(got) == nb
    for (wx, wi), (gx, gi) in zip(want, got):
        assert torch.equal(wi, gi) and torch.equal(wx.view(torch.int32), gx.view(torch.int32)) and wx.shape[0] > 0


# ------------------------------------------------------------------------------------------------------------------ 5. triplets
@pytest.mark.parametrize("dedup", [False, True], ids=["all-roots", "dedup-roots"])
@pytest.mark.parametrize("B", [24, 2049])
def test_triplets_equal_the_table_form_step(sp, B, dedup):
    M, m = 100, 2
    csr, h = _csr(M, m), _triplets(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED)
    rxz, rids, rsets = sp.sample_and_hgather(csr, h, buffers=sp.StepBuffers(csr, B, num_walks=M, num_steps=m, triplets=True), **kw)
    rsets.resolve()
    R = int(rids.seg_pointers[-1].item())
    new = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, triplets=True, small_rows=True, dedup_roots=dedup)
    assert new.small and new.keyrows and new.table is None and new.S == 4 * B
    for _ in range(2):
        xz, ids, sets = sp.sample_and_hgather(csr, h, buffers=new, small_rows=True, dedup_roots=dedup, **kw)
        sets.resolve()
        assert torch.equal(ids.seg_pointers, rids.seg_pointers) and torch.equal(ids[:R], rids[:R])
        assert torch.equal(xz[:R].view(torch.int32), rxz[:R].view(torch.int32))
    with pytest.raises(ValueError, match="small_rows"):
        sp.sample_and_hgather(csr, h, buffers=new, dedup_roots=dedup, **kw)


# ----------------------------------------------------------------------------------------------------------- 6. without buffers
@pytest.mark.parametrize("M,m", [(100, 2), (50, 1)])
def test_the_calls_without_buffers_equal_the_buffered_step(sp, M, m):
    csr, B = _csr(M, m), 64
    e, h = _pairs(M, m, B), _triplets(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, small_rows=True)
    for how in (dict(), dict(dedup_roots=True), dict(ptr=False), dict(rng="rand_r")):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, **how)
        rxz, rind, _, R = _step(sp, csr, e, bufs, **how, **kw)
        xz, ind, sets = sp.sample_and_gather(csr, e, **how, **kw)
        assert not sets.pending and xz.shape == (R, 2, m + 1) and torch.equal(ind, rind), how
        assert torch.equal(xz.view(torch.int32), rxz.view(torch.int32)), how
        if how.get("ptr") is False:
            assert torch.equal(ind.seg_pointers, bufs.seg)
    for dedup in (False, True):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, triplets=True, dedup_roots=dedup)
        rxz, rids, rsets = sp.sample_and_hgather(csr, h, buffers=bufs, dedup_roots=dedup, **kw)
        rsets.resolve()
        R = int(rids.seg_pointers[-1].item())
        xz, ids, sets = sp.sample_and_hgather(csr, h, dedup_roots=dedup, **kw)
        assert xz.shape == (R, 2, m + 1) and torch.equal(ids, rids[:R]) and torch.equal(ids.seg_pointers, rids.seg_pointers)
        assert torch.equal(xz.view(torch.int32), rxz[:R].view(torch.int32))
    out = torch.full((2 * B * (M * m + 1) * 2 * (m + 1) + 8,), -3.0, device="cuda")
    oxz, oind, _ = sp.sample_and_gather(csr, e, out=out, **kw)
    assert oxz.data_ptr() == out.data_ptr() and bool((out[oxz.numel():] == -3.0).all())


# ------------------------------------------------------------------------------------------------------------------ 7. 16-bit rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("M,m", ONE_PER_K)
def test_half_rows_equal_the_f32_step_rounded(sp, M, m, B, dtype):
    """pairs with pointers (subgacc_sjoin_fill_half) and with segment ids (subgacc_sjoin_fill_half_ids): xz bit for bit the f32 step's
    .to(dtype), indptr and ids equal; out= of the 16-bit type is the buffer written"""
    csr, e = _csr(M, m), _pairs(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, small_rows=True)
    for ptr in (True, False):
        rxz, rind, _, R = _step(sp, csr, e, sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, ptr=ptr), ptr=ptr, **kw)
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, small_rows=True, ptr=ptr, dtype=dtype)
        assert bufs.out.dtype == dtype and bufs.small and (ptr or bufs.segid.dtype == torch.int64)
        for _ in range(2):
            xz, ind, _, R2 = _step(sp, csr, e, bufs, ptr=ptr, dtype=dtype, **kw)
            assert R2 == R and xz.dtype == dtype and torch.equal(ind, rind) and _same_bits(xz, rxz.to(dtype)), ptr
    worst = 2 * B * (M * m + 1) * 2 * (m + 1)
    out = torch.full((worst + 16,), -3.0, dtype=dtype, device="cuda")
    oxz, oids, sets = sp.sample_and_gather(csr, e, buffers=bufs, out=out, ptr=False, dtype=dtype, **kw)
    sets.resolve()
    assert oxz.data_ptr() == out.data_ptr() and _same_bits(oxz[:R], rxz.to(dtype)) and torch.equal(oids[:R], rind)
    assert bool((out[R * 2 * (m + 1):] == -3.0).all())
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, e, buffers=bufs, ptr=False, **kw)


@pytest.mark.parametrize("dedup", [False, True], ids=["all-roots", "dedup-roots"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [24, 2049])
def test_half_rows_of_triplets(sp, B, dtype, dedup):
    M, m = 100, 2
    csr, h = _csr(M, m), _triplets(M, m, B)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, small_rows=True, dedup_roots=dedup)
    rxz, rids, rsets = sp.sample_and_hgather(csr, h, buffers=sp.StepBuffers(csr, B, num_walks=M, num_steps=m, triplets=True,
                                                                           small_rows=True, dedup_roots=dedup), **kw)
    rsets.resolve()
    R = int(rids.seg_pointers[-1].item())
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, triplets=True, small_rows=True, dedup_roots=dedup, dtype=dtype)
    xz, ids, sets = sp.sample_and_hgather(csr, h, buffers=bufs, dtype=dtype, **kw)
    sets.resolve()
    assert xz.dtype == dtype and ids.dtype == torch.int64 and torch.equal(ids.seg_pointers, rids.seg_pointers)
    assert torch.equal(ids[:R], rids[:R]) and _same_bits(xz[:R], rxz[:R].to(dtype))
    if B == 24:
        uxz, uids, _ = sp.sample_and_hgather(csr, h, dtype=dtype, **kw)
        assert torch.equal(uids, rids[:R]) and _same_bits(uxz, rxz[:R].to(dtype))

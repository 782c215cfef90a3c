"""GPU (MI355X): the LP encoder's attentional first stage on the on-demand step -- the attentional count form over strided key rows
(subgacc_sjoin_key_counts_attn / _backward) bit for bit against the kernel over a packed SFptr store (subgacc_sjoin_counts_attn /
_backward, code this file's subject does not touch) and against a float64 restatement, its flags and clamps, sample_and_attn_counts
against the all-nodes store, sample_and_attn_stage as one result whatever the route, against the reference form, and at its edges."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import _reference_style_attn, sp  # noqa: F401
from test_gpu_counts_attn import FWD_TOL, GRAD_FLOOR, GRAD_TOL
from test_gpu_horder import M, World
from test_gpu_step_stage import HOPS, LENS, STRIDE, Rows, _guarded, _lp_keys

pytestmark = pytest.mark.gpu

FILL = -7.0


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


# ----------------------------------------------------------------------------------------------------------- the kernels alone
def _lists(rows, blocks):
    """own = [a | b] (| [b | a]: a second mirrored block with the endpoints swapped), partner = its mirror"""
    a, b = rows.a, rows.b
    own = [a, b] if blocks == 1 else [a, b, b, a]
    par = [b, a] if blocks == 1 else [b, a, a, b]
    return np.concatenate(own), np.concatenate(par), len(a)


def _key_attn(rows, ukeys, count, T, g, dW=None, partner=True, blocks=1, want_len=True, lists=None, keep=True):
    """subgacc_sjoin_key_counts_attn (and its backward on dW) over `rows`; every output has GUARD words behind it that must stay
    untouched -> dict of W, max, den, len, Dg (device tensors) and flags"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    ids, keys, nsize = rows.device()
    own_h, par_h, P = _lists(rows, blocks) if lists is None else lists
    own = torch.from_numpy(own_h).cuda()
    par = torch.from_numpy(par_h).cuda() if partner else None
    S = own.numel()
    W, mx, den = _guarded(S * T, torch.float32, FILL), _guarded(S, torch.float32, FILL), _guarded(S, torch.float32, FILL)
    olen = _guarded(S, torch.int32, -7)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _lib.join_desc(_lib.JOIN_COUNTS, _lib.JOIN_KEY32, row_len=nsize, n_rows=rows.n, row_stride=rows.stride, ids=ids, payload=keys,
                       own=own, partner=par, S=S, pair_block=P, table_rows=T, num_walks=M, num_steps=HOPS, flags=flags)
    _lib.check(L.subgacc_sjoin_key_counts_attn(C.byref(d), _lib.ptr(ukeys), _lib.ptr(count), _lib.ptr(g), _lib.ptr(W),
                                               _lib.ptr(mx) if keep else None, _lib.ptr(den) if keep else None,
                                               _lib.ptr(olen) if want_len else None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((W[S * T:] == FILL).all()) and bool((mx[S:] == FILL).all()) and bool((den[S:] == FILL).all())
    assert bool((olen[S:] == -7).all())
    out = dict(W=W[: S * T].view(S, T), max=mx[:S], den=den[:S], len=olen[:S], flags=flags, Dg=None)
    if dW is not None:
        Dg = _guarded(S * T, torch.float32, FILL)
        _lib.check(L.subgacc_sjoin_key_counts_attn_backward(C.byref(d), _lib.ptr(ukeys), _lib.ptr(count), _lib.ptr(g), _lib.ptr(dW),
                                                            _lib.ptr(out["W"]), _lib.ptr(out["max"]), _lib.ptr(out["den"]), _lib.ptr(Dg),
                                                            _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((Dg[S * T:] == FILL).all())
        out["Dg"] = Dg[: S * T].view(S, T)
    return out


def _packed_attn(rows, ukeys_h, T, g, dW=None, partner=True, blocks=1, lists=None):
    """the same rows as a packed SFptr store -- the same ids, data = 1 + the rank of the key in ukeys_h (a key that is not there: an
    SFptr outside the table) -- through subgacc_sjoin_counts_attn / _backward"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    indptr = np.concatenate([[0], np.cumsum(rows.len)]).astype(np.int64)
    ids = np.concatenate([rows.ids[i, : rows.len[i]] for i in range(rows.n)]).astype(np.int32)
    keys = np.concatenate([rows.keys[i, : rows.len[i]] for i in range(rows.n)]).astype(np.uint32)
    at = np.searchsorted(ukeys_h, keys)
    found = (at < len(ukeys_h)) & (ukeys_h[np.minimum(at, max(len(ukeys_h) - 1, 0))] == keys) if len(ukeys_h) else np.zeros(len(keys), bool)
    data = np.where(found, at + 1, T + 7).astype(np.int32)
    indptr, ids, data = (torch.from_numpy(x).cuda() for x in (indptr, ids, data))
    own_h, par_h, P = _lists(rows, blocks) if lists is None else lists
    own = torch.from_numpy(own_h).cuda()
    par = torch.from_numpy(par_h).cuda() if partner else None
    S = own.numel()
    W = torch.full((S, T), FILL, dtype=torch.float32, device="cuda")
    mx, den = torch.full((S,), FILL, device="cuda"), torch.full((S,), FILL, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _lib.join_desc(_lib.JOIN_COUNTS, _lib.JOIN_SFPTR, row_off=indptr, ids=ids, payload=data, n_rows=rows.n, max_len=rows.stride,
                       own=own, partner=par, S=S, pair_block=P, table_rows=T, flags=flags)
    _lib.check(L.subgacc_sjoin_counts_attn(C.byref(d), _lib.ptr(g), _lib.ptr(W), _lib.ptr(mx), _lib.ptr(den), _lib.stream_ptr()))
    out = dict(W=W, max=mx, den=den, flags=flags, Dg=None)
    if dW is not None:
        Dg = torch.full((S, T), FILL, dtype=torch.float32, device="cuda")
        _lib.check(L.subgacc_sjoin_counts_attn_backward(C.byref(d), _lib.ptr(g), _lib.ptr(dW), _lib.ptr(W), _lib.ptr(mx), _lib.ptr(den),
                                                        _lib.ptr(Dg), _lib.stream_ptr()))
        out["Dg"] = Dg
    torch.cuda.synchronize()
    return out


def _keys_on_device(ukeys_h, T, count=None):
    """ukeys int32 [T - 1] (entries past the keys: 0) and the count word, as the columns pass leaves them"""
    u = np.zeros(T - 1, dtype=np.uint32)
    u[: len(ukeys_h)] = ukeys_h
    n = len(ukeys_h) if count is None else count
    return torch.from_numpy(u.view(np.int32)).cuda(), torch.tensor([n], dtype=torch.int64, device="cuda")


def _random(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


CASES = [
    pytest.param(299, 300, {}, id="T=c+1"),
    pytest.param(299, 339, {}, id="T=c+40"),
    pytest.param(1, 2, {}, id="one-key"),
    pytest.param(15, 16, {}, id="T-1-keys"),
    pytest.param(30, 31, {}, id="keys-fewer-than-a-row-D=T"),
    pytest.param(1500, 1501, dict(distinct=True), id="distinct-keys-D=2len"),
    pytest.param(299, 300, dict(partner=False), id="partner-None"),
    pytest.param(299, 300, dict(blocks=2), id="two-mirrored-blocks"),
]


@pytest.mark.parametrize("nkeys,T,opt", CASES)
def test_kernel_equals_the_packed_kernel_bit_for_bit(sp, nkeys, T, opt):
    """row lengths 0, 1, 255, 256, 257, 511, 512, 513 and a row that fills row_stride = 544; a row with itself and its neighbour, disjoint
    ids, full overlap, empty rows.  W, max, den and Dg equal those of subgacc_sjoin_counts_attn / _backward over the same rows as a
    packed store numbered by key rank (kappa's ascending-column order is the same sequence under both numberings)."""
    assert LENS == (0, 1, 255, 256, 257, 511, 512, 513, 544) and STRIDE == 544
    rows = Rows(_lp_keys(nkeys, 11 + nkeys), seed=nkeys, distinct=opt.get("distinct", False))
    present = rows.present()
    assert len(present) == nkeys
    partner, blocks = opt.get("partner", True), opt.get("blocks", 1)
    ukeys, count = _keys_on_device(present, T)
    g = _random((T,), 3)
    S = (2 if blocks == 1 else 4) * len(rows.a)
    dW = _random((S, T), 4)
    got = _key_attn(rows, ukeys, count, T, g, dW, partner=partner, blocks=blocks)
    want = _packed_attn(rows, present, T, g, dW, partner=partner, blocks=blocks)
    assert not got["flags"].any() and not want["flags"].any()
    for name in ("W", "max", "den", "Dg"):
        assert torch.equal(got[name], want[name]), name
    assert not bool(got["W"][:, nkeys + 1:].any()) and not bool(got["Dg"][:, nkeys + 1:].any())       # dead columns stay zero
    own = _lists(rows, blocks)[0]
    assert np.array_equal(got["len"].cpu().numpy(), rows.len[own])
    empty = torch.from_numpy(rows.len[own] == 0).cuda()
    assert bool(empty.any()) and not bool(got["W"][empty].any())
    assert not bool(got["max"][empty].any()) and not bool(got["den"][empty].any())
    # without out_max / out_den and without out_len: the same W
    bare = _key_attn(rows, ukeys, count, T, g, partner=partner, blocks=blocks, want_len=False, keep=False)
    assert torch.equal(bare["W"], got["W"]) and bool((bare["max"] == FILL).all()) and bool((bare["len"] == -7).all())


def test_w_is_the_softmax_weighted_count_in_float64(sp):
    """W restated in float64 NumPy from the rows themselves (neither kernel): within FWD_TOL of the largest entry; out_len = the own
    rows' lengths"""
    nkeys, T = 120, 140
    rows = Rows(_lp_keys(nkeys, 5), seed=9)
    present = rows.present()
    ukeys, count = _keys_on_device(present, T)
    g = _random((T,), 8, scale=2.0)
    got = _key_attn(rows, ukeys, count, T, g)
    gd = g.cpu().numpy().astype(np.float64)
    col = {int(k): i + 1 for i, k in enumerate(present)}
    own, par, _ = _lists(rows, 1)
    want = np.zeros((len(own), T))
    for j, (ra, rb) in enumerate(zip(own, par)):
        n = rows.len[ra]
        if n == 0:
            continue
        pos = {int(v): t for t, v in enumerate(rows.ids[rb, : rows.len[rb]])}
        p = np.array([col[int(k)] for k in rows.keys[ra, :n]])
        hit = [pos.get(int(v)) for v in rows.ids[ra, :n]]
        q = np.array([0 if h is None else col[int(rows.keys[rb, h])] for h in hit])
        l = gd[p] + gd[q]
        e = np.exp(l - l.max())
        alpha = e / e.sum()
        np.add.at(want[j], p, alpha)
        np.add.at(want[j], q, alpha)
    W = got["W"].cpu().numpy().astype(np.float64)
    assert np.abs(W - want).max() <= FWD_TOL * np.abs(want).max()
    assert not W[want == 0].any()
    assert np.array_equal(got["len"].cpu().numpy(), rows.len[own])


# ------------------------------------------------------------------------------------------------------------ flags and clamps
def test_a_key_that_is_not_in_the_list_reads_as_column_0(sp):
    nkeys, T = 60, 64
    rows = Rows(_lp_keys(nkeys, 21), seed=2)
    present = rows.present()
    kept = np.delete(present, nkeys // 2)
    ukeys, count = _keys_on_device(kept, T)
    g = _random((T,), 1)
    dW = _random((2 * len(rows.a), T), 2)
    got = _key_attn(rows, ukeys, count, T, g, dW)               # (_key_attn checks the guards)
    want = _packed_attn(rows, kept, T, g, dW)                   # the oracle reads an SFptr outside its table as row 0
    assert int(got["flags"][3]) & 2 and int(want["flags"][3]) & 2
    for name in ("W", "max", "den", "Dg"):
        assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("n_keys", [0, -5, "T+100"])
def test_n_keys_is_clamped(sp, n_keys):
    """*n_keys of 0 and -5 read no key (every slot is column 0, flags[3] & 2); T + 100 reads the T - 1 keys there are"""
    nkeys = 40
    T = nkeys + 1
    rows = Rows(_lp_keys(nkeys, 6), seed=3)
    present = rows.present()
    g = _random((T,), 5)
    word = T + 100 if n_keys == "T+100" else n_keys
    ukeys, count = _keys_on_device(present, T, count=word)
    got = _key_attn(rows, ukeys, count, T, g)
    if word > 0:
        want = _packed_attn(rows, present, T, g)
        assert not got["flags"].any()
    else:
        want = _packed_attn(rows, present[:0], T, g)
        assert int(got["flags"][3]) == 2 and not bool(got["W"][:, 1:].any())
    for name in ("W", "max", "den"):
        assert torch.equal(got[name], want[name]), name


def test_a_row_outside_the_store_is_an_empty_row(sp):
    nkeys, T = 40, 41
    rows = Rows(_lp_keys(nkeys, 6), seed=3)
    ukeys, count = _keys_on_device(rows.present(), T)
    g = _random((T,), 5)
    a, b = np.array([3, rows.n, 5]), np.array([rows.n + 9, 4, -1])
    lists = (np.concatenate([a, b]), np.concatenate([b, a]), 3)
    got = _key_attn(rows, ukeys, count, T, g, lists=lists)
    assert int(got["flags"][3]) == 16
    out = torch.tensor([1, 3, 5], device="cuda")           # the segments whose own row is outside the store
    assert not bool(got["W"][out].any()) and not bool(got["max"][out].any()) and not bool(got["den"][out].any())
    assert got["len"].tolist() == [int(rows.len[3]), 0, int(rows.len[5]), 0, int(rows.len[4]), 0]
    # their partners' segments: every member without a partner -- the rows joined with an empty row
    inside = torch.tensor([0, 2, 4], device="cuda")
    assert bool((got["den"][inside] > 0).all())
    lone = np.array([3, 5, 4])
    alone = _key_attn(rows, ukeys, count, T, g, lists=(np.concatenate([lone, [0, 0, 0]]), np.concatenate([[0, 0, 0], lone]), 3))
    assert torch.equal(got["W"][inside], alone["W"][:3])       # (row 0 of Rows is the empty row)


def test_a_list_that_is_not_mirrored_is_not_written(sp):
    nkeys, T = 40, 41
    rows = Rows(_lp_keys(nkeys, 6), seed=3)
    ukeys, count = _keys_on_device(rows.present(), T)
    g = _random((T,), 5)
    a, b = np.array([3, 4, 5, 6]), np.array([4, 5, 6, 7])
    own, par = np.concatenate([a, b]), np.concatenate([b, a])
    want = _key_attn(rows, ukeys, count, T, g, lists=(own, par, 4))
    bad = par.copy()
    bad[1] = 8                                                  # pair 1: the partner of (4, .) is not the own row of its mirror
    got = _key_attn(rows, ukeys, count, T, g, lists=(own, bad, 4))
    assert int(got["flags"][3]) == 4 and not want["flags"].any()
    skipped, written = [1, 5], [0, 2, 3, 4, 6, 7]
    for name in ("W", "max", "den"):
        assert bool((got[name][skipped] == FILL).all()) and torch.equal(got[name][written], want[name][written]), name
    assert bool((got["len"][skipped] == -7).all())


# --------------------------------------------------------------------------------------------------- sampled batches, the store
def _column_of_store_rows(step_table, store_table):
    """for every row of the store's table the column of the step whose feature row is the same (-1: the batch does not show it)"""
    cols = {np.ascontiguousarray(r).tobytes(): i for i, r in enumerate(step_table.cpu().numpy())}
    return np.array([cols.get(np.ascontiguousarray(r).tobytes(), -1) for r in store_table.cpu().numpy()])


@pytest.mark.parametrize("hops", [2, 3])
def test_sampled_batches_equal_the_kernel_over_the_store(sp, world, hops):
    """W, max, den of the step against subgacc_sjoin_counts_attn over the all-nodes store of the same seed, with g_store[r] = g_step[the
    column of row r's key]: bit for bit after mapping the columns.  The batch holds the isolated root, the hubs, every star centre,
    u == v."""
    from surel_plus_amd import spjoin
    z, table, lens = world.store(hops)
    B = 300
    e = world.pairs(B, 1)
    T = 1024
    g_step = _random((T,), 13).requires_grad_()
    bufs = sp.StepBuffers(world.csr, B, num_walks=M, num_steps=hops, stage="counts_attn", table_rows=T)
    W, sizes, tab, sets = sp.sample_and_attn_counts(world.csr, e, lambda t: g_step, num_walks=M, num_steps=hops, seed=5, buffers=bufs)
    sets.resolve()
    assert W.shape == (2 * B, T) and W.data_ptr() == bufs.counts.data_ptr() and W.requires_grad
    col = _column_of_store_rows(tab[: int(bufs.status[2]) + 1], table)
    assert col[0] == 0
    seen = torch.from_numpy(col >= 0).cuda()
    g_store = torch.zeros(table.shape[0], device="cuda")
    g_store[seen] = g_step.detach()[torch.from_numpy(col[col >= 0]).cuda()]
    join = spjoin._CountsAttnJoin(z, z.join_rows()[1], e.contiguous().view(-1), B, table.shape[0])
    Ws, mxs, dens = join.forward(g_store, True)
    assert not bool(Ws[:, ~seen].any())                                   # the batch reads no other row of the store's table
    at = torch.from_numpy(col[col >= 0]).cuda()
    assert torch.equal(W.detach()[:, at], Ws[:, seen])
    dead = torch.ones(T, dtype=torch.bool, device="cuda")
    dead[at] = False
    assert not bool(W.detach()[:, dead].any())
    assert torch.equal(bufs.smax, mxs) and torch.equal(bufs.sden, dens)
    assert np.array_equal(sizes.cpu().numpy(), lens[e.cpu().numpy().reshape(-1)])


# -------------------------------------------------------------------------------------------------------------------- the stage
def _nets(value=True, dtype=torch.float32, H=16):
    torch.manual_seed(7)
    mods = [torch.nn.Sequential(torch.nn.Linear(HOPS + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.Linear(H, 1),
            torch.nn.Linear(H, H) if value else None]
    return [m.to("cuda", dtype) if m is not None else None for m in mods]


def _params(nets):
    return [(n, p) for m in nets if m is not None for n, p in m.named_parameters()]


def _run(sp, csr, e, nets, w, **kw):
    for _, p in _params(nets):
        p.grad = None
    out = sp.sample_and_attn_stage(csr, e, *nets, **kw)
    (out * w).sum().backward()
    return out.detach().clone(), [p.grad.clone() for _, p in _params(nets)]


def _equal(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_one_result_whatever_the_route(sp, world):
    csr, B, T, H = world.csr, 300, 1024, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    nets = _nets()
    w = _random((2, B, H), 3)
    want1 = _run(sp, csr, e1, nets, w, table_rows=T, **kw)
    want2 = _run(sp, csr, e2, nets, w, table_rows=T, **kw)
    assert want1[0].shape == (2, B, H) and not torch.equal(want1[0], want2[0])
    assert _equal(_run(sp, csr, e1, nets, w, table_rows=T, **kw), want1)                          # two runs
    assert _equal(_run(sp, csr, e1, nets, w, table_rows=T, dedup_roots=True, **kw), want1)
    order = sp.locality_order(csr)
    assert _equal(_run(sp, csr, e1, nets, w, table_rows=T, order=order, **kw), want1)
    for dedup, ordr in ((False, None), (True, None), (False, order), (True, order)):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=dedup, order=ordr, stage="counts_attn", table_rows=T)
        assert bufs.out is None and bufs.counts.shape == (2 * B, T) and bufs.smax.shape == (2 * B,) and bufs.sden.shape == (2 * B,)
        for e, want in ((e1, want1), (e2, want2), (e1, want1)):             # a second step on the same buffers gives ITS batch
            got = _run(sp, csr, e, nets, w, buffers=bufs, dedup_roots=dedup, order=ordr, **kw)
            bufs.sets.prefetch().resolve()
            assert _equal(got, want)
    # permuted pairs give permuted rows, a flipped edge a flipped output
    perm = torch.from_numpy(np.random.default_rng(2).permutation(B)).cuda()
    with torch.no_grad():
        assert torch.equal(sp.sample_and_attn_stage(csr, e1[:, perm], *nets, table_rows=T, **kw), want1[0][:, perm])
        assert torch.equal(sp.sample_and_attn_stage(csr, e1.flip(0), *nets, table_rows=T, **kw), want1[0].flip(0))


def test_captured_step_replays_another_batch(sp, world):
    """forward and backward of the stage through StepBuffers under torch.cuda.graph; replayed with a second batch copied into the static
    edge tensor it gives the eager output and parameter gradients of that batch bit for bit"""
    csr, B, T, H = world.csr, 300, 1024, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    nets = _nets()
    w = _random((2, B, H), 3)
    want2 = _run(sp, csr, e2, nets, w, table_rows=T, **kw)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="counts_attn", table_rows=T)
    static = e1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # lazy code-object loads, cached segment lists and GEMM workspaces, uncaptured
        for _ in range(2):
            _run(sp, csr, static, nets, w, buffers=bufs, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for _, p in _params(nets):
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sp.sample_and_attn_stage(csr, static, *nets, buffers=bufs, **kw)
        (out * w).sum().backward()
    static.copy_(e2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want2[0])
    for (_, p), want in zip(_params(nets), want2[1]):
        assert torch.equal(p.grad, want)
    assert not int(bufs.status[1])                  # no overflow, no join flag


def _ref(sp, csr, e, nets, kw):
    xz, ind, _ = sp.sample_and_gather(csr, e, **kw)
    if nets[0][0].weight.dtype == torch.float64:
        xz = xz.double()
    val = nets[2] if nets[2] is not None else torch.nn.Identity()
    return _reference_style_attn(xz, ind, nets[0], nets[1], val).view(2, e.shape[1], -1)


@pytest.mark.parametrize("value", [True, False])
def test_trains_like_the_reference_first_stage(sp, world, value):
    """sample_and_attn_stage against gather -> pe_embedding -> sum(-2) -> AttentionalAggregation on the (xz, indptr) of sample_and_gather
    for the same seed, in float64 and float32, with the criteria of test_gpu_counts_attn.py::test_trains_like_the_reference_first_stage;
    and table_rows=None against table_rows = c + 40 (the centre over the live rows makes them analytically equal)"""
    csr, B, H = world.csr, 300, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e = world.pairs(B, 1)
    fa, fb, f64 = _nets(value), _nets(value), _nets(value, torch.float64)
    w = _random((2, B, H), 1)
    fused = sp.sample_and_attn_stage(csr, e, *fa, **kw)
    assert fused.shape == (2, B, H) and fused.dtype == torch.float32
    (fused * w).sum().backward()
    ref32 = _ref(sp, csr, e, fb, kw)
    (ref32 * w).sum().backward()
    truth = _ref(sp, csr, e, f64, kw)
    (truth * w.double()).sum().backward()
    scale = float(truth.detach().abs().max())
    err = float((fused.detach().double() - truth.detach()).abs().max())
    print("forward", err / scale)
    assert err <= FWD_TOL * scale
    for (n, pa), (_, pb), (_, pc) in zip(_params(fa), _params(fb), _params(f64)):
        if pa is fa[1].bias:
            assert float(pa.grad.abs().max()) == 0.0          # the gate bias: exactly zero
            continue
        gs = float(pc.grad.abs().max())
        err_fused = float((pa.grad.double() - pc.grad).abs().max()) / gs
        err_ref32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        print(n, err_fused, err_ref32)
        assert err_fused <= GRAD_TOL, (n, err_fused)
        assert err_fused <= max(4 * err_ref32, GRAD_FLOOR), (n, err_fused, err_ref32)
    c = sp.sample_and_attn_counts(csr, e, lambda t: t.sum(1), **kw)[2].shape[0] - 1
    with torch.no_grad():
        wide = sp.sample_and_attn_stage(csr, e, *fa, table_rows=c + 40, **kw)
    err = float((wide - fused.detach()).abs().max())
    print("c + 40", err / scale)
    assert err <= FWD_TOL * scale


# -------------------------------------------------------------------------------------------------------------------- edges
def test_empty_batch(sp, world):
    nets = _nets()
    e = torch.empty((2, 0), dtype=torch.int64, device="cuda")
    out = sp.sample_and_attn_stage(world.csr, e, *nets, num_walks=M, num_steps=HOPS)
    assert out.shape == (2, 0, 16) and out.dtype == torch.float32
    out.sum().backward()                   # an empty batch still trains (zero gradients)
    for _, p in _params(nets):
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0
    W, sizes, table, sets = sp.sample_and_attn_counts(world.csr, e, lambda t: t.sum(1), num_walks=M, num_steps=HOPS, table_rows=9)
    assert W.shape == (0, 9) and sizes.shape == (0,) and table.shape == (9, HOPS + 1) and sets is None


def test_self_pairs(sp, world):
    u = np.random.default_rng(7).integers(0, world.N, 100)
    u[: len(world.special)] = world.special
    e = torch.from_numpy(np.stack([u, u])).cuda()
    with torch.no_grad():
        out = sp.sample_and_attn_stage(world.csr, e, *_nets(), num_walks=M, num_steps=HOPS, seed=5)
    assert torch.equal(out[0], out[1]) and bool(out.any())


def test_no_grad_builds_no_graph(sp, world):
    nets = _nets()
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=1024)
    e = world.pairs(300, 1)
    with torch.no_grad():
        out = sp.sample_and_attn_stage(world.csr, e, *nets, **kw)
    assert not out.requires_grad and out.grad_fn is None
    assert torch.equal(out, sp.sample_and_attn_stage(world.csr, e, *nets, **kw).detach())


def test_more_distinct_rows_than_columns(sp, world):
    from surel_plus_amd import _lib
    nets = _nets()
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    bufs = sp.StepBuffers(world.csr, 64, stage="counts_attn", table_rows=8, num_walks=M, num_steps=HOPS)
    with torch.no_grad():
        x = sp.sample_and_attn_stage(world.csr, world.pairs(64, 1), *nets, buffers=bufs, **kw)
    assert x.shape == (2, 64, 16)
    with pytest.raises(_lib.SubgAccError, match="table_rows"):      # the stage returns the tensor alone: the step is checked here
        bufs.sets.resolve()
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        sp.sample_and_attn_stage(world.csr, world.pairs(64, 1), *nets, table_rows=8, **kw)


def test_a_backward_after_the_buffers_next_step_raises(sp, world):
    nets = _nets()
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    bufs = sp.StepBuffers(world.csr, 64, stage="counts_attn", table_rows=1024, num_walks=M, num_steps=HOPS)
    first = sp.sample_and_attn_stage(world.csr, world.pairs(64, 1), *nets, buffers=bufs, **kw)
    second = sp.sample_and_attn_stage(world.csr, world.pairs(64, 2), *nets, buffers=bufs, **kw)
    with pytest.raises(RuntimeError, match="step 1 .* took step 2"):
        first.sum().backward()
    second.sum().backward()                 # the step the buffers hold trains
    assert all(p.grad is not None for _, p in _params(nets))

"""GPU (MI355X): counts_attn_stage -- the LP encoder's first model stage with attentional aggregation fused with the count form of the
join (subgacc_sjoin_counts_attn / _backward, model.py:59-62,78-81) -- equals the reference form  gather -> pe_embedding -> sum(-2) ->
AttentionalAggregation  in its output and in every parameter gradient, writes the softmax-weighted count rows the index pairs give, and
gives the same bits over repeated runs, with or without the backward's outputs, for any order of the pairs and either order of a pair's
endpoints."""
import numpy as np
import pytest
import torch

import surel_plus_amd as spm
from gpu_helpers import _reference_style_attn, sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu

# the tolerances of test_gpu_join.py::test_attn_stage_trains_like_the_reference_first_stage: forward within 2e-5 of the largest entry
# of the float64 reference form; every gradient within 5e-4 of its largest entry and no worse than max(4x the fp32 reference form's own
# error, 1e-4)
FWD_TOL, GRAD_TOL, GRAD_FLOOR = 2e-5, 5e-4, 1e-4


@pytest.fixture(scope="module")
def lp(sp):
    """(z, table): a packed SFptr store over a graph with hub rows, and its feature table (row 0 = partner absent)"""
    ptr_, idx = sym_graph(3000, 15000, seed=6, hubs=2)
    z, sets = sp.sample_spg(sp.DeviceCSR(ptr_, idx), np.arange(3000), num_walks=64, num_steps=3, seed=2, rng="philox")
    return z, sets.feature_table()


def _nets(value=True, dtype=torch.float32, H=16):
    torch.manual_seed(7)
    mods = [torch.nn.Sequential(torch.nn.Linear(4, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.Linear(H, 1),
            torch.nn.Linear(H, H) if value else None]
    return [m.to("cuda", dtype) if m is not None else None for m in mods]


def _params(nets):
    return [(n, p) for m in nets if m is not None for n, p in m.named_parameters()]


def _edge(n_rows, B, seed=4):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, n_rows, (2, B))).cuda()


def _ref(edge, z, table, nets):
    xz, ind = spm.gather(edge, z, "cuda", ptr=True, encode=table)
    if nets[0][0].weight.dtype == torch.float64:
        xz = xz.double()
    val = nets[2] if nets[2] is not None else torch.nn.Identity()
    return _reference_style_attn(xz, ind, nets[0], nets[1], val).view(2, edge.shape[1], -1)


def _join(sp, z, table_rows, edge):
    """the library's W [2B, T], m, den for g (through the stage's own join object)"""
    from surel_plus_amd import spjoin
    e = edge.to(torch.int64)
    return spjoin._CountsAttnJoin(z, z.join_rows()[1], e.contiguous().view(-1), int(e.shape[1]), int(table_rows))


def _g(table, nets):
    with torch.no_grad():
        E = nets[0](table)
        return ((E - E.mean(0)) @ nets[1].weight.view(-1)).contiguous()


@pytest.mark.parametrize("value", [True, False])
def test_trains_like_the_reference_first_stage(sp, lp, value):
    z, table = lp
    edge = _edge(z.n_rows, 512)
    fa, fb, f64 = _nets(value), _nets(value), _nets(value, torch.float64)
    torch.manual_seed(1)
    H = 16
    w = torch.randn(2, 512, H, device="cuda")
    fused = sp.counts_attn_stage(edge, z, table, *fa)
    assert fused.shape == (2, 512, H) and fused.dtype == torch.float32
    (fused * w).sum().backward()
    ref32 = _ref(edge, z, table, fb)
    (ref32 * w).sum().backward()
    truth = _ref(edge, z, table, f64)
    (truth * w.double()).sum().backward()
    scale = float(truth.detach().abs().max())
    assert float((fused.detach().double() - truth.detach()).abs().max()) <= FWD_TOL * scale
    for (n, pa), (_, pb), (_, pc) in zip(_params(fa), _params(fb), _params(f64)):
        if pa is fa[1].bias:
            assert float(pa.grad.abs().max()) == 0.0          # the gate bias: exactly zero
            continue
        gs = float(pc.grad.abs().max())
        err_fused = float((pa.grad.double() - pc.grad).abs().max()) / gs
        err_ref32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        assert err_fused <= GRAD_TOL, (n, err_fused)
        assert err_fused <= max(4 * err_ref32, GRAD_FLOOR), (n, err_fused, err_ref32)


def test_w_is_the_softmax_weighted_count_of_the_index_pairs(sp, lp):
    z, table = lp
    edge = _edge(z.n_rows, 700, seed=9)
    nets = _nets()
    T = table.shape[0]
    g = _g(table, nets)
    W, mx, den = _join(sp, z, T, edge).forward(g, True)
    pairs, ind = sp.gather_index(edge, z)
    P, Q = pairs[:, 0].long(), pairs[:, 1].long()
    S = ind.numel() - 1
    seg = torch.repeat_interleave(torch.arange(S, device="cuda"), ind[1:] - ind[:-1])
    gd = g.double()
    lo = gd[P] + gd[Q]
    m = torch.full((S,), float("-inf"), device="cuda", dtype=torch.float64).scatter_reduce(0, seg, lo, "amax")
    e = torch.exp(lo - m[seg])
    dn = torch.zeros(S, device="cuda", dtype=torch.float64).index_add_(0, seg, e)
    alpha = e / dn[seg]
    want = torch.zeros((S, T), device="cuda", dtype=torch.float64)
    want.index_put_((seg, P), alpha, accumulate=True)
    want.index_put_((seg, Q), alpha, accumulate=True)
    assert float((W.double() - want).abs().max()) <= 1e-5
    n = ind[1:] - ind[:-1]
    assert not bool(W[want == 0].any())                            # zeros where r does not occur
    assert float((W[n > 0].double().sum(1) - 2).abs().max()) <= 1e-5
    assert not bool(W[n == 0].any())
    assert torch.equal(mx[n > 0].double(), m[n > 0].float().double())   # a max: exact
    assert float((den.double() - torch.where(n > 0, dn, torch.zeros_like(dn))).abs().max()) <= 1e-4 * float(dn.max())


def test_agrees_with_attn_stage(sp, lp):
    z, table = lp
    edge = _edge(z.n_rows, 1024, seed=3)
    for value in (True, False):
        nets = _nets(value)
        with torch.no_grad():
            got = sp.counts_attn_stage(edge, z, table, *nets)
            val = nets[2] if value else None
            want = sp.attn_stage(edge, z, table, nets[0], nets[1], val)
        assert float((got - want).abs().max()) <= FWD_TOL * float(want.abs().max())


def _run(sp, edge, z, table, nets, w):
    for _, p in _params(nets):
        p.grad = None
    out = sp.counts_attn_stage(edge, z, table, *nets)
    (out * w).sum().backward()
    return out.detach().clone(), [p.grad.clone() for _, p in _params(nets)]


def test_repeated_runs_give_the_same_bits(sp, lp):
    z, table = lp
    edge = _edge(z.n_rows, 2048, seed=5)
    nets = _nets()
    w = torch.randn(2, 2048, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    out0, g0 = _run(sp, edge, z, table, nets, w)
    for _ in range(3):
        out, gr = _run(sp, edge, z, table, nets, w)
        assert torch.equal(out, out0)
        for a, b in zip(gr, g0):
            assert torch.equal(a, b)


def test_w_with_and_without_max_and_den_gives_the_same_bits(sp, lp):
    z, table = lp
    edge = _edge(z.n_rows, 1000, seed=8)
    nets = _nets()
    g = _g(table, nets)
    j = _join(sp, z, table.shape[0], edge)
    W1, mx, den = j.forward(g, True)
    W0, none, _ = j.forward(g, False)
    assert none is None and torch.equal(W0, W1)


def test_permuted_pairs_and_swapped_endpoints_give_the_same_rows(sp, lp):
    z, table = lp
    B = 1500
    edge = _edge(z.n_rows, B, seed=12)
    nets = _nets()
    g = _g(table, nets)
    T = table.shape[0]
    W, mx, den = _join(sp, z, T, edge).forward(g, True)
    perm = torch.from_numpy(np.random.default_rng(2).permutation(B)).cuda()
    Wp, mxp, denp = _join(sp, z, T, edge[:, perm]).forward(g, True)
    rows = torch.cat([perm, perm + B])
    assert torch.equal(Wp, W[rows]) and torch.equal(mxp, mx[rows]) and torch.equal(denp, den[rows])
    Ws, mxs, dens = _join(sp, z, T, edge.flip(0)).forward(g, True)         # block 2t+1 <-> 2t: the other row staged
    sw = torch.cat([torch.arange(B, 2 * B), torch.arange(B)]).cuda()
    assert torch.equal(Ws, W[sw]) and torch.equal(mxs, mx[sw]) and torch.equal(dens, den[sw])
    with torch.no_grad():
        out = sp.counts_attn_stage(edge, z, table, *nets)
        assert torch.equal(sp.counts_attn_stage(edge[:, perm], z, table, *nets), out[:, perm])
        assert torch.equal(sp.counts_attn_stage(edge.flip(0), z, table, *nets), out.flip(0))
    # the backward too: permuted and swapped pairs give the same parameter gradients up to the order torch sums the segments in, and
    # the per-segment rows Dg themselves bit for bit
    dW = torch.randn_like(W)
    Dg = _join(sp, z, T, edge).backward(g, dW, W, mx, den)
    Dgp = _join(sp, z, T, edge[:, perm]).backward(g, dW[rows].contiguous(), Wp, mxp, denp)
    Dgs = _join(sp, z, T, edge.flip(0)).backward(g, dW[sw].contiguous(), Ws, mxs, dens)
    assert torch.equal(Dgp, Dg[rows]) and torch.equal(Dgs, Dg[sw])
    assert torch.equal(_join(sp, z, T, edge).backward(g, dW, W, mx, den), Dg)


def test_self_pairs(sp, lp):
    z, table = lp
    u = np.random.default_rng(7).integers(0, z.n_rows, 100)
    edge = torch.from_numpy(np.stack([u, u])).cuda()
    nets, truth = _nets(), _nets(dtype=torch.float64)
    with torch.no_grad():
        got = sp.counts_attn_stage(edge, z, table, *nets)
        want = _ref(edge, z, table, truth)
        assert float((got.double() - want).abs().max()) <= FWD_TOL * float(want.abs().max())
        assert torch.equal(got[0], got[1])


def test_hub_rows_at_max_len(sp, lp):
    """the longest rows of the store (the hubs', at SpG.max_len) against each other and against short rows"""
    z, table = lp
    lens = (z.indptr[1:] - z.indptr[:-1]).cpu().numpy()
    hubs = np.flatnonzero(lens == lens.max())
    assert int(lens.max()) <= z.max_len and len(hubs) >= 1
    rng = np.random.default_rng(5)
    a = np.concatenate([hubs, hubs, rng.integers(0, z.n_rows, 50)])
    b = np.concatenate([hubs[::-1], rng.integers(0, z.n_rows, len(hubs)), np.repeat(hubs[:1], 50)])
    edge = torch.from_numpy(np.stack([a, b])).cuda()
    nets, truth = _nets(), _nets(dtype=torch.float64)
    with torch.no_grad():
        got = sp.counts_attn_stage(edge, z, table, *nets)
        want = _ref(edge, z, table, truth)
    assert int(got.join_flags[3]) == 0
    assert float((got.double() - want).abs().max()) <= FWD_TOL * float(want.abs().max())


def test_empty_batch(sp, lp):
    z, table = lp
    nets = _nets()
    out = sp.counts_attn_stage(torch.empty((2, 0), dtype=torch.int64, device="cuda"), z, table, *nets)
    assert out.shape == (2, 0, 16) and out.dtype == torch.float32
    out.sum().backward()                   # an empty batch still trains (zero gradients)
    for _, p in _params(nets):
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0


def test_empty_rows_give_zero_rows(sp):
    ip = torch.tensor([0, 3, 3, 5, 5], dtype=torch.int64, device="cuda")
    ids = torch.tensor([1, 2, 3, 2, 3], dtype=torch.int32, device="cuda")
    data = torch.tensor([1, 2, 3, 2, 1], dtype=torch.int32, device="cuda")
    z = sp.SpG(ip, ids, data)
    table = torch.rand(4, 4, device="cuda")
    edge = torch.tensor([[0, 1, 1, 2], [1, 3, 0, 0]], device="cuda")
    nets, truth = _nets(), _nets(dtype=torch.float64)
    with torch.no_grad():
        got = sp.counts_attn_stage(edge, z, table, *nets)
        want = _ref(edge, z, table, truth)
    assert float((got.double() - want).abs().max()) <= FWD_TOL * float(want.abs().max())
    assert not bool(got[1, :2].any()) and not bool(got[0, 1:3].any()) and bool(got[0, 0].any())


def test_edge_out_of_range_raises(sp, lp):
    z, table = lp
    nets = _nets()
    for bad in (z.n_rows, -1):
        with pytest.raises(IndexError, match="row index out of range"):
            sp.counts_attn_stage(torch.tensor([[0, 5], [bad, 3]], device="cuda"), z, table, *nets)


def test_table_shorter_than_the_store_raises(sp, lp):
    z, table = lp
    nets = _nets()
    with pytest.raises(IndexError, match="out of bounds for the encode table"):
        sp.counts_attn_stage(_edge(z.n_rows, 256), z, table[: table.shape[0] // 2], *nets)


def test_no_grad_builds_no_graph(sp, lp):
    z, table = lp
    nets = _nets()
    edge = _edge(z.n_rows, 300)
    with torch.no_grad():
        out = sp.counts_attn_stage(edge, z, table, *nets)
    assert not out.requires_grad and out.grad_fn is None
    assert torch.equal(out, sp.counts_attn_stage(edge, z, table, *nets).detach())

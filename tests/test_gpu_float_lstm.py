"""GPU (MI355X): float_lstm_stage -- the first model stage of the PPR / SPD / DEG encoders with LSTM aggregation in the recurrent kernel
(subgacc_lstm_aggr_hinge / _backward, model.py:63-65,78-83) -- against the float64 reference form  gather -> pe_embedding -> sum(-2) ->
to_dense_batch -> nn.LSTM -> last position  evaluated on the stage's own gather output: stores, widths, batch shapes around the tile,
knots on the data, bit identity, and a B = 65,536 batch checked segment by segment.  Bounds: those of tests/test_gpu_lstm_aggr.py
(forward within 2e-5 of the largest entry, every gradient within 5e-4 of its largest entry)."""
import numpy as np
import pytest
import torch

import surel_plus_amd as spm
from gpu_helpers import _load, _spg_from_golden, dense_batch, sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 2e-5, 5e-4


def _nets(H=16, H1=16, H2=16, dtype=torch.float32, seed=1, bias=True):
    torch.manual_seed(seed)
    embed = torch.nn.Sequential(torch.nn.Linear(1, H, bias=bias), torch.nn.ReLU(), torch.nn.Linear(H, H1, bias=bias))
    lstm = torch.nn.LSTM(H1, H2, batch_first=True, bias=bias)
    return [embed.to("cuda", dtype), lstm.to("cuda", dtype)]


def _params(nets):
    return [(n, p) for m in nets for n, p in m.named_parameters()]


def _total_rows(edge, z):
    """the rows of the batch's segments (a batch without any asks the join for nothing)"""
    zz = z.to_spg() if hasattr(z, "to_spg") else z
    own = edge.reshape(-1)
    return int((zz.indptr[own + 1] - zz.indptr[own]).sum())


def _reference(xz, ind, nets):
    embed, lstm = nets
    x = embed(xz.to(embed[0].weight.dtype)).sum(dim=-2)
    L = max(int((ind[1:] - ind[:-1]).max()), 1) if ind.numel() > 1 else 1
    return lstm(dense_batch(x, ind, L))[0][:, -1].view(2, -1, lstm.hidden_size)


def _check(edge, z, H=16, H1=16, H2=16, bias=True, grads=True, nets=None):
    """forward and every gradient against the float64 reference form; prints each figure before it asserts"""
    edge = edge.cuda()
    B = edge.shape[1]
    fused = nets[0] if nets else _nets(H, H1, H2, bias=bias)
    truth = nets[1] if nets else _nets(H, H1, H2, torch.float64, bias=bias)
    xz, ind = (torch.zeros((0, 2, 1), device="cuda"), torch.zeros(2 * B + 1, dtype=torch.int64, device="cuda")) \
        if _total_rows(edge, z) == 0 else spm.gather(edge, z, "cuda", ptr=True)
    out = spm.float_lstm_stage(edge, z, *fused)
    assert out.shape == (2, B, fused[1].hidden_size) and out.dtype == torch.float32
    assert [int(v) for v in out.join_flags.tolist()][3] == 0
    r64 = _reference(xz, ind, truth)
    scale = float(r64.detach().abs().max())
    err = float((out.detach().double() - r64.detach()).abs().max())
    print(f"fwd err {err / scale:.3e} of the largest entry {scale:.3e}")
    assert err <= FWD_TOL * scale
    if grads:
        torch.manual_seed(2)
        w = torch.randn(2, B, fused[1].hidden_size, device="cuda")
        (out * w).sum().backward()
        (r64 * w.double()).sum().backward()
        for (n, pa), (_, pc) in zip(_params(fused), _params(truth)):
            assert pa.grad is not None and pa.grad.dtype == torch.float32, n
            gs = max(float(pc.grad.abs().max()), 1e-6)
            e = float((pa.grad.double() - pc.grad).abs().max()) / gs
            print(f"grad {n}: err {e:.3e} of the largest entry {gs:.3e}")
            assert e <= GRAD_TOL, (n, e)
    return out


def _store(kind, N=3000, hubs=0, seed=6):
    from surel_plus_amd import DeviceCSR, ppr
    indptr, indices = sym_graph(N, 5 * N, seed=seed, hubs=hubs)
    csr = DeviceCSR(indptr, indices)
    x = ppr.topk_ppr_matrix(csr, 0.5, 1e-4, np.arange(N), 30, normalization="sym")
    z, _ = ppr.encoding(x, csr if kind != "PPR" else None, kind)
    return z


@pytest.fixture(scope="module", params=["PPR", "SPD", "DEG"])
def store(request, sp):
    return request.param, _store(request.param)


def _row_store(lens, seed=0):
    """a float64 SpG whose row i has lens[i] members with scores in (0, 1]"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(max(lens) + 5, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    data = (rng.random(ids.size) + 0.1) / 1.1
    return spm.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(data).cuda())


# ------------------------------------------------------------------------------------------------ 1. stores
def test_golden_store_packed_and_headed(sp):
    g = _load("sjoin_float.npz")
    z = _spg_from_golden(sp, g)
    edge = torch.from_numpy(g["edge"]).cuda()
    out = _check(edge, z, 96, 24, 32)
    with torch.no_grad():
        headed = sp.float_lstm_stage(edge, z.aligned(), *_nets(96, 24, 32))
        truth = _reference(torch.from_numpy(g["xz_ptr1"]).cuda(), torch.from_numpy(g["ind_ptr1"]).cuda(), _nets(96, 24, 32, torch.float64))
    assert torch.equal(headed, out.detach())
    assert float((out.detach().double() - truth).abs().max()) <= FWD_TOL * float(truth.abs().max())


def test_ppr_spd_deg_stores_packed_and_headed(store):
    kind, z = store
    edge = torch.from_numpy(np.random.default_rng(4).integers(0, z.n_rows, (2, 200))).cuda()
    out = _check(edge, z, 96, 96, 96)
    headed = _check(edge, z.aligned(), 96, 96, 96)
    assert torch.equal(out.detach(), headed.detach())


# ------------------------------------------------------------------------------------------------ 2. widths
@pytest.mark.parametrize("H,H1,H2,bias", [(1, 8, 16, True), (16, 24, 48, False), (96, 96, 96, True), (256, 40, 128, True),
                                          (16, 16, 16, False), (96, 32, 128, False)])
def test_widths(sp, H, H1, H2, bias):
    z = _store("PPR", 800)
    edge = torch.from_numpy(np.random.default_rng(H).integers(0, 800, (2, 40))).cuda()
    _check(edge, z, H, H1, H2, bias)


# ------------------------------------------------------------------------------------------------ 3. batch shapes
@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])
def test_segment_counts_off_the_tile(sp, B):
    z = _row_store([int(v) for v in np.random.default_rng(B).integers(0, 12, 40)])
    edge = torch.from_numpy(np.random.default_rng(B + 1).integers(0, 40, (2, B)))
    edge[:, 0] = edge[0, 0]                                     # a (u, u) pair
    _check(edge, z, 16, 16, 32)


def test_boundaries(sp):
    """L = 1; a batch whose rows are all empty (padded steps alone); empty rows in the middle and at the end; one long segment among
    short ones"""
    z = _row_store([0, 1, 1, 0, 9, 3, 0, 60])
    for e in ([[1, 2], [2, 1]], [[1, 2, 0], [0, 3, 3]]):
        _check(torch.tensor(e), z)
    for e in ([[0, 3], [3, 6]], [[0], [0]]):
        out = _check(torch.tensor(e), z)
        assert out.shape[1] == len(e[0])
    _check(torch.tensor([[1, 0, 4, 5, 6, 0], [0, 4, 2, 4, 0, 3]]), z)
    _check(torch.tensor([[1, 7, 2, 5, 0, 1, 2, 5, 1], [2, 0, 1, 5, 3, 1, 4, 6, 2]]), z)


# ------------------------------------------------------------------------------------------------ 4. knots on the data
def test_knots_on_store_values_dead_channel_and_duplicate_knots(sp):
    z = _store("SPD", 800)
    vals = torch.unique(z.data).float()
    assert vals.numel() > 1
    H = 16
    nets = [_nets(H, 16, 32), _nets(H, 16, 32, torch.float64)]
    with torch.no_grad():
        w1 = nets[0][0][0].weight.view(-1)
        w1.copy_(torch.sign(w1) * torch.exp2(torch.round(torch.log2(w1.abs()))))     # powers of two: b1 = -w1 v is exact, so the
        w1[0] = 0.0                                             # pre-activation on a knot is exactly 0 in float32 and in float64
        b1 = nets[0][0][0].bias
        for c in range(1, H):                                   # every other knot exactly on a store value; channels 1 and 2 share one
            v = vals[(max(c, 2) - 2) % vals.numel()]
            b1[c] = -w1[c] * v
        nets[1][0][0].weight.copy_(nets[0][0][0].weight.double())
        nets[1][0][0].bias.copy_(b1.double())
    edge = torch.from_numpy(np.random.default_rng(8).integers(0, 800, (2, 100)))
    _check(edge, z, nets=nets)


# ------------------------------------------------------------------------------------------------ 5. bits
def _run(edge, z, H2=32):
    nets = _nets(16, 16, H2)
    out = spm.float_lstm_stage(edge, z, *nets)
    torch.manual_seed(4)
    (out * torch.randn_like(out)).sum().backward()
    return out.detach(), [p.grad.clone() for _, p in _params(nets)]


def test_bits(sp):
    """two runs: identical outputs and gradients; with and without the backward's state: the same output; permuted pairs: permuted
    rows of the result"""
    z = _store("PPR", 1500)
    edge = torch.from_numpy(np.random.default_rng(5).integers(0, 1500, (2, 77))).cuda()
    o1, g1 = _run(edge, z)
    o2, g2 = _run(edge, z)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    with torch.no_grad():
        assert torch.equal(spm.float_lstm_stage(edge, z, *_nets(16, 16, 32)), o1)
    perm = torch.from_numpy(np.random.default_rng(6).permutation(77)).cuda()
    o3, _ = _run(edge[:, perm], z)
    assert torch.equal(o3, o1[:, perm])


def test_a_pair_does_not_depend_on_its_tile_mates(sp):
    """pair 0 keeps its bits when the other pairs of its tile are replaced by pairs of equal or shorter rows (L held by a last pair)"""
    z = _row_store([9, 7, 3, 0, 5, 9, 2, 1, 12])
    a = torch.tensor([[0, 1, 2, 3, 4, 8], [1, 2, 3, 4, 0, 8]]).cuda()
    b = torch.tensor([[0, 6, 7, 3, 2, 8], [1, 7, 3, 6, 5, 8]]).cuda()
    with torch.no_grad():
        oa, ob = (spm.float_lstm_stage(e, z, *_nets(16, 16, 48)) for e in (a, b))
    assert torch.equal(oa[:, 0], ob[:, 0]) and torch.equal(oa[:, 5], ob[:, 5])


# ------------------------------------------------------------------------------------------------ 7. a large batch
def test_a_large_batch_segment_by_segment(sp):
    """B = 65,536 forward under no_grad over a top-60 store; the longest segment, an empty one and 256 random ones each against the
    float64 reference form of that segment alone padded to the batch's L"""
    from surel_plus_amd.graphs import ppr_like_spg
    N = 20000
    z = ppr_like_spg(N, topk=60, seed=3)
    lens = torch.full((N,), 60, dtype=torch.int64, device="cuda")
    short = torch.arange(0, N, 7, device="cuda")
    lens[short] = torch.arange(short.numel(), device="cuda") % 60           # rows of 0 .. 59 members among the full ones
    keep = torch.arange(60, device="cuda")[None, :] < lens[:, None]
    indptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lens, 0, out=indptr[1:])
    z = spm.SpG(indptr, z.indices.view(N, 60)[keep].contiguous(), z.data.view(N, 60)[keep].contiguous())
    edge = torch.from_numpy(np.random.default_rng(7).integers(0, N, (2, 65536))).cuda()
    edge[0, 11] = 0                                                          # row 0 is empty
    H, H2 = 32, 32
    nets, n64 = _nets(H, H, H2), _nets(H, H, H2, torch.float64)
    with torch.no_grad():
        out = spm.float_lstm_stage(edge, z, *nets).view(-1, H2)
        xz, ind = spm.gather(edge, z, "cuda", ptr=True)
        n = ind[1:] - ind[:-1]
        L = int(n.max())
        assert L == 60 and int(n[11]) == 0
        pick = np.union1d(np.random.default_rng(8).choice(2 * 65536, 256, replace=False), [11, int(n.argmax())])
        worst = 0.0
        for j in pick:
            x = n64[0](xz[int(ind[j]):int(ind[j + 1])].double()).sum(dim=-2)
            dense = torch.zeros((1, L, H), dtype=torch.float64, device="cuda")
            dense[0, :x.shape[0]] = x
            ref = n64[1](dense)[0][0, -1]
            e = float((out[j].double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-3)
            worst = max(worst, e)
            assert e <= FWD_TOL, (j, e)
    print(f"largest error over {len(pick)} segments: {worst:.3e}")

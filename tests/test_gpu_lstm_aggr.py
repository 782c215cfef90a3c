"""GPU: index_lstm_stage -- the LP encoder's first stage with LSTM aggregation folded into one recurrent kernel (subgacc_lstm_aggr /
_backward) -- against the float64 reference form (to_dense_batch -> nn.LSTM -> last position, model.py:63-65,78-83) and lstm_stage:
widths, batch boundaries, bit identity, and a B = 65,536 batch checked segment by segment."""
import numpy as np
import pytest
import torch

from gpu_helpers import sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu


def _store(sp, N=2000, E=9000, walks=32, seed=8):
    ptr_, idx = sym_graph(N, E, seed=seed, hubs=1)
    csr = sp.DeviceCSR(ptr_, idx)
    z, sets = sp.sample_spg(csr, np.arange(N), num_walks=walks, num_steps=3, seed=5, rng="philox")
    return csr, z, sets.feature_table()


def _nets(dtype, H=16, H2=16, bias=True, k=4):
    torch.manual_seed(11)
    return [torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).cuda().to(dtype),
            torch.nn.LSTM(H, H2, batch_first=True, bias=bias).cuda().to(dtype)]


def _reference_style_lstm(xz, ptr, embed, lstm):
    """gpu_helpers._reference_style_lstm padded to max(L, 1) positions, as lstm_stage pads a batch of empty segments only"""
    x = embed(xz).sum(dim=-2)
    S = ptr.numel() - 1
    lens = ptr[1:] - ptr[:-1]
    dense = x.new_zeros((S, max(int(lens.max()), 1), x.shape[-1]))
    for j in range(S):
        dense[j, : int(lens[j])] = x[int(ptr[j]): int(ptr[j + 1])]
    return lstm(dense)[0][:, -1]


def _check_against_reference(sp, edge, z, table, H, H2, bias=True, grads=True):
    fa, f64 = _nets(torch.float32, H, H2, bias, table.shape[1]), _nets(torch.float64, H, H2, bias, table.shape[1])
    B = edge.shape[1]
    own = edge.reshape(-1)
    if int((z.indptr[own + 1] - z.indptr[own]).sum()) == 0:          # no rows at all (gather() asks for none): the padded steps alone
        xz, ind = table.new_zeros((0, 2, table.shape[1])), torch.zeros(2 * B + 1, dtype=torch.int64, device="cuda")
    else:
        xz, ind = sp.gather(edge, z, "cuda", ptr=True, encode=table)
    torch.manual_seed(2)
    w = torch.randn(2, B, H2, device="cuda")
    fused = sp.index_lstm_stage(edge, z, table, *fa)
    assert fused.shape == (2, B, H2) and fused.dtype == torch.float32
    truth = _reference_style_lstm(xz.double(), ind, *f64).view(2, -1, H2)
    scale = float(truth.detach().abs().max())
    assert float((fused.detach().double() - truth.detach()).abs().max()) <= 2e-5 * scale
    if grads:
        (fused * w).sum().backward()
        (truth * w.double()).sum().backward()
        for (n, pa), (_, pc) in zip([(n, p) for mod in fa for n, p in mod.named_parameters()],
                                    [(n, p) for mod in f64 for n, p in mod.named_parameters()]):
            assert pa.grad is not None, n
            gs = float(pc.grad.abs().max())
            assert float((pa.grad.double() - pc.grad).abs().max()) <= 5e-4 * max(gs, 1e-6), n
    return fused


def test_index_lstm_stage_matches_the_reference_first_stage(sp):
    """forward within 2e-5 of the float64 reference form's largest entry, every parameter gradient within 5e-4 (the bounds of
    test_gather_index_and_lstm_stage_match_the_reference_first_stage); also close to lstm_stage in fp32"""
    csr, z, table = _store(sp)
    edge = torch.from_numpy(np.random.default_rng(9).integers(0, 2000, (2, 96))).cuda()
    edge[:, 5] = edge[0, 5]                                            # a (u, u) pair
    fused = _check_against_reference(sp, edge, z, table, 16, 16)
    with torch.no_grad():
        ref = sp.lstm_stage(edge, z, table, *_nets(torch.float32))
        nog = sp.index_lstm_stage(edge, z, table, *_nets(torch.float32))
    assert float((fused.detach() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    assert torch.equal(nog, fused.detach())                             # with or without the state for the backward: the same bits


@pytest.mark.parametrize("H,H2,bias", [(16, 16, True), (24, 32, False), (96, 96, True), (40, 128, True)])
def test_widths(sp, H, H2, bias):
    csr, z, table = _store(sp, 600, 2500, walks=16)
    edge = torch.from_numpy(np.random.default_rng(3).integers(0, 600, (2, 40))).cuda()
    _check_against_reference(sp, edge, z, table, H, H2, bias)


@pytest.mark.parametrize("H2", [100, 144, 8])
def test_widths_the_kernel_does_not_take_are_refused(sp, H2):
    csr, z, table = _store(sp, 300, 1200, walks=8)
    edge = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="lstm_stage"):
        sp.index_lstm_stage(edge, z, table, *_nets(torch.float32, 16, H2))


def _row_store(sp, lens, T=7, seed=0):
    """an SpG whose row i has lens[i] members (ids 0.., SFptr+1 drawn in [1, T))"""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(max(lens) + 5, n, replace=False)) for n in lens]).astype(np.int32) if sum(lens) else \
        np.zeros(0, np.int32)
    data = rng.integers(1, T, ids.size).astype(np.int32)
    z = sp.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(data).cuda())
    table = torch.from_numpy(rng.standard_normal((T, 3)).astype(np.float32)).cuda()
    return z, table


@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])
def test_segment_counts_off_the_tile(sp, B):
    z, table = _row_store(sp, [int(v) for v in np.random.default_rng(B).integers(0, 12, 40)])
    edge = torch.from_numpy(np.random.default_rng(B + 1).integers(0, 40, (2, B))).cuda()
    _check_against_reference(sp, edge, z, table, 16, 32)


def test_boundaries(sp):
    """L = 1; a batch of empty segments only; empty segments in the middle and at the end; a segment of exactly L rows beside
    segments of 0 and 1 rows"""
    z, table = _row_store(sp, [0, 1, 1, 0, 9, 3, 0])
    for e in ([[1, 2], [2, 1]], [[1, 2, 0], [0, 3, 3]]):               # L = 1 (rows of 1 and empty partners)
        _check_against_reference(sp, torch.tensor(e).cuda(), z, table, 16, 16)
    for e in ([[0, 3], [3, 6]], [[0], [0]]):                            # empty segments only: L padded steps from zero
        _check_against_reference(sp, torch.tensor(e).cuda(), z, table, 16, 16)
    _check_against_reference(sp, torch.tensor([[1, 0, 4, 5, 6, 0], [0, 4, 2, 4, 0, 3]]).cuda(), z, table, 16, 16)


def _bits(sp, edge, z, table, H2=32):
    fa = _nets(torch.float32, 16, H2)
    out = sp.index_lstm_stage(edge, z, table, *fa)
    torch.manual_seed(4)
    (out * torch.randn_like(out)).sum().backward()
    return out.detach(), [p.grad.clone() for mod in fa for p in mod.parameters()]


def test_bits(sp):
    """two runs: identical bits, outputs and gradients; permuted pairs: permuted output bits (L unchanged)"""
    csr, z, table = _store(sp)
    edge = torch.from_numpy(np.random.default_rng(5).integers(0, 2000, (2, 77))).cuda()
    o1, g1 = _bits(sp, edge, z, table)
    o2, g2 = _bits(sp, edge, z, table)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    perm = torch.from_numpy(np.random.default_rng(6).permutation(77)).cuda()
    o3, _ = _bits(sp, edge[:, perm], z, table)
    assert torch.equal(o3, o1[:, perm])


def test_packed_strided_and_key_row_batches_give_the_same_bits(sp):
    from surel_plus_amd.graphs import query_pairs
    ptr_, idx = sym_graph(2000, 9000, seed=8, hubs=1)
    csr = sp.DeviceCSR(ptr_, idx)
    e = query_pairs(csr, 200, seed=3)
    rows = torch.arange(400, device="cuda").view(2, 200)
    forms = []
    for kr in (False, True):
        _, _, bsets = sp.sample_and_gather(csr, e, num_walks=32, num_steps=3, seed=5, rng="philox", key_rows=kr)
        zs = sp.StridedSpG(bsets, csr.num_nodes)
        forms += [(kr, zs), (kr, zs.to_csr())]
    index = [sp.gather_index(rows, f) for _, f in forms]
    idx = [i for i, _ in index]
    T = max(int(i.max()) for i in idx) + 1
    table = torch.randn((T, 4), device="cuda")
    with torch.no_grad():
        outs = [sp.index_lstm_stage(rows, f, table, *_nets(torch.float32)) for _, f in forms]
        f64 = _nets(torch.float64)
        for out, (pairs, ind) in zip(outs, index):              # each form against the float64 reference form of its own rows
            truth = _reference_style_lstm(table.double()[pairs.long()], ind, *f64).view(2, -1, 16)
            assert float((out.double() - truth).abs().max()) <= 2e-5 * float(truth.abs().max())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3])
    if torch.equal(idx[0], idx[2]):
        assert torch.equal(outs[0], outs[2])


def test_refusals_on_the_device(sp):
    csr, z, table = _store(sp, 300, 1200, walks=8)
    edge = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    mlp, lstm = _nets(torch.float32)
    with pytest.raises(IndexError):
        sp.index_lstm_stage(edge, z, table[:1], mlp, lstm)
    with pytest.raises(ValueError, match="lstm_stage"):
        sp.index_lstm_stage(edge, z.aligned(), table, mlp, lstm)
    for bad in (torch.nn.LSTM(16, 16, batch_first=True, num_layers=2).cuda(), torch.nn.LSTM(16, 16, batch_first=False).cuda(),
                torch.nn.LSTM(16, 16, batch_first=True, bidirectional=True).cuda(), torch.nn.LSTM(16, 16, batch_first=True),
                torch.nn.LSTM(16, 16, batch_first=True).cuda().double(), torch.nn.GRU(16, 16, batch_first=True).cuda()):
        with pytest.raises((TypeError, ValueError), match="lstm_stage"):
            sp.index_lstm_stage(edge, z, table, mlp, bad)


def test_a_large_batch_segment_by_segment(sp):
    """B = 65,536 on a store with long rows, forward under no_grad; 64 sampled segments and those of at least L - 16 rows (the ones
    whose first rows still reach h_{L-1} under default init) against a float64 nn.LSTM on [1, L, H] padded to the batch's L (the
    dense batch is never built)"""
    csr, z, table = _store(sp, 20000, 120000, walks=100, seed=13)
    edge = torch.from_numpy(np.random.default_rng(7).integers(0, 20000, (2, 65536))).cuda()
    mlp, lstm = _nets(torch.float32, 32, 32)
    with torch.no_grad():
        out = sp.index_lstm_stage(edge, z, table, mlp, lstm).view(-1, 32)
        pairs, ind = sp.gather_index(edge, z)
        L = int((ind[1:] - ind[:-1]).max())
        assert L > 100
        m64, l64 = _nets(torch.float64, 32, 32)
        E = m64(table.double())
        longs = torch.nonzero(ind[1:] - ind[:-1] >= L - 16).view(-1).cpu().numpy()[:64]
        assert longs.size
        for j in np.union1d(np.random.default_rng(8).choice(2 * 65536, 64, replace=False), longs):
            p = pairs[int(ind[j]):int(ind[j + 1])].long()
            x = torch.zeros((1, L, 32), dtype=torch.float64, device="cuda")
            x[0, :p.shape[0]] = E[p[:, 0]] + E[p[:, 1]]
            ref = l64(x)[0][0, -1]
            assert float((out[j].double() - ref).abs().max()) <= 2e-5 * max(float(ref.abs().max()), 1e-3), j

"""GPU (MI355X): float_attn_stage -- the first model stage of the PPR / SPD / DEG encoders with attentional aggregation fused with the
join (subgacc_sjoin_relu_attn / _backward, model.py:59-62,78-81) -- equals the reference form  gather -> pe_embedding -> sum(-2) ->
AttentionalAggregation  in its output and in every parameter gradient; packed and headed stores, repeated runs and runs with or without
the backward's outputs give the same bits; rows too long to stage stream to the same result."""
import numpy as np
import pytest
import torch

import surel_plus_amd as spm
from gpu_helpers import _load, _spg_from_golden, sp, sym_graph  # noqa: F401
from gpu_helpers import _reference_attn_from_xz as _reference_from_xz

pytestmark = pytest.mark.gpu

STREAMED = 2        # flags[1] bit: a pair had a row too long to stage (include/subgacc.h, subgacc_sjoin_relu_attn)
# the tolerances of test_gpu_join.py::test_attn_stage_trains_like_the_reference_first_stage: forward within 2e-5 of the largest entry
# of the float64 reference form; every gradient within 5e-4 of its largest entry and no worse than max(4x the fp32 reference form's own
# error, 1e-4); the gate bias (analytically zero) under an absolute 1e-5
FWD_TOL, GRAD_TOL, GRAD_FLOOR, BIAS_ABS = 2e-5, 5e-4, 1e-4, 1e-5


def _nets(H, H2=16, H3=None, dtype=torch.float32, seed=1, bias=True):
    """(embed, gate_nn, value_nn or None) as the reference builds them for a float encoder, deterministic in `seed`"""
    torch.manual_seed(seed)
    embed = torch.nn.Sequential(torch.nn.Linear(1, H, bias=bias), torch.nn.ReLU(), torch.nn.Linear(H, H2))
    gate = torch.nn.Linear(H2, 1)
    val = torch.nn.Linear(H2, H3) if H3 else None
    return [m.to("cuda", dtype) if m is not None else None for m in (embed, gate, val)]


def _params(nets):
    return [p for m in nets if m is not None for p in m.parameters()]


def _reference(edge, x, nets):
    xz, ind = spm.gather(edge, x, "cuda", ptr=True)
    return _reference_from_xz(xz, ind, nets)


def _fwd_close(got, truth, tol=FWD_TOL):
    assert got.shape == truth.shape and got.dtype == torch.float32
    scale = float(truth.detach().abs().max())
    err = float((got.detach().double() - truth.detach().double()).abs().max())
    assert err <= tol * scale, (err, scale)


def _grads_close(fused, ref32, truth, tol=GRAD_TOL, floor=GRAD_FLOOR, bias_abs=BIAS_ABS):
    gate_bias = fused[1].bias
    for pa, pb, pc in zip(_params(fused), _params(ref32), _params(truth)):
        assert pa.grad is not None and pa.grad.dtype == torch.float32, tuple(pa.shape)
        if pa is gate_bias:                 # analytically zero (softmax is shift invariant)
            assert float(pa.grad.abs().max()) < bias_abs
            continue
        gs = float(pc.grad.abs().max())
        err_fused = float((pa.grad.double() - pc.grad).abs().max()) / gs
        err_ref32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        assert err_fused <= tol, (tuple(pa.shape), err_fused)
        assert err_fused <= max(4 * err_ref32, floor), (tuple(pa.shape), err_fused, err_ref32)


def _flags(out):
    return [int(v) for v in out.join_flags.tolist()]


def test_golden_store_matches_the_reference_form(sp):
    """over the golden float store: against the reference's own xz / indptr (sjoin_float.npz) and against gather's"""
    g = _load("sjoin_float.npz")
    z = _spg_from_golden(sp, g)
    edge = torch.from_numpy(g["edge"]).cuda()
    for H in (1, 96):
        nets = _nets(H)
        truth = _nets(H, dtype=torch.float64)
        with torch.no_grad():
            got = sp.float_attn_stage(edge, z, *nets)
            _fwd_close(got, _reference_from_xz(torch.from_numpy(g["xz_ptr1"]).cuda(), torch.from_numpy(g["ind_ptr1"]).cuda(), truth))
            _fwd_close(got, _reference(edge, z, truth))
        assert _flags(got) == [0, 0, 0, 0]


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


def _train_against_reference(edge, z, H, H3, tol=1.0):
    fused, ref32, truth = (_nets(H, H3=H3, dtype=d) for d in (torch.float32, torch.float32, torch.float64))
    H_out = H3 or 16
    torch.manual_seed(2)
    w = torch.randn(2, edge.shape[1], H_out, device="cuda")
    out = spm.float_attn_stage(edge, z, *fused)
    (out * w).sum().backward()
    r32 = _reference(edge, z, ref32)
    (r32 * w).sum().backward()
    r64 = _reference(edge, z, truth)
    (r64 * w.double()).sum().backward()
    _fwd_close(out, r64, tol * FWD_TOL)
    _grads_close(fused, ref32, truth, tol * GRAD_TOL, tol * GRAD_FLOOR, tol * BIAS_ABS)
    return out


@pytest.mark.parametrize("H3", [None, 24])
@pytest.mark.parametrize("H", [1, 96, 300])
def test_trains_like_the_reference_first_stage(store, H, H3):
    """forward and the gradients of every parameter of embed, gate_nn and value_nn against pe_embedding(xz).sum(-2) + attentional
    aggregation (model.py:59-62,78-81) evaluated in float64 on the full xz"""
    kind, z = store
    edge = torch.from_numpy(np.random.default_rng(H).integers(0, z.n_rows, (2, 512))).cuda()
    out = _train_against_reference(edge, z, H, H3)
    assert out.shape == (2, 512, H3 or 16)


def test_linear_without_bias_trains_too(sp):
    z = _store("PPR")
    edge = torch.from_numpy(np.random.default_rng(3).integers(0, z.n_rows, (2, 256))).cuda()
    fused, truth = _nets(96, bias=False), _nets(96, bias=False, dtype=torch.float64)
    w = torch.randn(2, 256, 16, device="cuda")
    (sp.float_attn_stage(edge, z, *fused) * w).sum().backward()
    (_reference(edge, z, truth) * w.double()).sum().backward()
    for pa, pc in zip(_params(fused), _params(truth)):
        gs = float(pc.grad.abs().max())
        if gs < 1e-9:
            assert float(pa.grad.abs().max()) < BIAS_ABS
        else:
            assert float((pa.grad.double() - pc.grad).abs().max()) <= GRAD_TOL * gs


def _run(edge, x, nets):
    """the stage's output and every gradient (for a fixed upstream gradient)"""
    for m in nets:
        if m is not None:
            m.zero_grad()
    out = spm.float_attn_stage(edge, x, *nets)
    torch.manual_seed(0)
    (out * torch.randn_like(out)).sum().backward()
    return out.detach(), [p.grad.clone() for p in _params(nets)], _flags(out)


def _bit_equal(a, b):
    assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])
    for ga, gb in zip(a[1], b[1]):
        assert torch.equal(ga, gb)


@pytest.mark.parametrize("kind", ["PPR", "DEG"])
def test_packed_headed_and_repeated_runs_give_the_same_bits(sp, kind):
    z = _store(kind)
    edge = torch.from_numpy(np.random.default_rng(5).integers(0, z.n_rows, (2, 700))).cuda()
    nets = _nets(96, H3=24)
    packed = _run(edge, z, nets)
    _bit_equal(packed, _run(edge, z, nets))
    _bit_equal(packed, _run(edge, z.aligned(), nets))
    with torch.no_grad():                  # the forward without m / den for the backward: the same A
        assert torch.equal(sp.float_attn_stage(edge, z.aligned(), *nets), packed[0])
        assert torch.equal(sp.float_attn_stage(edge, z, *nets), packed[0])


def test_hub_rows_past_the_lds_bound_stream(sp):
    """a DEG store whose hub rows are far longer than the 1,024 members the kernels stage: those pairs stream (flags[1] & 2) and give
    the reference form's result, packed and headed alike, bit for bit the same.  A hub segment sums ~4,200 terms one after the other
    in fp32 (the documented order), so this test allows 10x the short rows' tolerances."""
    z = _store("DEG", N=8000, hubs=2, seed=9)
    lens = z.indptr[1:] - z.indptr[:-1]
    assert int(lens[0]) > 1024 and int(lens[1]) > 1024
    rng = np.random.default_rng(2)
    e = rng.integers(0, z.n_rows, (2, 400))
    e[0, :40], e[1, 40:60], e[:, 60] = 0, 1, 0      # the hubs as left and right endpoints, and (hub, hub)
    edge = torch.from_numpy(e).cuda()
    fused = _train_against_reference(edge, z, 96, 24, tol=10.0)
    assert _flags(fused)[1] & STREAMED
    nets = _nets(96, H3=24)
    packed = _run(edge, z, nets)
    headed = _run(edge, z.aligned(), nets)
    assert packed[2][1] & STREAMED and headed[2][1] & STREAMED
    _bit_equal(packed, headed)
    with torch.no_grad():
        assert torch.equal(sp.float_attn_stage(edge, z.aligned(), *nets), packed[0])
        # no hub in the batch: nothing streams
        quiet = sp.float_attn_stage(torch.from_numpy(rng.integers(2, z.n_rows, (2, 64))).cuda(), z, *nets)
    assert not _flags(quiet)[1] & STREAMED


# ------------------------------------------------------------------------------------------------ edge cases
def test_self_pairs(sp):
    z = _store("PPR")
    u = np.random.default_rng(7).integers(0, z.n_rows, 100)
    edge = torch.from_numpy(np.stack([u, u])).cuda()
    nets = _nets(96)
    with torch.no_grad():
        got = sp.float_attn_stage(edge, z, *nets)
        _fwd_close(got, _reference(edge, z, _nets(96, dtype=torch.float64)))
        assert torch.equal(got[0], got[1])


def test_empty_rows_give_zero_rows(sp):
    g = _load("sjoin_float.npz")
    ip, ids, data = g["z_indptr"], g["z_indices"], g["z_data"]
    # every other row emptied: rows 0, 2, 4, ... keep nothing
    keep = np.repeat(np.arange(len(ip) - 1) % 2 == 1, np.diff(ip))
    nip = np.concatenate([[0], np.cumsum(np.where(np.arange(len(ip) - 1) % 2 == 1, np.diff(ip), 0))]).astype(np.int64)
    z = sp.SpG(torch.from_numpy(nip).cuda(), torch.from_numpy(ids[keep]).cuda(), torch.from_numpy(data[keep].astype(np.float64)).cuda())
    edge = torch.from_numpy(np.random.default_rng(1).integers(0, z.n_rows, (2, 300))).cuda()
    nets = _nets(96, H3=24)
    truth = _nets(96, H3=24, dtype=torch.float64)
    with torch.no_grad():
        for x in (z, z.aligned()):
            got = sp.float_attn_stage(edge, x, *nets)
            _fwd_close(got, _reference(edge, z, truth))
            empty = torch.from_numpy((np.asarray(edge.cpu()) % 2 == 0)).cuda()
            assert bool((got[empty] == 0).all()) and bool((got[~empty] != 0).any())


def test_empty_batch(sp):
    z = _store("PPR")
    nets = _nets(96, H2=24, H3=8)
    out = sp.float_attn_stage(torch.empty((2, 0), dtype=torch.int64, device="cuda"), z, *nets)
    assert out.shape == (2, 0, 8) and out.dtype == torch.float32
    out.sum().backward()                   # an empty batch still trains (zero gradients)
    for p in _params(nets):
        assert p.grad is not None and float(p.grad.abs().sum()) == 0.0


def test_row_outside_the_store_raises(sp):
    z = _store("PPR")
    nets = _nets(8)
    for bad in (z.n_rows, -1):
        edge = torch.tensor([[0, 5], [bad, 3]], device="cuda")
        for x in (z, z.aligned()):
            with pytest.raises(IndexError):
                sp.float_attn_stage(edge, x, *nets)


def test_mrr_shaped_list(sp):
    """the MRR evaluation (train.py:246-280): 1 source x 1,000 targets as the expanded [2, P*K] list"""
    z = _store("SPD")
    rng = np.random.default_rng(11)
    src, tgt = int(rng.integers(0, z.n_rows)), rng.integers(0, z.n_rows, 1000)
    edge = torch.from_numpy(np.stack([np.full(1000, src), tgt])).cuda()
    nets = _nets(96, H3=24)
    with torch.no_grad():
        got = sp.float_attn_stage(edge, z, *nets)
        _fwd_close(got, _reference(edge, z, _nets(96, H3=24, dtype=torch.float64)))
        assert torch.equal(sp.float_attn_stage(edge, z.aligned(), *nets), got)

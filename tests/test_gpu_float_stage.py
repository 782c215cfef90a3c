"""GPU (MI355X): float_mean_stage -- the first model stage of the PPR / SPD / DEG encoders fused with the join (subgacc_sjoin_relu_mean,
model.py:78-83) -- equals the reference form  gather -> pe_embedding -> sum(-2) -> segment mean  in its output and in all four
parameter gradients; packed and headed stores and repeated runs give the same bits; rows too long to stage stream to the same result."""
import numpy as np
import pytest
import torch

import surel_plus_amd as spm
from gpu_helpers import _load, _spg_from_golden, sp, sym_graph  # noqa: F401
from gpu_helpers import _reference_mean_from_xz as _reference_from_xz

pytestmark = pytest.mark.gpu

STREAMED = 2        # flags[1] bit: a pair had a row too long to stage (include/subgacc.h, subgacc_sjoin_relu_mean)
# the tolerances of test_gpu_join.py::test_mean_stage_trains_like_the_reference_first_stage: forward rtol 1e-4 / atol 1e-5,
# gradients 1e-4 of their largest entry.  Gradients are compared with the reference form evaluated in float64: in fp32 it sums ~1e5
# rows per entry of w1 / b1 with cancelling signs and is itself off by more than that (1.2e-4 of the entry at H = 1, DEG store).
RTOL, ATOL, GRAD_TOL = 1e-4, 1e-5, 1e-4


def _mlp(H, H2=16, seed=1, bias=True):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(1, H, bias=bias), torch.nn.ReLU(), torch.nn.Linear(H, H2)).cuda()


def _twin(mlp, dtype=torch.float64):
    """the same module, by default in float64 (the exact answer the fp32 forms are compared with)"""
    other = _mlp(mlp[0].out_features, mlp[2].out_features, bias=mlp[0].bias is not None)
    other.load_state_dict(mlp.state_dict())
    return other.to(dtype)


def _reference(edge, x, mlp):
    xz, ind = spm.gather(edge, x, "cuda", ptr=True)
    return _reference_from_xz(xz, ind, mlp)


def _close(got, want, rtol=RTOL, atol=ATOL):
    assert got.shape == want.shape and got.dtype == torch.float32
    want = want.detach().to(torch.float32)
    assert torch.allclose(got, want, rtol=rtol, atol=atol), float((got - want).abs().max())


def _grads_close(a, b, tol=GRAD_TOL):
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert pa.grad is not None and pb.grad is not None and pa.grad.dtype == torch.float32
        err = float((pa.grad.double() - pb.grad.double()).abs().max())
        assert err <= tol * float(pb.grad.abs().max()) + 1e-6, (tuple(pa.shape), err, float(pb.grad.abs().max()))


def _flags(out):
    return [int(v) for v in out.join_flags.tolist()]


def test_golden_store_matches_the_reference_form(sp):
    """over the golden float store: against the reference's own xz / indptr (sjoin_float.npz) and against gather's"""
    g = _load("sjoin_float.npz")
    z = _spg_from_golden(sp, g)
    edge = torch.from_numpy(g["edge"]).cuda()
    for H in (1, 96):
        mlp = _mlp(H)
        with torch.no_grad():
            got = sp.float_mean_stage(edge, z, mlp)
            want = _reference_from_xz(torch.from_numpy(g["xz_ptr1"]).cuda(), torch.from_numpy(g["ind_ptr1"]).cuda(), mlp)
            _close(got, want)
            _close(got, _reference(edge, z, mlp))
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


@pytest.mark.parametrize("H", [1, 96, 300])
def test_trains_like_the_reference_first_stage(store, H):
    """forward and the gradients of w1, b1, W2, b2 against pe_embedding(xz).sum(-2) + mean aggregation (model.py:78-83)"""
    kind, z = store
    edge = torch.from_numpy(np.random.default_rng(H).integers(0, z.n_rows, (2, 512))).cuda()
    mlp_a = _mlp(H)
    mlp_b = _twin(mlp_a)
    w = torch.randn(2, 512, 16, device="cuda")
    fused = spm.float_mean_stage(edge, z, mlp_a)
    (fused * w).sum().backward()
    ref = _reference(edge, z, mlp_b)
    (ref * w.double()).sum().backward()
    _close(fused, ref)
    with torch.no_grad():                  # and the forward against the reference form as it runs, in fp32
        _close(fused, _reference(edge, z, _twin(mlp_a, torch.float32)))
    _grads_close(mlp_a, mlp_b)


def test_linear_without_bias_trains_too(sp):
    z = _store("PPR")
    edge = torch.from_numpy(np.random.default_rng(3).integers(0, z.n_rows, (2, 256))).cuda()
    mlp_a = _mlp(96, bias=False)
    mlp_b = _twin(mlp_a)
    w = torch.randn(2, 256, 16, device="cuda")
    (sp.float_mean_stage(edge, z, mlp_a) * w).sum().backward()
    (_reference(edge, z, mlp_b) * w.double()).sum().backward()
    _grads_close(mlp_a, mlp_b)


def _run(edge, x, mlp):
    """the stage's output and its four gradients (for a fixed upstream gradient)"""
    mlp.zero_grad()
    out = spm.float_mean_stage(edge, x, mlp)
    torch.manual_seed(0)
    (out * torch.randn_like(out)).sum().backward()
    return out.detach(), [p.grad.clone() for p in mlp.parameters()], _flags(out)


def _bit_equal(a, b):
    assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])
    for ga, gb in zip(a[1], b[1]):
        assert torch.equal(ga, gb)


@pytest.mark.parametrize("kind", ["PPR", "DEG"])
def test_packed_headed_and_repeated_runs_give_the_same_bits(sp, kind):
    z = _store(kind)
    edge = torch.from_numpy(np.random.default_rng(5).integers(0, z.n_rows, (2, 700))).cuda()
    mlp = _mlp(96)
    packed = _run(edge, z, mlp)
    _bit_equal(packed, _run(edge, z, mlp))
    _bit_equal(packed, _run(edge, z.aligned(), mlp))
    with torch.no_grad():                  # the forward without the backward sums: the same M
        assert torch.equal(sp.float_mean_stage(edge, z.aligned(), mlp), packed[0])


def test_hub_rows_past_the_lds_bound_stream(sp):
    """a DEG store whose hub row (adjacency ~N/4 + its PPR set) is far longer than the 1,024 members the kernel stages: those pairs
    stream (flags[1] & 2) and give the reference form's result, packed and headed alike, bit for bit the same.  A hub segment adds
    ~4,200 terms one after the other in fp32 (the documented order): its rounding error grows with that count (n * 2^-24 = 2.5e-4 of
    the sum at most), so this test allows 10x the short rows' tolerances (measured: 8.3e-5 off the float64 form at rtol 1e-4)."""
    z = _store("DEG", N=8000, hubs=2, seed=9)
    lens = z.indptr[1:] - z.indptr[:-1]
    assert int(lens[0]) > 1024 and int(lens[1]) > 1024
    rng = np.random.default_rng(2)
    e = rng.integers(0, z.n_rows, (2, 400))
    e[0, :40], e[1, 40:60], e[:, 60] = 0, 1, 0      # the hubs as left and right endpoints, and (hub, hub)
    edge = torch.from_numpy(e).cuda()
    mlp_a = _mlp(96)
    mlp_b = _twin(mlp_a)
    w = torch.randn(2, 400, 16, device="cuda")
    fused = sp.float_mean_stage(edge, z, mlp_a)
    assert _flags(fused)[1] & STREAMED
    (fused * w).sum().backward()
    ref = _reference(edge, z, mlp_b)
    (ref * w.double()).sum().backward()
    _close(fused, ref, 10 * RTOL, 10 * ATOL)
    _grads_close(mlp_a, mlp_b, 10 * GRAD_TOL)
    packed = _run(edge, z, mlp_a)
    headed = _run(edge, z.aligned(), mlp_a)
    assert headed[2][1] & STREAMED
    _bit_equal(packed, headed)
    # no hub in the batch: nothing streams
    quiet = sp.float_mean_stage(torch.from_numpy(rng.integers(2, z.n_rows, (2, 64))).cuda(), z, mlp_a)
    assert not _flags(quiet)[1] & STREAMED


# ------------------------------------------------------------------------------------------------ edge cases
def test_self_pairs(sp):
    z = _store("PPR")
    u = np.random.default_rng(7).integers(0, z.n_rows, 100)
    edge = torch.from_numpy(np.stack([u, u])).cuda()
    mlp = _mlp(96)
    with torch.no_grad():
        got = sp.float_mean_stage(edge, z, mlp)
        _close(got, _reference(edge, z, mlp))
        assert torch.equal(got[0], got[1])


def test_empty_rows_give_zero_rows(sp):
    g = _load("sjoin_float.npz")
    ip, ids, data = g["z_indptr"], g["z_indices"], g["z_data"]
    # every other row emptied: rows 0, 2, 4, ... keep nothing
    keep = np.repeat(np.arange(len(ip) - 1) % 2 == 1, np.diff(ip))
    nip = np.concatenate([[0], np.cumsum(np.where(np.arange(len(ip) - 1) % 2 == 1, np.diff(ip), 0))]).astype(np.int64)
    z = sp.SpG(torch.from_numpy(nip).cuda(), torch.from_numpy(ids[keep]).cuda(), torch.from_numpy(data[keep].astype(np.float64)).cuda())
    edge = torch.from_numpy(np.random.default_rng(1).integers(0, z.n_rows, (2, 300))).cuda()
    mlp = _mlp(96)
    with torch.no_grad():
        for x in (z, z.aligned()):
            got = sp.float_mean_stage(edge, x, mlp)
            _close(got, _reference(edge, z, mlp))
            empty = torch.from_numpy((np.asarray(edge.cpu()) % 2 == 0)).cuda()
            assert bool((got[empty] == 0).all()) and bool((got[~empty] != 0).any())


def test_empty_batch(sp):
    z = _store("PPR")
    mlp = _mlp(96, H2=24)
    out = sp.float_mean_stage(torch.empty((2, 0), dtype=torch.int64, device="cuda"), z, mlp)
    assert out.shape == (2, 0, 24) and out.dtype == torch.float32
    out.sum().backward()                   # an empty batch still trains (zero gradients)
    assert float(mlp[0].weight.grad.abs().sum()) == 0.0


def test_row_outside_the_store_raises(sp):
    z = _store("PPR")
    mlp = _mlp(8)
    for bad in (z.n_rows, -1):
        edge = torch.tensor([[0, 5], [bad, 3]], device="cuda")
        for x in (z, z.aligned()):
            with pytest.raises(IndexError):
                sp.float_mean_stage(edge, x, mlp)


def test_mrr_shaped_list(sp):
    """the MRR evaluation (train.py:246-280): 1 source x 1,000 targets as the expanded [2, P*K] list"""
    z = _store("SPD")
    rng = np.random.default_rng(11)
    src, tgt = int(rng.integers(0, z.n_rows)), rng.integers(0, z.n_rows, 1000)
    edge = torch.from_numpy(np.stack([np.full(1000, src), tgt])).cuda()
    mlp = _mlp(96)
    with torch.no_grad():
        got = sp.float_mean_stage(edge, z, mlp)
        _close(got, _reference(edge, z, mlp))
        _close(sp.float_mean_stage(edge, z.aligned(), mlp), got)

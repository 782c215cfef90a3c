"""GPU (MI355X): the fused first stages -- float_mean_stage, float_attn_stage and counts_attn_stage (csrc/sjoin_f64stage.hip:
sjoin_f64mean_kernel, sjoin_f64attn_kernel; csrc/sjoin_forms.hip: sjoin_counts_attn_kernel) -- on stores whose row lengths sit at every boundary of the
kernels' code paths, and at every width boundary of their channel loops:
  * f64pair_stage's register trips (4 x 128 = 512 members), its span loop and the T rows it loads after them (513 ... 1,024), the staged
    / streamed cut (kMeanCap = 1,024), the streamed pairs' blocks of 128 channels (H > 128), H = 1,024 (the documented maximum);
  * the count kernel's S members past its two trips of 256, more than 256 distinct LP rows in a block, a table smaller than a block's
    members (D = T), and dynamic LDS past 64 KiB;
  * a store whose forward fits LDS and whose backward does not: refused before the forward under autograd, run under no_grad.
The truth is the oracle's join (oracle.gather, the C restatement the golden files pin) through the reference form in float64, never the
library's own join; the tolerances are those of test_gpu_float_stage.py, test_gpu_float_attn.py and test_gpu_counts_attn.py."""
import numpy as np
import pytest
import torch

import oracle
import surel_plus_amd as spm
from gpu_helpers import _reference_attn_from_xz, _reference_mean_from_xz, _reference_style_attn, sp  # noqa: F401

pytestmark = pytest.mark.gpu

STREAMED = 2        # flags[1] bit: a pair had a row too long to stage (include/subgacc.h, subgacc_sjoin_relu_mean / _attn)
STAGE_CAP = 1024    # kMeanCap: the longest row the float stages stage
# test_gpu_float_stage.py's tolerances (forward rtol / atol, gradients of their largest entry) ...
M_RTOL, M_ATOL, M_GRAD = 1e-4, 1e-5, 1e-4
# ... test_gpu_float_attn.py's and test_gpu_counts_attn.py's (forward of the largest entry; every gradient within GRAD of its largest
# entry and no worse than max(4x the fp32 reference form's own error, FLOOR); the float gate bias, analytically zero, under BIAS_ABS)
A_FWD, A_GRAD, A_FLOOR, A_BIAS = 2e-5, 5e-4, 1e-4, 1e-5
# a segment of a row longer than STAGE_CAP adds its terms one after the other in fp32 (the documented order): test_gpu_float_stage.py /
# test_gpu_float_attn.py's hub tests allow 10x the short rows' tolerances for it, and so do these
LONG = 10.0
# the fused attention backward forms beta_t = alpha_t (G_j . r_t - G_j . A_j) from two H-long fp32 dot products (the reference form's
# are H' = 16 long) and sums n_j of them one after the other.  The gate weight's gradient is the sum of those terms with most of it
# cancelling: past the register trips (segments of more than 512 members) its error reaches 3.5e-4 of its largest entry (max_len 513,
# H = 129; the fp32 reference form's own 7.6e-5 to 9.0e-5, varying from run to run with its atomic sums; every other gradient below
# 3e-6), so there the floor is the 5e-4 bound that holds for every gradient anyway
LONG_ATTN_FLOOR = 5.0
# the float64 reference holds [R, 2, H] activations: R * H stays under this
RH_BUDGET = 4e7


# ------------------------------------------------------------------------------------------------ stores with controlled row lengths
def _rows(max_len, N, seed):
    """N sorted, unique rows of lengths in [0, max_len] -- rows 0 and 1 of max_len, row 2 empty, row 3 of max_len - 1 -- over a span of
    1.75 max_len ids, so that partners share many members and miss many"""
    rs = np.random.default_rng(seed)
    span = max(2, int(1.75 * max_len))
    lens = rs.integers(0, max_len + 1, N)
    lens[:4] = [max_len, max_len, 0, max(max_len - 1, 0)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rs.choice(span, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rs, span, lens, indptr, ids


_STORES = {}


def _float_store(max_len, N=600):
    """(packed SpG, its headed form, lens, (indptr, ids, data) on the host): float64 payload in (0, 1]"""
    if max_len not in _STORES:
        rs, span, lens, indptr, ids = _rows(max_len, N, 1000 + max_len)
        data = 1.0 - rs.random(ids.size)
        z = spm.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(data).cuda(), max_len=max_len,
                    shape=(N, span))
        _STORES[max_len] = (z, z.aligned(), lens, (indptr, ids, data))
    return _STORES[max_len]


def _pairs(lens, H, seed, cap=160):
    """the boundary pairs -- (longest, longest), (longest, longest - 1), (longest, empty), (u, u), the longest row as the left and as the
    right endpoint (the kernels make the shorter row S) -- then random pairs while R * H stays within the budget"""
    e = np.array([[0, 0, 0, 3, 0, 2, 1, 5, 2, 3],
                  [1, 0, 3, 0, 2, 0, 0, 5, 2, 1]], np.int64)
    rs = np.random.default_rng(seed)
    R = int(lens[e].sum())
    n = int((RH_BUDGET / H - R) / (2 * lens.mean() + 1))
    n = max(8, min(cap - e.shape[1], n))
    return np.concatenate([e, rs.integers(0, len(lens), (2, n))], axis=1)


# ------------------------------------------------------------------------------------------------ the float stages
def _nets(stage, H, dtype):
    """float_mean_stage: [embed]; float_attn_stage: [embed, gate_nn, value_nn or None] -- the modules of test_gpu_float_stage.py /
    test_gpu_float_attn.py (seed 1, H' = 16, H'' = 24), the same values in every dtype"""
    torch.manual_seed(1)
    embed = torch.nn.Sequential(torch.nn.Linear(1, H), torch.nn.ReLU(), torch.nn.Linear(H, 16))
    mods = [embed] if stage == "mean" else [embed, torch.nn.Linear(16, 1), torch.nn.Linear(16, 24) if stage == "attn_value" else None]
    return [m.to("cuda", dtype) if m is not None else None for m in mods]


def _params(nets):
    return [p for m in nets if m is not None for p in m.parameters()]


def _fused(stage, edge, x, nets):
    return spm.float_mean_stage(edge, x, nets[0]) if stage == "mean" else spm.float_attn_stage(edge, x, *nets)


def _reference_form(stage, xz, ind, nets):
    return _reference_mean_from_xz(xz, ind, nets[0]) if stage == "mean" else _reference_attn_from_xz(xz, ind, nets)


def _run(stage, edge, x, nets, w):
    """the stage's output, every parameter gradient for the upstream gradient w, and the status words"""
    for p in _params(nets):
        p.grad = None
    out = _fused(stage, edge, x, nets)
    (out * w).sum().backward()
    return out.detach().clone(), [p.grad.clone() for p in _params(nets)], [int(v) for v in out.join_flags.tolist()]


def _bit_equal(a, b):
    assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])
    for ga, gb in zip(a[1], b[1]):
        assert torch.equal(ga, gb)


def _check_mean(fused, ref32, truth, nets, r32, r64, k):
    """test_gpu_float_stage.py's tolerances, each no tighter than 4x the fp32 reference form's own error"""
    out, grads = fused[0], fused[1]
    assert out.dtype == torch.float32 and out.shape == r64.shape
    t = r64.detach()
    den = M_ATOL + M_RTOL * t.abs()
    err = float(((out.double() - t).abs() / den).max())
    err32 = float(((r32.detach().double() - t).abs() / den).max())
    assert err <= max(4 * err32, k), ("forward: error / (atol + rtol |truth|)", err, err32)
    for ga, pb, pc in zip(grads, _params(ref32), _params(truth)):
        gs = float(pc.grad.abs().max())
        e = float((ga.double() - pc.grad).abs().max())
        e32 = float((pb.grad.double() - pc.grad).abs().max())
        assert e <= max(4 * e32, k * M_GRAD * gs + 1e-6), (tuple(ga.shape), e, e32, gs)


def _check_attn(fused, ref32, truth, nets, r32, r64, k, kf=1.0):
    """test_gpu_float_attn.py's tolerances: forward and every gradient no worse than max(4x the fp32 reference form's error, the floor),
    every gradient within GRAD of its largest entry, the gate bias's (analytically zero) under BIAS_ABS"""
    out, grads = fused[0], fused[1]
    assert out.dtype == torch.float32 and out.shape == r64.shape
    t = r64.detach()
    scale = float(t.abs().max())
    err = float((out.double() - t).abs().max()) / scale
    err32 = float((r32.detach().double() - t).abs().max()) / scale
    assert err <= max(4 * err32, k * A_FWD), ("forward", err, err32)
    gate_bias = nets[1].bias
    for ga, pa, pb, pc in zip(grads, _params(nets), _params(ref32), _params(truth)):
        if pa is gate_bias:
            assert float(ga.abs().max()) < k * A_BIAS
            continue
        gs = float(pc.grad.abs().max())
        if gs == 0.0:
            assert float(ga.abs().max()) == 0.0, tuple(ga.shape)
            continue
        e = float((ga.double() - pc.grad).abs().max()) / gs
        e32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        assert e <= k * A_GRAD, (tuple(ga.shape), e)
        assert e <= max(4 * e32, kf * k * A_FLOOR), (tuple(ga.shape), e, e32)


def _float_case(stage, max_len, H):
    z, zh, lens, host = _float_store(max_len)
    e = _pairs(lens, H, seed=max_len + H)
    edge = torch.from_numpy(e).cuda()
    B = e.shape[1]
    nets = _nets(stage, H, torch.float32)
    H_out = 16 if stage != "attn_value" else 24
    w = torch.randn(2, B, H_out, device="cuda", generator=torch.Generator("cuda").manual_seed(max_len + H))

    packed = _run(stage, edge, z, nets, w)
    # the status words: a pair streamed exactly when one of its rows is longer than the kernels stage; nothing refused
    streamed = bool((lens[e] > STAGE_CAP).any())
    assert bool(packed[2][1] & STREAMED) == streamed and packed[2][3] == 0, packed[2]

    # the truth: the oracle's join through the reference form in float64; the same form in fp32 for its own error
    oxz, oind = oracle.gather(e, host, ptr=True)
    xz, ind = torch.from_numpy(oxz).cuda(), torch.from_numpy(oind).cuda()
    assert ind.numel() == 2 * B + 1 and int(ind[-1]) == int(lens[e].sum())
    ref32, truth = _nets(stage, H, torch.float32), _nets(stage, H, torch.float64)
    r32 = _reference_form(stage, xz, ind, ref32)
    (r32 * w).sum().backward()
    r64 = _reference_form(stage, xz, ind, truth)
    (r64 * w.double()).sum().backward()
    k = LONG if streamed else 1.0
    if stage == "mean":
        _check_mean(packed, ref32, truth, nets, r32, r64, k)
    else:
        _check_attn(packed, ref32, truth, nets, r32, r64, k, LONG_ATTN_FLOOR if (lens[e] > 512).any() and not streamed else 1.0)

    # the same bits: a repeated run, the headed store, and the forward without the backward's outputs (mean: no P / Q; attention: no
    # m / den)
    _bit_equal(packed, _run(stage, edge, z, nets, w))
    headed = _run(stage, edge, zh, nets, w)
    _bit_equal(packed, headed)
    assert headed[2] == packed[2]
    with torch.no_grad():
        assert torch.equal(_fused(stage, edge, z, nets), packed[0])
        assert torch.equal(_fused(stage, edge, zh, nets), packed[0])


STAGES = ["mean", "attn", "attn_value"]


@pytest.mark.parametrize("max_len", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2100])
@pytest.mark.parametrize("stage", STAGES)
def test_float_stage_at_every_row_length_boundary(sp, stage, max_len):
    """64: a wave of S's spans; 128: the workgroup; 512: the register trips; 513 - 1,024: the span loop and T's rows loaded after the
    trips; 1,024 / 1,025: the staged / streamed cut; 2,100: streamed, the headed store too"""
    _float_case(stage, max_len, 96)


@pytest.mark.parametrize("H", [1, 127, 128, 129, 1024])
@pytest.mark.parametrize("max_len", [513, 1025])
@pytest.mark.parametrize("stage", STAGES)
def test_float_stage_at_every_width_boundary(sp, stage, max_len, H):
    """H around the 128 lanes of the channel loops, and the documented maximum 1,024, on a staged (513) and a streamed (1,025) store:
    the streamed pairs' blocks of 128 channels"""
    _float_case(stage, max_len, H)


@pytest.mark.parametrize("stage", STAGES)
def test_streamed_and_staged_segments_give_the_same_bits(sp, stage):
    """one own row (700 members) against a partner of 2,100 members (the pair streams) and against that partner cut down to the members
    they share plus a few others (the pair is staged): the own row's segment holds the same (a, b) members in the same order both times,
    and the kernels promise the same sequence of additions on both paths -- so the same bits, at H = 200 (two blocks of channels)"""
    rs = np.random.default_rng(31)
    span = 4000
    long_ = np.sort(rs.choice(span, 2100, replace=False))
    own = np.sort(np.concatenate([rs.choice(long_, 350, replace=False),
                                  rs.choice(np.setdiff1d(np.arange(span), long_), 350, replace=False)]))
    shared = np.intersect1d(long_, own)
    cut = np.sort(np.concatenate([shared, rs.choice(np.setdiff1d(long_, own), 60, replace=False)]))
    vals_long = 1.0 - rs.random(long_.size)
    rows = [(own, 1.0 - rs.random(own.size)), (long_, vals_long), (cut, vals_long[np.searchsorted(long_, cut)])]
    indptr = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    ids = np.concatenate([r[0] for r in rows]).astype(np.int32)
    data = np.concatenate([r[1] for r in rows])
    z = spm.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(data).cuda(), shape=(3, span))
    assert z.max_len == 2100 and len(cut) <= STAGE_CAP
    edge = torch.tensor([[0, 0, 1, 2], [1, 2, 0, 0]], device="cuda")      # row 0 as the left and as the right endpoint
    nets = _nets(stage, 200, torch.float32)
    with torch.no_grad():
        for x in (z, z.aligned()):
            out = _fused(stage, edge, x, nets)
            assert out.join_flags[1] & STREAMED
            assert torch.equal(out[0, 0], out[0, 1]) and torch.equal(out[1, 2], out[1, 3])
            assert bool(out[0, 0].ne(0).any())


# ------------------------------------------------------------------------------------------------ counts_attn_stage
def _counts_nets(dtype):
    """test_gpu_counts_attn.py's modules (seed 7, H = 16, a value net)"""
    torch.manual_seed(7)
    H = 16
    mods = [torch.nn.Sequential(torch.nn.Linear(4, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.Linear(H, 1),
            torch.nn.Linear(H, H)]
    return [m.to("cuda", dtype) for m in mods]


def _lp_store(max_len, T, N=600):
    """a packed SFptr store of rows of controlled length (SFptr in [1, T)) and a [T, 4] table; host arrays for the oracle"""
    rs, span, lens, indptr, ids = _rows(max_len, N, 2000 + max_len + T)
    data = rs.integers(1, T, ids.size).astype(np.int32)
    table = rs.random((T, 4)).astype(np.float32)
    z = spm.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(data).cuda(), max_len=max_len,
                shape=(N, span))
    return z, torch.from_numpy(table).cuda(), lens, (indptr, ids, data), table


def _counts_reference(e, host, table_np, nets, double):
    oxz, oind = oracle.gather(e, host, ptr=True, encode=table_np)
    xz, ind = torch.from_numpy(oxz).cuda(), torch.from_numpy(oind).cuda()
    return _reference_style_attn(xz.double() if double else xz, ind, nets[0], nets[1], nets[2]).view(2, e.shape[1], -1)


@pytest.mark.parametrize("T", [5, 300, 12000])
@pytest.mark.parametrize("max_len", [255, 256, 257, 511, 512, 513, 600])
def test_counts_attn_at_every_row_length_boundary(sp, max_len, T):
    """256: one trip of the workgroup; 512: the two trips held in registers, S's members past them read in the loop; T = 5: fewer LP rows
    than a block's members (D = T); T = 300: more than 256 distinct rows in a block; T = 12,000: forward ~122 KB and backward ~142 KB of
    LDS (past 64 KiB).  Forward and the gradients of embed, gate and value against the oracle's join through the reference form in
    float64; repeated runs, permuted pairs and swapped endpoints give the same bits."""
    z, table, lens, host, table_np = _lp_store(max_len, T)
    e = _pairs(lens, 16, seed=max_len + T, cap=128)
    edge = torch.from_numpy(e).cuda()
    B = e.shape[1]
    fa, fb, f64 = _counts_nets(torch.float32), _counts_nets(torch.float32), _counts_nets(torch.float64)
    w = torch.randn(2, B, 16, device="cuda", generator=torch.Generator("cuda").manual_seed(max_len + T))
    fused = spm.counts_attn_stage(edge, z, table, *fa)
    assert [int(v) for v in fused.join_flags.tolist()] == [0, 0, 0, 0]
    (fused * w).sum().backward()
    r32 = _counts_reference(e, host, table_np, fb, False)
    (r32 * w).sum().backward()
    truth = _counts_reference(e, host, table_np, f64, True)
    (truth * w.double()).sum().backward()
    scale = float(truth.detach().abs().max())
    assert float((fused.detach().double() - truth.detach()).abs().max()) <= A_FWD * scale
    for pa, pb, pc in zip(_params(fa), _params(fb), _params(f64)):
        if pa is fa[1].bias:
            assert float(pa.grad.abs().max()) == 0.0          # the gate bias: exactly zero
            continue
        gs = float(pc.grad.abs().max())
        err = float((pa.grad.double() - pc.grad).abs().max()) / gs
        err32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        assert err <= A_GRAD, (tuple(pa.shape), err)
        assert err <= max(4 * err32, A_FLOOR), (tuple(pa.shape), err, err32)

    # a repeated run: the same bits in the output and every gradient
    first = (fused.detach().clone(), [p.grad.clone() for p in _params(fa)])
    for p in _params(fa):
        p.grad = None
    again = spm.counts_attn_stage(edge, z, table, *fa)
    (again * w).sum().backward()
    _bit_equal(first, (again.detach(), [p.grad for p in _params(fa)]))
    # permuted pairs and swapped endpoints: the same rows, bit for bit (and without the backward's outputs the same output)
    perm = torch.from_numpy(np.random.default_rng(T).permutation(B)).cuda()
    with torch.no_grad():
        out = spm.counts_attn_stage(edge, z, table, *fa)
        assert torch.equal(out, first[0])
        assert torch.equal(spm.counts_attn_stage(edge[:, perm], z, table, *fa), out[:, perm])
        assert torch.equal(spm.counts_attn_stage(edge.flip(0), z, table, *fa), out.flip(0))


def test_counts_attn_refuses_a_forward_whose_backward_does_not_fit(sp):
    """rows of 1,500 members and 10,000 LP rows: the forward needs 146,032 B of LDS, the backward 194,032 B, of 160 KiB.  Under autograd
    the stage refuses (SUBGACC_ERR_LDS) before its forward runs (not inside .backward(), in the middle of a training step); under no_grad the forward runs
    (~146 KB of dynamic LDS) and gives the reference form's result"""
    z, table, lens, host, table_np = _lp_store(1500, 10000, N=200)
    e = _pairs(lens, 16, seed=5, cap=40)
    edge = torch.from_numpy(e).cuda()
    nets = _counts_nets(torch.float32)
    with pytest.raises(ValueError, match="the backward needs 194032 B of LDS"):      # SUBGACC_ERR_LDS, as _lib.check raises it
        spm.counts_attn_stage(edge, z, table, *nets)
    with torch.no_grad():
        got = spm.counts_attn_stage(edge, z, table, *nets)
        truth = _counts_reference(e, host, table_np, _counts_nets(torch.float64), True)
    assert [int(v) for v in got.join_flags.tolist()] == [0, 0, 0, 0]
    assert float((got.double() - truth).abs().max()) <= A_FWD * float(truth.abs().max())

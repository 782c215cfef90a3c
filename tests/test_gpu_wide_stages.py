"""GPU (MI355X): the on-demand model stages over 64-bit key rows (wide_keys=True: 4 hops, M = 128 .. 204 -- the paper's citation2
sampler setting is M = 200) -- sample_and_counts / sample_and_hcounts against gather_counts / hgather_counts over the 4-hop all-nodes
store, sample_and_index against the row form over KEY64 rows, sample_and_attn_counts against the packed store's attentional kernel,
one result whatever the route, the captured step, the three model stages against their reference forms with the tolerances of the
3-hop tests, the overflow, and the two ends of the shape range.  Counts, sizes, pairs, pointers and feature rows are compared bit
for bit."""
import numpy as np
import pytest
import torch

from gpu_helpers import _reference_style_attn, sp  # noqa: F401
from test_gpu_counts_attn import FWD_TOL, GRAD_FLOOR, GRAD_TOL
from test_gpu_horder import M, World
from test_gpu_lstm_aggr import _nets as _lstm_nets, _reference_style_lstm
from test_gpu_step_attn import _column_of_store_rows, _random
from test_gpu_step_stage import _dicts, _reference_stage

pytestmark = pytest.mark.gpu

HOPS = 4
MAX_T = 8192
KW = dict(num_walks=M, num_steps=HOPS, seed=5, wide_keys=True)


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, n=3):
    return all(x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a[:n], b[:n]))


# ------------------------------------------------------------------------------------------------------------------ the shape
def test_the_shape_has_64_bit_keys_and_is_refused_without_the_keyword(sp, world):
    from surel_plus_amd import sampler
    assert sampler.key_rows_form(M, HOPS) == 64
    e = world.pairs(40, 1)[:, :8].contiguous()
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_counts(world.csr, e, num_walks=M, num_steps=HOPS, seed=5)
    with pytest.raises(ValueError, match="table_rows = 8193"):
        sp.StepBuffers(world.csr, 8, num_walks=M, num_steps=HOPS, stage="counts", table_rows=8193, wide_keys=True)
    bufs = sp.StepBuffers(world.csr, 8, num_walks=M, num_steps=HOPS, stage="counts", table_rows=64, wide_keys=True)
    assert bufs.wide and bufs.key64 and bufs.slot.dtype == torch.int64 and bufs.stride == 832
    assert bufs.cols.dtype == torch.int32 and bufs.cols.shape == bufs.slot.shape and bufs.ukeys64.shape == (63,)
    assert bufs.ukeys.shape == (63,) and bufs.col_ws.numel() == 1024 * 8
    with pytest.raises(ValueError, match="buffers= serves the step its StepBuffers were made for"):
        sp.sample_and_counts(world.csr, e, num_walks=M, num_steps=HOPS, seed=5, buffers=bufs)       # the call lacks the keyword
    narrow = sp.StepBuffers(world.csr, 8, num_walks=M, num_steps=3, stage="counts", table_rows=64, wide_keys=True)
    assert not narrow.wide and not hasattr(narrow, "cols") and narrow.slot.dtype == torch.int32      # nothing changes at 3 hops
    a = sp.sample_and_counts(world.csr, e, num_walks=M, num_steps=3, seed=5, table_rows=2048, wide_keys=True)
    b = sp.sample_and_counts(world.csr, e, num_walks=M, num_steps=3, seed=5, table_rows=2048)
    assert _same(a, b)


# ------------------------------------------------------------------------------------------------------ counts against the store
def test_pair_counts_equal_gather_counts_over_the_store(sp, world):
    """per segment the same {feature row: count} and the same sizes as gather_counts over the 4-hop all-nodes store of the same seed.
    table_rows is the store's own row count: the reference path alone decides that no overflow occurs."""
    z, table, lens = world.store(HOPS)
    T = table.shape[0]
    print(f"the 4-hop store: {T - 1} distinct LP rows")
    assert T <= MAX_T
    e = world.pairs(300, 1)
    en = e.cpu().numpy()
    assert (en[0] == en[1]).any() and all((en == s).any() for s in world.special)
    Cr, sizes_r = sp.gather_counts(e, z, T)
    Cm, sizes, tab, sets = sp.sample_and_counts(world.csr, e, table_rows=T, **KW)
    assert Cm.shape == (600, T) and tab.shape == table.shape and sizes.dtype == torch.int32
    assert torch.equal(sizes.to(torch.int64), sizes_r) and np.array_equal(sizes.cpu().numpy(), lens[en.reshape(-1)])
    assert _dicts(Cm, tab) == _dicts(Cr, table)
    assert sets.key64 and sets.slot.dtype == torch.int64                    # the sets keep showing the 64-bit keys
    # without table_rows: exactly one column per distinct LP row of the batch, the same counts
    Cf, sizes_f, tab_f, _ = sp.sample_and_counts(world.csr, e, **KW)
    c = tab_f.shape[0] - 1
    print(f"B = 300: {c} distinct LP rows")
    assert 1 <= c <= T - 1 and Cf.shape == (600, c + 1) and bool((Cf.sum(0) > 0).all())
    assert torch.equal(Cf, Cm[:, : c + 1]) and not bool(Cm[:, c + 1:].any()) and torch.equal(_bits(tab_f), _bits(tab[: c + 1]))
    assert torch.equal(sizes_f, sizes)
    keys = (tab_f[1:].double() * M).round()                                        # ascending in their packed keys: a column is a rank
    packed = (((keys[:, 0] != 0).double() * 256 + keys[:, 1]) * 256 + keys[:, 2]) * 65536 + keys[:, 3] * 256 + keys[:, 4]
    assert bool((packed[1:] > packed[:-1]).all()) and float(packed.max()) >= 2 ** 32


def test_triplet_counts_equal_hgather_counts_over_the_store(sp, world):
    z, table, lens = world.store(HOPS)
    T = table.shape[0]
    assert T <= MAX_T
    h = world.triplets(128, 3)
    Cr, sizes_r = sp.hgather_counts(h, z, T)
    for dedup in (False, True):
        Cm, sizes, tab, sets = sp.sample_and_hcounts(world.csr, h, table_rows=T, dedup_roots=dedup, **KW)
        assert Cm.shape == (512, T)
        assert torch.equal(sizes.to(torch.int64), sizes_r)
        assert _dicts(Cm, tab) == _dicts(Cr, table)


@pytest.mark.parametrize("Mx,stride", [pytest.param(128, 544, id="M128-smallest"), pytest.param(204, 832, id="M204-largest")])
def test_the_ends_of_the_64_bit_range_against_the_store(sp, world, Mx, stride):
    from surel_plus_amd import sampler
    assert sampler.key_rows_form(Mx, HOPS) == 64 and sampler.key_rows_form(Mx - 1 if Mx == 128 else Mx + 1, HOPS) != 64
    z, sets_all = sp.sample_spg(world.csr, torch.arange(world.N, dtype=torch.int32, device="cuda"), num_walks=Mx, num_steps=HOPS, seed=5,
                                rng="philox")
    table = sets_all.feature_table()
    T = table.shape[0]
    print(f"M = {Mx}: the 4-hop store has {T - 1} distinct LP rows")
    assert T <= MAX_T
    e = world.pairs(64, 1)
    bufs = sp.StepBuffers(world.csr, 64, num_walks=Mx, num_steps=HOPS, stage="counts", table_rows=T, wide_keys=True)
    assert bufs.stride == stride and bufs.wide
    Cr, sizes_r = sp.gather_counts(e, z, T)
    Cm, sizes, tab, sets = sp.sample_and_counts(world.csr, e, num_walks=Mx, num_steps=HOPS, seed=5, buffers=bufs, wide_keys=True)
    sets.resolve()
    assert torch.equal(sizes.to(torch.int64), sizes_r) and _dicts(Cm, tab) == _dicts(Cr, table)


# ------------------------------------------------------------------------------------------------------ index against the row form
def test_the_index_step_equals_the_row_form_over_64_bit_rows(sp, world):
    """table[pairs] and indptr are, bit for bit, the xz and indptr of sample_and_gather at 4 hops (the row form over KEY64 rows)"""
    csr = world.csr
    e = world.pairs(64, 1)
    xz, ind, _ = sp.sample_and_gather(csr, e, num_walks=M, num_steps=HOPS, seed=5)
    pairs, indptr, table, sets = sp.sample_and_index(csr, e, **KW)
    R = int(ind[-1])
    assert pairs.dtype == torch.int32 and pairs.shape == (R, 2) and table.shape[1] == HOPS + 1
    assert torch.equal(indptr, ind)
    assert int(pairs[:, 0].min()) >= 1 and int(pairs.max()) == table.shape[0] - 1 and not bool(table[0].any())
    assert torch.equal(_bits(table[pairs.long()]), _bits(xz))
    c = table.shape[0] - 1
    p2, i2, t2, _ = sp.sample_and_index(csr, e, table_rows=c + 40, **KW)
    assert torch.equal(p2, pairs) and torch.equal(i2, indptr) and torch.equal(_bits(t2[: c + 1]), _bits(table)) and not bool(t2[c + 1:].any())


# ------------------------------------------------------------------------------------------------------ attention against the store
def test_attn_counts_equal_the_kernel_over_the_store(sp, world):
    """test_sampled_batches_equal_the_kernel_over_the_store at 4 hops: W, max, den of the step against subgacc_sjoin_counts_attn over
    the all-nodes store, g_store[r] = g_step[the column of row r's key] -- bit for bit after mapping the columns"""
    from surel_plus_amd import spjoin
    z, table, lens = world.store(HOPS)
    B = 300
    e = world.pairs(B, 1)
    T = table.shape[0]
    assert T <= MAX_T
    g_step = _random((T,), 13).requires_grad_()
    bufs = sp.StepBuffers(world.csr, B, num_walks=M, num_steps=HOPS, stage="counts_attn", table_rows=T, wide_keys=True)
    W, sizes, tab, sets = sp.sample_and_attn_counts(world.csr, e, lambda t: g_step, buffers=bufs, **KW)
    sets.resolve()
    assert W.shape == (2 * B, T) and W.data_ptr() == bufs.counts.data_ptr() and W.requires_grad
    col = _column_of_store_rows(tab[: int(bufs.status[2]) + 1], table)
    assert col[0] == 0
    seen = torch.from_numpy(col >= 0).cuda()
    at = torch.from_numpy(col[col >= 0]).cuda()
    g_store = torch.zeros(table.shape[0], device="cuda")
    g_store[seen] = g_step.detach()[at]
    join = spjoin._CountsAttnJoin(z, z.join_rows()[1], e.contiguous().view(-1), B, table.shape[0])
    Ws, mxs, dens = join.forward(g_store, True)
    assert not bool(Ws[:, ~seen].any())
    assert torch.equal(W.detach()[:, at], Ws[:, seen])
    dead = torch.ones(T, dtype=torch.bool, device="cuda")
    dead[at] = False
    assert not bool(W.detach()[:, dead].any())
    assert torch.equal(bufs.smax, mxs) and torch.equal(bufs.sden, dens)
    assert np.array_equal(sizes.cpu().numpy(), lens[e.cpu().numpy().reshape(-1)])


# ------------------------------------------------------------------------------------------------------ one result whatever the route
def _attn_nets(value=True, dtype=torch.float32, H=16):
    torch.manual_seed(7)
    mods = [torch.nn.Sequential(torch.nn.Linear(HOPS + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.Linear(H, 1),
            torch.nn.Linear(H, H) if value else None]
    return [m.to("cuda", dtype) if m is not None else None for m in mods]


def _params(nets):
    return [(n, p) for m in nets if m is not None for n, p in m.named_parameters()]


def _counts(sp, csr, e, **kw):
    return sp.sample_and_counts(csr, e, **KW, **kw)


def _index(sp, csr, e, **kw):
    pairs, indptr, table = sp.sample_and_index(csr, e, **KW, **kw)[:3]
    return pairs[: int(indptr[-1])].clone(), indptr.clone(), table.clone()


def _attn(sp, csr, e, **kw):
    nets = _attn_nets()
    w = _random((2, e.shape[1], 16), 3)
    out = sp.sample_and_attn_stage(csr, e, *nets, **KW, **kw)
    (out * w).sum().backward()
    return (out.detach().clone(),) + tuple(p.grad.clone() for _, p in _params(nets))


@pytest.mark.parametrize("stage,run", [("counts", _counts), ("counts_attn", _attn), ("index", _index)])
def test_one_result_whatever_the_route(sp, world, stage, run):
    """two runs, root dedup, order=, buffers (with dedup and order), and on one set of buffers another batch and the first again"""
    csr, B, T = world.csr, 64, 4096
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    n = 3 if stage != "counts_attn" else 9
    want1, want2 = run(sp, csr, e1, table_rows=T), run(sp, csr, e2, table_rows=T)
    assert not _same(want1, want2, n)
    assert _same(run(sp, csr, e1, table_rows=T), want1, n)
    assert _same(run(sp, csr, e1, table_rows=T, dedup_roots=True), want1, n)
    order = sp.locality_order(csr)
    assert _same(run(sp, csr, e1, table_rows=T, order=order), want1, n)
    for dedup, ordr in ((False, None), (True, order)):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=dedup, order=ordr, stage=stage, table_rows=T, wide_keys=True)
        assert bufs.wide and bufs.out is None
        for e, want in ((e1, want1), (e2, want2), (e1, want1)):
            got = run(sp, csr, e, buffers=bufs, dedup_roots=dedup, order=ordr)
            bufs.sets.prefetch().resolve()
            assert _same(got, want, n)


def test_captured_counts_step_replays_another_batch(sp, world):
    """the wide step with stage="counts" under torch.cuda.graph: replayed with a second batch in the static edge tensor it equals the
    eager result of that batch bit for bit"""
    csr, B, T = world.csr, 64, 4096
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    want2 = sp.sample_and_counts(csr, e2, table_rows=T, dedup_roots=True, **KW)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=True, stage="counts", table_rows=T, wide_keys=True)
    static = e1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # lazy code-object loads and cached segment lists, uncaptured
        sp.sample_and_counts(csr, static, buffers=bufs, dedup_roots=True, **KW)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = sp.sample_and_counts(csr, static, buffers=bufs, dedup_roots=True, **KW)
    static.copy_(e2)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(got, want2)
    assert int(bufs.status[2]) == int((want2[0].sum(0) > 0).sum()) - 1 and not int(bufs.status[1])


# ------------------------------------------------------------------------------------------------------------------ overflow
def test_more_distinct_rows_than_columns(sp, world):
    from surel_plus_amd import _lib
    e = world.pairs(64, 1)
    for stage, call in (("counts", sp.sample_and_counts), ("index", sp.sample_and_index)):
        bufs = sp.StepBuffers(world.csr, 64, num_walks=M, num_steps=HOPS, stage=stage, table_rows=8, wide_keys=True)
        out = call(world.csr, e, buffers=bufs, **KW)
        with pytest.raises(_lib.SubgAccError, match="table_rows"):
            out[3].resolve()
        if stage == "index":
            R = int(out[1][-1])
            assert int(out[0][:R].min()) >= 0 and int(out[0][:R].max()) <= 7        # every pair stays inside the table
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        sp.sample_and_counts(world.csr, e, table_rows=8, **KW)


# ------------------------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("triplets", [False, True], ids=["pairs", "triplets"])
def test_mean_stage_trains_like_the_reference_first_stage(sp, world, triplets):
    """test_gpu_step_stage.py's comparison at 4 hops, with its tolerances: forward rtol 1e-4, atol 1e-5; gradients 1e-4 of their
    largest entry"""
    csr, H = world.csr, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    torch.manual_seed(1)
    mlp_a = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b.load_state_dict(mlp_a.state_dict())
    if triplets:
        B, blocks = 64, 4
        h = world.triplets(B, 3)
        fused = sp.sample_and_hmean_stage(csr, h, mlp_a, **KW)
        xz, ids, _ = sp.sample_and_hgather(csr, h, **kw)
        seg = ids.seg_pointers
    else:
        B, blocks = 128, 2
        e = world.pairs(B, 1)
        fused = sp.sample_and_mean_stage(csr, e, mlp_a, **KW)
        xz, seg, _ = sp.sample_and_gather(csr, e, **kw)
    assert fused.shape == (blocks, B, H)
    w = torch.randn(blocks, B, H, device="cuda")
    (fused * w).sum().backward()
    ref = _reference_stage(mlp_b, xz, seg, blocks * B, H, blocks)
    (ref * w).sum().backward()
    print("forward: max abs error", float((fused - ref).detach().abs().max()))
    assert torch.allclose(fused, ref, rtol=1e-4, atol=1e-5)
    for pa, pb in zip(mlp_a.parameters(), mlp_b.parameters()):
        print("gradient:", float((pa.grad - pb.grad).abs().max()), "of", float(pb.grad.abs().max()))
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-4 * float(pb.grad.abs().max()) + 1e-6


@pytest.mark.parametrize("value", [True, False])
def test_attn_stage_trains_like_the_reference_first_stage(sp, world, value):
    """test_gpu_step_attn.py's comparison at 4 hops with the criteria of test_gpu_counts_attn.py (FWD_TOL, GRAD_TOL, GRAD_FLOOR)"""
    csr, B, H = world.csr, 128, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e = world.pairs(B, 1)
    fa, fb, f64 = _attn_nets(value), _attn_nets(value), _attn_nets(value, torch.float64)
    w = _random((2, B, H), 1)
    fused = sp.sample_and_attn_stage(csr, e, *fa, **KW)
    assert fused.shape == (2, B, H) and fused.dtype == torch.float32
    (fused * w).sum().backward()
    xz, ind, _ = sp.sample_and_gather(csr, e, **kw)

    def ref(nets, x):
        val = nets[2] if nets[2] is not None else torch.nn.Identity()
        return _reference_style_attn(x, ind, nets[0], nets[1], val).view(2, B, -1)

    ref32 = ref(fb, xz)
    (ref32 * w).sum().backward()
    truth = ref(f64, xz.double())
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


def test_lstm_stage_trains_like_the_float64_reference_form(sp, world):
    """test_gpu_step_index.py's comparison at 4 hops, M = 200 (segments of up to 801 members), with its tolerances: forward within 2e-5
    of the reference's largest entry, every parameter gradient within 5e-4 of that gradient's largest entry"""
    csr, B, H, H2 = world.csr, 40, 16, 16
    e = world.pairs(B, 1)
    fa, f64 = _lstm_nets(torch.float32, H, H2, True, HOPS + 1), _lstm_nets(torch.float64, H, H2, True, HOPS + 1)
    fused = sp.sample_and_lstm_stage(csr, e, *fa, **KW)
    assert fused.shape == (2, B, H2) and fused.dtype == torch.float32
    xz, ind, _ = sp.sample_and_gather(csr, e, num_walks=M, num_steps=HOPS, seed=5)
    assert int((ind[1:] - ind[:-1]).max()) > int((ind[1:] - ind[:-1]).min())
    truth = _reference_style_lstm(xz.double(), ind, *f64).view(2, -1, H2)
    scale = float(truth.detach().abs().max())
    err = float((fused.detach().double() - truth.detach()).abs().max())
    print(f"forward: max error {err:.3e}, bound {2e-5 * scale:.3e}")
    assert err <= 2e-5 * scale
    torch.manual_seed(2)
    w = torch.randn(2, B, H2, device="cuda")
    (fused * w).sum().backward()
    (truth * w.double()).sum().backward()
    named = lambda mods: [(n, p) for mod in mods for n, p in mod.named_parameters()]      # noqa: E731
    for (n, pa), (_, pc) in zip(named(fa), named(f64)):
        assert pa.grad is not None, n
        gs = float(pc.grad.abs().max())
        gerr = float((pa.grad.double() - pc.grad).abs().max())
        print(f"grad {n}: max error {gerr:.3e}, bound {5e-4 * max(gs, 1e-6):.3e}")
        assert gerr <= 5e-4 * max(gs, 1e-6), n

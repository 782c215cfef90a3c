"""GPU (MI355X): the LP encoder's mean first stage fused into the count join of an on-demand step -- subgacc_sjoin_key_mean alone on
synthetic key rows against the NumPy restatement of its chain (tests/fused_mean_ref.py) over the counts subgacc_sjoin_key_counts wrote
for the same call, bit for bit; integer-valued E against the stage it replaces, bit for bit; the LDS edges; too many distinct rows; one
result whatever the route (buffers, table_rows, root dedup, order=, triplets, stars, a small shape, 64-bit keys); the derived error
bound against float64; training against sample_and_mean_stage / sample_and_hmean_stage; the captured buffered step."""
import ctypes as C

import numpy as np
import pytest
import torch

from fused_mean_ref import bound, fused_mean
from gpu_helpers import sp  # noqa: F401
from test_gpu_horder import M, World
from test_gpu_step_stage import LENS, Rows, _columns, _key_counts, _lp_keys

pytestmark = pytest.mark.gpu

HOPS = 3
STRIDE = 544
GUARD = 64
WIDTHS = (1, 63, 64, 65, 96, 129, 257)


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _key_mean(rows, ukeys, count, T, E, partner=False, want_len=True):
    """subgacc_sjoin_key_mean over `rows` through _lib.join_desc, into guarded, poisoned out_mean and out_len"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    ids, keys, nsize = rows.device()
    own = torch.from_numpy(np.concatenate([rows.a, rows.b])).cuda()
    par = torch.from_numpy(np.concatenate([rows.b, rows.a])).cuda() if partner else None
    S, H = own.numel(), E.shape[1]
    out = torch.full((S * H + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    olen = torch.full((S + GUARD,), -7, dtype=torch.int32, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _lib.join_desc(_lib.JOIN_COUNTS, _lib.JOIN_KEY32, row_len=nsize, n_rows=rows.n, row_stride=rows.stride, ids=ids, payload=keys,
                       own=own, partner=par, S=S, pair_block=S // 2, table_rows=T, num_walks=M, num_steps=HOPS, flags=flags)
    _lib.check(L.subgacc_sjoin_key_mean(C.byref(d), _lib.ptr(ukeys), _lib.ptr(count), _lib.ptr(E), H, _lib.ptr(out),
                                        _lib.ptr(olen) if want_len else None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out[S * H:] == -7.0).all()) and bool((olen[S:] == -7).all())
    if not want_len:
        assert bool((olen == -7).all())
    return out[: S * H].view(S, H).cpu().numpy(), olen[:S].cpu().numpy(), flags.cpu().numpy()


def _normal(T, H, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((T, H)).astype(np.float32)).cuda()


# ------------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("nkeys,T", [pytest.param(1, 2, id="one-key"), pytest.param(1, 40, id="one-key-wide"),
                                     pytest.param(15, 16, id="T-1-keys"), pytest.param(299, 300, id="299-keys"),
                                     pytest.param(700, 1030, id="700-keys-T1030")])
def test_the_kernel_equals_the_restatement_of_its_chain(sp, nkeys, T):
    """the rows of LENS (0, 1, 255, 256, 257, 511, 512, 513, 544), a row with itself, disjoint ids, full overlap, empty rows; one
    column, T - 1 keys, T no multiple of 64; H = 1 .. 257; partner given and NULL, out_len given and NULL; E random normal.  Bit for
    bit the restatement over the counts subgacc_sjoin_key_counts wrote for the same call; guards untouched, flags clear; the rows of E
    past c and the columns no segment holds poisoned with NaN: the same bits (a row whose count is zero is never read)."""
    assert len(LENS) == 9
    rows = Rows(_lp_keys(nkeys, 11 + nkeys), seed=nkeys)
    ukeys, count, feat, flags = _columns(sp, rows, T)
    assert int(count) == nkeys and not flags.any()
    Cm, sizes, fl = _key_counts(sp, rows, ukeys, count, T)
    assert not fl.any()
    unheld = np.flatnonzero(Cm.sum(0) == 0)
    assert (unheld > nkeys).all() or unheld.size == 0          # every key stands somewhere: only columns past c are free
    how = [(False, True), (True, True), (False, False), (True, False)]
    for i, H in enumerate(WIDTHS):
        E = _normal(T, H, 100 + H)
        want = fused_mean(Cm, sizes, E.cpu().numpy())
        assert np.isfinite(want).all() and not want[sizes == 0].any() and want[sizes > 0].any(1).all()
        for partner, want_len in (how if H == 96 else [how[i % 4]]):
            got, olen, fl = _key_mean(rows, ukeys, count, T, E, partner=partner, want_len=want_len)
            assert not fl.any()
            assert np.array_equal(_bits(got), _bits(want)), (H, partner, want_len, np.abs(got - want).max())
            if want_len:
                assert np.array_equal(olen, sizes)
        Ep = E.clone()
        Ep[nkeys + 1:] = float("nan")
        Ep[torch.from_numpy(unheld).cuda()] = float("nan")
        got, _, fl = _key_mean(rows, ukeys, count, T, Ep)
        assert not fl.any() and np.array_equal(_bits(got), _bits(want)), H


# ------------------------------------------------------------------------------------------------------ 2. integer-valued E
@pytest.mark.parametrize("nkeys,T,H", [(15, 16, 65), (299, 300, 96)])
def test_integer_rows_give_the_bits_of_the_stage_it_replaces(sp, nkeys, T, H):
    """E of small whole numbers: every product and sum is exact in float32, so the chain, whatever its order, is (C @ E) / sizes --
    bit for bit spjoin._step_mean(C, sizes, ...) of the existing path"""
    from surel_plus_amd import spjoin
    rows = Rows(_lp_keys(nkeys, 11 + nkeys), seed=nkeys)
    ukeys, count, feat, _ = _columns(sp, rows, T)
    Cm, sizes, _ = _key_counts(sp, rows, ukeys, count, T)
    E = torch.from_numpy(np.random.default_rng(H).integers(-3, 4, (T, H)).astype(np.float32)).cuda()
    got, olen, fl = _key_mean(rows, ukeys, count, T, E)
    assert not fl.any() and np.array_equal(olen, sizes)
    want = spjoin._step_mean(torch.from_numpy(Cm).cuda(), torch.from_numpy(sizes).cuda(), feat, None, lambda table: E, 2)
    assert np.array_equal(_bits(got), _bits(want.reshape(-1, H).cpu().numpy()))
    assert np.array_equal(_bits(got), _bits(fused_mean(Cm, sizes, E.cpu().numpy())))


# ------------------------------------------------------------------------------------------------------ 3. LDS edges
def _lds_bytes(T, max_len=STRIDE):
    return max_len * 8 + T * 12 + 16            # the header's formula


_T_64K = (64 * 1024 - 16 - STRIDE * 8) // 12


@pytest.mark.parametrize("T", [_T_64K, _T_64K + 1, 8192], ids=["last-T-within-64KiB", "first-T-above-64KiB", "T-8192"])
def test_lds_edges(sp, T):
    """the largest T whose LDS request stays within the 64 KiB a kernel gets by default, the next one (the launch raises the limit),
    and the wide limit 8,192 -- a handful of pairs of rows 0, 5, 300 and 544 long"""
    assert _lds_bytes(_T_64K) <= 64 * 1024 < _lds_bytes(_T_64K + 1) and _T_64K == 5097
    rows = Rows(_lp_keys(60, 4), seed=T, lens=(0, 5, 300, STRIDE))
    ukeys, count, feat, _ = _columns(sp, rows, T)
    Cm, sizes, fl = _key_counts(sp, rows, ukeys, count, T)
    assert not fl.any() and int(count) == 60
    E = _normal(T, 96, T)
    E[61:] = float("nan")
    got, olen, fl = _key_mean(rows, ukeys, count, T, E)
    assert not fl.any() and np.array_equal(olen, sizes)
    assert np.array_equal(_bits(got), _bits(fused_mean(Cm, sizes, E.cpu().numpy())))


# ------------------------------------------------------------------------------------------------------ 4. too many distinct rows
def test_more_distinct_rows_than_columns(sp, world):
    """T - 1 one less than the keys present: the join meets keys that are not in its list -- flags[3] & 2, those slots not counted,
    the result the restatement over the count kernel's own flagged C; the buffered step's sets.resolve() raises and names table_rows"""
    from surel_plus_amd import _lib
    nkeys = 40
    rows = Rows(_lp_keys(nkeys, 3), seed=5)
    T = nkeys
    ukeys, count, feat, flags = _columns(sp, rows, T)
    assert int(flags[2]) & 1 and int(count) == T - 1
    Cm, sizes, fl = _key_counts(sp, rows, ukeys, count, T)
    assert int(fl[3]) & 2
    E = _normal(T, 65, 9)
    got, olen, fl = _key_mean(rows, ukeys, count, T, E)
    assert int(fl[3]) & 2 and np.array_equal(olen, sizes)
    assert np.array_equal(_bits(got), _bits(fused_mean(Cm, sizes, E.cpu().numpy())))
    embed = torch.nn.Linear(HOPS + 1, 4).cuda()
    bufs = sp.StepBuffers(world.csr, 64, num_walks=M, num_steps=HOPS, stage="mean", table_rows=8, width=4)
    with torch.no_grad():
        x = sp.sample_and_fused_mean_stage(world.csr, world.pairs(64, 1), embed, num_walks=M, num_steps=HOPS, seed=5, buffers=bufs)
    assert x.shape == (2, 64, 4)
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        bufs.sets.resolve()
    with pytest.raises(_lib.SubgAccError, match="table_rows"), torch.no_grad():
        sp.sample_and_fused_mean_stage(world.csr, world.pairs(64, 1), embed, num_walks=M, num_steps=HOPS, seed=5, table_rows=8)


# ------------------------------------------------------------------------------------------------------ 5. one result whatever the route
def _mlp(k, H, seed=1):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(k, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()


class _RowWise(torch.nn.Module):
    """a Linear-ReLU-Linear embed evaluated in blocks of 64 rows (zero rows behind the last): a row's bits do not depend on how
    many rows the table has, whatever GEMM the library picks for a shape -- what `embed is row-wise` means bit for bit"""

    def __init__(self, mlp):
        super().__init__()
        self.mlp = mlp

    def forward(self, table):
        T = table.shape[0]
        pad = torch.zeros(((T + 63) // 64 * 64, table.shape[1]), dtype=table.dtype, device=table.device)
        pad[:T] = table
        return torch.cat([self.mlp(blk) for blk in pad.split(64)])[:T]


def _restated(sp, csr, counts_call, args, embed, **kw):
    """the restatement over the (C, sizes, table) of the existing count call for the same step"""
    Cm, sizes, table, _ = counts_call(csr, *args, **kw)
    with torch.no_grad():
        E = embed(table)
    return fused_mean(Cm.cpu().numpy(), sizes.cpu().numpy(), E.cpu().numpy())


@pytest.mark.parametrize("B", [64, 300])
def test_one_result_whatever_the_route(sp, world, B):
    csr, T, H = world.csr, 1024, 96
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    embed = _RowWise(_mlp(HOPS + 1, H))
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    order = sp.locality_order(csr)
    with torch.no_grad():
        want1 = sp.sample_and_fused_mean_stage(csr, e1, embed, **kw)                  # no buffers, table_rows=None
        want2 = sp.sample_and_fused_mean_stage(csr, e2, embed, **kw)
        assert want1.shape == (2, B, H) and want1.dtype == torch.float32 and not torch.equal(want1, want2)
        ref = _restated(sp, csr, sp.sample_and_counts, (e1,), embed, table_rows=T, **kw)
        assert np.array_equal(_bits(want1.reshape(-1, H).cpu().numpy()), _bits(ref))
        assert torch.equal(sp.sample_and_fused_mean_stage(csr, e1, embed, table_rows=T, **kw), want1)
        assert torch.equal(sp.sample_and_fused_mean_stage(csr, e1, embed, table_rows=T, dedup_roots=True, **kw), want1)
        assert torch.equal(sp.sample_and_fused_mean_stage(csr, e1, embed, order=order, **kw), want1)
        for dedup, ordr in ((False, None), (True, None), (False, order), (True, order)):
            bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=dedup, order=ordr, stage="mean", table_rows=T, width=H)
            assert bufs.counts is None and bufs.out is None and bufs.mean.shape == (2 * B, H)
            for e, want in ((e1, want1), (e2, want2), (e1, want1)):         # a second step on the same buffers gives ITS batch
                got = sp.sample_and_fused_mean_stage(csr, e, embed, buffers=bufs, dedup_roots=dedup, order=ordr, **kw)
                assert got.data_ptr() == bufs.mean.data_ptr()
                bufs.sets.prefetch().resolve()
                assert torch.equal(got, want)
        # (a sampled set holds its root: no segment of a step is empty -- the empty rows are the synthetic ones of the kernel test)
        sizes = sp.sample_and_counts(csr, e1, table_rows=T, **kw)[1]
        assert bool((sizes > 0).all()) and bool(want1.reshape(-1, H).any(1).all())
        # an embed of another width, or another type, is refused by name
        with pytest.raises(ValueError, match="sample_and_fused_mean_stage.*width=96"):
            sp.sample_and_fused_mean_stage(csr, e1, _mlp(HOPS + 1, 32), buffers=bufs, dedup_roots=True, order=order, **kw)
        with pytest.raises(ValueError, match="sample_and_fused_mean_stage: embed"):
            sp.sample_and_fused_mean_stage(csr, e1, lambda t: embed(t).double(), **kw)
        with pytest.raises(ValueError, match="sample_and_fused_mean_stage: embed"):
            sp.sample_and_fused_mean_stage(csr, e1, lambda t: embed(t)[1:], **kw)


def test_triplets_give_one_result_whatever_the_route(sp, world):
    csr, T, H, B = world.csr, 1024, 65, 128
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    embed = _RowWise(_mlp(HOPS + 1, H))
    h = world.triplets(B, 3)
    with torch.no_grad():
        want = sp.sample_and_fused_hmean_stage(csr, h, embed, **kw)
        assert want.shape == (4, B, H)
        ref = _restated(sp, csr, sp.sample_and_hcounts, (h,), embed, table_rows=T, **kw)
        assert np.array_equal(_bits(want.reshape(-1, H).cpu().numpy()), _bits(ref))
        assert torch.equal(sp.sample_and_fused_hmean_stage(csr, h, embed, table_rows=T, **kw), want)
        assert torch.equal(sp.sample_and_fused_hmean_stage(csr, h, embed, dedup_roots=True, **kw), want)
        assert torch.equal(sp.sample_and_fused_hmean_stage(csr, h, embed, order=sp.locality_order(csr), **kw), want)
        hb = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, triplets=True, dedup_roots=True, stage="mean", table_rows=T, width=H)
        for _ in range(2):
            got = sp.sample_and_fused_hmean_stage(csr, h, embed, buffers=hb, dedup_roots=True, **kw)
            hb.sets.resolve()
            assert torch.equal(got, want)


@pytest.mark.parametrize("P,K", [(5, 3), (9, 7)])
def test_the_star_calls_equal_the_calls_over_the_expanded_list(sp, world, P, K):
    """K = 3 and K = 7 with P*K no multiple of 64, pairs and triplets, with and without buffers"""
    assert (P * K) % 64
    csr, T, H = world.csr, 1024, 96
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    embed = _RowWise(_mlp(HOPS + 1, H))
    rng = np.random.default_rng(P * K)
    src = torch.from_numpy(np.array((world.special + list(rng.integers(0, world.N, P)))[:P])).cuda()
    v = torch.from_numpy(rng.integers(0, world.N, P)).cuda()
    tg = torch.from_numpy(rng.integers(0, world.N, (P, K))).cuda()
    tg[0, 0], tg[1, 1] = world.isolated, src[1]
    with torch.no_grad():
        e = torch.stack([src.repeat_interleave(K), tg.reshape(-1)])
        want = sp.sample_and_fused_mean_stage(csr, e, embed, **kw)
        assert torch.equal(sp.sample_and_fused_mean_stage_star(csr, src, tg, embed, **kw), want)
        assert torch.equal(sp.sample_and_fused_mean_stage_star(csr, src, tg, embed, table_rows=T, **kw), want)
        bufs = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=HOPS, stage="mean", table_rows=T, width=H, star=K)
        got = sp.sample_and_fused_mean_stage_star(csr, src, tg, embed, buffers=bufs, **kw)
        bufs.sets.resolve()
        assert torch.equal(got, want)
        h = torch.stack([src.repeat_interleave(K), v.repeat_interleave(K), tg.reshape(-1)])
        hwant = sp.sample_and_fused_hmean_stage(csr, h, embed, **kw)
        uv = torch.stack([src, v])
        assert torch.equal(sp.sample_and_fused_hmean_stage_star(csr, uv, tg, embed, **kw), hwant)
        hb = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=HOPS, triplets=True, stage="mean", table_rows=T, width=H, star=K)
        got = sp.sample_and_fused_hmean_stage_star(csr, uv, tg, embed, buffers=hb, **kw)
        hb.sets.resolve()
        assert torch.equal(got, hwant)


@pytest.mark.parametrize("walks,hops,wide", [pytest.param(100, 2, False, id="small-100x2"), pytest.param(200, 4, True, id="wide-200x4")])
def test_a_small_shape_and_the_64_bit_keys(sp, world, walks, hops, wide):
    csr, B, T, H = world.csr, 64, 2048, 96
    kw = dict(num_walks=walks, num_steps=hops, seed=5, wide_keys=wide)
    embed = _RowWise(_mlp(hops + 1, H))
    e = world.pairs(B, 1)
    with torch.no_grad():
        want = sp.sample_and_fused_mean_stage(csr, e, embed, **kw)
        ref = _restated(sp, csr, sp.sample_and_counts, (e,), embed, table_rows=T, **kw)
        assert np.array_equal(_bits(want.reshape(-1, H).cpu().numpy()), _bits(ref))
        bufs = sp.StepBuffers(csr, B, num_walks=walks, num_steps=hops, stage="mean", table_rows=T, width=H, wide_keys=wide)
        assert bufs.wide == wide and bufs.small == (not wide)
        got = sp.sample_and_fused_mean_stage(csr, e, embed, buffers=bufs, **kw)
        bufs.sets.resolve()
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------ 6. against the mathematics
def test_the_result_lies_within_the_derived_bound_of_the_exact_mean(sp, world):
    """float64 (C @ E) / size against the kernel: every element within gamma_m (C @ |E|) / size, gamma_m = m u / (1 - m u), u = 2^-24,
    m = the segment's non-zero columns + 2 -- the standard bound of a float32 sum of n terms (n - 1 adds) with the product's and the
    division's roundings; derived, not measured.  E's non-zero magnitudes are >= 2^-20, so no intermediate is subnormal."""
    csr, B, T, H = world.csr, 300, 1024, 96
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    mlp = _RowWise(_mlp(HOPS + 1, H, seed=3))

    def embed(table):
        E = mlp(table)
        return torch.where(E.abs() < 2.0 ** -20, torch.zeros_like(E), E)

    e = world.pairs(B, 2)
    with torch.no_grad():
        got = sp.sample_and_fused_mean_stage(csr, e, embed, table_rows=T, **kw).reshape(-1, H).cpu().numpy().astype(np.float64)
        Cm, sizes, table, _ = sp.sample_and_counts(csr, e, table_rows=T, **kw)
        E = embed(table).cpu().numpy()
    Cm, sizes = Cm.cpu().numpy(), sizes.cpu().numpy()
    exact = (Cm.astype(np.float64) @ E.astype(np.float64)) / np.maximum(sizes, 1)[:, None]
    lim = bound(Cm, sizes, E)
    err = np.abs(got - exact)
    print(f"largest error / bound: {float((err / np.maximum(lim, 1e-300)).max()):.3f}; largest error {float(err.max()):.3e}")
    assert (err <= lim).all()
    # and on the synthetic rows with normal E (rows up to 544 members, 299 columns)
    rows = Rows(_lp_keys(299, 310), seed=299)
    ukeys, count, feat, _ = _columns(sp, rows, 300)
    Cs, ss, _ = _key_counts(sp, rows, ukeys, count, 300)
    En = _normal(300, 129, 6)
    En = torch.where(En.abs() < 2.0 ** -20, torch.zeros_like(En), En)
    gs, _, _ = _key_mean(rows, ukeys, count, 300, En)
    exact = (Cs.astype(np.float64) @ En.cpu().numpy().astype(np.float64)) / np.maximum(ss, 1)[:, None]
    assert (np.abs(gs.astype(np.float64) - exact) <= bound(Cs, ss, En.cpu().numpy())).all()


# ------------------------------------------------------------------------------------------------------ 7. training
@pytest.mark.parametrize("triplets", [False, True], ids=["pairs", "triplets"])
def test_the_fused_stage_trains_like_the_stage_it_replaces(sp, world, triplets):
    """forward and every parameter gradient of sample_and_fused_mean_stage / sample_and_fused_hmean_stage against sample_and_mean_stage /
    sample_and_hmean_stage with the same modules, with the tolerances test_stage_trains_like_the_reference_first_stage states (forward
    rtol 1e-4, atol 1e-5; gradients 1e-4 of their largest entry)"""
    csr, H = world.csr, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    mlp_a, mlp_b = _mlp(HOPS + 1, H), _mlp(HOPS + 1, H)
    mlp_b.load_state_dict(mlp_a.state_dict())
    if triplets:
        B, blocks, e = 128, 4, world.triplets(128, 3)
        fused = sp.sample_and_fused_hmean_stage(csr, e, mlp_a, **kw)
        ref = sp.sample_and_hmean_stage(csr, e, mlp_b, **kw)
    else:
        B, blocks, e = 300, 2, world.pairs(300, 1)
        fused = sp.sample_and_fused_mean_stage(csr, e, mlp_a, **kw)
        ref = sp.sample_and_mean_stage(csr, e, mlp_b, **kw)
    assert fused.shape == (blocks, B, H) and fused.requires_grad
    w = torch.randn(blocks, B, H, device="cuda")
    (fused * w).sum().backward()
    (ref * w).sum().backward()
    assert torch.allclose(fused, ref, rtol=1e-4, atol=1e-5)
    for pa, pb in zip(mlp_a.parameters(), mlp_b.parameters()):
        assert pa.grad is not None
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-4 * float(pb.grad.abs().max()) + 1e-6


class _IntRows(torch.nn.Module):
    """an embed whose rows are whole numbers: row p of a parameter, whatever the feature row"""

    def __init__(self, T, H, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.rows = torch.nn.Parameter(torch.randint(-3, 4, (T, H)).float())

    def forward(self, table):
        return self.rows[: table.shape[0]] + 0.0 * table[:, :1]


def test_integer_rows_train_bit_for_bit_and_a_late_backward_is_refused(sp, world):
    csr, B, T, H = world.csr, 64, 1024, 24
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=T)
    emb_a, emb_b = _IntRows(T, H, 4).cuda(), _IntRows(T, H, 4).cuda()
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="mean", table_rows=T, width=H)
    fused = sp.sample_and_fused_mean_stage(csr, e1, emb_a, buffers=bufs, **kw)
    ref = sp.sample_and_mean_stage(csr, e1, emb_b, **kw)
    assert torch.equal(fused, ref)                                      # every sum exact: the same bits
    w = torch.randint(-2, 3, (2, B, H), device="cuda").float()
    (fused * w).sum().backward()
    (ref * w).sum().backward()
    ga, gb = emb_a.rows.grad, emb_b.rows.grad
    assert bool(ga.abs().sum() > 0) and float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max()) + 1e-6
    # the backward of a step whose buffers have moved on: RuntimeError naming the step, never another batch's rows
    first = sp.sample_and_fused_mean_stage(csr, e1, emb_a, buffers=bufs, **kw)
    step = bufs.step_id
    sp.sample_and_fused_mean_stage(csr, e2, emb_a, buffers=bufs, **kw)
    with pytest.raises(RuntimeError, match=f"step {step} "):
        first.sum().backward()


def test_no_count_matrix_exists_under_no_grad(sp, world):
    """peak memory above the buffers stays below S*T*4 bytes: no C was made (the unfused call allocates it)"""
    csr, B, T, H = world.csr, 300, 2048, 96
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=T)
    embed = _mlp(HOPS + 1, H)
    e = world.pairs(B, 1)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="mean", table_rows=T, width=H)
    with torch.no_grad():
        sp.sample_and_fused_mean_stage(csr, e, embed, buffers=bufs, **kw)       # cached segment lists, lazy loads
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sp.sample_and_fused_mean_stage(csr, e, embed, buffers=bufs, **kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert peak < 2 * B * T * 4, peak
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sp.sample_and_mean_stage(csr, e, embed, **kw)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base >= 2 * B * T * 4


# ------------------------------------------------------------------------------------------------------ 8. capture
def test_captured_step_replays_another_batch(sp, world):
    """the buffered step with stage="mean", embed included, under torch.cuda.graph and no_grad; replayed with a second batch copied
    into the static edge tensor it equals the eager result of that batch bit for bit"""
    csr, B, T, H = world.csr, 300, 1024, 96
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    embed = _mlp(HOPS + 1, H)
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    with torch.no_grad():
        want2 = sp.sample_and_fused_mean_stage(csr, e2, embed, table_rows=T, dedup_roots=True, **kw)
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=True, stage="mean", table_rows=T, width=H)
        static = e1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # lazy code-object loads and cached segment lists, uncaptured
            sp.sample_and_fused_mean_stage(csr, static, embed, buffers=bufs, dedup_roots=True, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = sp.sample_and_fused_mean_stage(csr, static, embed, buffers=bufs, dedup_roots=True, **kw)
        static.copy_(e2)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(got, want2)
    assert not int(bufs.status[1])

"""GPU (MI355X): the LP encoder's attentional first stage fused into the attentional count join of an on-demand step --
subgacc_sjoin_key_attn alone on synthetic key rows against the NumPy restatement of its chain (tests/fused_attn_ref.py) over the W
that subgacc_sjoin_key_counts_attn wrote for the same call, bit for bit, with m, den and the lengths bit for bit the unfused
kernel's; the edges of the column words; flags and clamps; the derived error bound against float64; sample_and_fused_attn_stage
against sample_and_attn_stage and as one result whatever the route; stars, a small shape, 64-bit keys; training against the float64
reference form; no [S, T] tensor under no_grad; the captured buffered step."""
import ctypes as C

import numpy as np
import pytest
import torch

from fused_attn_ref import bound, fused_attn
from gpu_helpers import sp  # noqa: F401
from test_gpu_counts_attn import FWD_TOL, GRAD_FLOOR, GRAD_TOL
from test_gpu_horder import M, World
from test_gpu_step_attn import CASES, FILL, _key_attn, _keys_on_device, _lists, _nets, _params, _random, _ref
from test_gpu_step_stage import HOPS, LENS, STRIDE, Rows, _guarded, _lp_keys

pytestmark = pytest.mark.gpu

WIDTHS = (1, 63, 64, 65, 96, 129, 257, 1024)


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view(np.uint32)


def _fused(rows, ukeys, count, T, g, E, partner=True, blocks=1, want_len=True, lists=None, keep=True):
    """subgacc_sjoin_key_attn over `rows` with the lists of test_gpu_step_attn._key_attn; every output has GUARD words behind it that
    must stay untouched -> dict of A, max, den, len (device tensors) and flags"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    ids, keys, nsize = rows.device()
    own_h, par_h, P = _lists(rows, blocks) if lists is None else lists
    own = torch.from_numpy(own_h).cuda()
    par = torch.from_numpy(par_h).cuda() if partner else None
    S, H = own.numel(), E.shape[1]
    A, mx, den = _guarded(S * H, torch.float32, FILL), _guarded(S, torch.float32, FILL), _guarded(S, torch.float32, FILL)
    olen = _guarded(S, torch.int32, -7)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _lib.join_desc(_lib.JOIN_COUNTS, _lib.JOIN_KEY32, row_len=nsize, n_rows=rows.n, row_stride=rows.stride, ids=ids, payload=keys,
                       own=own, partner=par, S=S, pair_block=P, table_rows=T, num_walks=M, num_steps=HOPS, flags=flags)
    _lib.check(L.subgacc_sjoin_key_attn(C.byref(d), _lib.ptr(ukeys), _lib.ptr(count), _lib.ptr(g), _lib.ptr(E), H, _lib.ptr(A),
                                        _lib.ptr(mx) if keep else None, _lib.ptr(den) if keep else None,
                                        _lib.ptr(olen) if want_len else None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((A[S * H:] == FILL).all()) and bool((mx[S:] == FILL).all()) and bool((den[S:] == FILL).all())
    assert bool((olen[S:] == -7).all())
    return dict(A=A[: S * H].view(S, H), max=mx[:S], den=den[:S], len=olen[:S], flags=flags)


def _table(T, H, live, seed):
    """E float32 [T, H]: standard normal on the rows 0 .. live, NaN behind them (rows no segment may read)"""
    E = torch.from_numpy(np.random.default_rng(seed).standard_normal((T, H)).astype(np.float32))
    E[live + 1:] = float("nan")
    return E.cuda().contiguous()


def _check_against_the_unfused_kernel(rows, ukeys, count, T, g, widths, live, flag=0, **how):
    """W, m, den, len of subgacc_sjoin_key_counts_attn for the same call; out_a = the restatement over that W for every width, m, den
    and len the same bits; once more without out_max / out_den / out_len: the same out_a"""
    ref = _key_attn(rows, ukeys, count, T, g, **how)
    assert int(ref["flags"][3]) == flag
    W = ref["W"].cpu().numpy()
    own = (_lists(rows, how.get("blocks", 1)) if how.get("lists") is None else how["lists"])[0]
    empty = rows.len[own] == 0
    for H in widths:
        E = _table(T, H, live, 100 + H)
        want = fused_attn(W, E.cpu().numpy())
        assert np.isfinite(want).all() and not want[empty].any()
        got = _fused(rows, ukeys, count, T, g, E, **how)
        assert int(got["flags"][3]) == flag
        assert np.array_equal(_bits(got["A"]), _bits(want)), (H, np.abs(got["A"].cpu().numpy() - want).max())
        for name in ("max", "den", "len"):
            assert torch.equal(got[name], ref[name]), (H, name)
        bare = _fused(rows, ukeys, count, T, g, E, want_len=False, keep=False, **how)
        assert torch.equal(bare["A"], got["A"]) and bool((bare["max"] == FILL).all()) and bool((bare["den"] == FILL).all())
        assert bool((bare["len"] == -7).all())
    return ref


# ------------------------------------------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("nkeys,T,opt", CASES)
def test_the_kernel_equals_the_restatement_of_its_chain(sp, nkeys, T, opt):
    """the rows of LENS (0, 1, 255, 256, 257, 511, 512, 513, 544) at row_stride 544, a row with itself and its neighbour, disjoint ids,
    full overlap, empty rows; the (nkeys, T) cases of test_gpu_step_attn at width 96, and every width 1 .. 1,024 at T = c + 40; E
    standard normal on the rows 0 .. c and NaN behind them.  Bit for bit the restatement over the W of the unfused kernel; m, den and
    the lengths bit for bit that kernel's; guards untouched, flags clear, empty segments zero rows."""
    assert LENS == (0, 1, 255, 256, 257, 511, 512, 513, 544) and STRIDE == 544
    rows = Rows(_lp_keys(nkeys, 11 + nkeys), seed=nkeys, distinct=opt.get("distinct", False))
    present = rows.present()
    assert len(present) == nkeys
    ukeys, count = _keys_on_device(present, T)
    g = _random((T,), 3)
    how = dict(partner=opt.get("partner", True), blocks=opt.get("blocks", 1))
    ref = _check_against_the_unfused_kernel(rows, ukeys, count, T, g, WIDTHS if T == nkeys + 40 else (96,), nkeys, **how)
    own = _lists(rows, how["blocks"])[0]
    empty = torch.from_numpy(rows.len[own] == 0).cuda()
    assert bool(empty.any()) and not bool(ref["max"][empty].any()) and not bool(ref["den"][empty].any())


@pytest.mark.parametrize("c", [0, 63, 64, 127])
def test_the_edges_of_the_column_words(sp, c):
    """c + 1 = 1, 64, 65 and 128 columns: the last ballot word holds one column, is full, one over, and exactly two words.  c = 0: the
    count word says no key, every feature slot reads column 0 (flags[3] = 2, as in the unfused kernel) -- segments whose only non-zero
    column is 0"""
    nkeys = max(c, 1)
    T = max(c + 1, 2)
    rows = Rows(_lp_keys(nkeys, 40 + c), seed=c)
    ukeys, count = _keys_on_device(rows.present(), T, count=c)
    g = _random((T,), 6)
    ref = _check_against_the_unfused_kernel(rows, ukeys, count, T, g, (65, 96), c, flag=0 if c else 2)
    if not c:
        assert not bool(ref["W"][:, 1:].any()) and bool(ref["W"][:, 0].any())


def test_one_key_rows_without_a_partner_list(sp):
    """one key, T = 2, partner = NULL (the list's mirror taken from pair_block): W has the columns 0 and 1 alone"""
    rows = Rows(_lp_keys(1, 12), seed=1)
    ukeys, count = _keys_on_device(rows.present(), 2)
    _check_against_the_unfused_kernel(rows, ukeys, count, 2, _random((2,), 3), (1, 64, 257), 1, partner=False)


# ------------------------------------------------------------------------------------------------------ 2. flags and clamps
def test_a_key_that_is_not_in_the_list_reads_as_column_0(sp):
    nkeys, T = 60, 64
    rows = Rows(_lp_keys(nkeys, 21), seed=2)
    kept = np.delete(rows.present(), nkeys // 2)
    ukeys, count = _keys_on_device(kept, T)
    _check_against_the_unfused_kernel(rows, ukeys, count, T, _random((T,), 1), (65,), nkeys - 1, flag=2)


@pytest.mark.parametrize("n_keys", [-5, "T+100"])
def test_n_keys_is_clamped(sp, n_keys):
    """*n_keys of -5 reads no key (every slot is column 0, flags[3] = 2); T + 100 reads the T - 1 keys there are: as the unfused kernel"""
    nkeys = 40
    T = nkeys + 1
    rows = Rows(_lp_keys(nkeys, 6), seed=3)
    word = T + 100 if n_keys == "T+100" else n_keys
    ukeys, count = _keys_on_device(rows.present(), T, count=word)
    live = nkeys if word > 0 else 0
    _check_against_the_unfused_kernel(rows, ukeys, count, T, _random((T,), 5), (96,), live, flag=0 if word > 0 else 2)


def test_a_list_that_is_not_mirrored_is_not_written(sp):
    nkeys, T, H = 40, 41, 65
    rows = Rows(_lp_keys(nkeys, 6), seed=3)
    ukeys, count = _keys_on_device(rows.present(), T)
    g, E = _random((T,), 5), _table(T, H, nkeys, 7)
    a, b = np.array([3, 4, 5, 6]), np.array([4, 5, 6, 7])
    own, par = np.concatenate([a, b]), np.concatenate([b, a])
    want = _fused(rows, ukeys, count, T, g, E, lists=(own, par, 4))
    bad = par.copy()
    bad[1] = 8                                                  # pair 1: the partner of (4, .) is not the own row of its mirror
    got = _fused(rows, ukeys, count, T, g, E, lists=(own, bad, 4))
    assert int(got["flags"][3]) == 4 and not want["flags"].any()
    skipped, written = [1, 5], [0, 2, 3, 4, 6, 7]
    for name in ("A", "max", "den"):
        assert bool((got[name][skipped] == FILL).all()) and torch.equal(got[name][written], want[name][written]), name
    assert bool((got["len"][skipped] == -7).all()) and torch.equal(got["len"][written], want["len"][written])


# ------------------------------------------------------------------------------------------------------ 3. against the mathematics
def test_the_result_lies_within_the_derived_bound(sp):
    """W taken as the float32 matrix the unfused kernel wrote: |out_a - float64(W) @ float64(E)| <= gamma_m (W @ |E|) elementwise,
    gamma_m = m u / (1 - m u), u = 2^-24, m = the segment's non-zero columns + 1 -- the standard bound of a float32 sum of n rounded
    products; derived, not measured.  E's non-zero magnitudes are >= 2^-20 and W's entries >= 2^-60 or zero, so no product is
    subnormal."""
    nkeys, T, H = 299, 339, 129
    rows = Rows(_lp_keys(nkeys, 310), seed=299)
    ukeys, count = _keys_on_device(rows.present(), T)
    g = _random((T,), 8)
    W = _key_attn(rows, ukeys, count, T, g)["W"].cpu().numpy()
    assert (W[W != 0] >= 2.0 ** -60).all()
    E = torch.from_numpy(np.random.default_rng(6).standard_normal((T, H)).astype(np.float32)).cuda()
    E = torch.where(E.abs() < 2.0 ** -20, torch.zeros_like(E), E).contiguous()
    got = _fused(rows, ukeys, count, T, g, E)["A"].cpu().numpy().astype(np.float64)
    Eh = E.cpu().numpy()
    err, lim = np.abs(got - W.astype(np.float64) @ Eh.astype(np.float64)), bound(W, Eh)
    print(f"largest error / bound: {float((err / np.maximum(lim, 1e-300)).max()):.3f}; largest error {float(err.max()):.3e}")
    assert (err <= lim).all()


# ------------------------------------------------------------------------------------------------------ 4. the stage
def _fwd(call, *args, **kw):
    with torch.no_grad():
        return call(*args, **kw)


@pytest.mark.parametrize("T", [None, 2048], ids=["table_rows-None", "table_rows-2048"])
@pytest.mark.parametrize("B", [64, 300])
def test_the_stage_agrees_with_its_twin_and_is_one_result_whatever_the_route(sp, world, B, T):
    """sample_and_fused_attn_stage against sample_and_attn_stage at (200, 3): within FWD_TOL of the largest entry (the two differ by
    the GEMM's summation order alone); the same bits with and without buffers=, with dedup_roots=True and with an order="""
    csr, H = world.csr, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=T)
    nets = _nets()
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    order = sp.locality_order(csr)
    want1 = _fwd(sp.sample_and_fused_attn_stage, csr, e1, *nets, **kw)
    want2 = _fwd(sp.sample_and_fused_attn_stage, csr, e2, *nets, **kw)
    assert want1.shape == (2, B, H) and want1.dtype == torch.float32 and not want1.requires_grad and not torch.equal(want1, want2)
    for e, want in ((e1, want1), (e2, want2)):
        twin = _fwd(sp.sample_and_attn_stage, csr, e, *nets, **kw)
        scale = float(twin.abs().max())
        err = float((want - twin).abs().max())
        print("against the unfused stage", err / scale)
        assert scale > 0 and err <= FWD_TOL * scale
    assert torch.equal(_fwd(sp.sample_and_fused_attn_stage, csr, e1, *nets, dedup_roots=True, **kw), want1)
    assert torch.equal(_fwd(sp.sample_and_fused_attn_stage, csr, e1, *nets, order=order, **kw), want1)
    if T is None:
        return
    for dedup, ordr in ((False, None), (True, None), (False, order)):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=dedup, order=ordr, stage="attn", table_rows=T, width=H)
        assert bufs.counts is None and bufs.out is None and bufs.attn.shape == (2 * B, H) and bufs.smax.shape == (2 * B,)
        for e, want in ((e1, want1), (e2, want2), (e1, want1)):         # a second step on the same buffers gives ITS batch
            got = _fwd(sp.sample_and_fused_attn_stage, csr, e, *nets, buffers=bufs, dedup_roots=dedup, order=ordr, **kw)
            bufs.sets.prefetch().resolve()
            assert torch.equal(got, want)
    # without value_nn the result is the aggregation itself: a view of `attn`
    got = _fwd(sp.sample_and_fused_attn_stage, csr, e1, nets[0], nets[1], None, buffers=bufs, order=order, **kw)
    assert got.shape == (2, B, H)
    # an embed of another width than the buffers', and buffers of another stage, are refused by name
    other = _nets(H=32)
    with pytest.raises(ValueError, match="sample_and_fused_attn_stage.*width=16"):
        _fwd(sp.sample_and_fused_attn_stage, csr, e1, *other, buffers=bufs, order=order, **kw)
    unfused = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="counts_attn", table_rows=T)
    with pytest.raises(ValueError, match="stage='attn'"):
        _fwd(sp.sample_and_fused_attn_stage, csr, e1, *nets, buffers=unfused, **kw)


@pytest.mark.parametrize("P,K", [(5, 3), (9, 7)])
def test_the_star_call_equals_the_call_over_the_expanded_list(sp, world, P, K):
    assert (P * K) % 64
    csr, T, H = world.csr, 2048, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=T)
    nets = _nets()
    rng = np.random.default_rng(P * K)
    src = torch.from_numpy(np.array((world.special + list(rng.integers(0, world.N, P)))[:P])).cuda()
    tg = torch.from_numpy(rng.integers(0, world.N, (P, K))).cuda()
    tg[0, 0], tg[1, 1] = world.isolated, src[1]
    e = torch.stack([src.repeat_interleave(K), tg.reshape(-1)])
    want = _fwd(sp.sample_and_fused_attn_stage, csr, e, *nets, **kw)
    assert torch.equal(_fwd(sp.sample_and_fused_attn_stage_star, csr, src, tg, *nets, **kw), want)
    bufs = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=HOPS, stage="attn", table_rows=T, width=H, star=K)
    got = _fwd(sp.sample_and_fused_attn_stage_star, csr, src, tg, *nets, buffers=bufs, **kw)
    bufs.sets.resolve()
    assert torch.equal(got, want)


def _nets_of(hops, H=16):
    torch.manual_seed(7)
    return [m.cuda() for m in (torch.nn.Sequential(torch.nn.Linear(hops + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)),
                               torch.nn.Linear(H, 1), torch.nn.Linear(H, H))]


@pytest.mark.parametrize("walks,hops,wide", [pytest.param(100, 2, False, id="small-100x2"), pytest.param(200, 4, True, id="wide-200x4")])
def test_a_small_shape_and_the_64_bit_keys(sp, world, walks, hops, wide):
    csr, B, T = world.csr, 64, 2048
    kw = dict(num_walks=walks, num_steps=hops, seed=5, wide_keys=wide, table_rows=T)
    nets = _nets_of(hops)
    e = world.pairs(B, 1)
    want = _fwd(sp.sample_and_fused_attn_stage, csr, e, *nets, **kw)
    twin = _fwd(sp.sample_and_attn_stage, csr, e, *nets, **kw)
    scale = float(twin.abs().max())
    assert scale > 0 and float((want - twin).abs().max()) <= FWD_TOL * scale
    bufs = sp.StepBuffers(csr, B, num_walks=walks, num_steps=hops, stage="attn", table_rows=T, width=16, wide_keys=wide)
    assert bufs.wide == wide and bufs.small == (not wide)
    got = _fwd(sp.sample_and_fused_attn_stage, csr, e, *nets, buffers=bufs, **kw)
    bufs.sets.resolve()
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------ 5. training
@pytest.mark.parametrize("value", [True, False])
def test_trains_like_the_reference_first_stage(sp, world, value):
    """sample_and_fused_attn_stage against gather -> pe_embedding -> sum(-2) -> AttentionalAggregation on the (xz, indptr) of
    sample_and_gather for the same seed in float64 (the truth test_gpu_step_attn.py builds): every gradient within GRAD_TOL of its
    largest entry and within max(4 x err32, GRAD_FLOOR), err32 the unfused float32 stage's error (DESIGN 4.7c's criterion, as
    test_gpu_step_attn.py applies it); the gate bias's gradient exactly zero"""
    csr, B, H = world.csr, 300, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e = world.pairs(B, 1)
    fa, fb, f64 = _nets(value), _nets(value), _nets(value, torch.float64)
    w = _random((2, B, H), 1)
    fused = sp.sample_and_fused_attn_stage(csr, e, *fa, **kw)
    assert fused.shape == (2, B, H) and fused.dtype == torch.float32 and fused.requires_grad
    (fused * w).sum().backward()
    unfused = sp.sample_and_attn_stage(csr, e, *fb, **kw)
    (unfused * w).sum().backward()
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
        err32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        print(n, err_fused, err32)
        assert err_fused <= GRAD_TOL, (n, err_fused)
        assert err_fused <= max(4 * err32, GRAD_FLOOR), (n, err_fused, err32)


def test_a_backward_after_the_buffers_next_step_raises(sp, world):
    nets = _nets()
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    bufs = sp.StepBuffers(world.csr, 64, stage="attn", table_rows=1024, width=16, num_walks=M, num_steps=HOPS)
    first = sp.sample_and_fused_attn_stage(world.csr, world.pairs(64, 1), *nets, buffers=bufs, **kw)
    second = sp.sample_and_fused_attn_stage(world.csr, world.pairs(64, 2), *nets, buffers=bufs, **kw)
    with pytest.raises(RuntimeError, match="sample_and_fused_attn_stage.*step 1 .* took step 2"):
        first.sum().backward()
    second.sum().backward()                 # the step the buffers hold trains
    assert all(p.grad is not None for _, p in _params(nets))


# ------------------------------------------------------------------------------------------------------ 6. memory
def test_no_weight_matrix_exists_under_no_grad(sp, world):
    """B = 300, table_rows = 2,048: S*T*4 = 4.9 MB.  With buffers the peak allocation above them stays below half of that (the
    result, E, g and the centre are well under a megabyte): no [S, T] tensor was made.  The unfused call without buffers allocates
    at least S*T*4.  A condition, not a measurement."""
    csr, B, T, H = world.csr, 300, 2048, 96
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=T)
    nets = _nets(H=H)
    e = world.pairs(B, 1)
    W_bytes = 2 * B * T * 4
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="attn", table_rows=T, width=H)
    with torch.no_grad():
        sp.sample_and_fused_attn_stage(csr, e, *nets, buffers=bufs, **kw)       # cached segment lists, lazy loads
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sp.sample_and_fused_attn_stage(csr, e, *nets, buffers=bufs, **kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        print("peak above the buffers", peak, "of", W_bytes)
        assert peak < W_bytes // 2, peak
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        sp.sample_and_attn_stage(csr, e, *nets, **kw)
        torch.cuda.synchronize()
        assert torch.cuda.max_memory_allocated() - base >= W_bytes


# ------------------------------------------------------------------------------------------------------ 7. capture
def test_captured_step_replays_another_batch(sp, world):
    """the buffered step with stage="attn", the modules included, under torch.cuda.graph and no_grad; replayed with a second batch
    copied into the static edge tensor it equals the eager result of that batch bit for bit"""
    csr, B, T, H = world.csr, 300, 1024, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5, table_rows=T)
    nets = _nets()
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    with torch.no_grad():
        want2 = sp.sample_and_fused_attn_stage(csr, e2, *nets, dedup_roots=True, **kw)
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=True, stage="attn", table_rows=T, width=H)
        static = e1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # lazy code-object loads, cached segment lists and GEMM workspaces, uncaptured
            for _ in range(2):
                sp.sample_and_fused_attn_stage(csr, static, *nets, buffers=bufs, dedup_roots=True, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = sp.sample_and_fused_attn_stage(csr, static, *nets, buffers=bufs, dedup_roots=True, **kw)
        static.copy_(e2)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(got, want2)
    assert not int(bufs.status[1])                  # no overflow, no join flag

"""GPU (MI355X): the on-demand step for one source against K targets -- StepBuffers(star=K), sample_and_gather_star /
sample_and_hgather_star, the count and attentional stages of that name, and subgacc_step_prologue_star called directly.  The reference
of every test is the step this change leaves untouched: the same call over the EXPANDED list (source.repeat_interleave(K) against
targets.view(-1)) with the same seed.  Everything is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_helpers import dir_graph, sp  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 17
N = 900                       # dir_graph: the last third of the nodes has no out-edges (dead-end roots)
DEAD = 700
# (num_walks, num_steps, keywords of the shape): the fused-row kernel's 32-bit key rows (packed hand-over by default), the same at two
# hops, the one-wave kernel's key rows under the row-form join, and the 64-bit key rows of four hops
SHAPES = {"200x3": (200, 3, {}), "200x2": (200, 2, {}), "100x2-small": (100, 2, dict(small_rows=True)), "200x4-key64": (200, 4, {})}
# (2, 1024) and (3, 683) lie on both sides of the join's 2,048-pair split
PK = [(1, 1), (1, 7), (3, 1), (5, 13), (64, 33), (2, 1024), (3, 683)]
FORMS_PK = [(5, 13), (64, 33)]


@functools.lru_cache(maxsize=1)
def _csr():
    from surel_plus_amd.sampler import DeviceCSR
    return DeviceCSR(*dir_graph(N, 5000, seed=3, hubs=1))


def _star(P, K, seed=1, outside=False):
    """source [P], targets [P, K] with, where they fit: a target equal to its source, a target repeated under one source, a source
    repeated across P, a node that is a source of one star and a target of another, a dead-end root; outside: a target beyond the
    graph, a negative id and an id beyond int32"""
    rng = np.random.default_rng(seed + 1000 * P + K)
    src, tg = rng.integers(0, 600, P), rng.integers(0, N, (P, K))
    tg[0, 0] = src[0]
    tg[-1, K - 1] = DEAD if P * K > 1 else tg[-1, K - 1]
    if K >= 3:
        tg[0, 2] = tg[0, 1]
    if P >= 2:
        src[1] = src[0]
        tg[1, 0] = src[P - 1]
    if P >= 3:
        src[2] = DEAD + 1
        tg[2, K - 1] = src[0]
    if outside:
        assert K >= 7
        tg[0, 3], tg[0, 4], tg[0, 5] = N + 5, -7, 2 ** 33 + 1
    return torch.from_numpy(src).cuda(), torch.from_numpy(tg).cuda()


def _expand(src, tg):
    return torch.stack([src.repeat_interleave(tg.shape[1]), tg.reshape(-1)])


def _hstar(P, K, seed=2):
    """uv [2, P], w [P, K]: _star's sources and targets with a second kept node v -- v == u once, v == a w once"""
    u, w = _star(P, K, seed)
    v = torch.from_numpy(np.random.default_rng(seed + P).integers(0, N, P)).cuda()
    v[0] = u[0] if P > 1 else w[0, K - 1]
    v[-1] = w[-1, 0]
    return torch.stack([u, v]), w


def _hexpand(uv, w):
    K = w.shape[1]
    return torch.stack([uv[0].repeat_interleave(K), uv[1].repeat_interleave(K), w.reshape(-1)])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _cut(res, bufs, resolve=True):
    """a buffered step's lazy result, resolved -> (xz [R], indptr or ids [R], seg pointers, the status words)"""
    xz, ind, sets = res
    if resolve:
        sets.resolve()
    seg = ind if bufs.ptr else ind.seg_pointers
    R = int(seg[-1].item())
    return xz[:R].clone(), (ind.clone() if bufs.ptr else ind[:R].clone()), seg.clone(), bufs.status.clone()


def _same(got, want):
    (xz, ind, seg, st), (rxz, rind, rseg, rst) = got, want
    assert xz.shape == rxz.shape and xz.dtype == rxz.dtype and xz.shape[0] > 0
    assert torch.equal(seg, rseg) and torch.equal(ind, rind) and ind.dtype == rind.dtype
    assert torch.equal(_bits(xz), _bits(rxz))
    assert torch.equal(st[:2], rst[:2])           # the four int32 status flags, flags[3] among them


# ------------------------------------------------------------------------------------------------- 1. pairs, the f32 row form
@pytest.mark.parametrize("P,K", PK)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_star_step_equals_the_expanded_step(sp, shape, P, K):
    M, m, how = SHAPES[shape]
    csr, (src, tg) = _csr(), _star(P, K)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, **how)
    plain = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, **how)
    star = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, star=K, **how)
    assert (star.star, star.P, star.n, star.S, star.B) == (K, P, P + P * K, 2 * P * K, P * K) and plain.n == 2 * P * K
    assert star.roots.numel() == star.nsize.numel() == star.n and star.seg.numel() == star.S + 1
    assert (star.packed, star.keyrows, star.key64, star.small) == (plain.packed, plain.keyrows, plain.key64, plain.small)
    want = _cut(sp.sample_and_gather(csr, _expand(src, tg), buffers=plain, **kw), plain)
    got = _cut(sp.sample_and_gather_star(csr, src, tg, buffers=star, **kw), star)
    _same(got, want)
    # every source stands once: the rows are [sources | targets], the set of source j is the set of its K expanded rows
    assert torch.equal(star.roots.long(), torch.cat([src, tg.reshape(-1)]))
    assert torch.equal(star.nsize[:P].repeat_interleave(K), plain.nsize[: P * K]) and torch.equal(star.nsize[P:], plain.nsize[P * K:])
    assert int(star.nsize.min()) >= 1 and star.walk_order == "batch"


def test_the_sorted_work_list_runs(sp):
    """n = P + P*K >= 16,384 rows: the walk takes them in ascending order of their root's id"""
    from surel_plus_amd import spjoin
    M, m, P, K = 200, 2, 16, 1024
    csr, (src, tg) = _csr(), _star(P, K)
    kw = dict(num_walks=M, num_steps=m, seed=SEED)
    plain = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m)
    star = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, star=K)
    assert star.n == 16400 >= spjoin.SORT_ROOTS_MIN
    want = _cut(sp.sample_and_gather(csr, _expand(src, tg), buffers=plain, **kw), plain)
    got = _cut(sp.sample_and_gather_star(csr, src, tg, buffers=star, **kw), star)
    _same(got, want)
    assert star.walk_order == plain.walk_order == "id"


@pytest.mark.parametrize("shape", ["200x3", "100x2-small", "200x4-key64"])
def test_roots_outside_the_graph_are_flagged_as_in_the_expanded_step(sp, shape):
    """a target beyond the graph, a negative id, an id beyond int32: empty rows, flags[3] & 16, IndexError at resolve() -- both ways"""
    M, m, how = SHAPES[shape]
    P, K = 5, 13
    csr, (src, tg) = _csr(), _star(P, K, outside=True)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, **how)
    plain = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, **how)
    star = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, star=K, **how)
    res, ref = sp.sample_and_gather_star(csr, src, tg, buffers=star, **kw), sp.sample_and_gather(csr, _expand(src, tg), buffers=plain, **kw)
    _same(_cut(res, star, resolve=False), _cut(ref, plain, resolve=False))
    assert int(star.status.view(torch.int32)[3].item()) & 16
    assert star.roots[P + 3: P + 6].tolist() == [N + 5, -1, -1] and star.nsize[P + 3: P + 6].tolist() == [0, 0, 0]
    for sets in (res[2], ref[2]):
        with pytest.raises(IndexError):
            sets.resolve()


# ------------------------------------------------------------------------------------------------------ 2. every other form
def _form_cases():
    out = []
    for shape, forms in [("200x3", ["segids", "bf16", "fp16", "packed_half", "two_planes", "order", "out", "unbuffered", "two_steps", "numpy"]),
                         ("100x2-small", ["segids", "bf16_segids", "order", "out", "unbuffered", "two_steps"]),
                         ("200x4-key64", ["segids", "bf16_wide", "unbuffered"])]:
        out += [pytest.param(shape, f, id=f"{shape}-{f}") for f in forms]
    return out


@pytest.mark.parametrize("P,K", FORMS_PK)
@pytest.mark.parametrize("shape,form", _form_cases())
def test_each_form_of_the_pair_step(sp, shape, form, P, K):
    M, m, how = SHAPES[shape]
    csr, (src, tg) = _csr(), _star(P, K)
    e = _expand(src, tg)
    made = dict(num_walks=M, num_steps=m, **how)                    # StepBuffers' keywords
    call = dict(num_walks=M, num_steps=m, seed=SEED, **how)         # the call's
    extra = {"segids": dict(ptr=False), "bf16": dict(dtype=torch.bfloat16), "fp16": dict(dtype=torch.float16),
             "bf16_segids": dict(dtype=torch.bfloat16, ptr=False), "bf16_wide": dict(dtype=torch.bfloat16, wide_keys=True)}.get(form, {})
    made.update(extra), call.update(extra)
    if form == "packed_half":
        made.update(dtype=torch.bfloat16, packed_half=True), call.update(dtype=torch.bfloat16)
    if form == "two_planes":
        made.update(packed_rows=False)
    if form == "order":
        order = sp.locality_order(csr)
        made.update(order=order), call.update(order=order)
    if form == "unbuffered":
        rxz, rind, rsets = sp.sample_and_gather(csr, e, **call)
        for lazy in (False, True):
            xz, ind, sets = sp.sample_and_gather_star(csr, src, tg, lazy=lazy, **call)
            if lazy:
                assert sets.pending
                sets.resolve()
                xz = xz[: int(ind[-1].item())]
            assert not sets.pending and not rsets.pending and xz.shape == rxz.shape and xz.shape[0] > 0
            assert torch.equal(ind, rind) and torch.equal(_bits(xz), _bits(rxz))
        xz, ids, _ = sp.sample_and_gather_star(csr, src, tg, ptr=False, **call)
        rxz, rids, _ = sp.sample_and_gather(csr, e, ptr=False, **call)
        assert torch.equal(ids, rids) and torch.equal(ids.seg_pointers, rids.seg_pointers) and torch.equal(_bits(xz), _bits(rxz))
        return
    plain, star = sp.StepBuffers(csr, P * K, **made), sp.StepBuffers(csr, P * K, star=K, **made)
    if form == "packed_half":
        assert star.packed and star.half and plain.packed
    if form == "two_planes":
        assert not star.packed and sp.StepBuffers(csr, P * K, star=K, num_walks=M, num_steps=m).packed
    if form == "out":
        worst = 2 * P * K * (M * m + 1) * 2 * (m + 1)
        out, rout = torch.full((worst + 8,), -3.0, device="cuda"), torch.full((worst + 8,), -3.0, device="cuda")
        want = _cut(sp.sample_and_gather(csr, e, buffers=plain, out=rout, **call), plain)
        res = sp.sample_and_gather_star(csr, src, tg, buffers=star, out=out, **call)
        assert res[0].data_ptr() == out.data_ptr()
        _same(_cut(res, star), want)
        assert torch.equal(out.view(torch.int32), rout.view(torch.int32))        # and nothing behind the rows
        return
    if form == "numpy":
        want = _cut(sp.sample_and_gather(csr, e, buffers=plain, **call), plain)
        _same(_cut(sp.sample_and_gather_star(csr, src.cpu().numpy(), tg.cpu().numpy().tolist(), buffers=star, **call), star), want)
        return
    for seed in ((SEED, SEED + 1, SEED) if form == "two_steps" else (SEED,)):       # the buffers used again, with another seed
        call["seed"] = seed
        want = _cut(sp.sample_and_gather(csr, e, buffers=plain, **call), plain)
        got = _cut(sp.sample_and_gather_star(csr, src, tg, buffers=star, **call), star)
        _same(got, want)
    if form == "order":
        assert star.walk_order == plain.walk_order == "rank"
    if "segids" in form:
        assert got[1].dtype == torch.int64 and int(got[1].max()) == 2 * P * K - 1


# ------------------------------------------------------------------------------------------------------------------ 3. triplets
@pytest.mark.parametrize("shape,P,K", [("200x3", P, K) for P, K in PK] + [("100x2-small", P, K) for P, K in FORMS_PK] +
                         [("200x2", 5, 13), ("200x4-key64", 5, 13)])
def test_the_triplet_star_equals_the_expanded_triplets(sp, shape, P, K):
    M, m, how = SHAPES[shape]
    csr, (uv, w) = _csr(), _hstar(P, K)
    h = _hexpand(uv, w)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, **how)
    plain = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, triplets=True, **how)
    star = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, triplets=True, star=K, **how)
    assert (star.n, star.S, plain.n) == (2 * P + P * K, 4 * P * K, 3 * P * K) and star.partner is None
    for seed in (SEED, SEED + 5):
        kw["seed"] = seed
        want = _cut(sp.sample_and_hgather(csr, h, buffers=plain, **kw), plain)
        got = _cut(sp.sample_and_hgather_star(csr, uv, w, buffers=star, **kw), star)
        _same(got, want)
    assert torch.equal(star.roots.long(), torch.cat([uv.reshape(-1), w.reshape(-1)]))
    if (P, K) == (5, 13):       # and without buffers
        xz, ids, sets = sp.sample_and_hgather_star(csr, uv, w, **kw)
        rxz, rids, _ = sp.sample_and_hgather(csr, h, **kw)
        assert not sets.pending and torch.equal(ids, rids) and torch.equal(ids.seg_pointers, rids.seg_pointers)
        assert torch.equal(_bits(xz), _bits(rxz)) and xz.shape[0] > 0


def test_half_rows_of_a_triplet_star(sp):
    M, m, how = SHAPES["100x2-small"]
    P, K = 5, 13
    csr, (uv, w) = _csr(), _hstar(P, K)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, dtype=torch.bfloat16, **how)
    plain = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, triplets=True, dtype=torch.bfloat16, **how)
    star = sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, triplets=True, dtype=torch.bfloat16, star=K, **how)
    want = _cut(sp.sample_and_hgather(csr, _hexpand(uv, w), buffers=plain, **kw), plain)
    _same(_cut(sp.sample_and_hgather_star(csr, uv, w, buffers=star, **kw), star), want)
    assert want[0].dtype == torch.bfloat16


# -------------------------------------------------------------------------------------------------------------------- 4. stages
STAGE_SHAPES = [pytest.param(200, 3, {}, id="200x3"), pytest.param(100, 2, {}, id="100x2-small"),
                pytest.param(200, 4, dict(wide_keys=True), id="200x4-wide")]


def _nets(m, H=16, seed=0):
    torch.manual_seed(seed)
    mods = [torch.nn.Sequential(torch.nn.Linear(m + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.Linear(H, 1), torch.nn.Linear(H, H)]
    return [mod.cuda() for mod in mods]


def _trained(fn, nets, w):
    """(output, the gradient of every parameter) of fn() under the loss (out * w).sum()"""
    prm = [p for mod in nets for p in mod.parameters()]
    for p in prm:
        p.grad = None
    out = fn()
    (out * w[: out.numel()].view(out.shape)).sum().backward()
    return out.detach().clone(), [None if p.grad is None else p.grad.clone() for p in prm]


def _same_training(got, want):
    assert got[0].shape == want[0].shape and torch.equal(_bits(got[0]), _bits(want[0])) and float(got[0].abs().sum()) > 0
    for a, b in zip(got[1], want[1]):
        assert (a is None) == (b is None) and (a is None or torch.equal(_bits(a), _bits(b)))


@pytest.mark.parametrize("buffered", [False, True], ids=["fit", "buffers"])
@pytest.mark.parametrize("P,K", FORMS_PK)
@pytest.mark.parametrize("M,m,how", STAGE_SHAPES)
def test_the_count_stage_of_a_star(sp, M, m, how, P, K, buffered):
    csr, (src, tg) = _csr(), _star(P, K)
    e = _expand(src, tg)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, **how)
    T = 4096
    mk = lambda **more: sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, stage="counts", table_rows=T, **how, **more)  # noqa: E731
    a, b = ((mk(star=K), mk()) if buffered else (None, None))
    C, sizes, table, sets = sp.sample_and_counts_star(csr, src, tg, buffers=a, **kw)
    rC, rsizes, rtable, rsets = sp.sample_and_counts(csr, e, buffers=b, **kw)
    sets.resolve(), rsets.resolve()
    assert C.shape == rC.shape == (2 * P * K, T if buffered else table.shape[0]) and table.shape[0] > 2
    assert torch.equal(_bits(C), _bits(rC)) and torch.equal(sizes, rsizes) and torch.equal(_bits(table), _bits(rtable))
    assert int(sizes.min()) >= 1 and float(C.sum()) == 2.0 * float(sizes.sum())
    nets, w = _nets(m), torch.randn(2 * P * K * 16, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    got = _trained(lambda: sp.sample_and_mean_stage_star(csr, src, tg, nets[0], buffers=a, **kw), nets[:1], w)
    want = _trained(lambda: sp.sample_and_mean_stage(csr, e, nets[0], buffers=b, **kw), nets[:1], w)
    assert got[0].shape == (2, P * K, 16)
    _same_training(got, want)


@pytest.mark.parametrize("buffered", [False, True], ids=["fit", "buffers"])
@pytest.mark.parametrize("P,K", FORMS_PK)
@pytest.mark.parametrize("M,m,how", STAGE_SHAPES)
def test_the_attentional_stage_of_a_star(sp, M, m, how, P, K, buffered):
    csr, (src, tg) = _csr(), _star(P, K)
    e = _expand(src, tg)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, **how)
    T = 4096
    mk = lambda **more: sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, stage="counts_attn", table_rows=T, **how, **more)  # noqa: E731
    a, b = ((mk(star=K), mk()) if buffered else (None, None))
    gate = lambda t: t @ torch.linspace(-1.0, 1.0, m + 1, device="cuda")  # noqa: E731
    W, sizes, table, sets = sp.sample_and_attn_counts_star(csr, src, tg, gate, buffers=a, **kw)
    W, sizes, table = W.clone(), sizes.clone(), table.clone()
    rW, rsizes, rtable, rsets = sp.sample_and_attn_counts(csr, e, gate, buffers=b, **kw)
    sets.resolve(), rsets.resolve()
    assert W.shape == rW.shape and torch.equal(_bits(W), _bits(rW)) and torch.equal(sizes, rsizes) and torch.equal(_bits(table), _bits(rtable))
    assert float(W.abs().sum()) > 0
    nets, w = _nets(m), torch.randn(2 * P * K * 16, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    got = _trained(lambda: sp.sample_and_attn_stage_star(csr, src, tg, *nets, buffers=a, **kw), nets, w)
    want = _trained(lambda: sp.sample_and_attn_stage(csr, e, *nets, buffers=b, **kw), nets, w)
    assert got[0].shape == (2, P * K, 16)
    _same_training(got, want)


@pytest.mark.parametrize("buffered", [False, True], ids=["fit", "buffers"])
@pytest.mark.parametrize("P,K", FORMS_PK)
@pytest.mark.parametrize("M,m,how", STAGE_SHAPES)
def test_the_triplet_count_stage_of_a_star(sp, M, m, how, P, K, buffered):
    csr, (uv, w3) = _csr(), _hstar(P, K)
    h = _hexpand(uv, w3)
    kw = dict(num_walks=M, num_steps=m, seed=SEED, **how)
    T = 4096
    mk = lambda **more: sp.StepBuffers(csr, P * K, num_walks=M, num_steps=m, stage="counts", table_rows=T, triplets=True, **how, **more)  # noqa: E731
    a, b = ((mk(star=K), mk()) if buffered else (None, None))
    C, sizes, table, sets = sp.sample_and_hcounts_star(csr, uv, w3, buffers=a, **kw)
    rC, rsizes, rtable, rsets = sp.sample_and_hcounts(csr, h, buffers=b, **kw)
    sets.resolve(), rsets.resolve()
    assert C.shape == rC.shape and C.shape[0] == 4 * P * K
    assert torch.equal(_bits(C), _bits(rC)) and torch.equal(sizes, rsizes) and torch.equal(_bits(table), _bits(rtable))
    nets, w = _nets(m), torch.randn(4 * P * K * 16, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    got = _trained(lambda: sp.sample_and_hmean_stage_star(csr, uv, w3, nets[0], buffers=a, **kw), nets[:1], w)
    want = _trained(lambda: sp.sample_and_hmean_stage(csr, h, nets[0], buffers=b, **kw), nets[:1], w)
    assert got[0].shape == (4, P * K, 16)
    _same_training(got, want)


# ------------------------------------------------------------------------------------------- 4b. buffers of the other geometry
@pytest.mark.parametrize("K", [1, 13])
def test_the_plain_calls_refuse_star_buffers_and_the_star_calls_plain_ones(sp, K):
    """an expanded tensor handed to StepBuffers(star=K) is a ValueError that names the geometry -- with K = 1 too, where the sizes
    would fit -- and so are triplets; nothing is launched"""
    csr, P = _csr(), 5
    src, tg = _star(P, K)
    star, plain = sp.StepBuffers(csr, P * K, star=K), sp.StepBuffers(csr, P * K)
    hstar = sp.StepBuffers(csr, P * K, star=K, triplets=True)
    roots = star.roots.clone()
    with pytest.raises(ValueError, match=rf"made for {P} sources against \[{P}, {K}\] targets \(star={K}\)"):
        sp.sample_and_gather(csr, _expand(src, tg), buffers=star)
    with pytest.raises(ValueError, match=rf"made for {P} pairs \(u, v\) against \[{P}, {K}\] targets \(star={K}\)"):
        sp.sample_and_hgather(csr, _hexpand(*_hstar(P, K)), buffers=hstar)
    with pytest.raises(ValueError, match="another geometry"):
        sp.sample_and_gather_star(csr, src, tg, buffers=plain)
    assert torch.equal(star.roots, roots) and getattr(star, "step_id", 0) == 0


# ---------------------------------------------------------------------------------------------------------------- 5. empty stars
@pytest.mark.parametrize("P,K", [(0, 5), (3, 0)])
def test_an_empty_star_is_the_expanded_calls_empty_batch(sp, P, K):
    """what the expanded calls answer for [2, 0] / [3, 0] today, stated: sample_and_hgather and sample_and_attn_counts return empty
    results; sample_and_counts / _hcounts refuse (their StepBuffers take no zero pairs), and sample_and_gather fails in its join's
    view of zero rows -- the star calls answer the same, result or exception, and so do StepBuffers(csr, 0, star=K)"""
    csr = _csr()
    src, tg = torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros((P, K), dtype=torch.int64, device="cuda")
    uv = torch.zeros((2, P), dtype=torch.int64, device="cuda")
    e0, h0 = torch.empty((2, 0), dtype=torch.int64, device="cuda"), torch.empty((3, 0), dtype=torch.int64, device="cuda")
    kw = dict(num_walks=200, num_steps=3, seed=SEED)
    gate = lambda t: t.sum(1)  # noqa: E731
    for got, want in [(sp.sample_and_hgather_star(csr, uv, tg, **kw), sp.sample_and_hgather(csr, h0, **kw)),
                      (sp.sample_and_attn_counts_star(csr, src, tg, gate, **kw), sp.sample_and_attn_counts(csr, e0, gate, **kw))]:
        tensors = [(a, b) for a, b in zip(got, want) if torch.is_tensor(b)]
        assert len(got) == len(want) and len(tensors) >= 2
        for a, b in tensors:
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    for err, match, star, plain in [
            (ValueError, "pairs = 0 is not a whole number of batches", lambda: sp.sample_and_counts_star(csr, src, tg, **kw), lambda: sp.sample_and_counts(csr, e0, **kw)),
            (ValueError, "pairs = 0 is not a whole number of batches", lambda: sp.sample_and_hcounts_star(csr, uv, tg, **kw), lambda: sp.sample_and_hcounts(csr, h0, **kw)),
            (RuntimeError, "cannot reshape tensor of 0 elements", lambda: sp.sample_and_gather_star(csr, src, tg, **kw), lambda: sp.sample_and_gather(csr, e0, **kw)),
            (ValueError, "pairs = 0 is not a whole number of batches", lambda: sp.StepBuffers(csr, 0, star=max(K, 1)), lambda: sp.StepBuffers(csr, 0))]:
        with pytest.raises(err, match=match) as a:
            star()
        with pytest.raises(err, match=match) as b:
            plain()
        assert str(a.value) == str(b.value)


# --------------------------------------------------------------------------------------------- 6. the prologue kernel, called directly
RIM = 64
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _ids(n, seed):
    """n int64 ids with the int32 limits and what lies beyond them in front"""
    edge = [0, 2 ** 31 - 1, 2 ** 31, -1, 2 ** 40, -2 ** 40, 2 ** 31 - 2, 2 ** 63 - 1, -2 ** 63, 2 ** 32]
    v = np.random.default_rng(seed).integers(0, 2 ** 31, n)
    v[: min(n, len(edge))] = edge[:n]
    return torch.from_numpy(v).cuda()


@pytest.mark.parametrize("cap", [0, 1024], ids=["no-table", "table-1024"])
@pytest.mark.parametrize("nh,nt", [(0, 0), (1, 0), (0, 1), (255, 0), (0, 256), (128, 129), (257, 1), (1, 255), (1000, 777), (10, 2049)])
def test_the_prologue_kernel_between_poisoned_rims(sp, nh, nt, cap):
    from surel_plus_amd import _lib
    L, n, n_zero = _lib.lib(), nh + nt, 4
    heads, tails = _ids(nh, 1), _ids(nt, 2).flip(0)
    roots = torch.full((n + 2 * RIM,), POISON32, dtype=torch.int32, device="cuda")
    words = torch.full((n_zero + 2 * RIM,), POISON64, dtype=torch.int64, device="cuda")
    tbytes = L.subgacc_uniq_table_bytes(cap) if cap else 0
    assert tbytes == cap * 20
    table = torch.full((tbytes + 2 * RIM * 8,), 0x5A, dtype=torch.uint8, device="cuda")
    p = lambda t, off, size: C.c_void_p(t.data_ptr() + off * size)  # noqa: E731
    rc = L.subgacc_step_prologue_star(p(table, RIM, 8) if cap else None, cap if cap else 12345, p(words, RIM, 8), n_zero,
                                      C.c_void_p(heads.data_ptr()) if nh else None, nh, C.c_void_p(tails.data_ptr()) if nt else None, nt,
                                      p(roots, RIM, 4) if n else None, _lib.stream_ptr())
    assert rc == 0, L.subgacc_last_error()
    torch.cuda.synchronize()
    both = torch.cat([heads, tails])
    want = torch.where((both < 0) | (both > 2 ** 31 - 1), torch.full_like(both, -1), both).to(torch.int32)
    assert torch.equal(roots[RIM: RIM + n], want)
    assert bool((roots[:RIM] == POISON32).all()) and bool((roots[RIM + n:] == POISON32).all())
    assert bool((words[RIM: RIM + n_zero] == 0).all()) and bool((words[:RIM] == POISON64).all()) and bool((words[RIM + n_zero:] == POISON64).all())
    assert bool((table[: RIM * 8] == 0x5A).all()) and bool((table[RIM * 8 + tbytes:] == 0x5A).all())
    if cap:         # the reset of subgacc_uniq_reset: keys and min tags all ones, ids -1
        body = table[RIM * 8: RIM * 8 + tbytes]
        assert bool((body[: cap * 16].view(torch.int64) == -1).all()) and bool((body[cap * 16:].view(torch.int32) == -1).all())
        ref = torch.full((tbytes,), 0x33, dtype=torch.uint8, device="cuda")
        assert L.subgacc_uniq_reset(C.c_void_p(ref.data_ptr()), cap, _lib.stream_ptr()) == 0
        assert torch.equal(body, ref)
    if n >= 10:     # the narrowing is the plain prologue's
        plain = torch.full((n,), POISON32, dtype=torch.int32, device="cuda")
        assert L.subgacc_step_prologue(None, 0, None, 0, C.c_void_p(both.data_ptr()), C.c_void_p(plain.data_ptr()), n, _lib.stream_ptr()) == 0
        assert torch.equal(plain, want)


def test_the_prologue_zeroes_more_words_than_it_has_roots(sp):
    """the launch spans the largest of (capacity, n_zero, n): 300 words with 3 roots and no table"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    words = torch.full((300 + 2 * RIM,), POISON64, dtype=torch.int64, device="cuda")
    roots = torch.full((3 + 2 * RIM,), POISON32, dtype=torch.int32, device="cuda")
    heads, tails = _ids(1, 1), _ids(2, 2)
    rc = L.subgacc_step_prologue_star(None, 0, C.c_void_p(words.data_ptr() + RIM * 8), 300, C.c_void_p(heads.data_ptr()), 1,
                                      C.c_void_p(tails.data_ptr()), 2, C.c_void_p(roots.data_ptr() + RIM * 4), _lib.stream_ptr())
    assert rc == 0, L.subgacc_last_error()
    assert bool((words[RIM: RIM + 300] == 0).all()) and bool((words[:RIM] == POISON64).all()) and bool((words[RIM + 300:] == POISON64).all())
    assert roots[RIM: RIM + 3].tolist() == [0, 0, 2 ** 31 - 1] and bool((roots[RIM + 3:] == POISON32).all())

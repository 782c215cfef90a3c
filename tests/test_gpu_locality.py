"""GPU (MI355X): the locality order (csrc/locality.hip, sampler.locality_order) equals its NumPy restatement bit for bit, and every
walk path that takes `order=` gives bit for bit the result of the default order -- with the rank path shown to have run
(walk_order == "rank"): the order of the walk is unobservable (Philox keys a walk by its root, the list-order entry points keep
every row's rand_r stream position)."""
import numpy as np
import pytest
import torch

from gpu_helpers import sp, sym_graph  # noqa: F401
from locality_ref import locality_labels, order_and_rank

pytestmark = pytest.mark.gpu


def _with_isolated(ptr_, idx, extra):
    """`extra` isolated nodes appended to the graph"""
    return np.concatenate([ptr_, np.full(extra, ptr_[-1], dtype=ptr_.dtype)]), idx


def _graphs(sp):
    from surel_plus_amd.graphs import community_graph, powerlaw_graph
    c = community_graph(20000, 12.0, seed=5, block=500, device="cpu")
    p = powerlaw_graph(6000, 9.0, seed=2, device="cpu")
    hp, hx = sym_graph(3000, 40000, seed=23, hubs=3)             # hubs of several hundred neighbours: above cap
    ip, ix = _with_isolated(hp, hx, 250)
    return {"community": (c.indptr.numpy(), c.indices.numpy()), "powerlaw": (p.indptr.numpy(), p.indices.numpy()),
            "hubs_isolated": (ip, ix)}


@pytest.mark.parametrize("name", ["community", "powerlaw", "hubs_isolated"])
@pytest.mark.parametrize("rounds,cap,i64", [(8, 64, False), (5, 16, False), (8, 64, True), (3, 1, True)])
def test_device_order_equals_the_numpy_restatement(sp, name, rounds, cap, i64):
    ip, ix = _graphs(sp)[name]
    if name == "hubs_isolated":
        deg = np.diff(ip)
        assert deg.max() > 64 and (deg == 0).sum() >= 250
    csr = sp.DeviceCSR(ip.astype(np.int64) if i64 else ip, ix)
    assert csr.indptr64 == i64
    lo = sp.locality_order(csr, rounds=rounds, cap=cap)
    lab = locality_labels(ip, ix, rounds=rounds, cap=cap)
    order, rank = order_and_rank(lab)
    assert lo.num_nodes == csr.num_nodes
    assert lo.rank.dtype == lo.order.dtype == torch.int32 and lo.rank.is_cuda and lo.order.is_cuda
    assert np.array_equal(lo.labels.cpu().numpy(), lab)
    assert np.array_equal(lo.order.cpu().numpy(), order) and np.array_equal(lo.rank.cpu().numpy(), rank)
    assert np.array_equal(np.sort(lo.rank.cpu().numpy()), np.arange(csr.num_nodes))
    again = sp.locality_order(csr, rounds=rounds, cap=cap)
    assert torch.equal(again.labels, lo.labels) and torch.equal(again.rank, lo.rank) and torch.equal(again.order, lo.order)


def _orders(sp, csr):
    g = torch.Generator().manual_seed(11)
    perm_rank = torch.randperm(csr.num_nodes, generator=g).to(torch.int32).cuda()
    return {"perm": perm_rank, "locality": sp.locality_order(csr)}


@pytest.fixture(scope="module")
def scattered(sp):
    """a community graph with its ids scattered (graphs.relabeled with a random permutation)"""
    from surel_plus_amd.graphs import community_graph, relabeled
    g = community_graph(30000, 12.0, seed=5, block=1000, device="cuda")
    return relabeled(g, torch.randperm(30000, generator=torch.Generator().manual_seed(3)).cuda())


@pytest.mark.parametrize("dedup", [False, True])
def test_sample_and_gather_in_rank_order(sp, scattered, dedup):
    from surel_plus_amd.graphs import query_pairs
    csr = scattered
    e = query_pairs(csr, 20000, seed=4)
    xz, ind, sets = sp.sample_and_gather(csr, e, num_walks=200, num_steps=3, seed=5, dedup_roots=dedup)
    for key, order in _orders(sp, csr).items():
        oxz, oind, osets = sp.sample_and_gather(csr, e, num_walks=200, num_steps=3, seed=5, dedup_roots=dedup, order=order)
        assert osets.walk_order == "rank", key
        assert torch.equal(ind, oind) and torch.equal(xz[: int(ind[-1])], oxz[: int(oind[-1])]), key


@pytest.mark.parametrize("form", ["one", "batch", "rand_r", "dedup"])
def test_step_buffers_in_rank_order(sp, form):
    ptr_, idx = sym_graph(3000, 40000, seed=23, hubs=3)
    csr = sp.DeviceCSR(ptr_, idx)
    B, M, hops = 2048, 200, 3
    kw = dict(num_walks=M, num_steps=hops)
    if form == "batch":
        kw["batch"] = 512
    if form == "rand_r":
        kw["rng"] = "rand_r"
    if form == "dedup":
        kw["dedup_roots"] = True
    rng = np.random.default_rng(7)
    for key, order in _orders(sp, csr).items():
        plain = sp.StepBuffers(csr, B, **kw)
        ranked = sp.StepBuffers(csr, B, order=order, **kw)
        for s in range(2):
            hi = (300, 3000)[s]
            e = torch.from_numpy(rng.integers(0, hi, (2, B))).cuda()
            if form == "batch":
                e = e.view(2, 4, 512).permute(1, 0, 2).contiguous()
            call = dict(num_walks=M, num_steps=hops, seed=9, rng=kw.get("rng", "philox"), dedup_roots=form == "dedup")
            xz, ind, sets = sp.sample_and_gather(csr, e, buffers=plain, **call)
            sets.resolve()
            R = int(ind[-1].item())
            rxz, rind, rsets = sp.sample_and_gather(csr, e, buffers=ranked, **call)
            rsets.resolve()
            assert ranked.walk_order == "rank" and rsets.walk_order == "rank", (key, form)
            assert plain.walk_order != "rank"
            assert torch.equal(ind, rind) and torch.equal(xz[:R], rxz[:R]), (key, form, s)


def test_sample_and_gather_many_in_rank_order(sp, scattered):
    from surel_plus_amd.graphs import query_pairs
    csr = scattered
    e = query_pairs(csr, 4 * 1024, seed=6).view(2, 4, 1024).permute(1, 0, 2).contiguous()
    views, sets = sp.sample_and_gather_many(csr, e, num_walks=200, num_steps=3, seed=5)
    for key, order in _orders(sp, csr).items():
        oviews, osets = sp.sample_and_gather_many(csr, e, num_walks=200, num_steps=3, seed=5, order=order)
        assert osets.walk_order == "rank", key
        for (a, ai), (b, bi) in zip(views, oviews):
            assert torch.equal(ai, bi) and torch.equal(a, b), key


@pytest.mark.parametrize("rng", ["philox", "rand_r"])
def test_offline_subg_matrix_in_rank_order(sp, rng):
    ptr_, idx = sym_graph(3000, 40000, seed=23, hubs=3)
    csr = sp.DeviceCSR(ptr_, idx)
    N = csr.num_nodes
    z, enc = sp.subg_matrix(csr, np.arange(N), num_walks=200, num_steps=4, rng=rng)
    for key, order in _orders(sp, csr).items():
        for q in (np.arange(N), torch.arange(N, device="cuda")):       # host query: the order is the list; device: by rank
            oz, oenc = sp.subg_matrix(csr, q, num_walks=200, num_steps=4, rng=rng, order=order)
            assert oz.sets.walk_order == "rank", key
            assert torch.equal(z.indptr, oz.indptr) and torch.equal(z.indices, oz.indices) and torch.equal(z.data, oz.data), key
            assert np.array_equal(enc, oenc), key
    assert z.sets.walk_order == "batch"


def test_by_rank_with_the_identity_equals_by_root(sp):
    from surel_plus_amd import _lib
    from surel_plus_amd._lib import ptr
    L = _lib.lib()
    N, n = 50000, 70000
    rng = np.random.default_rng(1)
    roots_h = rng.integers(0, N, n).astype(np.int32)
    roots_h[rng.random(n) < 0.1] = -2 ** 31                 # SUBGACC_NO_ROOT: left out
    roots_h[:3] = [-1, 2 ** 31 - 1, -5]                      # outside the graph: the last bucket of both
    roots = torch.from_numpy(roots_h).cuda()
    rank = torch.arange(N, dtype=torch.int32, device="cuda")
    out = {}
    for name in ("root", "rank"):
        wl = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        nw = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.zeros(L.subgacc_worklist_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        st = _lib.stream_ptr()
        for _ in range(2):      # the workspace is left zeroed for the next call
            if name == "root":
                _lib.check(L.subgacc_worklist_by_root(ptr(roots), n, N, ptr(wl), ptr(nw), ptr(ws), ws.numel(), st))
            else:
                _lib.check(L.subgacc_worklist_by_rank(ptr(roots), n, ptr(rank), N, ptr(wl), ptr(nw), ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        assert int(ws.view(torch.int32)[4:4 + 1024].abs().sum()) == 0
        k = int(nw.item())
        out[name] = wl[:k].cpu().numpy()
    a, b = out["root"], out["rank"]
    listed = np.flatnonzero(roots_h != -2 ** 31)
    assert np.array_equal(np.sort(a), listed) and np.array_equal(np.sort(b), listed)
    shift = 0
    while (N - 1) >> shift >= 1024:
        shift += 1
    ba = np.minimum((roots_h[a].astype(np.int64) & 0xFFFFFFFF) >> shift, 1023)
    bb = np.minimum((roots_h[b].astype(np.int64) & 0xFFFFFFFF) >> shift, 1023)
    assert np.all(np.diff(ba) >= 0) and np.array_equal(ba, bb)


def test_order_argument_is_checked(sp, scattered):
    from surel_plus_amd.graphs import query_pairs
    csr = scattered
    e = query_pairs(csr, 256, seed=4)
    N = csr.num_nodes
    for bad in (torch.arange(N - 1, dtype=torch.int32, device="cuda"), torch.arange(N, dtype=torch.int64, device="cuda"),
                torch.arange(N, dtype=torch.int32), list(range(N)), "rank"):
        with pytest.raises(ValueError):
            sp.sample_and_gather(csr, e, num_walks=200, num_steps=3, order=bad)
        with pytest.raises(ValueError):
            sp.StepBuffers(csr, 256, order=bad)
        with pytest.raises(ValueError):
            sp.sample_sets(csr, e[0], num_walks=200, num_steps=3, root_order=bad)
    small = sp.DeviceCSR(*sym_graph(300, 2000, seed=1))
    with pytest.raises(ValueError):
        sp.subg_matrix(csr, np.arange(N), num_walks=20, num_steps=3, order=sp.locality_order(small))

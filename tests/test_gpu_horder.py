"""GPU (MI355X): the higher-order path (main_horder.py; model_horder.py:42-59; train.py:48-72, 142-172) on demand -- segment ids from
the strided rows of an on-demand step (pairs with ptr=False, triplets always), sample_and_hgather with and without root dedup,
hgather_counts and the fused HONet first stage hmean_stage.  Every comparison of xz, ids, pointers and counts is bit for bit; the
model stage is compared with the tolerances test_mean_stage_trains_like_the_reference_first_stage states."""
import numpy as np
import pytest
import torch

import oracle
from gpu_helpers import _load, _spg_from_golden, sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu

M = 200
STARS = (63, 64, 65, 127, 128, 129)        # a star's centre with L - 1 <= M leaves: the first hop goes to every leaf once, its set has L members
# hops, key_rows: 32-bit keys (2 and 3 hops), 64-bit keys (4 hops with M = 200), table slots
VARIANTS = [pytest.param(2, True, id="2hops-key32"), pytest.param(3, True, id="3hops-key32"), pytest.param(4, True, id="4hops-key64"),
            pytest.param(3, False, id="3hops-slots")]


class World:
    """One graph for the file: a random graph of N0 nodes with two hubs (nodes 0, 1), behind it one star per length of STARS (centre
    first) and one isolated node; the all-nodes store of a hop count is sampled once."""

    def __init__(self, sp, N0=6000, E=30000, seed=7):
        import scipy.sparse as sps
        rng = np.random.default_rng(seed)
        r, c = rng.integers(0, N0, E), rng.integers(0, N0, E)
        r = np.concatenate([r, np.repeat(np.arange(2), N0 // 2)])
        c = np.concatenate([c, rng.integers(0, N0, 2 * (N0 // 2))])
        nxt, self.centre = N0, {}
        for L in STARS:
            self.centre[L] = nxt
            r, c = np.concatenate([r, np.full(L - 1, nxt)]), np.concatenate([c, nxt + 1 + np.arange(L - 1)])
            nxt += L
        self.isolated, self.N, self.N0, self.hubs = nxt, nxt + 1, N0, (0, 1)
        A = sps.csr_matrix((np.ones(len(r)), (r, c)), shape=(self.N, self.N))
        A = sps.csr_matrix(A + A.T)
        A.setdiag(0)
        A.eliminate_zeros()
        A.sort_indices()
        self.indptr, self.indices = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        assert self.indptr[self.isolated + 1] == self.indptr[self.isolated]
        self.sp, self.csr, self._stores = sp, sp.DeviceCSR(self.indptr, self.indices), {}

    @property
    def special(self):
        return [self.isolated, *self.hubs, *self.centre.values()]

    def store(self, hops):
        """(z, table, lens): the store of ALL nodes with seed 5, its Z_SF table, its row lengths on the host"""
        if hops not in self._stores:
            z, sets = self.sp.sample_spg(self.csr, torch.arange(self.N, dtype=torch.int32, device="cuda"), num_walks=M, num_steps=hops,
                                         seed=5, rng="philox")
            self._stores[hops] = (z, sets.feature_table(), np.diff(z.indptr.cpu().numpy()))
        return self._stores[hops]

    def pairs(self, B, seed):
        """[2, B] pairs: every special root against itself, against another special root and against random nodes, then random pairs"""
        rng = np.random.default_rng(seed)
        e = rng.integers(0, self.N, (2, B))
        s = self.special
        k = len(s)
        e[:, :k] = [s, s]
        e[:, k:2 * k] = [s, s[1:] + s[:1]]
        e[0, 2 * k:3 * k] = s
        e[1, 3 * k:4 * k] = s
        return torch.from_numpy(e).cuda()

    def triplets(self, B, seed):
        """[3, B] triplets with u == v, u == w, u == v == w, the isolated root, a hub and every star centre in every role"""
        rng = np.random.default_rng(seed)
        h = rng.integers(0, self.N, (3, B))
        a, b = int(h[0, 0]), int(h[1, 0]) if h[1, 0] != h[0, 0] else int(h[0, 0]) + 1
        h[:, 0], h[:, 1], h[:, 2] = (a, a, b), (a, b, a), (b, b, b)
        s = self.special
        for role in range(3):
            h[role, 3 + role * len(s): 3 + (role + 1) * len(s)] = s
        at = 3 + 3 * len(s)
        h[:, at] = (self.isolated,) * 3
        h[:, at + 1] = (self.hubs[0], self.hubs[1], self.hubs[0])
        h[:, at + 2] = (self.centre[63], self.centre[64], self.centre[65])
        h[:, at + 3] = (self.centre[129], self.centre[128], self.centre[127])
        return torch.from_numpy(h).cuda()


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _assert_same(got, want):
    (xz, ids), (wxz, wids) = got, want
    assert xz.shape == wxz.shape and torch.equal(xz, wxz)
    assert ids.dtype == torch.int64 and torch.equal(ids, wids)
    assert torch.equal(ids.seg_pointers, wids.seg_pointers)


def _assert_buffered(xz_b, ids_b, R, want):
    """a buffered step answers with views of its buffers: their first R rows are the result, the pointers ride on the ids"""
    wxz, wids = want
    assert R == wxz.shape[0] and torch.equal(xz_b[:R], wxz)
    assert ids_b.dtype == torch.int64 and torch.equal(ids_b[:R], wids)
    assert torch.equal(ids_b.seg_pointers, wids.seg_pointers)


# -------------------------------------------------------------------------------------------------- 1. pairs, ptr=False, on demand
@pytest.mark.parametrize("hops,key_rows", VARIANTS)
def test_pairs_on_demand_with_segment_ids(sp, world, hops, key_rows):
    """sample_and_gather(ptr=False) (train.py:25-30 on the on-demand path): the xz of ptr=True, the ids its pointers spell, both equal
    to gather(ptr=False) over the all-nodes store; allocating, deduplicated, and through StepBuffers(ptr=False) batch after batch"""
    from surel_plus_amd.sampler import key_rows_form
    csr, B = world.csr, 300
    z, table, _ = world.store(hops)
    kw = dict(num_walks=M, num_steps=hops, seed=5, rng="philox", key_rows=key_rows)
    assert key_rows_form(M, hops) == (64 if hops == 4 else 32)
    batches = [world.pairs(B, 1), world.pairs(B, 2)]
    want = [sp.gather(e, z, "cuda", ptr=False, encode=table) for e in batches]
    assert want[0][0].shape[0] != want[1][0].shape[0]                      # two different batches
    e = batches[0]
    xz_p, ind_p, _ = sp.sample_and_gather(csr, e, **kw)
    xz_i, ids, sets = sp.sample_and_gather(csr, e, ptr=False, **kw)
    assert sets.strided and bool(sets.keyrows) == key_rows and (not key_rows or sets.key64 == (hops == 4))
    assert torch.equal(xz_i, xz_p) and torch.equal(ids.seg_pointers, ind_p)
    assert torch.equal(ids, torch.repeat_interleave(torch.arange(2 * B, device="cuda"), ind_p[1:] - ind_p[:-1]))
    _assert_same((xz_i, ids), want[0])
    xz_d, ids_d, sets_d = sp.sample_and_gather(csr, e, ptr=False, dedup_roots=True, **kw)
    assert sets_d.nsize.numel() == np.unique(e.cpu().numpy()).size < 2 * B
    _assert_same((xz_d, ids_d), want[0])
    for dedup in (False, True):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=hops, ptr=False, dedup_roots=dedup, key_rows=key_rows)
        assert bufs.keyrows == key_rows and bufs.segid is not None
        for e_b, (wxz, wids) in zip(batches + batches[:1], want + want[:1]):
            xz_b, ids_b, sets_b = sp.sample_and_gather(csr, e_b, ptr=False, buffers=bufs, dedup_roots=dedup, **kw)
            sets_b.prefetch().resolve()
            R = int(sets_b.extra[0])
            _assert_buffered(xz_b, ids_b, R, (wxz, wids))
            if dedup:
                assert sets_b.n_distinct == np.unique(e_b.cpu().numpy()).size


# ---------------------------------------------------------------------------------------------------------- 2. triplets on demand
@pytest.mark.parametrize("hops,key_rows", VARIANTS)
def test_triplets_on_demand_equal_hgather_over_the_store(sp, world, hops, key_rows):
    """sample_and_hgather == hgather(hedge, z, encode=table) from the all-nodes store of the same seed, allocating and buffered; the
    batch holds u == v, u == w, u == v == w, an isolated root and (3 hops and more) a hub row of more than 512 members"""
    csr, B = world.csr, 256
    z, table, lens = world.store(hops)
    kw = dict(num_walks=M, num_steps=hops, seed=5, key_rows=key_rows)
    batches = [world.triplets(B, 3), world.triplets(B, 4)]
    for h in batches:
        hn = h.cpu().numpy()
        u, v, w = hn
        assert ((u == v) & (u != w)).any() and ((u == w) & (u != v)).any() and ((u == v) & (v == w)).any()
        assert all((hn[role] == world.isolated).any() for role in range(3)) and lens[world.isolated] == 1
        assert all((hn[role] == world.hubs[0]).any() for role in range(3))
        if hops >= 3:
            assert lens[world.hubs[0]] > 512 and lens[world.hubs[1]] > 512      # the late spans: rows beyond kRegTrips * NT members
        assert all(lens[c] == L for L, c in world.centre.items())
    want = [sp.hgather(h, z, "cuda", encode=table) for h in batches]
    assert want[0][0].shape[0] != want[1][0].shape[0]
    h = batches[0]
    xz, ids, sets = sp.sample_and_hgather(csr, h, **kw)
    assert sets.strided and bool(sets.keyrows) == key_rows and sets.nsize.numel() == 3 * B      # 3B roots walked, not 4B
    assert int(ids.max()) == 4 * B - 1 and ids.seg_pointers.numel() == 4 * B + 1
    _assert_same((xz, ids), want[0])
    assert np.array_equal(sets.nsize.cpu().numpy(), lens[h.cpu().numpy().reshape(-1)])
    out = torch.full((xz.numel() + 64,), -7.0, device="cuda")
    xz_o, ids_o, _ = sp.sample_and_hgather(csr, h.cpu().numpy(), out=out, **kw)               # NumPy triplets, a caller's buffer
    _assert_same((xz_o, ids_o), want[0])
    assert xz_o.data_ptr() == out.data_ptr() and bool((out[xz.numel():] == -7.0).all())
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=hops, triplets=True, key_rows=key_rows)
    assert bufs.triplets and not bufs.ptr and bufs.roots.numel() == 3 * B and bufs.seg.numel() == 4 * B + 1
    for h_b, (wxz, wids) in zip(batches + batches[:1], want + want[:1]):
        xz_b, ids_b, sets_b = sp.sample_and_hgather(csr, h_b, buffers=bufs, **kw)
        sets_b.prefetch().resolve()
        R = int(sets_b.extra[0])
        assert sets_b.X == int(lens[h_b.cpu().numpy()].sum())          # w is joined twice and counted once
        _assert_buffered(xz_b, ids_b, R, (wxz, wids))


# ------------------------------------------------------------------------------------------------------- 3. root dedup for triplets
def _reference_shaped(world, P, K, seed):
    """P positives (u, v, w), each followed by its K negatives -- (u, v) kept, w drawn at random (dataloader.py:265-268, 275) --, with
    nodes that appear in different roles: some w are drawn from the u's and v's of other triplets"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, world.N, (3, P))
    pos[:, 0] = (world.hubs[0], world.isolated, world.centre[129])
    h = np.repeat(pos, K + 1, axis=1)
    neg = rng.integers(0, world.N, P * (K + 1))
    mixed = rng.random(P * (K + 1)) < 0.2
    neg[mixed] = pos[rng.integers(0, 2, mixed.sum()), rng.integers(0, P, mixed.sum())]
    is_neg = np.tile(np.arange(K + 1) > 0, P)
    h[2, is_neg] = neg[is_neg]
    return torch.from_numpy(h).cuda()


@pytest.mark.parametrize("hops,key_rows", VARIANTS)
def test_triplet_root_dedup_changes_nothing_but_the_walks(sp, world, hops, key_rows):
    """dedup_roots=True through subgacc_step_prologue_dedup_roles: the (xz, ids) of the plain step, np.unique(hedge).size roots walked,
    batch after batch through the same buffers"""
    csr, P, K = world.csr, 40, 12
    B = P * (K + 1)
    z, table, lens = world.store(hops)
    kw = dict(num_walks=M, num_steps=hops, seed=5, key_rows=key_rows)
    batches = [_reference_shaped(world, P, K, 11), _reference_shaped(world, P, K, 12)]
    for h in batches:
        u, v, w = h.cpu().numpy()
        assert np.intersect1d(w, np.concatenate([u, v])).size > 5 and np.unique(h.cpu().numpy()).size < 3 * B // 2
    h = batches[0]
    plain = sp.sample_and_hgather(csr, h, **kw)
    _assert_same(plain[:2], sp.hgather(h, z, "cuda", encode=table))
    xz_d, ids_d, sets_d = sp.sample_and_hgather(csr, h, dedup_roots=True, **kw)
    assert sets_d.nsize.numel() == np.unique(h.cpu().numpy()).size
    _assert_same((xz_d, ids_d), plain[:2])
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=hops, triplets=True, dedup_roots=True, key_rows=key_rows)
    for h_b in batches + batches[:1]:
        wxz, wids = sp.hgather(h_b, z, "cuda", encode=table)
        xz_b, ids_b, sets_b = sp.sample_and_hgather(csr, h_b, buffers=bufs, dedup_roots=True, **kw)
        sets_b.prefetch().resolve()
        R = int(sets_b.extra[0])
        hn = h_b.cpu().numpy()
        assert sets_b.n_distinct == np.unique(hn).size
        _assert_buffered(xz_b, ids_b, R, (wxz, wids))
        # the sets sit in the rows of the first occurrences over [u | v | w], every other row is empty
        flat = hn.reshape(-1)
        first = np.zeros(flat.size, bool)
        first[np.unique(flat, return_index=True)[1]] = True
        roots = bufs.roots.cpu().numpy()
        assert np.array_equal(roots[first], flat[first]) and (roots[~first] == -2 ** 31).all()
        assert np.array_equal(bufs.nsize.cpu().numpy(), np.where(first, lens[flat], 0))
        assert sets_b.X == int(lens[flat[first]].sum())


# ------------------------------------------------------------------------------------ 4. segment-length boundaries with ids requested
def test_segment_ids_at_every_length_boundary(sp, world):
    """segments of 1, 63, 64, 65, 127, 128, 129 and more than 512 rows -- one span, a span boundary, the register trips' end and the late
    spans of sjoin_keypair_kernel -- joined with ids from strided rows of every payload, as pairs and as triplets, against
    oracle.sjoin over the same rows pulled to the host"""
    csr = world.csr
    rs = np.random.default_rng(21)
    roots = np.concatenate([world.special, rs.integers(0, world.N0, 24)])
    n, k = roots.size, len(world.special)
    seen = set()
    for hops, walks, key_rows in ((3, M, True), (3, M, False), (4, M, True), (2, M, True), (2, M, False)):
        zs, sets = sp.sample_spg(csr, torch.from_numpy(roots).to("cuda", torch.int32), num_walks=walks, num_steps=hops, seed=5, rng="philox",
                                 strided=True, key_rows=key_rows, number_rows=False)      # (as the on-demand step samples: numbered on demand)
        assert sets.strided and bool(sets.keyrows) == key_rows and sets.key64 == (key_rows and hops == 4)
        # every special row against itself, against every other special row, and against random rows, in both places of a pair
        a, b = np.meshgrid(np.arange(k), np.arange(n), indexing="ij")
        e = np.concatenate([np.stack([a.ravel(), b.ravel()]), np.stack([b.ravel(), a.ravel()])[:, ::3]], axis=1)
        h = np.stack([e[0], e[1], np.roll(e[0], 5)])[:, : e.shape[1] // 2]
        xz, ids = sp.gather(e, zs, "cuda", ptr=False, encode=zs.slot_table())
        hxz, hids = sp.hgather(h, zs, "cuda", encode=zs.slot_table())
        # the same rows on the host: packed, payload = SFptr + 1 into Z_SF = enc / M (main.py:174) with the zero row in front
        zc = zs.to_csr()
        rows_h = (zc.indptr.cpu().numpy(), zc.indices.cpu().numpy(), zc.data.cpu().numpy())
        zsf = oracle.enc_table(sets.enc_int16().cpu().numpy()).astype(np.float32) / np.float32(walks)
        for (got_xz, got_ids), (own, partner) in (((xz, ids), oracle.pair_segments(e)), ((hxz, hids), oracle.triplet_segments(h))):
            seg, pairs = oracle.sjoin(*rows_h, own, partner)
            assert np.array_equal(got_ids.seg_pointers.cpu().numpy(), seg)
            assert np.array_equal(got_ids.cpu().numpy(), np.repeat(np.arange(own.size), np.diff(seg)))
            assert np.array_equal(got_xz.cpu().numpy(), zsf[pairs])
            lens = np.diff(seg)
            seen |= {int(v) for v in np.unique(lens) if v in (1,) + STARS} | ({">512"} if lens.max() > 512 else set())
            if hops >= 3:
                assert lens.max() > 512
    assert seen == {1, *STARS, ">512"}, seen


# ------------------------------------------------------------------------------------------------------------- 5. hgather_counts
def _oracle_hcounts(spg, hedge, rows):
    own, partner = oracle.triplet_segments(hedge)
    seg, pairs = oracle.sjoin(spg[0], spg[1], spg[2], own, partner)
    C = np.zeros((len(own), rows), np.float32)
    segid = np.repeat(np.arange(len(own)), np.diff(seg))
    np.add.at(C, (segid, pairs[:, 0]), 1)
    np.add.at(C, (segid, pairs[:, 1]), 1)
    return C, np.diff(seg)


def test_hgather_counts_match_the_oracle(sp):
    """C[j, p] over hgather's four blocks, exactly; two slots per output row"""
    g = _load("hjoin_int.npz")
    cases = [(g, g["hedge"], g["encode"].shape[0])]
    ge = _load("sjoin_int_emptyrows.npz")
    n_rows = ge["z_indptr"].size - 1
    he = np.random.default_rng(3).integers(0, n_rows, (3, 700))
    assert (np.diff(ge["z_indptr"])[he] == 0).any(axis=1).all()                 # empty rows are hit in every role
    cases.append((ge, he, ge["encode"].shape[0]))
    for g_, hedge, rows in cases:
        z = _spg_from_golden(sp, g_)
        C, sizes = sp.hgather_counts(hedge, z, rows)
        oC, osz = _oracle_hcounts((g_["z_indptr"], g_["z_indices"], g_["z_data"]), hedge, rows)
        assert C.shape == (4 * hedge.shape[1], rows) and sizes.dtype == torch.int64
        assert np.array_equal(C.cpu().numpy(), oC) and np.array_equal(sizes.cpu().numpy(), osz)
        assert np.array_equal(C.sum(1).cpu().numpy(), 2 * osz)
    # a sampled store of a few thousand nodes
    ptr_, idx = sym_graph(5000, 30000, seed=3, hubs=1)
    zz, sets = sp.sample_spg(sp.DeviceCSR(ptr_, idx), np.arange(5000), num_walks=100, num_steps=3, seed=1, rng="philox")
    rows = sets.feature_table().shape[0]
    hedge = np.random.default_rng(0).integers(0, 5000, (3, 3000))
    hedge[:, 0], hedge[:, 1], hedge[:, 2] = (7, 7, 9), (7, 9, 7), (9, 9, 9)
    C, sizes = sp.hgather_counts(torch.from_numpy(hedge).cuda(), zz, rows)
    oC, osz = _oracle_hcounts((zz.indptr.cpu().numpy(), zz.indices.cpu().numpy(), zz.data.cpu().numpy()), hedge, rows)
    assert np.array_equal(C.cpu().numpy(), oC) and np.array_equal(sizes.cpu().numpy(), osz)
    assert np.array_equal(C.sum(1).cpu().numpy(), 2 * osz)


# ---------------------------------------------------------------------------------------------------------------- 6. hmean_stage
def _check_hmean(sp, hedge, z, table, xz, ind, B, H=16):
    """model_horder.py:56-57 restated -- x = pe_embedding(xz).sum(-2); scatter_mean(x, ind).view(4, -1, H), the segment mean by
    index_add_ -- against hmean_stage, forward and parameter gradients"""
    torch.manual_seed(1)
    k = table.shape[1]
    mlp_a = torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).cuda()
    mlp_b = torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).cuda()
    mlp_b.load_state_dict(mlp_a.state_dict())
    wgt = torch.randn(4, B, H, device="cuda")
    fused = sp.hmean_stage(hedge, z, table, mlp_a)
    assert fused.shape == (4, B, H) and fused.dtype == torch.float32
    (fused * wgt).sum().backward()
    x = mlp_b(xz).sum(dim=-2)
    cnt = torch.zeros(4 * B, device="cuda").index_add_(0, ind, torch.ones(ind.numel(), device="cuda"))
    ref = (torch.zeros(4 * B, H, device="cuda").index_add_(0, ind, x) / cnt.clamp(min=1)[:, None]).view(4, B, H)
    (ref * wgt).sum().backward()
    assert torch.allclose(fused, ref, rtol=1e-4, atol=1e-5)
    assert bool((fused.view(4 * B, H)[cnt == 0] == 0).all())                      # empty segments: zero rows
    for pa, pb in zip(mlp_a.parameters(), mlp_b.parameters()):
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-4 * float(pb.grad.abs().max()) + 1e-6


def test_hmean_stage_trains_like_the_reference_first_stage(sp):
    """forward and parameter gradients of the fused stage against model_horder.py:56-57 computed from the reference's own hgather output
    (tests/golden/hjoin_int.npz), and from hgather over a sampled store at the reference's batch of 2,048 triplets (main_horder.py:33)"""
    g = _load("hjoin_int.npz")
    z = _spg_from_golden(sp, g)
    table = torch.from_numpy(g["encode"]).cuda().float()
    _check_hmean(sp, g["hedge"], z, table, torch.from_numpy(g["xz"]).cuda(), torch.from_numpy(g["ind"]).cuda(), g["hedge"].shape[1])
    ptr_, idx = sym_graph(5000, 30000, seed=6, hubs=1)
    zz, sets = sp.sample_spg(sp.DeviceCSR(ptr_, idx), np.arange(5000), num_walks=64, num_steps=3, seed=2, rng="philox")
    table = sets.feature_table()
    hedge = torch.from_numpy(np.random.default_rng(4).integers(0, 5000, (3, 2048))).cuda()
    xz, ind = sp.hgather(hedge, zz, "cuda", encode=table)
    _check_hmean(sp, hedge, zz, table, xz, ind, 2048)


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_the_higher_order_calls_refuse_what_they_cannot_serve(sp, world):
    g = _load("hjoin_int.npz")
    z = _spg_from_golden(sp, g)
    table = torch.from_numpy(g["encode"]).cuda().float()
    rows, hedge = table.shape[0], g["hedge"]
    mlp = torch.nn.Linear(table.shape[1], 8).cuda()
    calls = (lambda h, x: sp.hgather_counts(h, x, rows), lambda h, x: sp.hmean_stage(h, x, table, mlp))
    zf = _spg_from_golden(sp, _load("sjoin_float.npz"))
    hf = np.zeros((3, 4), np.int64)
    enc0 = torch.cat([torch.zeros((1, 4), dtype=torch.int16, device="cuda"), torch.ones((rows - 1, 4), dtype=torch.int16, device="cuda")])
    for call in calls:
        with pytest.raises(TypeError):
            call(hf, zf)                                         # a float store
        with pytest.raises(TypeError):
            call(hedge, z.keyed(enc0, 100))                      # a keyed store
        with pytest.raises(ValueError):
            call(hedge, z.aligned())                             # headed rows
        for bad in (hedge[:2], hedge.reshape(-1), np.concatenate([hedge, hedge[:1]])):
            with pytest.raises(ValueError):
                call(bad, z)                                     # not [3, B]
        for bad_val in (z.n_rows, -1, 1 << 40):
            hb = hedge.copy()
            hb[2, 1] = bad_val
            with pytest.raises(IndexError):
                call(hb, z)                                      # a row outside the store
    with pytest.raises(IndexError):
        sp.hgather_counts(hedge, z, 3)                           # table too small
    C, _ = sp.hgather_counts(hedge, z, rows)                     # the device is fine afterwards
    assert float(C.sum()) > 0
    # the on-demand step
    csr, B = world.csr, 32
    h = world.triplets(64, 3)[:, :B].contiguous()
    kw = dict(num_walks=64, num_steps=3, seed=5)
    with pytest.raises(ValueError):
        sp.sample_and_hgather(csr, h, rng="rand_r", **kw)
    with pytest.raises(ValueError):
        sp.StepBuffers(csr, B, num_walks=64, num_steps=3, triplets=True, rng="rand_r")
    with pytest.raises(ValueError):
        sp.StepBuffers(csr, B, num_walks=64, num_steps=3, triplets=True, batch=B // 2)
    for bad in (h[:2], h.reshape(-1)):
        with pytest.raises(ValueError):
            sp.sample_and_hgather(csr, bad, **kw)
    hb = h.clone()
    hb[1, 3] = world.N
    with pytest.raises(IndexError):
        sp.sample_and_hgather(csr, hb, **kw)
    tb = sp.StepBuffers(csr, B, num_walks=64, num_steps=3, triplets=True)
    pb = sp.StepBuffers(csr, B, num_walks=64, num_steps=3)
    ib = sp.StepBuffers(csr, B, num_walks=64, num_steps=3, ptr=False)
    e = h[:2].contiguous()
    with pytest.raises(ValueError):
        sp.sample_and_hgather(csr, h, buffers=pb, **kw)                        # made for pairs
    with pytest.raises(ValueError):
        sp.sample_and_hgather(csr, h[:, : B // 2].contiguous(), buffers=tb, **kw)     # another B
    with pytest.raises(ValueError):
        sp.sample_and_hgather(csr, h, buffers=tb, num_walks=32, num_steps=3)   # another M
    with pytest.raises(ValueError):
        sp.sample_and_hgather(csr, h, buffers=tb, dedup_roots=True, **kw)      # made without dedup
    with pytest.raises(ValueError):
        sp.sample_and_gather(csr, e, buffers=tb, **kw)                         # made for triplets
    with pytest.raises(ValueError):
        sp.sample_and_gather(csr, e, buffers=pb, ptr=False, **kw)              # made for pointers
    with pytest.raises(ValueError):
        sp.sample_and_gather(csr, e, buffers=ib, **kw)                         # made for ids
    xz, ids, sets = sp.sample_and_hgather(csr, h, buffers=tb, **kw)            # and the buffers serve their own shape afterwards
    sets.prefetch().resolve()
    wxz, wids, _ = sp.sample_and_hgather(csr, h, **kw)
    R = int(sets.extra[0])
    assert R == wxz.shape[0] and torch.equal(xz[:R], wxz) and torch.equal(ids[:R], wids)

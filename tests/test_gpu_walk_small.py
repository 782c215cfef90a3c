"""GPU (MI355X): key rows for the small walk shapes (csrc/walk_small.hip: subgacc_walk_keyrows_small) and the on-demand model stages
over them.
  (a) the entry point driven through the C ABI into poisoned outputs between poisoned guards, bit for bit against rows built from
      the oracle's sets: ids ascending, keys packed from `enc` -- on the edge graph of tests/walk_rows_edges.py (root degrees 0, 1,
      M - 1, M, M + 1, 2M, self loops, a hub, repeated roots), both RNGs, int32 and int64 row offsets, two pitches, bad roots,
      n on either side of the four waves of a workgroup, work lists;
  (b) the same roots through the general kernel (sample_sets(fused_rows=True, strided=True, key_rows=False)): equal ids, and keys
      equal to the key column of the table of distinct rows at the member's slot;
  (c) the stages end to end against the row-form step (which runs the general kernel: the two producers are independent), with the
      comparisons and tolerances of tests/test_gpu_step_stage.py, test_gpu_step_attn.py and test_gpu_step_index.py."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_walk_rows_edges as R
import walk_rows_edges as W
from gpu_helpers import _oracle_spg, _reference_style_attn, sp, sym_graph  # noqa: F401
from test_gpu_counts_attn import FWD_TOL, GRAD_FLOOR, GRAD_TOL
from test_gpu_lstm_aggr import _nets as _lstm_nets, _reference_style_lstm
from test_gpu_step_stage import _dicts, _reference_stage
from walk_rows_edges import NO_ROOT, POISON

pytestmark = pytest.mark.gpu

SEED = 13
RNGS = ("rand_r", "philox")
# (M, m): Q = 51 fills a 64-slot table to 80 %; 52 and 102 are the ends of the 128-slot table, 103 the first of the 256-slot one;
# Q = 201 .. 204 fill the 256-slot table to 80 % at every hop count
SHAPES = ((50, 1), (51, 1), (101, 1), (50, 2), (51, 2), (34, 3), (100, 2), (101, 2), (67, 3), (50, 4), (203, 1))
STEP_SHAPES = ((100, 2), (50, 1), (101, 2), (50, 4))


# --------------------------------------------------------------------------------------------------------------------- plumbing
def _graph(M, m):
    """the edge graph of the shape; a one-hop shape walks the two-hop graph of its M (the trees need two hops to be built, and a walk
    of one hop never stands on their leaves with a hop left)"""
    return W.edge_graph(M, max(m, 2))


@functools.lru_cache(maxsize=4)
def _csrs(M, m):
    from surel_plus_amd.sampler import DeviceCSR
    g = _graph(M, m)
    return {False: DeviceCSR(g["indptr"], g["indices"]), True: DeviceCSR(g["indptr"].astype(np.int64), g["indices"])}


@functools.lru_cache(maxsize=None)
def _expected(M, m, rng):
    """THE reference, once per (shape, rng): the oracle's sets of the graph's batch as finished rows (walk_rows_edges.expected_rows
    for a graph that may have been built for another hop count)"""
    import oracle
    g = _graph(M, m)
    nsize, remap, enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng)
    off = np.concatenate([[0], np.cumsum(nsize)]).astype(np.int64)
    order = np.lexsort((remap[0], np.repeat(np.arange(len(nsize)), nsize)))
    ukeys = W.lp_keys(enc, M, m)
    assert len(np.unique(ukeys)) == len(ukeys) and int(ukeys.max()) < 1 << 25
    out = dict(nsize=nsize, off=off, ids=remap[0][order], keys=ukeys[remap[1][order]])
    for v in out.values():
        v.setflags(write=False)
    return out


def _rows_of(exp, rows):
    """the expected rows of another batch: row j of the result is row rows[j] of `exp` (Philox: a set is a function of its root)"""
    rows = np.asarray(rows, dtype=np.int64)
    lens = exp["nsize"][rows].astype(np.int64)
    src = np.repeat(exp["off"][rows], lens) + np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    return dict(nsize=exp["nsize"][rows], off=np.concatenate([[0], np.cumsum(lens)]), ids=exp["ids"][src], keys=exp["keys"][src])


def _launch(csr, q, M, m, rng, pitch=0, work=None, n_work=None, cap_root=True):
    """one call of subgacc_walk_keyrows_small into poisoned, guarded outputs -> what test_gpu_walk_rows_edges._check reads"""
    from surel_plus_amd import _lib as L, sampler
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n, Q = len(q), M * m + 1
    P = pitch if pitch > 0 else Q
    d_q = R._dev(np.asarray(q, dtype=np.int32))
    cfg = sampler.make_cfg(csr, M, m, -1, SEED, rng, cap_root_degree=cap_root, records=False, row_pitch=pitch)
    rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st)
    w_ids, ids = R._guarded(n * P, torch.int32)
    w_pay, pay = R._guarded(n * P, torch.int32)
    w_ns, nsize = R._guarded(n, torch.int32)
    w_fl, flags = R._guarded(4, torch.int32, np.zeros(4, np.int32))
    d_wl = R._dev(np.asarray(work, dtype=np.int32)) if work is not None else None
    d_nw = R._dev(np.array([n_work], dtype=np.int64)) if work is not None else None
    L.check(lib.subgacc_walk_keyrows_small(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, ptr(rp), ptr(rs),
                                           ptr(d_wl), ptr(d_nw), ptr(ids), ptr(pay), ptr(nsize), ptr(flags), st))
    torch.cuda.synchronize()
    return dict(P=P, n=n, form="keys32", ids=R._back(w_ids, n * P).reshape(n, P), pay=R._back(w_pay, n * P).reshape(n, P),
                nsize=R._back(w_ns, n), flags=R._back(w_fl, 4))


# ------------------------------------------------------------------------------------------------- (a) the entry point, directly
@pytest.mark.parametrize("M,m", SHAPES)
def test_rows_equal_the_oracle_at_every_shape(sp, M, m):
    """both RNGs, int32 and int64 row offsets, pitch Q and Q rounded up to 32; the tail of every row and the words between a row's
    capacity and the pitch keep their poison"""
    g, csrs, Q = _graph(M, m), _csrs(M, m), M * m + 1
    degs = W.out_degree(g, g["batch"])
    assert {0, 1, M - 1, M, M + 1, 2 * M} <= set(degs.tolist()) and len(np.unique(g["batch"])) < len(g["batch"])
    for rng in RNGS:
        exp = _expected(M, m, rng)
        assert int(exp["nsize"].max()) <= Q and int(exp["nsize"].min()) == 1
        for idx64 in (False, True):
            for pitch in (0, (Q + 31) // 32 * 32):
                R._check(_launch(csrs[idx64], g["batch"], M, m, rng, pitch), exp, what=(rng, idx64, pitch))
    print(f"M = {M}, m = {m}: Q = {Q}, {W.table_size_for(Q)} slots, rows = {len(g['batch'])}, largest set = {int(exp['nsize'].max())}")


@pytest.mark.parametrize("M,m", [(50, 1), (100, 2), (50, 4)])
def test_rows_without_a_root_and_roots_outside_the_graph(sp, M, m):
    """SUBGACC_NO_ROOT: nsize 0 and nothing else; a root outside [0, num_nodes): nsize 0 and flags[3] |= 16; the rows between them
    are sampled as ever"""
    g, csr = _graph(M, m), _csrs(M, m)[False]
    q = g["batch"].copy()
    n, N = len(q), g["num_nodes"]
    none, bad = [1, 4, n - 1], {0: N, 7: -1, 9: 2 ** 31 - 1, n - 2: N + 5}
    q[none] = NO_ROOT
    for i, v in bad.items():
        q[i] = v
    keep = np.setdiff1d(np.arange(n), none + list(bad))
    exp = _expected(M, m, "philox")
    R._check(_launch(csr, q, M, m, "philox"), exp, listed=keep, empty=none + list(bad), flags=(0, 0, 0, 16))
    q2 = g["batch"].copy()
    q2[none] = NO_ROOT
    R._check(_launch(csr, q2, M, m, "philox", 224 if M * m + 1 <= 224 else 0), exp, listed=np.setdiff1d(np.arange(n), none), empty=none)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_batches_on_either_side_of_a_workgroup(sp, n):
    """four roots to a workgroup: n = 1, 3, 4, 5 and 257 roots"""
    for M, m in ((50, 1), (100, 2)):
        g, csr = _graph(M, m), _csrs(M, m)[True]
        rows = np.resize(np.arange(len(g["batch"])), n)
        R._check(_launch(csr, g["batch"][rows], M, m, "philox", 0), _rows_of(_expected(M, m, "philox"), rows), what=(M, m, n))


@pytest.mark.parametrize("M,m", [(50, 1), (100, 2), (67, 3)])
def test_work_lists(sp, M, m):
    """a list naming every second row, *n_work = 0, a list in descending order, a list longer than *n_work: the listed rows equal
    the oracle's (rand_r: at their places in the whole batch's stream), every other row keeps its poison"""
    g, csrs = _graph(M, m), _csrs(M, m)
    q = g["batch"]
    n = len(q)
    lists = [("every second", np.arange(0, n, 2), (n + 1) // 2), ("none", np.arange(n), 0), ("descending", np.arange(n)[::-1], n),
             ("a prefix", np.arange(n)[::-1], 5), ("longer than n", np.arange(n), n + 9)]
    for rng in RNGS:
        exp = _expected(M, m, rng)
        for name, wl, nw in lists:
            got = _launch(csrs[rng == "rand_r"], q, M, m, rng, 0, work=wl, n_work=nw)
            R._check(got, exp, listed=wl[: min(nw, n)], what=(rng, name))


# ------------------------------------------------------------------------------------------------- (b) against the general kernel
@pytest.mark.parametrize("M,m", [(50, 1), (51, 2), (100, 2), (67, 3), (50, 4), (203, 1)])
def test_rows_equal_the_general_kernels(sp, M, m):
    from surel_plus_amd import sampler
    g, csr, Q = _graph(M, m), _csrs(M, m)[False], M * m + 1
    assert sampler.walk_kernel_name(csr, M, m, True) == "walk_sets_kernel<SPG>"
    for rng in RNGS:
        sets = sampler.sample_sets(csr, g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng, fused_rows=True, strided=True,
                                   key_rows=False)
        assert sets.strided and not sets.keyrows and sets.stride == Q
        got = _launch(csr, g["batch"], M, m, rng, 0)
        ns = sets.nsize.cpu().numpy()
        assert np.array_equal(got["nsize"], ns)
        member = np.arange(Q)[None, :] < ns[:, None]
        ids, slot = sets.ids.cpu().numpy().reshape(-1, Q), sets.slot.cpu().numpy().reshape(-1, Q)
        tkeys = sets.table[: sets.capacity * 8].view(torch.int64).cpu().numpy()
        assert np.array_equal(got["ids"][member], ids[member])
        assert np.array_equal(got["pay"][member].astype(np.int64), tkeys[slot[member]])
        assert (got["ids"][~member] == POISON).all() and (got["pay"][~member] == POISON).all()


# --------------------------------------------------------------------------------------------------------- (c) the stages, end to end
B, BT, H = 40, 24, 16


class Small:
    """600 nodes, one hub; 40 pairs with a (u, u) pair, a repeated pair and a repeated endpoint; 24 triplets with u == v and u == w"""

    def __init__(self, sp):
        self.ptr, self.idx = sym_graph(600, 2400, seed=3, hubs=1)
        self.csr = sp.DeviceCSR(self.ptr, self.idx)
        e = np.random.default_rng(4).integers(0, 600, (2, B))
        e[:, 0] = (7, 7)
        e[:, 1] = e[:, 2]
        e[0, 3] = e[0, 4]
        h = np.random.default_rng(5).integers(0, 600, (3, BT))
        h[1, 0], h[2, 1], h[:, 2] = h[0, 0], h[0, 1], 11
        self.e_host, self.e, self.h = e, torch.from_numpy(e).cuda(), torch.from_numpy(h).cuda()


@pytest.fixture(scope="module")
def small(sp):
    return Small(sp)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _xz_dicts(xz, ind):
    """per segment {feature row as bytes: how often it stands in either slot of the segment's rows of xz}"""
    x, p = np.ascontiguousarray(xz.cpu().numpy()), ind.cpu().numpy()
    out = []
    for j in range(len(p) - 1):
        d = {}
        for r in range(p[j], p[j + 1]):
            for s in (0, 1):
                k = x[r, s].tobytes()
                d[k] = d.get(k, 0.0) + 1.0
        out.append(d)
    return out


@pytest.mark.parametrize("M,m", STEP_SHAPES)
def test_index_and_counts_equal_the_row_form_step(sp, small, M, m):
    """table[pairs] is the xz of sample_and_gather over the same seed bit for bit and indptr its indptr; the counts are the counts
    rebuilt from that xz; the same bits with dedup_roots, with order=, and with and without buffers="""
    csr, e = small.csr, small.e
    kw = dict(num_walks=M, num_steps=m, seed=5)
    xz, ind, _ = sp.sample_and_gather(csr, e, **kw)
    pairs, indptr, table, sets = sp.sample_and_index(csr, e, **kw)
    Rr = int(ind[-1])
    assert sets.keyrows and sets.small_rows and not sets.key64
    assert pairs.dtype == torch.int32 and pairs.shape == (Rr, 2) and table.shape[1] == m + 1 and torch.equal(indptr, ind)
    assert int(pairs[:, 0].min()) >= 1 and int(pairs.max()) == table.shape[0] - 1 and not bool(table[0].any())
    assert torch.equal(_bits(table[pairs.long()]), _bits(xz))
    Cm, sizes, tab, _ = sp.sample_and_counts(csr, e, **kw)
    assert torch.equal(_bits(tab), _bits(table)) and torch.equal(sizes.to(torch.int64), ind[1:] - ind[:-1])
    assert _dicts(Cm, tab) == _xz_dicts(xz, ind)
    T = table.shape[0] + 40
    want_i = sp.sample_and_index(csr, e, table_rows=T, **kw)
    want_c = sp.sample_and_counts(csr, e, table_rows=T, **kw)
    assert torch.equal(want_i[0], pairs) and torch.equal(want_c[0][:, : table.shape[0]], Cm) and not bool(want_c[0][:, table.shape[0]:].any())
    order = sp.locality_order(csr)
    for route in (dict(dedup_roots=True), dict(order=order), dict(dedup_roots=True, order=order)):
        gi, gc = sp.sample_and_index(csr, e, table_rows=T, **route, **kw), sp.sample_and_counts(csr, e, table_rows=T, **route, **kw)
        assert torch.equal(gi[0], pairs) and torch.equal(gi[1], ind) and torch.equal(_bits(gi[2]), _bits(want_i[2])), route
        assert all(torch.equal(x, y) for x, y in zip(gc[:3], want_c[:3])), route
    for dedup, ordr in ((False, None), (True, None), (False, order), (True, order)):
        bi = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, dedup_roots=dedup, order=ordr, stage="index", table_rows=T)
        bc = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, dedup_roots=dedup, order=ordr, stage="counts", table_rows=T)
        assert bi.small and bi.keyrows and not bi.key64 and bi.table is None and bi.slot.dtype == torch.int32
        for _ in range(2):                                  # and the buffers used again
            gi = sp.sample_and_index(csr, e, buffers=bi, dedup_roots=dedup, order=ordr, **kw)
            gc = sp.sample_and_counts(csr, e, buffers=bc, dedup_roots=dedup, order=ordr, **kw)
            gi[3].resolve(), gc[3].resolve()
            assert torch.equal(gi[0][:Rr], pairs) and torch.equal(gi[1], ind) and torch.equal(_bits(gi[2]), _bits(want_i[2]))
            assert all(torch.equal(x, y) for x, y in zip(gc[:3], want_c[:3]))
        assert bi.walk_order == ("rank" if ordr is not None else "batch")


@pytest.mark.parametrize("M,m", STEP_SHAPES)
def test_mean_stage_trains_like_the_reference_first_stage(sp, small, M, m):
    """test_gpu_step_stage.py::test_stage_trains_like_the_reference_first_stage at a small shape: forward rtol 1e-4, atol 1e-5; every
    parameter gradient within 1e-4 of its largest entry"""
    csr, e = small.csr, small.e
    kw = dict(num_walks=M, num_steps=m, seed=5)
    torch.manual_seed(1)
    mlp_a = torch.nn.Sequential(torch.nn.Linear(m + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b = torch.nn.Sequential(torch.nn.Linear(m + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b.load_state_dict(mlp_a.state_dict())
    fused = sp.sample_and_mean_stage(csr, e, mlp_a, **kw)
    xz, seg, _ = sp.sample_and_gather(csr, e, **kw)
    assert fused.shape == (2, B, H)
    w = torch.randn(2, B, H, device="cuda")
    (fused * w).sum().backward()
    ref = _reference_stage(mlp_b, xz, seg, 2 * B, H, 2)
    (ref * w).sum().backward()
    assert torch.allclose(fused, ref, rtol=1e-4, atol=1e-5)
    for pa, pb in zip(mlp_a.parameters(), mlp_b.parameters()):
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-4 * float(pb.grad.abs().max()) + 1e-6


def test_hmean_stage_on_triplets(sp, small):
    """sample_and_hmean_stage on [3, B] triplets at HONet's own configuration (M = 100, 2 hops) against pe_embedding(xz).sum(-2) +
    scatter_mean on the (xz, ids) of sample_and_hgather; with and without root dedup and buffers the same bits"""
    csr, h, M, m = small.csr, small.h, 100, 2
    kw = dict(num_walks=M, num_steps=m, seed=5)
    torch.manual_seed(1)
    mlp_a = torch.nn.Sequential(torch.nn.Linear(m + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b = torch.nn.Sequential(torch.nn.Linear(m + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b.load_state_dict(mlp_a.state_dict())
    fused = sp.sample_and_hmean_stage(csr, h, mlp_a, **kw)
    xz, ids, _ = sp.sample_and_hgather(csr, h, **kw)
    assert fused.shape == (4, BT, H)
    w = torch.randn(4, BT, H, device="cuda")
    (fused * w).sum().backward()
    ref = _reference_stage(mlp_b, xz, ids.seg_pointers, 4 * BT, H, 4)
    (ref * w).sum().backward()
    assert torch.allclose(fused, ref, rtol=1e-4, atol=1e-5)
    for pa, pb in zip(mlp_a.parameters(), mlp_b.parameters()):
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-4 * float(pb.grad.abs().max()) + 1e-6
    T = 512
    with torch.no_grad():
        want = sp.sample_and_hmean_stage(csr, h, mlp_a, table_rows=T, **kw)
        assert torch.equal(sp.sample_and_hmean_stage(csr, h, mlp_a, table_rows=T, dedup_roots=True, **kw), want)
        bufs = sp.StepBuffers(csr, BT, num_walks=M, num_steps=m, triplets=True, dedup_roots=True, stage="counts", table_rows=T)
        for _ in range(2):
            assert torch.equal(sp.sample_and_hmean_stage(csr, h, mlp_a, buffers=bufs, dedup_roots=True, **kw), want)
            bufs.sets.resolve()


def _attn_nets(k, dtype=torch.float32):
    torch.manual_seed(7)
    mods = [torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.Linear(H, 1), torch.nn.Linear(H, H)]
    return [mod.to("cuda", dtype) for mod in mods]


def _params(nets):
    return [(n, p) for mod in nets for n, p in mod.named_parameters()]


def _attn_ref(sp, csr, e, nets, kw):
    xz, ind, _ = sp.sample_and_gather(csr, e, **kw)
    if nets[0][0].weight.dtype == torch.float64:
        xz = xz.double()
    return _reference_style_attn(xz, ind, *nets).view(2, e.shape[1], -1)


@pytest.mark.parametrize("M,m", STEP_SHAPES)
def test_attn_stage_trains_like_the_reference_first_stage(sp, small, M, m):
    """test_gpu_step_attn.py::test_trains_like_the_reference_first_stage at a small shape, with its criteria: forward within FWD_TOL of
    the float64 reference's largest entry; every gradient within GRAD_TOL, and within 4x the float32 reference's own error (floor
    GRAD_FLOOR); the gate bias exactly zero"""
    csr, e = small.csr, small.e
    kw = dict(num_walks=M, num_steps=m, seed=5)
    fa, fb, f64 = _attn_nets(m + 1), _attn_nets(m + 1), _attn_nets(m + 1, torch.float64)
    w = (torch.randn((2, B, H), generator=torch.Generator().manual_seed(1))).cuda()
    fused = sp.sample_and_attn_stage(csr, e, *fa, **kw)
    assert fused.shape == (2, B, H) and fused.dtype == torch.float32
    (fused * w).sum().backward()
    ref32 = _attn_ref(sp, csr, e, fb, kw)
    (ref32 * w).sum().backward()
    truth = _attn_ref(sp, csr, e, f64, kw)
    (truth * w.double()).sum().backward()
    scale = float(truth.detach().abs().max())
    err = float((fused.detach().double() - truth.detach()).abs().max())
    print("forward", err / scale)
    assert err <= FWD_TOL * scale
    for (n, pa), (_, pb), (_, pc) in zip(_params(fa), _params(fb), _params(f64)):
        if pa is fa[1].bias:
            assert float(pa.grad.abs().max()) == 0.0
            continue
        gs = float(pc.grad.abs().max())
        err_fused = float((pa.grad.double() - pc.grad).abs().max()) / gs
        err_ref32 = float((pb.grad.double() - pc.grad).abs().max()) / gs
        print(n, err_fused, err_ref32)
        assert err_fused <= GRAD_TOL, (n, err_fused)
        assert err_fused <= max(4 * err_ref32, GRAD_FLOOR), (n, err_fused, err_ref32)


@pytest.mark.parametrize("M,m", STEP_SHAPES)
def test_lstm_stage_trains_like_the_float64_reference_form(sp, small, M, m):
    """test_gpu_step_index.py::test_stage_trains_like_the_float64_reference_form at a small shape: forward within 2e-5 of the
    reference's largest entry, every parameter gradient within 5e-4 of that gradient's largest entry; the same bits through buffers
    with root dedup"""
    csr, e, H2 = small.csr, small.e, 16
    kw = dict(num_walks=M, num_steps=m, seed=5)
    fa, f64 = _lstm_nets(torch.float32, H, H2, True, m + 1), _lstm_nets(torch.float64, H, H2, True, m + 1)
    fused = sp.sample_and_lstm_stage(csr, e, *fa, **kw)
    assert fused.shape == (2, B, H2) and fused.dtype == torch.float32
    xz, ind, _ = sp.sample_and_gather(csr, e, **kw)
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
    T = 512
    with torch.no_grad():
        want = sp.sample_and_lstm_stage(csr, e, *fa, table_rows=T, **kw)
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, dedup_roots=True, stage="index", table_rows=T)
        assert torch.equal(sp.sample_and_lstm_stage(csr, e, *fa, buffers=bufs, dedup_roots=True, **kw), want)


@pytest.mark.parametrize("M,m", [(100, 2), (50, 1)])
def test_numbering_and_packed_rows_of_a_step(sp, small, M, m):
    """sets.number() / enc_int16() / to_csr() of a stage's step: such a batch is sampled again by the general kernel with the table
    form -- the oracle's numbering and its SpG, with and without root dedup (a repeated endpoint's row is then empty)"""
    from surel_plus_amd.spg import StridedSpG
    csr, e = small.csr, small.e
    roots = small.e_host.reshape(-1)
    (o_ptr, o_idx, o_data), o_enc = _oracle_spg(small.ptr, small.idx, roots, M, m, 5, "philox")
    sets = sp.sample_and_counts(csr, e, num_walks=M, num_steps=m, seed=5)[3]
    assert sets.small_rows and sets.ukeys is None
    assert np.array_equal(sets.enc_int16().cpu().numpy(), o_enc)
    assert sets.c == len(o_enc) and np.array_equal(sets.ukeys.cpu().numpy().view(np.uint64), W.lp_keys(o_enc, M, m))
    z = StridedSpG(sets, csr.num_nodes).to_csr()
    assert np.array_equal(z.indptr.cpu().numpy(), o_ptr) and np.array_equal(z.indices.cpu().numpy(), o_idx)
    assert np.array_equal(z.data.cpu().numpy(), o_data)
    dd = sp.sample_and_counts(csr, e, num_walks=M, num_steps=m, seed=5, dedup_roots=True)[3]
    assert np.array_equal(dd.enc_int16().cpu().numpy(), o_enc)
    first = np.array([i == roots.tolist().index(r) for i, r in enumerate(roots.tolist())])
    zd = StridedSpG(dd, csr.num_nodes).to_csr()
    lens = np.where(first, np.diff(o_ptr), 0)
    assert np.array_equal(np.diff(zd.indptr.cpu().numpy()), lens)
    keep = np.repeat(first, np.diff(o_ptr))
    assert np.array_equal(zd.indices.cpu().numpy(), o_idx[keep]) and np.array_equal(zd.data.cpu().numpy(), o_data[keep])

"""GPU (MI355X): gather_star -- one source against K targets (the MRR evaluation of train.py:246-280 over utils.py:93-95's
neg_edge = stack([source.repeat_interleave(K), target_neg.view(-1)])) -- is bit for bit gather() over the expanded pairs and the
oracle's join of those pairs, on every store it accepts, and the star kernel itself ran (the join's flags[1] & 1).  gather_star's
default route -- the expanded list through the pair kernels -- answers the same."""
import numpy as np
import pytest
import torch

import oracle
import surel_plus_amd as spm
from gpu_helpers import _load, _spg_from_golden, sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu

STAR_RAN, FALLBACK_RAN = 1, 2       # flags[1] bits of a star join (include/subgacc.h, SUBGACC_JOIN_OPT_STAR)


def gather_star(*args, **kw):
    """the star kernel itself (gather_star's default joins the expanded list with the pair kernels)"""
    return spm.gather_star(*args, kernel="star", **kw)


def _expanded(source, targets):
    source, targets = np.asarray(source, np.int64), np.asarray(targets, np.int64)
    return np.stack([np.repeat(source, targets.shape[1]), targets.reshape(-1)])


def _star_flags(ind):
    return int(ind.join_flags[1].item())


def _check_star(x, source, targets, encode, ptr, oracle_store=None, oracle_encode=None, want_fallback=False):
    """gather_star == gather over the expanded pairs (and == the oracle's join of them when a store is given); the star kernel ran"""
    e = _expanded(source, targets)
    xz, ind = gather_star(source, targets, x, "cuda", ptr=ptr, encode=encode)
    wxz, wind = spm.gather(e, x, "cuda", ptr=ptr, encode=encode)
    assert xz.dtype == wxz.dtype == torch.float32 and ind.dtype == wind.dtype == torch.int64
    assert xz.device == wxz.device and ind.device == wind.device
    assert xz.shape == wxz.shape and torch.equal(xz, wxz) and torch.equal(ind, wind)
    f = _star_flags(ind)
    assert f & STAR_RAN
    assert bool(f & FALLBACK_RAN) == want_fallback
    if oracle_store is not None:
        seg, pairs = oracle.sjoin(*oracle_store, *oracle.pair_segments(e))
        if pairs.dtype == np.float32:
            oxz = pairs[:, :, None]
        else:
            oxz = oracle_encode[pairs]
        assert np.array_equal(xz.cpu().numpy(), oxz)
        if ptr:
            assert np.array_equal(ind.cpu().numpy(), seg)
        else:
            assert np.array_equal(ind.cpu().numpy(), np.repeat(np.arange(len(seg) - 1), np.diff(seg)))
    return xz, ind


def _queries(n_rows, P, K, seed):
    """P sources, K targets each: uniform rows, with a target equal to its source and a repeated target in every run"""
    rng = np.random.default_rng(seed)
    source = rng.integers(0, n_rows, P)
    targets = rng.integers(0, n_rows, (P, K))
    if K >= 2:
        targets[:, 0] = source
        targets[:, K - 1] = targets[:, K // 2]
    return source, targets


@pytest.mark.parametrize("name", ["sjoin_int.npz", "sjoin_int_emptyrows.npz", "sjoin_float.npz"])
@pytest.mark.parametrize("layout", ["packed", "headed"])
@pytest.mark.parametrize("ptr", [True, False])
@pytest.mark.parametrize("K", [1, 2, 7, 64, 1000])
def test_star_matches_gather_and_oracle_on_goldens(sp, name, layout, ptr, K):
    g = _load(name)
    z = _spg_from_golden(sp, g)
    x = z.aligned() if layout == "headed" else z
    enc = torch.from_numpy(g["encode"]).cuda() if g["encode"].size else None
    P = 64 if K <= 64 else 24
    source, targets = _queries(z.n_rows, P, K, seed=K)
    _check_star(x, source, targets, enc, ptr, (g["z_indptr"], g["z_indices"], g["z_data"]), g["encode"])
    # torch arguments on the device (as the reference's loop has them) give the same answer
    xz, ind = gather_star(torch.from_numpy(source).cuda(), torch.from_numpy(targets).cuda().int(), x, "cuda", ptr=ptr, encode=enc)
    wxz, wind = sp.gather(_expanded(source, targets), x, "cuda", ptr=ptr, encode=enc)
    assert torch.equal(xz, wxz) and torch.equal(ind, wind)


@pytest.fixture(scope="module")
def lp_store(sp):
    """a store sampled at M = 200, 3 hops (rows of up to 601 members) over a graph with hubs: SFptr + table, keyed, both headed"""
    ptr_, idx = sym_graph(4000, 30000, seed=17, hubs=3)
    csr = sp.DeviceCSR(ptr_, idx)
    M = 200
    z, sets = sp.sample_spg(csr, np.arange(4000), num_walks=M, num_steps=3, seed=3, rng="philox")
    table = sets.feature_table()
    enc = oracle.enc_table(sets.enc_int16().cpu().numpy())
    zk = z.keyed(enc, M)
    return z, table, zk, enc.astype(np.float32) / np.float32(M)


@pytest.mark.parametrize("store", ["table", "keyed", "table-headed", "keyed-headed"])
@pytest.mark.parametrize("ptr", [True, False])
@pytest.mark.parametrize("K", [1, 7, 1000])
def test_star_on_sampled_lp_store(sp, lp_store, store, ptr, K):
    z, table, zk, oenc = lp_store
    assert z.max_len > 300            # long rows: several 64-row spans of the source per target
    x = zk if store.startswith("keyed") else z
    if store.endswith("headed"):
        x = x.aligned()
    enc = x.slot_table() if store.startswith("keyed") else table
    P = 256 if K <= 7 else 16
    source, targets = _queries(z.n_rows, P, K, seed=100 + K)
    source[:3] = [0, 1, 2]          # the hubs' rows
    _check_star(x, source, targets, enc, ptr, tuple(t.cpu().numpy() for t in (z.indptr, z.indices, z.data)), oenc)


def _with_hub(z, hub_len, seed, float_payload):
    """z's rows plus one more, `hub_len` members long -- past the star kernel's LDS staging bound"""
    rng = np.random.default_rng(seed)
    indptr, indices, data = (t.cpu().numpy() for t in (z.indptr, z.indices, z.data))
    hub_ids = np.sort(rng.choice(3 * hub_len, hub_len, replace=False)).astype(np.int32)
    if float_payload:
        data = rng.random(len(indices))
        hub_data = rng.random(hub_len)
    else:
        hub_data = data[rng.integers(0, len(data), hub_len)]
    indptr = np.concatenate([indptr, [indptr[-1] + hub_len]]).astype(np.int64)
    indices = np.concatenate([indices, hub_ids]).astype(np.int32)
    data = np.concatenate([data, hub_data])
    return spm.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(), torch.from_numpy(data).cuda()), (indptr, indices, data)


@pytest.mark.parametrize("payload", ["int", "float"])
@pytest.mark.parametrize("ptr", [True, False])
def test_hub_source_past_the_staging_bound_takes_the_fallback(sp, lp_store, payload, ptr):
    """a source longer than the star kernel stages (~13k members with a table, ~8k float members) is joined by the one-segment-per-wave
    kernel on the same list: the other sources still take the star kernel, and the result is gather()'s, bit for bit"""
    z, table, _, oenc = lp_store
    zh, host = _with_hub(z, 16000, seed=9, float_payload=payload == "float")
    hub = zh.n_rows - 1
    enc = table if payload == "int" else None
    source, targets = _queries(zh.n_rows, 12, 64, seed=4)
    source[3] = source[7] = hub
    targets[5, :4] = hub
    _check_star(zh, source, targets, enc, ptr, host, oenc, want_fallback=True)
    # without the hub among the sources nothing takes the fallback
    _check_star(zh, source[:3], targets[:3], enc, ptr, want_fallback=False)


def test_star_edge_cases(sp):
    g = _load("sjoin_int_emptyrows.npz")
    z = _spg_from_golden(sp, g)
    enc = torch.from_numpy(g["encode"]).cuda()
    lens = np.diff(g["z_indptr"])
    empty = np.flatnonzero(lens == 0)
    assert len(empty) >= 2
    full = np.flatnonzero(lens > 0)
    for x in (z, z.aligned()):
        for source, targets in ((np.zeros(0, np.int64), np.zeros((0, 5), np.int64)),         # P = 0
                                (np.arange(4), np.zeros((4, 0), np.int64))):                 # K = 0
            xz, ind = gather_star(source, targets, x, "cuda", encode=enc)
            wxz, wind = sp.gather(_expanded(source, targets), x, "cuda", encode=enc)
            assert xz.shape == wxz.shape and torch.equal(ind, wind) and ind.dtype == torch.int64
        # empty source rows, empty target rows, a target equal to its source, repeated targets, a run of one target repeated
        source = np.array([empty[0], full[0], full[1], empty[1], full[2]])
        targets = np.array([[full[0], empty[0], full[3], full[3], empty[1]],
                            [full[0], full[0], empty[0], full[1], full[0]],
                            [empty[0], empty[1], empty[0], empty[1], empty[0]],
                            [empty[1], empty[1], full[4], empty[0], full[5]],
                            [full[6], full[6], full[6], full[6], full[6]]])
        for ptr in (True, False):
            _check_star(x, source, targets, enc, ptr, (g["z_indptr"], g["z_indices"], g["z_data"]), g["encode"])


def test_star_out_reuse_and_lazy(sp):
    g = _load("sjoin_int.npz")
    z = _spg_from_golden(sp, g)
    enc = torch.from_numpy(g["encode"]).cuda()
    for x in (z, z.aligned()):
        worst = 2 * 40 * 30 * int(z.max_len)
        buf = torch.empty(worst * 2 * 3 + 64, dtype=torch.float32, device="cuda")
        for seed in (1, 2):                       # the same buffer serves two calls
            source, targets = _queries(z.n_rows, 40, 30, seed)
            wxz, wind = sp.gather(_expanded(source, targets), x, "cuda", encode=enc)
            xz, ind = gather_star(source, targets, x, "cuda", encode=enc, out=buf)
            assert xz.data_ptr() == buf.data_ptr() and torch.equal(xz, wxz) and torch.equal(ind, wind)
            lxz, lind = gather_star(source, targets, x, "cuda", encode=enc, out=buf, lazy=True)
            sp.spjoin.lazy_join_status(lind)
            R = int(lind[-1].item())
            assert torch.equal(lind, wind) and torch.equal(lxz[:R], wxz) and lxz.data_ptr() == buf.data_ptr()
        with pytest.raises(ValueError, match="out="):
            gather_star(source, targets, x, "cuda", encode=enc, out=buf[:10])
    # the float store: lazily without a table
    gf = _load("sjoin_float.npz")
    zf = _spg_from_golden(sp, gf)
    source, targets = _queries(zf.n_rows, 16, 64, 3)
    buf = torch.empty(2 * 16 * 64 * int(zf.max_len) * 2, dtype=torch.float32, device="cuda")
    lxz, lind = gather_star(source, targets, zf, "cuda", out=buf, lazy=True)
    wxz, wind = sp.gather(_expanded(source, targets), zf, "cuda")
    assert torch.equal(lind, wind) and torch.equal(lxz[: int(lind[-1].item())], wxz)


def test_star_rows_out_of_range(sp):
    """a row number outside the store: gather's IndexError (eager), lazy_join_status's (lazy); such a row reads as empty"""
    g = _load("sjoin_int.npz")
    z = _spg_from_golden(sp, g)
    enc = torch.from_numpy(g["encode"]).cuda()
    source, targets = _queries(z.n_rows, 8, 16, 5)
    for x in (z, z.aligned()):
        for s, t in ((np.where(np.arange(8) == 3, z.n_rows, source), targets),
                     (source, np.where(np.arange(16) == 9, -1, targets))):
            with pytest.raises(IndexError) as want:
                sp.gather(_expanded(s, t), x, "cuda", encode=enc)
            with pytest.raises(IndexError) as got:
                gather_star(s, t, x, "cuda", encode=enc)
            assert str(got.value) == str(want.value)
            buf = torch.empty(2 * 8 * 16 * int(z.max_len) * 6, dtype=torch.float32, device="cuda")
            _, lind = gather_star(s, t, x, "cuda", encode=enc, out=buf, lazy=True)
            with pytest.raises(IndexError):
                sp.spjoin.lazy_join_status(lind)


@pytest.mark.parametrize("name", ["sjoin_int.npz", "sjoin_float.npz"])
def test_default_route_is_the_pair_kernels_with_the_same_result(sp, name):
    g = _load(name)
    z = _spg_from_golden(sp, g)
    enc = torch.from_numpy(g["encode"]).cuda() if g["encode"].size else None
    source, targets = _queries(z.n_rows, 32, 100, 8)
    for x in (z, z.aligned()):
        for ptr in (True, False):
            sxz, sind = gather_star(source, targets, x, "cuda", ptr=ptr, encode=enc)
            dxz, dind = sp.gather_star(source, targets, x, "cuda", ptr=ptr, encode=enc)
            assert torch.equal(sxz, dxz) and torch.equal(sind, dind)
            assert _star_flags(sind) & STAR_RAN and getattr(dind, "join_flags", None) is None
    with pytest.raises(ValueError, match="kernel"):
        sp.gather_star(source, targets, z, "cuda", encode=enc, kernel="fast")

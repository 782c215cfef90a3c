"""GPU (MI355X): csrc/ppr.hip and csrc/encode.hip at the places their own tests never aimed at (inputs: tests/ppr_edges.py, shown to be
what they claim by tests/test_ppr_edges_cpu.py).

The push: many claimants of one free slot in one trip and chains that wrap past the last slot; root degrees on both sides of the
64-lane, 256-neighbour and 512-neighbour edges of a trip; both sides of the refusal bound; one wave that runs refused and accepted
roots in turn and must hand its slab back clean; the radix select of the top-K with its cut among equal scores, among all-zero
scores and at np - 1, np, np + 1; the retry ceiling of ppr.ppr_topk.  Normalise / encode at 255 / 256 / 257 entries with empty rows,
degree-0 roots and columns, the maximum in the last wave and a launch larger than the entries.  The DEG / SPD union kernels at
63 / 64 / 65 entries of either list, every diagonal case, empty rows, both sides of 64 KiB of LDS and the longest row allowed.

Every comparison is a bit pattern against oracle.ppr_topk / orc_ppr_normalize / ppr_encode / encoding_scipy.  Outputs of the
direct calls are poisoned first: row i must be untouched beyond out_count[i], a refused row entirely."""
import ctypes as C

import numpy as np
import pytest
import torch

import ppr_edges as E
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
POISON64 = 0x5A5A5A5A5A5A5A5A
FREE_SLOT = 0x00000000FFFFFFFF          # kFreeSlot of csrc/ppr.hip
COLLIDING = [(190, [1023]), (256, [1023, 0]), (300, [1023, 1022])]


@pytest.fixture(scope="module")
def ppr():
    import os
    from surel_plus_amd import _lib, ppr
    assert os.path.exists(_lib.LIB_PATH), "libsubgacc_hip.so must be built (no fallback)"
    assert _lib.lib().subgacc_device_count() >= 1, "no gfx950 device"
    return ppr


def _L():
    from surel_plus_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------- the oracle, per root
_ORACLE = {}


def _oracle_rows(key, indptr, indices, roots, alpha, eps, topk):
    """[(ids, score bits, pushes)] per root, computed once per (graph, parameters)"""
    out = []
    for r in roots:
        k = (key, int(r), alpha, eps, topk)
        if k not in _ORACLE:
            _, ids, vals, pushes = orc.ppr_topk(indptr, indices, [r], alpha, eps, topk, table_log2=16)
            _ORACLE[k] = (ids, vals.view(np.int32), pushes)
        out.append(_ORACLE[k])
    return out


# ------------------------------------------------------------------------------------------------------------- the direct call
def _push(indptr, indices, roots, alpha, eps, topk, log2=10, waves=None, what=""):
    """subgacc_ppr_slab_reset + subgacc_ppr_topk as ppr._launch makes them, over poisoned outputs.
    -> (rc, out_count, out_ids [n, topk], score bits [n, topk], flags, pushes, slab as uint64 [waves, 3, cap])"""
    L = _L()
    lib = L.lib()
    n = len(roots)
    waves = max(1, min(n, 64)) if waves is None else waves
    d_ptr, d_idx, d_roots = _dev(indptr), _dev(indices), _dev(np.asarray(roots, dtype=np.int32))
    nbytes = lib.subgacc_ppr_slab_bytes(log2, waves)
    assert nbytes == waves * 24 << log2
    slab = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lib.subgacc_ppr_slab_reset(L.ptr(slab), log2, waves, L.stream_ptr()) == 0
    cnt = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    ids = torch.full((n * topk,), POISON, dtype=torch.int32, device="cuda")
    vals = torch.full((n * topk,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    pushes = torch.zeros(2, dtype=torch.int64, device="cuda")
    rc = lib.subgacc_ppr_topk(L.ptr(d_ptr), int(d_ptr.dtype == torch.int64), L.ptr(d_idx), len(indptr) - 1, L.ptr(d_roots), n,
                              float(alpha), float(eps), int(topk), L.ptr(slab), log2, waves, L.ptr(cnt), L.ptr(ids), L.ptr(vals),
                              L.ptr(flags), L.ptr(pushes), L.stream_ptr())
    torch.cuda.synchronize()
    cnt, flags, pushes = cnt.cpu().numpy(), flags.cpu().numpy(), pushes.cpu().numpy()
    print(f"ppr_topk {what}: log2 = {log2}, waves = {waves}, roots = {n}, topk = {topk}, ({alpha}, {eps}): rc = {rc}, flags = "
          f"{flags.tolist()}, refused = {np.flatnonzero(cnt == -1).tolist()}, pushes = {pushes.tolist()}")
    return (rc, cnt, ids.cpu().numpy().reshape(n, topk), vals.view(torch.int32).cpu().numpy().reshape(n, topk), flags, pushes,
            slab.view(torch.int64).cpu().numpy().view(np.uint64).reshape(waves, 3, 1 << log2))


def _check_push(res, want, accepted=None):
    """rows against the oracle's [(ids, bits, pushes)]; accepted[i] False: row i refused and untouched"""
    rc, cnt, ids, bits, flags, pushes, slab = res
    assert rc == 0
    accepted = [True] * len(want) if accepted is None else accepted
    for i, (w_ids, w_bits, _) in enumerate(want):
        if not accepted[i]:
            assert cnt[i] == -1
            assert (ids[i] == POISON).all() and (bits[i] == POISON).all(), "a refused row was written"
            continue
        c = len(w_ids)
        assert cnt[i] == c
        np.testing.assert_array_equal(ids[i, :c], w_ids)
        np.testing.assert_array_equal(bits[i, :c], w_bits)
        assert (ids[i, c:] == POISON).all() and (bits[i, c:] == POISON).all(), "a row was written beyond its count"
    assert (flags[2] & 1) == (0 if all(accepted) else 1) and flags[[0, 1, 3]].tolist() == [0, 0, 0]
    assert pushes[0] == sum(w[2] for w, a in zip(want, accepted) if a)      # abandoned attempts do not count
    assert (slab[:, 0] == np.uint64(FREE_SLOT)).all() and (slab[:, 1] == 0).all(), "the slab did not come back clean"


def _check_rows(got, want):
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1])
    np.testing.assert_array_equal(got[2].cpu().numpy().view(np.int32), want[2].view(np.int32))


# ------------------------------------------------------------------------------------------------------------- the push
@pytest.mark.parametrize("root_slot", [None, 1023])
@pytest.mark.parametrize("K,slots", COLLIDING)
def test_claimants_of_one_slot_and_wrapping_chains(ppr, K, slots, root_slot):
    indptr, indices, root, leaves = E.colliding_star(K, slots, root_slot=root_slot)
    roots = [root] + leaves[[0, K // 2, K - 1]].tolist()
    key = ("colliding", K, root_slot)
    for alpha, eps, topk in ((E.ALPHA, E.EPS, 4096), (E.ALPHA, E.EPS, 100), (0.3, 1e-3, 4096)):     # 1 - 0.3 is not a float32
        want = _oracle_rows(key, indptr, indices, roots, alpha, eps, topk)
        res = _push(indptr, indices, roots, alpha, eps, topk, what=f"colliding star K = {K}, slots {slots}, root slot {root_slot}")
        _check_push(res, want)                                   # touched <= K + 1 <= 383: accepted at the first attempt
        full = _oracle_rows(key, indptr, indices, roots, alpha, eps, 4096)
        assert res[5][1] == sum(E.touched_count(indptr, indices, w[0]) for w in full)


@pytest.mark.parametrize("d,idx64", [(d, False) for d in (1, 63, 64, 65, 255, 256, 257, 382)] + [(64, True), (257, True)])
def test_star_degrees_around_the_trip(ppr, d, idx64):
    indptr, indices = E.star(d)
    if idx64:
        indptr = indptr.astype(np.int64)
    for alpha, eps in [(0.5, 1e-4)] + ([(0.15, 1e-5)] if d <= 65 else []):
        want = _oracle_rows(("star", d), indptr, indices, [0, 1], alpha, eps, 4096)
        _check_push(_push(indptr, indices, [0, 1], alpha, eps, 4096, what=f"star({d}), int64 = {idx64}"), want)


@pytest.mark.parametrize("d", [512, 600])
def test_stars_past_the_refusal_bound_are_refused(ppr, d):
    indptr, indices = E.star(d)
    want = _oracle_rows(("star", d), indptr, indices, [0, 1], E.ALPHA, E.EPS, 700)
    res = _push(indptr, indices, [0, 1], E.ALPHA, E.EPS, 700, what=f"star({d})")
    _check_push(res, want, accepted=[False, False])
    assert res[5].tolist() == [0, 0]


@pytest.mark.parametrize("d", [510, 511])
def test_stars_between_the_bounds_match_whichever_attempt_accepts(ppr, d):
    from surel_plus_amd import DeviceCSR
    indptr, indices = E.star(d)
    want = orc.ppr_topk(indptr, indices, [0, 1], E.ALPHA, E.EPS, 700, table_log2=16)
    got = ppr.ppr_topk(DeviceCSR(indptr, indices), E.ALPHA, E.EPS, [0, 1], 700, table_log2=10)
    _check_rows(got, want)
    assert got[3] == want[3]


@pytest.fixture(scope="module")
def mixed():
    indptr, indices, parts = E.mixed_graph()
    c, s7 = parts["colliding"], parts["star7"]
    bad = [parts["star512"][0], parts["star600"][0], int(parts["star512"][1][3]), int(parts["star600"][1][-1])]
    roots = [c[0], bad[0], int(c[1][0]), bad[1], s7[0], bad[2], int(c[1][150]), bad[3], int(s7[1][2]), bad[0], int(c[1][299])]
    accepted = [r not in bad for r in roots]
    return indptr, indices, roots, accepted


@pytest.mark.parametrize("waves", [1, 4])
def test_one_wave_runs_refused_and_accepted_roots_in_turn(ppr, mixed, waves):
    indptr, indices, roots, accepted = mixed
    if waves == 4:                                   # n = num_waves + 1: wave 0 runs a refused root, then an accepted one
        pick = [1, 0, 3, 2, 4]
        roots, accepted = [roots[i] for i in pick], [accepted[i] for i in pick]
    want = _oracle_rows("mixed", indptr, indices, roots, E.ALPHA, E.EPS, 128)
    res = _push(indptr, indices, roots, E.ALPHA, E.EPS, 128, waves=waves, what=f"mixed roots, accepted = {accepted}")
    _check_push(res, want, accepted)
    full = _oracle_rows("mixed", indptr, indices, roots, E.ALPHA, E.EPS, 4096)
    assert res[5][1] == sum(E.touched_count(indptr, indices, w[0]) for w, a in zip(full, accepted) if a)


def test_retried_rows_are_scattered_back_into_place(ppr, mixed, monkeypatch):
    from surel_plus_amd import DeviceCSR
    indptr, indices, roots, accepted = mixed
    monkeypatch.setattr(ppr, "MAX_WAVES", 1)
    want = orc.ppr_topk(indptr, indices, roots, E.ALPHA, E.EPS, 128, table_log2=16)
    got = ppr.ppr_topk(DeviceCSR(indptr, indices), E.ALPHA, E.EPS, roots, 128, table_log2=10)
    _check_rows(got, want)
    assert got[3] == want[3] and ppr.LAST_STATS["roots"] == len(roots)


# ------------------------------------------------------------------------------------------------------------- the top-K
def test_topk_cut_among_equal_scores(ppr):
    indptr, indices = E.star(255)                                # np = 256, 5 distinct scores
    for topk in (1, 2, 63, 64, 65, 255, 256, 257, 4096):
        want = _oracle_rows(("star", 255), indptr, indices, [0, 1], E.ALPHA, E.EPS, topk)
        _check_push(_push(indptr, indices, [0, 1], E.ALPHA, E.EPS, topk, what="star(255)"), want)


def test_topk_cut_among_equal_scores_past_two_trips(ppr):
    from surel_plus_amd import DeviceCSR
    indptr, indices = E.star(512)                                # np = 513, 3 distinct scores; refused at 2^10 slots
    csr = DeviceCSR(indptr, indices)
    for topk in (1, 2, 63, 64, 65, 512, 513, 514, 4096):
        want = orc.ppr_topk(indptr, indices, [0, 1], E.ALPHA, E.EPS, topk, table_log2=16)
        got = ppr.ppr_topk(csr, E.ALPHA, E.EPS, [0, 1], topk)
        _check_rows(got, want)
        assert got[3] == want[3]


def test_topk_of_a_row_of_one_with_hundreds_touched(ppr):
    indptr, indices = E.complete_bipartite(20, 300)
    for topk in (1, 5):
        want = _oracle_rows("K(20,300)", indptr, indices, [0, 25], E.ALPHA, E.EPS, topk)
        assert len(want[0][0]) == 1
        res = _push(indptr, indices, [0, 25], E.ALPHA, E.EPS, topk, what="K(20, 300)")
        _check_push(res, want)


def test_topk_above_4096_is_a_bad_argument(ppr):
    indptr, indices = E.star(5)
    assert _push(indptr, indices, [0], E.ALPHA, E.EPS, 4097, what="topk = 4097")[0] == _L().ERR_BADARG
    assert _push(indptr, indices, [0], E.ALPHA, E.EPS, 4096, what="topk = 4096")[0] == 0


@pytest.mark.parametrize("topk", [5, 100])
def test_alpha_one_cuts_among_zero_scores(ppr, topk):
    from surel_plus_amd import DeviceCSR
    indptr, indices = E.directed_graph(1500, 9000, 4)
    roots = np.arange(1500, dtype=np.int32)
    want = orc.ppr_topk(indptr, indices, roots, 1.0, 1e-4, topk, table_log2=16)
    got = ppr.ppr_topk(DeviceCSR(indptr, indices), 1.0, 1e-4, roots, topk)
    _check_rows(got, want)
    assert got[3] == want[3]


# ------------------------------------------------------------------------------------------------------------- the retry ceiling
def test_a_hub_wider_than_the_pushed_bound_is_not_refused(ppr):
    """star(1500) at (0.5, 1e-2): one push touches 1,501 nodes; 1 / (alpha * eps) = 200 bounds the PUSHED nodes only"""
    from surel_plus_amd import DeviceCSR
    indptr, indices = E.star(1500)
    csr = DeviceCSR(indptr, indices)
    want = orc.ppr_topk(indptr, indices, [0], 0.5, 1e-2, 100, table_log2=16)
    assert want[1].tolist() == [0] and want[3] == 1
    for log2 in (None, 10):
        got = ppr.ppr_topk(csr, 0.5, 1e-2, [0], 100, table_log2=log2)
        _check_rows(got, want)
        assert got[3] == 1
    off, ids, data = orc.topk_ppr_matrix(indptr, indices, 0.5, 1e-2, [0], 100, normalization="sym", table_log2=16)
    z = ppr.topk_ppr_matrix(csr, 0.5, 1e-2, [0], 100, normalization="sym")
    np.testing.assert_array_equal(z.indptr.cpu().numpy(), off)
    np.testing.assert_array_equal(z.indices.cpu().numpy(), ids)
    np.testing.assert_array_equal(z.data.cpu().numpy().view(np.int64), data.view(np.int64))


def test_a_repeated_entry_still_raises(ppr):
    from surel_plus_amd import DeviceCSR
    indptr, indices = E.repeated_entry_star()
    csr = DeviceCSR(indptr, indices)
    for log2 in (None, 10):
        with pytest.raises(MemoryError, match="repeated entries in a CSR row"):
            ppr.ppr_topk(csr, 0.5, 1e-2, [0], 100, table_log2=log2)
    want = orc.ppr_topk(*E.star(399), [0, 1], 0.5, 1e-2, 100, table_log2=16)      # the same star without the repeats
    _check_rows(ppr.ppr_topk(DeviceCSR(*E.star(399)), 0.5, 1e-2, [0, 1], 100), want)


def test_the_retry_slab_stays_inside_the_budget(ppr):
    for log2 in range(10, 27):
        w = ppr._waves(log2)
        assert 1 <= w <= ppr.MAX_WAVES and (w == 1 or w * (24 << log2) <= ppr.SLAB_BUDGET)
    assert ppr._waves(16) == ppr.MAX_WAVES and ppr._waves(22) == 85 and ppr._waves(23) == 42 and ppr._waves(26) == 5


# ------------------------------------------------------------------------------------------------------------- normalise / encode
@pytest.fixture(scope="module")
def sink_graph():
    indptr, indices = E.directed_graph(1500, 9000, 4)
    deg = np.diff(indptr)
    return indptr, indices, np.flatnonzero(deg == 0), np.flatnonzero(deg > 0)


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("nnz", [0, 1, 255, 256, 257, 1000])
def test_normalize_and_encode_at_block_and_wave_edges(ppr, sink_graph, nnz, mode, idx64):
    L = _L()
    lib = L.lib()
    indptr, indices, sinks, nonsinks = sink_graph
    roots, row_off, ids, vals = E.packed_rows(nnz, 1500, sinks, nonsinks)
    n, max_nnz = len(roots), nnz + 300                           # the launch covers more than the entries
    want = np.zeros(nnz, np.float64)
    ip64 = np.ascontiguousarray(indptr, dtype=np.int64)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    orc.lib().orc_ppr_normalize(p(ip64, C.c_int64), p(roots, C.c_int32), C.c_int64(n), p(row_off, C.c_int64), p(ids, C.c_int32),
                                p(vals, C.c_float), C.c_int(mode), p(want, C.c_double))
    if nnz:
        assert want.argmax() == nnz - 1                          # the maximum sits in the last wave that holds entries
    pad = lambda a: np.r_[a, np.zeros(300, a.dtype)]
    d_ptr = _dev(ip64 if idx64 else indptr)
    d_roots, d_off, d_ids, d_vals = _dev(roots), _dev(row_off), _dev(pad(ids)), _dev(pad(vals))
    out = torch.full((max_nnz,), POISON64, dtype=torch.int64, device="cuda")
    mx = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = lib.subgacc_ppr_normalize(L.ptr(d_ptr), int(idx64), L.ptr(d_roots), n, L.ptr(d_off), max_nnz, L.ptr(d_ids), L.ptr(d_vals),
                                   mode, L.ptr(out), L.ptr(mx), L.stream_ptr())
    torch.cuda.synchronize()
    h, hmx = out.cpu().numpy(), int(mx.item())
    print(f"ppr_normalize: nnz = {nnz} of {max_nnz}, mode = {mode}, int64 = {idx64}: rc = {rc}, max bits = {hmx:#x}")
    assert rc == 0
    np.testing.assert_array_equal(h[:nnz], want.view(np.int64))
    assert (h[nnz:] == POISON64).all(), "normalize wrote past the entries"
    assert hmx == (int(want.max().view(np.int64)) if nnz else 0)
    d_nnz = _dev(row_off[-1:])
    rc = lib.subgacc_ppr_encode(L.ptr(out), max_nnz, L.ptr(d_nnz), L.ptr(mx), L.stream_ptr())
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    print(f"ppr_encode: rc = {rc}")
    assert rc == 0
    np.testing.assert_array_equal(h[:nnz], orc.ppr_encode(want).view(np.int64))
    assert (h[nnz:] == POISON64).all(), "encode wrote past *nnz_dev"


# ------------------------------------------------------------------------------------------------------------- DEG / SPD
def _check_encoding(ppr, key, X, A, enc, idx64, gather=True):
    import surel_plus_amd as sp
    from surel_plus_amd import DeviceCSR, SpG
    N = X.shape[0]
    if (key, enc) not in _SCIPY:                                 # the reference once per input, shared by both offset widths
        _SCIPY[(key, enc)] = orc.encoding_scipy(X, A, enc)
    want, wagg = _SCIPY[(key, enc)]
    x = SpG.from_scipy(X)
    csr = DeviceCSR(A.indptr.astype(np.int64 if idx64 else np.int32), A.indices.astype(np.int32))
    z, agg = ppr.encoding(x, csr, enc)
    got = z.to_scipy()
    print(f"encoding {enc}: N = {N}, longest x row = {x.max_len}, int64 = {idx64}: {got.nnz} entries, longest row {z.max_len}")
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data.view(np.int64), want.data.astype(np.float64).view(np.int64))
    if enc == "DEG":
        ga = agg.to_scipy()
        np.testing.assert_array_equal(ga.indptr, wagg.indptr)
        np.testing.assert_array_equal(ga.indices, wagg.indices)
        np.testing.assert_array_equal(ga.data.view(np.int64), wagg.data.view(np.int64))
    else:
        assert agg is None and wagg is None
    if gather:
        full = np.flatnonzero(np.diff(want.indptr) > 0)          # the join is not under test here: rows with entries only
        edge = np.random.default_rng(0).choice(full, (2, 200))
        edge[:, :6] = [[0, 10, 50, N - 1, 30, 40], [50, 20, 50, 0, 40, N // 2]]
        xz, ip = sp.gather(torch.from_numpy(edge).cuda(), z, "cuda", ptr=True, encode=None)
        wxz, wip = orc.gather_numpy(edge, (want.indptr.astype(np.int64), want.indices, want.data.astype(np.float64)), ptr=True,
                                    encode=None)
        np.testing.assert_array_equal(ip.cpu().numpy(), wip)
        np.testing.assert_array_equal(xz.cpu().numpy(), wxz)


_SCIPY = {}


@pytest.fixture(scope="module")
def edge_inputs():
    return E.edge_inputs_for_encoders()


@pytest.mark.parametrize("idx64", [False, True])
@pytest.mark.parametrize("enc", ["DEG", "SPD"])
def test_union_kernels_at_lane_and_diagonal_edges(ppr, edge_inputs, enc, idx64):
    X, A = edge_inputs
    _check_encoding(ppr, "edges", X, A, enc, idx64)


@pytest.fixture(scope="module", params=[6551, 6552, 8192])
def long_row(request):
    return E.long_row_inputs(request.param)


@pytest.mark.parametrize("enc", ["DEG", "SPD"])
def test_union_kernels_on_both_sides_of_64k_of_lds(ppr, long_row, enc):
    X, A, s = long_row
    kmax = int(X.getnnz(axis=1).max())
    _check_encoding(ppr, kmax, X, A, enc, idx64=kmax == 6552, gather=False)


@pytest.mark.parametrize("enc", ["DEG", "SPD"])
def test_a_row_past_8192_entries_is_refused(ppr, enc):
    from surel_plus_amd import DeviceCSR, SpG
    X, A, s = E.long_row_inputs(8193)
    with pytest.raises(TypeError, match="8192"):
        ppr.encoding(SpG.from_scipy(X), DeviceCSR(A.indptr.astype(np.int32), A.indices.astype(np.int32)), enc)

"""GPU (MI355X): the join over the step's packed rows written in fp16 / bf16 (include/subgacc_packed_half.h) -- the entry point over
hand-made rows against the f32 packed join rounded by torch and against the two-plane half join over the unpacked rows, bit for bit,
and the step of StepBuffers(dtype=, packed_half=True) against the two-plane half step and the oracle.  The rows are those of
tests/packed_rows.py and tests/packed_half_rows.py; every output is poisoned before the launch and stands between poisoned guards."""
import numpy as np
import pytest
import torch

import packed_half_rows as H
import packed_rows as P
import test_gpu_packed_rows as TP
from gpu_helpers import sp  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
SMALL_BATCH_PAIRS = 2048     # packhalf_threads: pairs * 2 <= 4096 take 256 lanes at every pitch


def _same(res, what, via_half=True):
    assert torch.equal(res["got"], res["want"]), (what, H.first_difference(res["got"], res["want"]))
    if via_half:
        assert torch.equal(res["got"], res["half"]), (what, "two-plane half join", H.first_difference(res["got"], res["half"]))


# ------------------------------------------------------------------------------------------------------------- the entry point
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("m,M,N,pitch", P.JOIN_SHAPES)
def test_every_pair_of_the_hand_made_rows(sp, m, M, N, pitch, dtype):
    """every ordered pair of the rows of P.join_rows and H.edge_rows -- (u, u), an empty row on either side, S longer and shorter than
    T, lengths at every trip and form boundary, 0 / 1 / 63 / 64 / 65 / all escapes, escapes at chunk ends, the quotients row -- as a
    small batch (256 lanes) and as one beyond the small-batch rule (the shape's own form: 128 x 4, 128 x 5 or 256 x 4)"""
    rows = H.edge_rows(M, m, N, pitch)
    pl = H.planes(rows, M, m, pitch)
    n = len(rows["ids"])
    assert n * n <= SMALL_BATCH_PAIRS
    for count in (n * n, SMALL_BATCH_PAIRS + 1):
        res = H.join(M, m, N, pitch, pl, P.join_pairs(n, count), dtype)
        assert res["flags"] == [0, 0, 0, 0] and res["flags32"] == [0, 0, 0, 0] and res["flags_half"] == [0, 0, 0, 0], (count, res["flags"])
        assert res["R"] > 0 and bool(res["written"].all())
        _same(res, (count,))
    print(f"M = {M}, m = {m}, pitch {pitch}, {dtype}: {n} rows, {res['R']} output rows, lanes x trips {P.join_lanes(pitch)}")


@pytest.mark.parametrize("m,M,N,pitch", P.JOIN_SHAPES)
def test_the_quotients_row_is_rounded_in_both_types(sp, m, M, N, pitch):
    """the row whose hop-1 count is 0 .. M joined with itself: column 1 of both halves of xz is c / M for every c, and torch alone
    says that most of those quotients are not 16-bit numbers -- the rounding is exercised.  (M = 256 is the exception: c / 256 with
    c <= 256 has at most 8 significant bits, which both types hold -- there every quotient must come through unchanged.)"""
    rows = H.edge_rows(M, m, N, pitch)
    i = rows["names"].index("quotients")
    q = (torch.arange(M + 1, dtype=torch.float32) / M)
    for dtype in DTYPES:
        inexact = int((q.to(dtype).to(torch.float32) != q).sum())
        assert (inexact == 0) if M & (M - 1) == 0 else (inexact > (M + 1) // 2), (dtype, inexact)
        res = H.join(M, m, N, pitch, H.planes(rows, M, m, pitch), np.array([[i], [i]]), dtype)
        assert res["flags"] == [0, 0, 0, 0] and res["R"] == 2 * (M + 1)
        _same(res, dtype)
        x = res["x32"]
        assert torch.equal(x[: M + 1, 1].cpu(), q) and torch.equal(x[: M + 1, m + 2].cpu(), q)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("count", [1, SMALL_BATCH_PAIRS, SMALL_BATCH_PAIRS + 1])
def test_batches_on_both_sides_of_the_small_batch_rule(sp, count, dtype):
    """1, 2,048 and 2,049 pairs of short rows (0, 1, 63, 64, 65 members) at a pitch of 608: 256 lanes up to 2,048 pairs, 128 x 5 above"""
    m, M, N, pitch = P.JOIN_SHAPES[0]
    rows = P.join_rows(M, m, N, pitch)
    short = {k: v[:5] if k in ("ids", "keys", "names") else v for k, v in rows.items()}
    assert [len(r) for r in short["ids"]] == [0, 1, 63, 64, 65]
    pairs = P.join_pairs(5, count + 7)[:, 7:]            # the first pair is (1, 2): a batch of one pair is not two empty rows
    res = H.join(M, m, N, pitch, H.planes(short, M, m, pitch), pairs, dtype)
    assert res["flags"] == [0, 0, 0, 0] and res["R"] > 0 and bool(res["written"].all())
    _same(res, count)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("m,M,N,pitch", [P.JOIN_SHAPES[4], P.JOIN_SHAPES[0], P.JOIN_SHAPES[5]])
def test_output_rows_at_every_phase_of_16_bytes(sp, m, M, N, pitch, dtype):
    """segments that begin 0, 1, 2 and 3 output rows later: the 12-byte rows of k = 3 and the 20-byte rows of k = 5 begin at every
    4-byte phase of 16 (k = 4: always aligned), a segment's first row odd and even; the rows in front keep their poison"""
    rows = H.edge_rows(M, m, N, pitch)
    pl = H.planes(rows, M, m, pitch)
    n = len(rows["ids"])
    for shift in range(4):
        res = H.join(M, m, N, pitch, pl, P.join_pairs(n, 3 * n + 5), dtype, seg_shift=shift)
        assert res["flags"] == [0, 0, 0, 0]
        assert not bool(res["written"][:shift].any()) and bool(res["written"][shift:].all())
        assert bool((res["got"][:shift] == H.POISON).all())
        _same(res, shift)


# ------------------------------------------------------------------------------------------------------------- the status words
def test_a_corrupted_escape_count_is_flagged_and_reads_as_the_f32_join_reads_it(sp):
    """nesc above the list, below it (and: 0, negative) and beyond the pitch: flags[3] & 2, and every key reads as
    subgacc_sjoin_fill_packed and subgacc_unpack_packed_rows read it -- an escape at or beyond nesc is key 0, never dereferenced"""
    m, M, N, pitch = P.JOIN_SHAPES[0]
    rows = P.join_rows(M, m, N, pitch)
    pl = H.planes(rows, M, m, pitch)
    n = len(rows["ids"])
    at = {name: i for i, name in enumerate(rows["names"])}
    pairs = P.join_pairs(n, n * n)
    ne = pl["nesc"]
    for dtype in DTYPES:
        for row, value in ((at["all"], int(ne[at["all"]]) + 3), (at["many"], 10), (at["many"], 0), (at["many"], -5), (at["many"], pitch + 7),
                           (at["many"], 70)):
            res = H.join(M, m, N, pitch, pl, pairs, dtype, nesc_edit={row: value})
            assert res["flags"] == [0, 0, 0, 2] and res["flags32"] == [0, 0, 0, 2], (row, value, res["flags"])
            assert bool(res["written"].all())
            _same(res, (row, value))


def test_a_row_longer_than_the_pitch_and_an_unmirrored_pair_leave_their_segments_unwritten(sp):
    m, M, N, pitch = P.JOIN_SHAPES[0]
    rows = P.join_rows(M, m, N, pitch)
    pl = H.planes(rows, M, m, pitch)
    n = len(rows["ids"])
    pairs = P.join_pairs(n, n * n)
    B = pairs.shape[1]
    for dtype in DTYPES:
        # row 3 claims pitch + 1 members: every pair with it is skipped, flags[3] & 1
        res = H.join(M, m, N, pitch, pl, pairs, dtype, nsize_edit={3: pitch + 1}, via_half=False)
        assert res["flags"] == [0, 0, 0, 1] == res["flags32"]
        skipped = int((~res["written"]).sum())
        assert skipped >= (2 * n - 1) * (pitch + 1) and skipped < res["R"]
        _same(res, "long row", via_half=False)
        assert bool((res["got"][~res["written"]] == H.POISON).all())
        # segment 5's partner is not the own row of its mirror: flags[3] & 4, both segments stay poison
        j = 5
        wrong = int(pairs[1, j] + 1) % n
        res = H.join(M, m, N, pitch, pl, pairs, dtype, partner_edit={j: wrong}, via_half=False)
        assert res["flags"][3] & 4 and res["flags32"][3] & 4 and res["flags"] == res["flags32"]
        _same(res, "unmirrored", via_half=False)
        assert bool((res["got"][~res["written"]] == H.POISON).all()) and int((~res["written"]).sum()) > 0
        assert B == n * n


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_a_row_number_outside_the_store_is_an_empty_row(sp, dtype):
    """own rows n, n + 5 and -1: never dereferenced, their segments are empty and their partners' rows have the zero row beside them"""
    m, M, N, pitch = P.JOIN_SHAPES[0]
    rows = P.join_rows(M, m, N, pitch)
    pl = H.planes(rows, M, m, pitch)
    n = len(rows["ids"])
    pairs = np.array([[n, 4, -1, n + 5, 6], [5, n, 7, n + 5, 6]], dtype=np.int64)
    res = H.join(M, m, N, pitch, pl, pairs, dtype, via_half=False)
    ns = pl["nsize"]
    assert res["R"] == int(ns[5] + ns[4] + ns[7] + 2 * ns[6]) and bool(res["written"].all())
    assert res["flags"] == res["flags32"] and not res["flags"][3] & 7
    _same(res, "outside", via_half=False)
    k = m + 1
    assert bool((res["x32"][: int(ns[4]), k:] == 0).all())          # segment 1 = row 4 | nothing


# --------------------------------------------------------------------------------------------------------------------- the step
def _golden_step(sp, M=200, m=3, B=96, seed=21, rng_seed=5):
    ptr_, idx = TP._golden_graph()
    N = len(ptr_) - 1
    csr = sp.DeviceCSR(ptr_, idx)
    e = np.random.default_rng(rng_seed).integers(0, N, (2, B))
    e[1, :4] = e[0, :4]                      # (u, u)
    e[:, 4:20] = e[:, 20:36]                 # repeated endpoints
    return csr, N, e, torch.from_numpy(e).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("dedup,order", [(False, False), (True, False), (False, True), (True, True)])
def test_packed_half_step_equals_the_two_plane_half_step_and_the_oracle(sp, dedup, order, dtype):
    """StepBuffers(dtype=, packed_half=True) on the golden graph, M = 200, 3 hops, B = 96: packed and half; (xz, indptr) are those of
    StepBuffers(dtype=) bit for bit and the oracle's gather rounded by torch, with root dedup and order=, into out=, twice in a row;
    the sets show the two planes when looked at, and the step itself allocated nothing"""
    import oracle
    from surel_plus_amd.spg import StridedSpG
    M, m, B, seed = 200, 3, 96, 21
    csr, N, e, edge = _golden_step(sp, M, m, B, seed)
    assert sp.sampler.packed_rows_form(N, M, m) == P.fmt(N, m)
    lo = sp.sampler.locality_order(csr) if order else None
    kw = dict(num_walks=M, num_steps=m, dedup_roots=dedup, order=lo, dtype=dtype)
    bp = sp.StepBuffers(csr, B, packed_half=True, **kw)
    bu = sp.StepBuffers(csr, B, **kw)
    assert bp.packed and bp.half and bu.half and not bu.packed and bp.out.dtype == dtype
    assert sp.StepBuffers(csr, B, packed_half=True, packed_rows=True, **kw).packed
    call = dict(num_walks=M, num_steps=m, seed=seed, rng="philox", dedup_roots=dedup, dtype=dtype)
    spg, table = TP._oracle_store(M, m, seed, "philox")
    e2 = np.random.default_rng(77).integers(0, N, (2, B))
    # two steps in a row on the same buffers (the second into out=): each gives its own result
    mine = torch.full((2 * B * (M * m + 1) * 2 * (m + 1),), -1, dtype=torch.int16, device="cuda").view(dtype)
    for step, (eh, ed, out) in enumerate(((e2, torch.from_numpy(e2).cuda(), None), (e, edge, mine))):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        xz_p, ind_p, sets_p = sp.sample_and_gather(csr, ed, buffers=bp, out=out, **call)
        if step:        # (the first step makes the work-list buffers; from then on nothing is allocated)
            assert torch.cuda.memory_allocated() == before, "the step allocated"
        xz_u, ind_u, sets_u = sp.sample_and_gather(csr, ed, buffers=bu, **call)
        sets_p.resolve(), sets_u.resolve()
        R = int(ind_u[-1].item())
        assert xz_p.dtype == dtype and torch.equal(ind_p, ind_u)
        assert torch.equal(xz_p[:R].view(torch.int16), xz_u[:R].view(torch.int16)), step
        oxz, oind = oracle.gather(eh, spg, ptr=True, encode=table)
        assert np.array_equal(ind_p.cpu().numpy(), oind)
        want = torch.from_numpy(oxz.astype(np.float32)).to(dtype)
        assert torch.equal(xz_p[:R].cpu().view(torch.int16), want.view(torch.int16)), step
        if out is not None:
            assert xz_p.data_ptr() == mine.data_ptr()
    assert bp._unpacked is None, "the step unpacked its rows"
    # what looks at the rows sees the two planes
    ns = bu.nsize.cpu().numpy()
    assert np.array_equal(bp.nsize.cpu().numpy(), ns)
    live = (np.arange(bu.stride)[None, :] < ns[:, None]).reshape(-1)
    for a, b in ((sets_p.ids, sets_u.ids), (sets_p.slot, sets_u.slot), (bp.ids, bu.ids), (bp.slot, bu.slot)):
        assert np.array_equal(a.cpu().numpy()[live], b.cpu().numpy()[live])
    assert bp._unpacked is not None and not bp._unpack_flags.any()
    zp, zu = StridedSpG(sets_p, N).to_csr(), StridedSpG(sets_u, N).to_csr()
    for name in ("indptr", "indices", "data"):
        assert torch.equal(getattr(zp, name), getattr(zu, name)), name
    assert sets_p.X == sets_u.X and sets_p.c == sets_u.c
    assert sets_p.number() is not None


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_packed_half_step_in_rand_r_mode(sp, dtype):
    """rng="rand_r": the two-plane half step and the oracle's sequential stream"""
    import oracle
    M, m, B, seed = 200, 3, 96, 21
    csr, N, e, edge = _golden_step(sp, M, m, B, seed, rng_seed=4)
    bp = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, rng="rand_r", dtype=dtype, packed_half=True)
    bu = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, rng="rand_r", dtype=dtype)
    assert bp.packed and bp.half and not bu.packed
    call = dict(num_walks=M, num_steps=m, seed=seed, rng="rand_r", dtype=dtype)
    xz_p, ind_p, s_p = sp.sample_and_gather(csr, edge, buffers=bp, **call)
    xz_u, ind_u, s_u = sp.sample_and_gather(csr, edge, buffers=bu, **call)
    s_p.resolve(), s_u.resolve()
    R = int(ind_u[-1].item())
    assert torch.equal(ind_p, ind_u) and torch.equal(xz_p[:R].view(torch.int16), xz_u[:R].view(torch.int16))
    nsize, remap, enc = oracle.gset_sampler(*TP._golden_graph(), e.reshape(-1), num_walks=M, num_steps=m, seed=seed, rng="rand_r")
    oxz, oind = oracle.gather(np.stack([np.arange(B), np.arange(B, 2 * B)]), oracle.spg_build(nsize, remap), ptr=True, encode=TP._zsf(enc, M))
    assert np.array_equal(ind_p.cpu().numpy(), oind)
    assert torch.equal(xz_p[:R].cpu().view(torch.int16), torch.from_numpy(oxz.astype(np.float32)).to(dtype).view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("m,M", [(2, 256), (4, 102)])
def test_packed_half_step_at_two_and_four_hops(sp, m, M, dtype):
    """k = 3 and k = 5 on the golden graph: the two-plane half step, bit for bit, and the f32 step rounded by torch"""
    B, seed = 96, 8
    csr, N, e, edge = _golden_step(sp, M, m, B, seed)
    assert (m, M) in P.SHAPES and sp.sampler.packed_rows_form(N, M, m) is not None
    kw = dict(num_walks=M, num_steps=m)
    bp = sp.StepBuffers(csr, B, dtype=dtype, packed_half=True, **kw)
    bu = sp.StepBuffers(csr, B, dtype=dtype, **kw)
    bf = sp.StepBuffers(csr, B, packed_rows=False, **kw)
    assert bp.packed and bp.half and not bu.packed and not bf.packed
    xz_p, ind_p, s_p = sp.sample_and_gather(csr, edge, seed=seed, buffers=bp, dtype=dtype, **kw)
    xz_u, ind_u, s_u = sp.sample_and_gather(csr, edge, seed=seed, buffers=bu, dtype=dtype, **kw)
    xz_f, ind_f, s_f = sp.sample_and_gather(csr, edge, seed=seed, buffers=bf, **kw)
    s_p.resolve(), s_u.resolve(), s_f.resolve()
    R = int(ind_f[-1].item())
    assert R > 0 and torch.equal(ind_p, ind_u) and torch.equal(ind_p, ind_f)
    assert torch.equal(xz_p[:R].view(torch.int16), xz_u[:R].view(torch.int16))
    assert torch.equal(xz_p[:R].view(torch.int16), xz_f[:R].to(dtype).view(torch.int16))


def test_the_keyword_is_refused_on_the_device_build_as_on_the_host(sp):
    """every ValueError of StepBuffers(packed_half=True), with a real graph: the keyword and the reason are named, nothing is
    allocated; without the keyword a 16-bit step keeps the two planes and packed_rows=True beside it still raises"""
    ptr_, idx = TP._golden_graph()
    csr = sp.DeviceCSR(ptr_, idx)
    bf = torch.bfloat16
    for kw, reason in ((dict(dtype=None), "dtype=None"), (dict(dtype=torch.float32), "dtype=torch.float32"),
                       (dict(packed_rows=False), "packed_rows=False"), (dict(ptr=False), "ptr=False"), (dict(triplets=True), "triplets=True"),
                       (dict(stage="counts"), "stage='counts'"), (dict(key_rows=False), "key_rows=False"), (dict(batch=16), "batch="),
                       (dict(num_steps=2), "no packed form"), (dict(num_walks=200, num_steps=4), "no packed form"),
                       (dict(num_walks=200, num_steps=4, wide_keys=True), "no packed form"), (dict(num_walks=300), "no packed form")):
        kw = {"num_walks": 200, "num_steps": 3, "dtype": bf, **kw}
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError, match="packed_half=True") as err:
            sp.StepBuffers(csr, 64, packed_half=True, **kw)
        assert reason in str(err.value), (kw, str(err.value))
        assert torch.cuda.memory_allocated() == before
    assert not sp.StepBuffers(csr, 64, num_walks=200, num_steps=3, dtype=bf).packed
    with pytest.raises(ValueError, match="packed_rows=True"):
        sp.StepBuffers(csr, 64, num_walks=200, num_steps=3, dtype=bf, packed_rows=True)
    bufs = sp.StepBuffers(csr, 64, num_walks=200, num_steps=3, dtype=bf, packed_half=True)
    edge = torch.zeros((2, 64), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, edge, num_walks=200, num_steps=3, buffers=bufs, dtype=torch.float16)
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, edge, num_walks=200, num_steps=3, buffers=bufs)

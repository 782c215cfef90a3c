"""GPU: the recurrent kernel of index_lstm_stage (subgacc_lstm_aggr / _backward) at every step of every segment and at every width
LSTM_WIDTHS builds, against the float64 step reference gpu_helpers.lstm_steps (pinned to nn.LSTM in test_lstm_aggr_cpu.py).

Under nn.LSTM's default init the recurrence forgets within ~20 steps, so h_{L-1} and the parameter gradients see only the last rows of a
segment.  These tests read h_t / c_t at every step, and run a long-memory regime (+5 on the forget gate's bias, -3 on the input gate's) in which step 0 moves the
output; there every tolerance is an fp32 yardstick computed here -- CPU torch fp32 on the same inputs against float64 -- times FACTOR,
with a floor of FLOOR times the largest entry.  dG's ordered sum is checked bit for bit at its piece boundaries, and the C-level edges
(L past the longest segment, indices outside the table, segments longer than L) against the header's contract."""
import copy

import numpy as np
import pytest
import torch

from gpu_helpers import dense_batch, lstm_steps, sp, sym_graph  # noqa: F401

pytestmark = pytest.mark.gpu

FORGET = 5.0        # the long-memory regime: added to the forget gate's bias (0.993 per step at zero input; L <= ~300 keeps fp32
INPUT = -3.0        # near float64) and to the input gate's, so that c stays off tanh's flat tails and h_{L-1} still sees step 0
FACTOR = 20.0       # a tolerance is FACTOR times the fp32 yardstick's error ...
FLOOR = 1e-5        # ... and at least FLOOR times the largest entry of the float64 truth
STEP_BOUND = 2e-5   # h_t / c_t under default init: the forward bound of test_gpu_lstm_aggr.py, per step (CPU fp32: within 1e-6)
COUNTS = (1, 1023, 1024, 1025, 2048, 2049, 3073)   # entries of one index around dG's pieces of 1024


def _widths():
    from surel_plus_amd.spjoin import LSTM_WIDTHS
    assert LSTM_WIDTHS == tuple(range(16, 129, 16))
    return LSTM_WIDTHS


WIDTHS = _widths()


# ------------------------------------------------------------------------------------------------------------------- inputs
def _inputs(H2, T, long=False, bias=True, seed=0, k=12):
    """fp32 (G [T, 4H'], b [4H'] or None, W_hh [4H', H']) on the CPU: a default-initialised nn.LSTM(k, H') over random rows E [T, k],
    G = E W_ih^T, b = b_ih + b_hh; long: FORGET and INPUT added to its forget- and input-gate slices"""
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(k, H2, batch_first=True, bias=bias)
    with torch.no_grad():
        G = torch.randn((T, k)) @ lstm.weight_ih_l0.t()
        b = (lstm.bias_ih_l0 + lstm.bias_hh_l0) if bias else None
        if long:
            b[H2:2 * H2] += FORGET
            b[:H2] += INPUT
        return G.contiguous(), b, lstm.weight_hh_l0.detach().clone()


def _segments(lens, T, seed=0):
    """pairs (int32 [R, 2], indices drawn in [0, T)) and indptr (int64 [S + 1]) of segments of the given lengths, on the CPU"""
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    pairs = torch.from_numpy(np.random.default_rng(seed).integers(0, T, (int(indptr[-1]), 2)).astype(np.int32))
    return pairs, indptr


def _per_row(pairs, G):
    """one table row per (row, side) entry holding G of its index, and the pairs (2k, 2k+1) that read it: the recurrence sees the same
    floats, and dG's row 2k (and 2k+1) is row k's dgates alone"""
    R = pairs.shape[0]
    return torch.arange(2 * R, dtype=torch.int32).view(R, 2), G[pairs.view(-1).long()].contiguous()


def _cuda(t):
    return None if t is None else t.cuda().contiguous()


def _forward(pairs, indptr, L, T, G, b, w):
    """_LstmJoin(...).forward(keep=True) on the device: (join, h [S, H'], h_state, c_state [S, L, H'])"""
    from surel_plus_amd.spjoin import _LstmJoin
    join = _LstmJoin(_cuda(pairs), _cuda(indptr), L, T, w.shape[1])
    return (join, *join.forward(_cuda(G), _cuda(b), _cuda(w), True))


def _backward(join, G, b, w, hs, cs, dh, rows):
    """subgacc_lstm_aggr_backward as _LstmJoin.backward calls it, into the caller's ws_rows `rows`: (dG, db, dW_hh), sums over tiles"""
    from surel_plus_amd._lib import check, lib, ptr, stream_ptr
    from surel_plus_amd.spjoin import _nonnull
    G, b, w, dh = _cuda(G), _cuda(b), _cuda(w), _cuda(dh)
    S, H2, T = join.S, join.H2, join.T
    tiles = (S + 15) // 16
    order, piece_off, P, run_piece = join.grouping()
    pieces = torch.empty((P, 4 * H2), dtype=torch.float32, device="cuda") if P else None
    dG = torch.empty((T, 4 * H2), dtype=torch.float32, device="cuda")
    dw = torch.empty((tiles, 4 * H2, H2), dtype=torch.float32, device="cuda")
    db = torch.empty((tiles, 4 * H2), dtype=torch.float32, device="cuda")
    check(lib().subgacc_lstm_aggr_backward(ptr(_nonnull(join.pairs)), ptr(join.indptr), S, join.L, T, H2, ptr(G), ptr(b), ptr(w), ptr(hs),
                                           ptr(cs), ptr(dh), ptr(_nonnull(order)), ptr(piece_off), P, ptr(run_piece), ptr(rows),
                                           ptr(pieces), ptr(dG), ptr(dw), ptr(db), ptr(join.flags), stream_ptr()))
    torch.cuda.synchronize()
    return dG, db.sum(0), dw.sum(0)


def _reference(G, b, w, pairs, indptr, L, dtype=torch.float64):
    return lstm_steps(G.to(dtype), None if b is None else b.to(dtype), w.to(dtype), pairs, indptr, L)


# ---------------------------------------------------------------------------------------------------------------- checks
def _check_steps(hs, cs, ref, bound=STEP_BOUND):
    """h_t and c_t of every (segment, step) within `bound` times that step's largest entry of the float64 truth"""
    for what, got, want in (("h", hs, ref[0]), ("c", cs, ref[1])):
        assert got.shape == want.shape, what
        err = (got.cpu().double() - want).abs().amax(dim=(0, 2))
        scale = want.abs().amax(dim=(0, 2))
        bad = torch.nonzero(err > bound * scale).view(-1)
        assert bad.numel() == 0, f"{what}_t off at steps {bad[:8].tolist()} of {want.shape[1]}: error {float(err.max()):.3g}"


def _within_yardstick(got, want, y32, what):
    """|got - want| <= max(FACTOR |fp32 yardstick - want|, FLOOR max|want|), want the float64 truth"""
    got, want, y32 = (t.detach().cpu().double() for t in (got, want, y32))
    assert got.shape == want.shape, what
    scale = float(want.abs().max())
    yard = float((y32 - want).abs().max())
    err = float((got - want).abs().max())
    tol = max(FACTOR * yard, FLOOR * scale)
    assert err <= tol, f"{what}: error {err:.3g} > {tol:.3g} (fp32 yardstick {yard:.3g}, largest entry {scale:.3g})"


def _rows_within_yardstick(got, want, y32, what, floor=1e-6):
    """per row: |got - want| <= FACTOR r32 (max|want row| + floor max|want|), r32 the fp32 yardstick's largest such relative error"""
    got, want, y32 = (t.detach().cpu().double() for t in (got, want, y32))
    den = want.abs().amax(1) + floor * float(want.abs().max())
    r32 = float(((y32 - want).abs().amax(1) / den).max())
    rel = (got - want).abs().amax(1) / den
    bad = torch.nonzero(rel > FACTOR * r32).view(-1)
    assert bad.numel() == 0, f"{what}: rows {bad[:8].tolist()} off by {float(rel.max()):.3g} relative (fp32 yardstick {r32:.3g})"


# ------------------------------------------------------------------------------------------------------ every step, every width
@pytest.mark.parametrize("S", [1, 15, 16, 17, 33, 250])
@pytest.mark.parametrize("H2", WIDTHS)
def test_every_step_of_every_segment(sp, H2, S):
    """h_t / c_t at every (segment, step) of random segments (0 to 40 rows), at L = the longest segment and L = the longest + 7"""
    rng = np.random.default_rng(100 * S + H2)
    lens = rng.integers(0, 41, S)
    lens[rng.integers(S)] = 40
    T = 50
    pairs, indptr = _segments(lens, T, seed=S)
    G, b, w = _inputs(H2, T, seed=H2)
    for L in (40, 47):
        _, h, hs, cs = _forward(pairs, indptr, L, T, G, b, w)
        _check_steps(hs, cs, _reference(G, b, w, pairs, indptr, L))
        assert torch.equal(h, hs[:, -1])


@pytest.mark.parametrize("H2", WIDTHS)
def test_sixteen_lengths_in_one_tile(sp, H2):
    """the middle tile of three holds 16 segments of 16 different lengths (0, 1 and L among them), permuted across the lane quads; the
    same with T = 1 and b = None; a tile's bits do not depend on the tiles beside it"""
    L = 31
    rng = np.random.default_rng(H2)
    tile = rng.permutation([0, 1, 2, 3, 4, 5, 7, 9, 12, 14, 17, 20, 23, 26, 29, 31])
    lens = np.concatenate([rng.integers(0, 32, 16), tile, rng.integers(0, 32, 5)])
    for T, bias in ((40, True), (1, False)):
        pairs, indptr = _segments(lens, T, seed=H2)
        G, b, w = _inputs(H2, T, bias=bias, seed=H2 + 1)
        _, h, hs, cs = _forward(pairs, indptr, L, T, G, b, w)
        _check_steps(hs, cs, _reference(G, b, w, pairs, indptr, L))
        lo, hi = int(indptr[16]), int(indptr[32])
        _, h1, hs1, cs1 = _forward(pairs[lo:hi], indptr[16:33] - lo, L, T, G, b, w)
        assert torch.equal(hs1, hs[16:32]) and torch.equal(cs1, cs[16:32]) and torch.equal(h1, h[16:32])


# ------------------------------------------------------------------------------------------------------------- C-level edges
def test_an_index_outside_the_table_reads_row_zero_and_sets_the_flag(sp):
    """indices T and -1 on a few real rows: the bits of the same run with those indices replaced by 0, and flags[3] & 2"""
    lens = [5, 9, 0, 12, 3] * 4
    T = 20
    pairs, indptr = _segments(lens, T, seed=3)
    bad = pairs.clone()
    bad[2, 0], bad[7, 1], bad[30, 0], bad[30, 1], bad[-1, 1] = T, -1, T, -1, T
    fixed = torch.where((bad < 0) | (bad >= T), 0, bad)
    G, b, w = _inputs(32, T, seed=5)
    jb, hb, hsb, csb = _forward(bad, indptr, 12, T, G, b, w)
    jf, hf, hsf, csf = _forward(fixed, indptr, 12, T, G, b, w)
    assert int(jb.flags[3]) & 2 and not int(jf.flags[3]) & 2
    assert torch.equal(hb, hf) and torch.equal(hsb, hsf) and torch.equal(csb, csf)
    _check_steps(hsb, csb, _reference(G, b, w, fixed, indptr, 12))


@pytest.mark.parametrize("H2", (16, 112))
def test_segments_longer_than_l_run_l_steps_and_give_zero_dgates_past_l(sp, H2):
    """L below some segments' lengths (the header's contract): the forward runs their first L rows; the backward writes zero dgates for
    the rows past L (ws_rows is filled with NaN first), so h, dG, dW_hh and db equal those of the segments cut to L rows"""
    lens = np.array([30, 4, 25, 12, 0, 40, 19, 21] * 3)
    L, T = 20, 30
    pairs, indptr = _segments(lens, T, seed=7)
    cut = np.minimum(lens, L)
    keep = torch.from_numpy(np.concatenate([np.arange(s, s + c) for s, c in zip(indptr[:-1].tolist(), cut)]))
    tpairs, tindptr = pairs[keep], torch.from_numpy(np.concatenate([[0], np.cumsum(cut)]))
    G, b, w = _inputs(H2, T, long=True, seed=9)
    dh = torch.randn((len(lens), H2), generator=torch.Generator().manual_seed(1))
    runs = []
    for p, ip in ((pairs, indptr), (tpairs, tindptr)):
        join, h, hs, cs = _forward(p, ip, L, T, G, b, w)
        rows = torch.full((p.shape[0], 4 * H2), float("nan"), device="cuda")
        runs.append((h, hs, cs, rows, *_backward(join, G, b, w, hs, cs, dh, rows)))
    (h, hs, cs, rows, dG, db, dw), (th, ths, tcs, trows, tdG, tdb, tdw) = runs
    _check_steps(hs, cs, _reference(G, b, w, tpairs, tindptr, L))
    assert torch.equal(h, th) and torch.equal(hs, ths) and torch.equal(cs, tcs)
    past = torch.ones(pairs.shape[0], dtype=torch.bool)
    past[keep] = False
    assert past.sum() > 0 and torch.equal(rows[past.cuda()], torch.zeros_like(rows[past.cuda()]))
    assert torch.equal(rows[keep.cuda()], trows)
    assert bool(torch.isfinite(dG).all())
    assert torch.equal(dG, tdG) and torch.equal(db, tdb) and torch.equal(dw, tdw)


# ------------------------------------------------------------------------------------------- per-row dgates, long memory
@pytest.mark.parametrize("H2", WIDTHS)
def test_every_row_of_dgates_in_the_long_memory_regime(sp, H2):
    """a per-row table (one row per (row, side) entry): dG's rows are the rows' dgates, each against float64 autograd's dL/dG row;
    dW_hh and db over S = 37 segments (three tiles, the last partial) against float64; the first steps must matter"""
    rng = np.random.default_rng(H2 + 7)
    S, T, L = 37, 60, 250
    lens = rng.integers(0, 200, S)
    lens[[3, 20]] = L
    pairs, indptr = _segments(lens, T, seed=H2)
    G, b, w = _inputs(H2, T, long=True, seed=H2 + 2)
    rp, Gr = _per_row(pairs, G)
    dh = torch.randn((S, H2), generator=torch.Generator().manual_seed(H2))
    join, h, hs, cs = _forward(rp, indptr, L, Gr.shape[0], Gr, b, w)
    dG, db, dw = join.backward(_cuda(Gr), _cuda(b), _cuda(w), hs, cs, _cuda(dh))
    assert torch.equal(dG[0::2], dG[1::2])

    def ref(dtype):
        Gl, bl, wl = (t.to(dtype).requires_grad_() for t in (Gr, b, w))
        hl, _ = lstm_steps(Gl, bl, wl, rp, indptr, L)
        (hl[:, -1] * dh.to(dtype)).sum().backward()
        return hl[:, -1].detach(), Gl.grad[0::2], bl.grad, wl.grad
    r64, r32 = ref(torch.float64), ref(torch.float32)
    _within_yardstick(h, r64[0], r32[0], "h")
    _rows_within_yardstick(dG[0::2], r64[1], r32[1], "dgates")
    _within_yardstick(db, r64[2], r32[2], "db")
    _within_yardstick(dw, r64[3], r32[3], "dW_hh")
    first = r64[1][indptr[[3, 20]]].abs().max()                     # step 0's dgates of the two segments of L rows
    assert float(first) >= 1e-3 * float(r64[1].abs().max())


# ----------------------------------------------------------------------------------------------- dG's order, bit for bit
def _ordered_dg(flat, D, T, piece=1024):
    """dG in the header's fp32 order: each index's entries as a stable sort of the flat indices lists them, cut into pieces of `piece`
    consecutive entries each summed from 0 in order, then the pieces summed from 0 in order; D [R, 4H'] the rows' dgates"""
    perm = np.argsort(flat, kind="stable")
    rows, srt = perm // 2, flat[perm]
    out = np.zeros((T, D.shape[1]), np.float32)
    for r in range(T):
        mine = rows[srt == r]
        total = np.zeros(D.shape[1], np.float32)
        for k in range(0, len(mine), piece):
            acc = np.zeros(D.shape[1], np.float32)
            for j in mine[k:k + piece]:
                acc = acc + D[j]
            total = total + acc
        out[r] = total
    return out


def _dg_bits(H2, counts, T, fill, seed):
    """index 1 + i on exactly counts[i] entries, `fill` more (an even total) on indices 9 .. T-2, none on 0, 8 and T-1; the shared run's
    dG against _ordered_dg of the per-row run's dgates, bit for bit"""
    rng = np.random.default_rng(seed)
    flat = np.concatenate([np.full(c, 1 + i) for i, c in enumerate(counts)] + [rng.integers(9, T - 1, fill)])
    flat = rng.permutation(flat[: len(flat) - len(flat) % 2])
    R = len(flat) // 2
    lens = []
    while sum(lens) < R:
        lens.append(min(int(rng.integers(1, 49)), R - sum(lens)))
    pairs = torch.from_numpy(flat.reshape(R, 2).astype(np.int32))
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    L = max(lens)
    G, b, w = _inputs(H2, T, long=True, seed=seed)
    dh = torch.randn((len(lens), H2), generator=torch.Generator().manual_seed(seed))
    join, h, hs, cs = _forward(pairs, indptr, L, T, G, b, w)
    dG = join.backward(_cuda(G), _cuda(b), _cuda(w), hs, cs, _cuda(dh))[0].cpu().numpy()
    rp, Gr = _per_row(pairs, G)
    jr, hr, hsr, csr = _forward(rp, indptr, L, 2 * R, Gr, b, w)
    assert torch.equal(hsr, hs) and torch.equal(csr, cs)                # the same floats through the recurrence
    D = jr.backward(_cuda(Gr), _cuda(b), _cuda(w), hsr, csr, _cuda(dh))[0][0::2].cpu().numpy()
    want = _ordered_dg(flat, D, T)
    bad = np.nonzero((dG.view(np.int32) != want.view(np.int32)).any(1))[0]
    assert bad.size == 0, f"dG rows {bad.tolist()} (counts {np.bincount(flat, minlength=T)[bad].tolist()}) differ from the ordered sum"
    return dG, flat


@pytest.mark.parametrize("H2", (16, 80, 128))
def test_dg_sums_every_index_in_the_documented_order_bit_for_bit(sp, H2):
    """one index on exactly 1, 1023, 1024, 1025, 2048, 2049 and 3073 entries; indices no entry uses get rows of exact zeros"""
    T = 16
    dG, flat = _dg_bits(H2, COUNTS, T, fill=1500, seed=H2)
    assert [int(v) for v in np.bincount(flat, minlength=T)[1:8]] == list(COUNTS)
    for r in (0, 8, T - 1):
        assert not (flat == r).any() and np.array_equal(dG[r].view(np.int32), np.zeros(4 * H2, np.int32))


def test_dg_of_a_one_row_table(sp):
    """T = 1: every entry on index 0, 2,200 of them (three pieces)"""
    rng = np.random.default_rng(4)
    R = 1100
    lens = np.diff(np.concatenate([[0], np.sort(rng.choice(np.arange(1, R), 29, replace=False)), [R]]))
    pairs = torch.zeros((R, 2), dtype=torch.int32)
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    L = int(lens.max())
    G, b, w = _inputs(32, 1, long=True, seed=4)
    dh = torch.randn((len(lens), 32), generator=torch.Generator().manual_seed(4))
    join, h, hs, cs = _forward(pairs, indptr, L, 1, G, b, w)
    dG = join.backward(_cuda(G), _cuda(b), _cuda(w), hs, cs, _cuda(dh))[0].cpu().numpy()
    rp, Gr = _per_row(pairs, G)
    jr, hr, hsr, csr = _forward(rp, indptr, L, 2 * R, Gr, b, w)
    D = jr.backward(_cuda(Gr), _cuda(b), _cuda(w), hsr, csr, _cuda(dh))[0][0::2].cpu().numpy()
    assert np.array_equal(dG.view(np.int32), _ordered_dg(np.zeros(2 * R, np.int64), D, 1).view(np.int32))


# --------------------------------------------------------------------------------- long memory, end to end (index_lstm_stage)
def _store(sp, N, E, walks, seed):
    ptr_, idx = sym_graph(N, E, seed=seed, hubs=1)
    z, sets = sp.sample_spg(sp.DeviceCSR(ptr_, idx), np.arange(N), num_walks=walks, num_steps=3, seed=5, rng="philox")
    return z, sets.feature_table()


@pytest.fixture(scope="module")
def long_store(sp):
    """100 walks per root: the longest joined segments run to a few hundred rows"""
    return _store(sp, 2000, 9000, walks=100, seed=8)


@pytest.fixture(scope="module")
def large_store(sp):
    return _store(sp, 20000, 120000, walks=100, seed=13)


def _long_nets(H2, k, H=32):
    """(fp32 CPU, fp32 device, float64 device) copies of one (embed, lstm): default init, FORGET and INPUT added to bias_hh's forget-
    and input-gate slices"""
    torch.manual_seed(H2)
    nets = [torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)), torch.nn.LSTM(H, H2, batch_first=True)]
    with torch.no_grad():
        nets[1].bias_hh_l0[H2:2 * H2] += FORGET
        nets[1].bias_hh_l0[:H2] += INPUT
    return nets, [copy.deepcopy(m).cuda() for m in nets], [copy.deepcopy(m).double().cuda() for m in nets]


def _reference_form(nets, xz, ind, L):
    """model.py:78-83: pe_embedding(xz).sum(-2), to_dense_batch to L steps, the LSTM's output at position L-1"""
    embed, lstm = nets
    return lstm(dense_batch(embed(xz).sum(dim=-2), ind, L))[0][:, -1]


def _step0_matters(f64, xz, ind, L, segs):
    """zeroing step 0's input row of the segments `segs` moves their float64 output by >= 1e-3 of its largest entry"""
    with torch.no_grad():
        x = dense_batch(f64[0](xz.double()).sum(dim=-2), ind, L)[segs]
        x0 = x.clone()
        x0[:, 0] = 0
        o, o0 = (f64[1](v)[0][:, -1] for v in (x, x0))
    assert float((o0 - o).abs().max()) >= 1e-3 * float(o.abs().max())


def _sub(pairs, ind, segs):
    """the rows of the segments `segs`: (pairs, indptr) of those segments alone"""
    ind = ind.cpu()
    rows = torch.cat([torch.arange(int(ind[j]), int(ind[j + 1])) for j in segs.tolist()])
    lens = (ind[1:] - ind[:-1])[segs]
    return pairs.cpu()[rows], torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]), rows


@pytest.mark.parametrize("H2", WIDTHS)
def test_long_memory_end_to_end(sp, long_store, H2):
    """index_lstm_stage in the long-memory regime on segments of up to a few hundred rows: the output and every parameter gradient against the float64
    reference form, within FACTOR times CPU fp32's error on the same; step 0 of the longest segments moves the output"""
    z, table = long_store
    edge = torch.from_numpy(np.random.default_rng(12).integers(0, 2000, (2, 24))).cuda()
    xz, ind = sp.gather(edge, z, "cuda", ptr=True, encode=table)
    lens = ind[1:] - ind[:-1]
    L = int(lens.max())
    assert 100 < L <= 400
    cpu, gpu, f64 = _long_nets(H2, table.shape[1])
    out = sp.index_lstm_stage(edge, z, table, *gpu).view(-1, H2)
    t64 = _reference_form(f64, xz.double(), ind, L)
    t32 = _reference_form(cpu, xz.float().cpu(), ind.cpu(), L)
    _within_yardstick(out, t64, t32, "output")
    w = torch.randn(t64.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(H2))
    (out * w.float().cuda()).sum().backward()
    (t64 * w.cuda()).sum().backward()
    (t32 * w.float()).sum().backward()
    for (n, pa), p64, p32 in zip([(n, p) for m in gpu for n, p in m.named_parameters()], [p for m in f64 for p in m.parameters()],
                                 [p for m in cpu for p in m.parameters()]):
        _within_yardstick(pa.grad, p64.grad, p32.grad, n)
    _step0_matters(f64, xz, ind, L, torch.argsort(lens, descending=True)[:4])


# ------------------------------------------------------------------------------------------------------------ large batches
def _sample(lens, L, n, seed):
    """n random segments and up to n of those with at least L - 16 rows"""
    rng = np.random.default_rng(seed)
    longs = torch.nonzero(lens >= L - 16).view(-1).cpu().numpy()
    return torch.from_numpy(np.unique(np.concatenate([rng.choice(lens.numel(), n, replace=False), longs[:n]])))


def test_a_large_batch_in_the_long_memory_regime(sp, large_store):
    """B = 65,536 under no_grad in the long-memory regime; 64 random segments and the longest ones against the float64 reference form"""
    z, table = large_store
    edge = torch.from_numpy(np.random.default_rng(7).integers(0, 20000, (2, 65536))).cuda()
    cpu, gpu, f64 = _long_nets(32, table.shape[1])
    with torch.no_grad():
        out = sp.index_lstm_stage(edge, z, table, *gpu).view(-1, 32)
        pairs, ind = sp.gather_index(edge, z)
        lens = ind[1:] - ind[:-1]
        L = int(lens.max())
        assert L > 100
        pick = _sample(lens, L, 64, 8)
        sp_pairs, sp_ind, _ = _sub(pairs, ind, pick)
        xz = table.cpu()[sp_pairs.long()]
        t64 = _reference_form(f64, xz.double().cuda(), sp_ind.cuda(), L)
        t32 = _reference_form(cpu, xz.float(), sp_ind, L)
    _within_yardstick(out[pick.cuda()], t64, t32, "h_{L-1} of the sampled segments")
    _step0_matters(f64, xz.cuda(), sp_ind.cuda(), L, torch.argsort(sp_ind[1:] - sp_ind[:-1], descending=True)[:4])


def test_the_backward_of_a_large_batch(sp, large_store):
    """B = 4,096 in the long-memory regime and L > 100: every parameter gradient against the float64 reference form, and the dgates of every row of
    a sample of segments (the backward's ws_rows) against float64 autograd"""
    from surel_plus_amd.spjoin import _LstmJoin
    z, table = large_store
    edge = torch.from_numpy(np.random.default_rng(17).integers(0, 20000, (2, 4096))).cuda()
    cpu, gpu, f64 = _long_nets(32, table.shape[1])
    out = sp.index_lstm_stage(edge, z, table, *gpu).view(-1, 32)
    xz, ind = sp.gather(edge, z, "cuda", ptr=True, encode=table)
    lens = ind[1:] - ind[:-1]
    L = int(lens.max())
    assert L > 100
    t64 = _reference_form(f64, xz.double(), ind, L)
    t32 = _reference_form(cpu, xz.float().cpu(), ind.cpu(), L)
    del xz
    w = torch.randn(t64.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    (out * w.float().cuda()).sum().backward()
    (t64 * w.cuda()).sum().backward()
    (t32 * w.float()).sum().backward()
    for (n, pa), p64, p32 in zip([(n, p) for m in gpu for n, p in m.named_parameters()], [p for m in f64 for p in m.parameters()],
                                 [p for m in cpu for p in m.parameters()]):
        _within_yardstick(pa.grad, p64.grad, p32.grad, n)
    # the rows' dgates: the library's two calls on the same G, b, W_hh and upstream gradient
    pairs, ind = sp.gather_index(edge, z)
    lstm = gpu[1]
    with torch.no_grad():
        G = (gpu[0](table.float()) @ lstm.weight_ih_l0.t()).contiguous()
        b = (lstm.bias_ih_l0 + lstm.bias_hh_l0).contiguous()
        W = lstm.weight_hh_l0.detach().contiguous()
    join = _LstmJoin(pairs.contiguous(), ind.contiguous(), L, table.shape[0], 32)
    _, hs, cs = join.forward(G, b, W, True)
    rows = torch.empty((pairs.shape[0], 128), device="cuda")
    _backward(join, G, b, W, hs, cs, w.float().contiguous(), rows)
    pick = _sample(lens, L, 24, 9)
    sp_pairs, sp_ind, sel = _sub(pairs, ind, pick)
    rp, Gr = _per_row(sp_pairs, G.detach().cpu())

    def ref(dtype):
        Gl = Gr.to(dtype).requires_grad_()
        hl, _ = lstm_steps(Gl, b.detach().cpu().to(dtype), W.cpu().to(dtype), rp, sp_ind, L)
        (hl[:, -1] * w[pick].to(dtype)).sum().backward()
        return Gl.grad[0::2]
    _rows_within_yardstick(rows[sel.cuda()], ref(torch.float64), ref(torch.float32), "dgates of the sampled rows")

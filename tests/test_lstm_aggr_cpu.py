"""CPU: the argument contract of the LP encoder's first stage with LSTM aggregation folded into one recurrent kernel
(subgacc_lstm_aggr / subgacc_lstm_aggr_backward, spjoin.index_lstm_stage) -- what the library refuses before it launches anything, what
index_lstm_stage refuses before any device work -- and the identity the kernel rests on, restated in float64 over the golden LP join
against nn.LSTM on the padded dense batch.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NAMES = ("subgacc_lstm_aggr", "subgacc_lstm_aggr_backward")
# argument names in signature order; ints are the accepted values, None marks a pointer
_ARGS = {
    NAMES[0]: ("pairs", "indptr", "S", "L", "T", "H", "G", "b", "w_hh", "out_h", "h_state", "c_state", "flags"),
    NAMES[1]: ("pairs", "indptr", "S", "L", "T", "H", "G", "b", "w_hh", "h_state", "c_state", "dh", "order", "piece_off", "n_pieces",
               "run_piece", "ws_rows", "ws_pieces", "out_dg", "out_dw", "out_db", "flags"),
}
_INTS = dict(S=4, L=3, T=16, H=32, n_pieces=2)


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_lstm_aggr_is_exported_at_abi_7(L):
    from surel_plus_amd import _lib
    for name in NAMES:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert L.subgacc_abi_version() == 7


def _call(L, name, change):
    """call `name` with accepted arguments, one change applied -- its pointers are host memory, so it is only ever passed with a change
    the library refuses; (status, message)"""
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    args = {k: _INTS.get(k, here) for k in _ARGS[name]}
    args.update(change)
    rc = getattr(L, name)(*[args[k] for k in _ARGS[name]], None)
    return rc, L.subgacc_last_error()


_COMMON = [
    (dict(S=-1), b"S = -1"),
    (dict(L=0), b"L = 0"),
    (dict(L=-3), b"L = -3"),
    (dict(H=8), b"multiple of 16"),
    (dict(H=100), b"multiple of 16"),
    (dict(H=144), b"multiple of 16"),
    (dict(H=0), b"multiple of 16"),
    (dict(T=0), b"T = 0"),
    (dict(pairs=None), b"are required"),
    (dict(indptr=None), b"are required"),
    (dict(G=None), b"are required"),
    (dict(w_hh=None), b"are required"),
    (dict(flags=None), b"are required"),
]


@pytest.mark.parametrize("change,cause", _COMMON + [
    (dict(out_h=None), b"out_h is required"),
    (dict(h_state=None), b"h_state and c_state go together"),
    (dict(c_state=None), b"h_state and c_state go together"),
])
def test_lstm_aggr_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[0], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"lstm_aggr: ") and cause in msg, msg


@pytest.mark.parametrize("change,cause", _COMMON + [
    (dict({k: None}), b"are required") for k in ("h_state", "c_state", "dh", "order", "piece_off", "run_piece", "ws_rows", "out_dg",
                                                 "out_dw", "out_db")
] + [(dict(ws_pieces=None), b"ws_pieces required"), (dict(n_pieces=-1), b"n_pieces = -1")])
def test_lstm_aggr_backward_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[1], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"lstm_aggr_backward: ") and cause in msg, msg


def test_l_may_be_zero_only_for_an_empty_batch(L):
    """the forward of S = 0 segments with L = 0 is accepted (nothing to run, nothing launched); S > 0 with L = 0 is refused by both"""
    rc, _ = _call(L, NAMES[0], dict(S=0, L=0))
    assert rc == 0
    for name in NAMES:
        rc, msg = _call(L, name, dict(S=1, L=0))
        assert rc != 0 and b"L = 0" in msg


# --------------------------------------------------------------------------------------------- refusals of index_lstm_stage
def _lp_spg():
    from surel_plus_amd.spg import SpG
    return SpG(torch.tensor([0, 2, 3]), torch.tensor([0, 1, 1], dtype=torch.int32), torch.tensor([1, 2, 3], dtype=torch.int32))


@pytest.fixture
def no_device(monkeypatch):
    """index_lstm_stage with every device path disabled: a refusal must come first"""
    import surel_plus_amd as sp
    from surel_plus_amd import spjoin

    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(spjoin, "gather_index", boom)
    monkeypatch.setattr(spjoin, "lib", boom)
    return sp


E = np.zeros((2, 1), np.int64)


def _embed():
    return torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, 16))


@pytest.mark.parametrize("lstm,exc", [
    (lambda: torch.nn.LSTM(16, 16, batch_first=True, num_layers=2), ValueError),
    (lambda: torch.nn.LSTM(16, 16, batch_first=False), ValueError),
    (lambda: torch.nn.LSTM(16, 16, batch_first=True, bidirectional=True), ValueError),
    (lambda: torch.nn.LSTM(16, 32, batch_first=True, proj_size=16), ValueError),
    (lambda: torch.nn.LSTM(16, 100, batch_first=True), ValueError),
    (lambda: torch.nn.LSTM(16, 144, batch_first=True), ValueError),
    (lambda: torch.nn.LSTM(16, 16, batch_first=True).double(), ValueError),
    (lambda: torch.nn.GRU(16, 16, batch_first=True), TypeError),
    (lambda: torch.nn.Linear(16, 16), TypeError),
])
def test_index_lstm_stage_refuses_other_lstms(no_device, lstm, exc):
    with pytest.raises(exc, match="lstm_stage"):
        no_device.index_lstm_stage(E, _lp_spg(), torch.zeros((4, 3)), _embed(), lstm())


def test_index_lstm_stage_refuses_float_stores(no_device):
    from surel_plus_amd.spg import SpG
    f = SpG(torch.tensor([0, 1]), torch.tensor([0], dtype=torch.int32), torch.tensor([0.5], dtype=torch.float64))
    with pytest.raises(TypeError, match="lstm_stage"):
        no_device.index_lstm_stage(E, f, torch.zeros((4, 3)), _embed(), torch.nn.LSTM(16, 16, batch_first=True))
    with pytest.raises(TypeError):
        no_device.index_lstm_stage(E, np.zeros((3, 3)), torch.zeros((4, 3)), _embed(), torch.nn.LSTM(16, 16, batch_first=True))


def test_index_lstm_stage_refuses_a_bad_table_or_edge(no_device):
    lstm = torch.nn.LSTM(16, 16, batch_first=True)
    with pytest.raises(ValueError, match="encode must be the"):
        no_device.index_lstm_stage(E, _lp_spg(), torch.zeros(4), _embed(), lstm)
    with pytest.raises(ValueError, match="edge must be"):
        no_device.index_lstm_stage(np.zeros((3, 2), np.int64), _lp_spg(), torch.zeros((4, 3)), _embed(), lstm)


# ------------------------------------------------------------------------------------------------ the identity, in float64
def _golden_pairs(g):
    """the index pairs (p, q) of gather()'s rows over the golden LP join, checked against the oracle's xz rows"""
    ip, ix, dat, edge = g["z_indptr"], g["z_indices"], g["z_data"], g["edge"]
    own, par = np.concatenate([edge[0], edge[1]]), np.concatenate([edge[1], edge[0]])
    P, Q, seg = [], [], []
    for j, (a, b) in enumerate(zip(own, par)):
        pb = dict(zip(ix[ip[b]:ip[b + 1]].tolist(), dat[ip[b]:ip[b + 1]].tolist()))
        for t in np.argsort(ix[ip[a]:ip[a + 1]], kind="stable"):
            P.append(int(dat[ip[a] + t]))
            Q.append(pb.get(int(ix[ip[a] + t]), 0))
            seg.append(j)
    P, Q, seg = np.array(P), np.array(Q), np.array(seg)
    np.testing.assert_array_equal(np.stack([g["encode"][P], g["encode"][Q]], 1), g["xz_ptr1"])
    np.testing.assert_array_equal(np.bincount(seg, minlength=len(own)), np.diff(g["ind_ptr1"]))
    return P, Q, len(own)


@pytest.mark.parametrize("golden", ["sjoin_int.npz", "sjoin_int_emptyrows.npz"])
@pytest.mark.parametrize("bias", [True, False])
def test_table_folded_recurrence_equals_nn_lstm_on_the_padded_batch(golden, bias):
    """gates_t = (G[p_t] + G[q_t]) + b + W_hh h_{t-1} with G = E W_ih^T, zero input (b alone) for n_j <= t < L, unrolled by hand in the
    kernel's order (include/subgacc.h), equals nn.LSTM on the zero-padded dense batch of pe_embedding(xz).sum(-2) at position L-1"""
    g = np.load(f"{GOLDEN}/{golden}")
    P, Q, S = _golden_pairs(g)
    ind = g["ind_ptr1"].astype(np.int64)
    lens = np.diff(ind)
    Lmax = max(int(lens.max()), 1)
    H, H2 = 12, 16
    torch.manual_seed(0)
    embed = torch.nn.Sequential(torch.nn.Linear(3, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).double()
    lstm = torch.nn.LSTM(H, H2, batch_first=True, bias=bias).double()
    with torch.no_grad():
        x = embed(torch.from_numpy(g["xz_ptr1"].astype(np.float64))).sum(dim=-2)
        dense = x.new_zeros((S, Lmax, H))
        for j in range(S):
            dense[j, :lens[j]] = x[ind[j]:ind[j + 1]]
        truth = lstm(dense)[0][:, -1].numpy()
        E = embed(torch.from_numpy(g["encode"].astype(np.float64))).numpy()
    Wih, Whh = lstm.weight_ih_l0.detach().numpy(), lstm.weight_hh_l0.detach().numpy()
    b = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().numpy() if bias else np.zeros(4 * H2)
    G = E @ Wih.T
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))           # noqa: E731
    out = np.zeros((S, H2))
    for j in range(S):
        h, c = np.zeros(H2), np.zeros(H2)
        for t in range(Lmax):
            r = ind[j] + t
            a = ((G[P[r]] + G[Q[r]]) if t < lens[j] else np.zeros(4 * H2)) + b
            a = a + Whh @ h
            i, f, gg, o = sig(a[:H2]), sig(a[H2:2 * H2]), np.tanh(a[2 * H2:3 * H2]), sig(a[3 * H2:])
            c = f * c + i * gg
            h = o * np.tanh(c)
        out[j] = h
    np.testing.assert_allclose(out, truth, rtol=0, atol=1e-12)


# ----------------------------------------------------------------- the step reference the GPU tests compare against, pinned
@pytest.mark.parametrize("bias,forget,pad", [(True, 0.0, 0), (True, 5.0, 0), (False, 0.0, 6), (True, 0.0, 7)])
def test_step_reference_equals_nn_lstm_on_the_padded_batch(bias, forget, pad):
    """gpu_helpers.lstm_steps over the index form equals float64 nn.LSTM on the zero-padded dense batch of G rows: the whole h trajectory
    and the final c within 1e-12, with segments of 0, 1 and L rows, L past the longest segment, and a long-memory forget bias"""
    from gpu_helpers import dense_batch, lstm_steps
    rng = np.random.default_rng(int(forget) + pad)
    lens = np.array([0, 1, 23, 5, 0, 17, 23, 2, 9, 11, 1, 20, 3])
    T, H, H2 = 9, 6, 16
    L = int(lens.max()) + pad
    indptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]))
    pairs = torch.from_numpy(rng.integers(0, T, (int(indptr[-1]), 2)).astype(np.int32))
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(H, H2, batch_first=True, bias=bias).double()
    E = torch.randn((T, H), dtype=torch.float64)
    with torch.no_grad():
        if bias:
            lstm.bias_hh_l0[H2:2 * H2] += forget
        dense = dense_batch(E[pairs[:, 0].long()] + E[pairs[:, 1].long()], indptr, L)
        out, (_, c_n) = lstm(dense)
        G = E @ lstm.weight_ih_l0.t()
        b = (lstm.bias_ih_l0 + lstm.bias_hh_l0) if bias else None
        hs, cs = lstm_steps(G, b, lstm.weight_hh_l0, pairs, indptr, L)
    assert hs.shape == cs.shape == (len(lens), L, H2)
    torch.testing.assert_close(hs, out, rtol=0, atol=1e-12)
    torch.testing.assert_close(cs[:, -1], c_n[0], rtol=0, atol=1e-12)


def test_step_reference_runs_l_steps_of_a_longer_segment():
    """a segment longer than L runs its first L rows: the same trajectory as the segment cut to L rows"""
    from gpu_helpers import lstm_steps
    rng = np.random.default_rng(1)
    G, w, b = torch.from_numpy(rng.standard_normal((5, 32))), torch.from_numpy(rng.standard_normal((32, 8))) / 4, None
    pairs = torch.from_numpy(rng.integers(0, 5, (30, 2)).astype(np.int32))
    full = lstm_steps(G, b, w, pairs, torch.tensor([0, 12, 30]), 10)
    cut = lstm_steps(G, b, w, torch.cat([pairs[:10], pairs[12:22]]), torch.tensor([0, 10, 20]), 10)
    assert all(torch.equal(a, c) for a, c in zip(full, cut))


# ------------------------------------------------------------------------------------ dG's ordered sum: grouping()'s pieces
@pytest.mark.parametrize("counts", [(1, 1023, 1024, 1025, 2048, 2049, 3073), (2200,), (0, 1024, 0, 1)])
def test_grouping_cuts_every_index_run_into_pieces_of_at_most_1024_in_order(counts):
    """order lists the row of every (row, side) entry of a stable sort of the 2R indices; pieces cover it in sequence, each inside one
    index's run, every piece but an index's last full (1024 entries), ceil(count / 1024) pieces per index, run_piece their ranges"""
    from surel_plus_amd.spjoin import _LSTM_PIECE, _LstmJoin
    assert _LSTM_PIECE == 1024
    T = len(counts) + 2                                       # the first and the last index are used by no entry
    flat = np.concatenate([np.full(c, 1 + i) for i, c in enumerate(counts)])
    flat = np.random.default_rng(len(flat)).permutation(np.concatenate([flat, np.ones(len(flat) % 2, flat.dtype)]))
    cnt = np.bincount(flat, minlength=T)
    pairs = torch.from_numpy(flat.reshape(-1, 2).astype(np.int32))
    join = _LstmJoin(pairs, torch.tensor([0, pairs.shape[0]]), 1, T, 16)
    order, piece_off, P, run_piece = (v.numpy() if torch.is_tensor(v) else v for v in join.grouping())
    perm = np.argsort(flat, kind="stable")
    np.testing.assert_array_equal(order, perm // 2)
    start = np.concatenate([[0], np.cumsum(cnt)])
    npc = -(-cnt // 1024)
    assert P == npc.sum() and len(piece_off) == P + 1 and piece_off[0] == 0 and piece_off[-1] == len(flat)
    np.testing.assert_array_equal(run_piece, np.concatenate([[0], np.cumsum(npc)]))
    for r in range(T):
        cuts = piece_off[run_piece[r]:run_piece[r + 1] + 1]
        if cnt[r] == 0:
            assert run_piece[r] == run_piece[r + 1]
            continue
        assert cuts[0] == start[r] and cuts[-1] == start[r + 1]
        np.testing.assert_array_equal(cuts[:-1], start[r] + 1024 * np.arange(npc[r]))
        assert np.all(np.diff(cuts) >= 1) and np.all(np.diff(cuts) <= 1024)

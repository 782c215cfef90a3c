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

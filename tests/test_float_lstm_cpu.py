"""CPU: the argument contract of the float encoders' first stage with LSTM aggregation in the recurrent kernel (subgacc_lstm_aggr_hinge /
subgacc_lstm_aggr_hinge_backward, spjoin.float_lstm_stage) -- what the library refuses before it launches anything, what float_lstm_stage
refuses before any device work --, the table builder (spjoin.hinge_tables) against direct evaluation, and the identity the kernel rests
on, restated in float64 over the golden float join against nn.LSTM on the padded dense batch.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

NAMES = ("subgacc_lstm_aggr_hinge", "subgacc_lstm_aggr_hinge_backward")
# argument names in signature order; ints are the accepted values, None marks a pointer
_ARGS = {
    NAMES[0]: ("vals", "idx", "indptr", "S", "L", "K", "H", "tab", "c_real", "c_pad", "w_hh", "out_h", "h_state", "c_state", "flags"),
    NAMES[1]: ("vals", "idx", "indptr", "S", "L", "K", "H", "tab", "c_real", "c_pad", "w_hh", "h_state", "c_state", "dh", "order",
               "piece_off", "n_pieces", "run_piece", "ws_rows", "ws_pieces", "out_dp", "out_dq", "out_dw", "out_dc_real", "out_dc_pad",
               "flags"),
}
_INTS = dict(S=4, L=3, K=33, H=32, n_pieces=2)


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_the_hinge_entry_points_are_declared_bound_and_exported_at_abi_7(L):
    from surel_plus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "subgacc.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert L.subgacc_abi_version() == 7


def _call(L, name, change):
    """call `name` with accepted arguments, one change applied -- its pointers are host memory, so it is only ever passed with a change
    the library refuses (or with S = 0, where nothing is launched); (status, message)"""
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    args = {k: _INTS.get(k, here) for k in _ARGS[name]}
    for k, v in change.items():
        args[k] = here + 4 if v == "odd" else v
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
    (dict(K=0), b"K = 0"),
    (dict(K=-2), b"K = -2"),
    (dict(vals=None), b"are required"),
    (dict(idx=None), b"are required"),
    (dict(indptr=None), b"are required"),
    (dict(tab=None), b"are required"),
    (dict(w_hh=None), b"are required"),
    (dict(flags=None), b"are required"),
    (dict(vals="odd"), b"8-byte"),
    (dict(idx="odd"), b"8-byte"),
    (dict(tab="odd"), b"8-byte"),
]


@pytest.mark.parametrize("change,cause", _COMMON + [
    (dict(out_h=None), b"out_h is required"),
    (dict(h_state=None), b"h_state and c_state go together"),
    (dict(c_state=None), b"h_state and c_state go together"),
])
def test_hinge_forward_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[0], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"lstm_aggr_hinge: ") and cause in msg, msg


@pytest.mark.parametrize("change,cause", _COMMON + [
    (dict({k: None}), b"are required") for k in ("h_state", "c_state", "dh", "order", "piece_off", "run_piece", "ws_rows", "out_dp",
                                                 "out_dq", "out_dw", "out_dc_real", "out_dc_pad")
] + [(dict(ws_pieces=None), b"ws_pieces required"), (dict(n_pieces=-1), b"n_pieces = -1")])
def test_hinge_backward_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[1], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"lstm_aggr_hinge_backward: ") and cause in msg, msg


def test_l_may_be_zero_only_for_an_empty_batch(L):
    """the forward of S = 0 segments with L = 0 is accepted (nothing launched), the biases may be NULL; S > 0 with L = 0 is refused"""
    rc, _ = _call(L, NAMES[0], dict(S=0, L=0, c_real=None, c_pad=None))
    assert rc == 0
    for name in NAMES:
        rc, msg = _call(L, name, dict(S=1, L=0))
        assert rc != 0 and b"L = 0" in msg


# --------------------------------------------------------------------------------------------- refusals of float_lstm_stage
@pytest.fixture
def no_device(monkeypatch):
    """every path from float_lstm_stage to the library or a device raises"""
    from surel_plus_amd import _lib, spjoin

    def device_work(*a, **k):
        raise AssertionError("device work before the argument check")
    for name in ("lib", "join_fill", "stream_ptr", "check", "ptr", "_as_rows", "_as_spg", "_seg_and_flags", "sjoin", "gather"):
        monkeypatch.setattr(spjoin, name, device_work)
    for name in ("lib", "join_desc", "join_fill", "stream_ptr"):
        monkeypatch.setattr(_lib, name, device_work)
    return spjoin


def _mlp(d_in=1, H=8, act=torch.nn.ReLU, H1=16):
    return torch.nn.Sequential(torch.nn.Linear(d_in, H), act(), torch.nn.Linear(H, H1))


def _lstm(H1=16, H2=16, **kw):
    return torch.nn.LSTM(H1, H2, **{"batch_first": True, **kw})


def _float_spg(dtype=torch.float64):
    from surel_plus_amd.spg import SpG
    indptr = torch.tensor([0, 2, 3, 3], dtype=torch.int64)
    data = torch.tensor([0.5, 0.25, 1.0], dtype=dtype) if dtype == torch.float64 else torch.tensor([1, 2, 1], dtype=torch.int32)
    return SpG(indptr, torch.tensor([0, 2, 1], dtype=torch.int32), data, max_len=2)


E = np.zeros((2, 3), np.int64)


def test_float_lstm_stage_is_exported():
    import surel_plus_amd as sp
    assert callable(sp.float_lstm_stage) and callable(sp.hinge_tables)


def test_float_lstm_stage_refuses_an_integer_store_and_a_non_store(no_device):
    with pytest.raises(TypeError, match="index_lstm_stage"):
        no_device.float_lstm_stage(E, _float_spg(torch.int32), _mlp(), _lstm())
    with pytest.raises(TypeError, match="float_lstm_stage"):
        no_device.float_lstm_stage(E, np.zeros((3, 3)), _mlp(), _lstm())


def test_float_lstm_stage_refuses_a_strided_store(no_device):
    from types import SimpleNamespace
    from surel_plus_amd.spg import StridedSpG
    n, pitch = 3, 32
    ids = torch.zeros(n * pitch, dtype=torch.int32)
    sets = SimpleNamespace(strided=True, ids=ids, slot=ids.clone(), nsize=torch.zeros(n, dtype=torch.int32), stride=pitch, table=None,
                           capacity=0, num_walks=8, num_steps=2)
    with pytest.raises(TypeError, match="StridedSpG"):
        no_device.float_lstm_stage(E, StridedSpG(sets, 10), _mlp(), _lstm())


@pytest.mark.parametrize("embed", [
    _mlp(d_in=2),
    _mlp(act=torch.nn.Tanh),
    torch.nn.Linear(1, 8),
    torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.ReLU(), torch.nn.Linear(8, 16), torch.nn.ReLU()),
])
def test_float_lstm_stage_refuses_other_embed_modules(no_device, embed):
    with pytest.raises(TypeError, match="gather") as e:
        no_device.float_lstm_stage(E, _float_spg(), embed, _lstm())
    assert "float_lstm_stage" in str(e.value) and "Sequential(Linear(1, H), ReLU(), Linear(H, H'))" in str(e.value)


def test_float_lstm_stage_refuses_h_beyond_the_kernel(no_device):
    with pytest.raises(ValueError, match="1 <= H <= 1024"):
        no_device.float_lstm_stage(E, _float_spg(), _mlp(H=1025), _lstm())


@pytest.mark.parametrize("lstm,exc", [
    (lambda: _lstm(num_layers=2), ValueError),
    (lambda: _lstm(batch_first=False), ValueError),
    (lambda: _lstm(bidirectional=True), ValueError),
    (lambda: _lstm(16, 32, proj_size=16), ValueError),
    (lambda: _lstm(16, 100), ValueError),
    (lambda: _lstm(16, 144), ValueError),
    (lambda: _lstm().double(), ValueError),
    (lambda: torch.nn.GRU(16, 16, batch_first=True), TypeError),
    (lambda: torch.nn.Linear(16, 16), TypeError),
    (lambda: _lstm(24, 16), ValueError),                    # input_size != H1
])
def test_float_lstm_stage_refuses_other_lstms(no_device, lstm, exc):
    with pytest.raises(exc, match=r"gather\(edge, x\)") as e:
        no_device.float_lstm_stage(E, _float_spg(), _mlp(), lstm())
    assert "float_lstm_stage" in str(e.value)


@pytest.mark.parametrize("edge", [
    np.zeros((3, 4), np.int64),
    np.zeros(4, np.int64),
    np.zeros((2, 4), np.float32),
    torch.zeros((2, 4), dtype=torch.float64),
    torch.zeros((2, 4), dtype=torch.bool),
    [[0, 1, 2], [0, 1]],
])
def test_float_lstm_stage_refuses_a_malformed_edge(no_device, edge):
    with pytest.raises(ValueError, match=r"float_lstm_stage: edge must be a \[2, B\] integer"):
        no_device.float_lstm_stage(edge, _float_spg(), _mlp(), _lstm())


def test_index_lstm_stage_points_a_float_store_to_float_lstm_stage(no_device):
    with pytest.raises(TypeError, match="float_lstm_stage"):
        no_device.index_lstm_stage(E, _float_spg(), torch.zeros((4, 3)), _mlp(3), _lstm())


# --------------------------------------------------------------------------------------------------- the table builder
def _net(w1, b1, H1=5, H2=16, seed=0):
    """(lin1, lin2, W_ih) in float64 with Linear(1, H)'s weight and bias set to w1, b1 (b1 None: no biases anywhere)"""
    torch.manual_seed(seed)
    H = len(w1)
    lin1 = torch.nn.Linear(1, H, bias=b1 is not None).double()
    lin2 = torch.nn.Linear(H, H1, bias=b1 is not None).double()
    with torch.no_grad():
        lin1.weight.copy_(torch.tensor(w1, dtype=torch.float64).view(-1, 1))
        if b1 is not None:
            lin1.bias.copy_(torch.tensor(b1, dtype=torch.float64))
    return lin1, lin2, torch.randn(4 * H2, H1, dtype=torch.float64)


_TABLE_NETS = {
    "generic": ([0.7, -1.3, 2.0, -0.4, 1.1], [0.2, 0.5, -1.0, -0.3, 0.0]),
    "dead channels of each bias sign": ([0.7, 0.0, -1.3, 0.0, 0.0], [0.2, 0.9, 0.5, -0.9, 0.0]),
    "duplicate knots": ([1.0, 2.0, -1.0, -3.0, 0.5], [-0.5, -1.0, 0.5, 1.5, 0.3]),
    "H = 1": ([-0.8], [0.4]),
    "no biases": ([0.7, -1.3, 2.0], None),
}


@pytest.mark.parametrize("which", sorted(_TABLE_NETS))
def test_hinge_tables_equal_direct_evaluation(which):
    """P[k(s)] s + Q[k(s)] == V relu(w1 s + b1) in float64 inside every interval, beyond both ends and exactly on every knot, within
    1e-12 of the largest entry (measured: 1.1e-15); k(s) = hinge_intervals(s, knots), the rule of include/subgacc.h (2r behind r knots,
    2r - 1 on a knot)"""
    from surel_plus_amd.spjoin import hinge_intervals, hinge_tables
    w1, b1 = _TABLE_NETS[which]
    lin1, lin2, w_ih = _net(w1, b1)
    with torch.no_grad():
        knots, P, Q, c_real, c_pad = hinge_tables(lin1, lin2, w_ih)
        H = len(w1)
        assert knots.shape == (H,) and P.shape == Q.shape == (2 * H + 1, w_ih.shape[0]) and c_pad is None
        assert bool((knots[1:] >= knots[:-1]).all())
        fin = knots[torch.isfinite(knots)]
        pts = [fin] if fin.numel() else []
        edges = torch.cat([fin[:1] - 3.0, fin, fin[-1:] + 3.0]) if fin.numel() else torch.tensor([-1.0, 1.0], dtype=torch.float64)
        pts += [(edges[1:] + edges[:-1]) / 2, edges[:1] - 100.0, edges[-1:] + 100.0, torch.zeros(1, dtype=torch.float64)]
        s = torch.cat(pts)
        k = hinge_intervals(s, knots)
        assert int(k.min()) >= 0 and int(k.max()) <= 2 * H
        assert bool((k[:fin.numel()] % 2 == 1).all()) and bool((k[-3:-1] % 2 == 0).all())     # on a knot: odd; beyond the ends: even
        got = P[k] * s[:, None] + Q[k]
        want = torch.relu(lin1(s[:, None])) @ (w_ih @ lin2.weight).t()
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
        if b1 is not None:
            torch.testing.assert_close(c_real, w_ih @ (2 * lin2.bias), rtol=0, atol=1e-14)
        else:
            assert c_real is None


# ------------------------------------------------------------------------------------------------ the identity, in float64
def _reference(xz, ind, L_, embed, lstm):
    x = embed(xz).sum(dim=-2)
    S = len(ind) - 1
    dense = x.new_zeros((S, L_, x.shape[-1]))
    for j in range(S):
        dense = dense.index_put((torch.full((int(ind[j + 1] - ind[j]),), j), torch.arange(int(ind[j + 1] - ind[j]))), x[ind[j]:ind[j + 1]])
    return lstm(dense)[0][:, -1]


def _table_form(xz, ind, L_, embed, lstm):
    """the recurrence unrolled in the order of include/subgacc.h: ((P[ka] a + Q[ka]) + (P[kb] b + Q[kb])) + c_real on a real step,
    c_pad on a padded one, then + W_hh h_{t-1}; torch ops, so autograd goes through the tables"""
    from surel_plus_amd.spjoin import hinge_intervals, hinge_tables
    bias = lstm.bias
    knots, P, Q, c_real, c_pad = hinge_tables(embed[0], embed[2], lstm.weight_ih_l0, lstm.bias_ih_l0 if bias else None,
                                              lstm.bias_hh_l0 if bias else None)
    a, b = xz[:, 0, 0], xz[:, 1, 0]
    ka, kb = hinge_intervals(a, knots), hinge_intervals(b, knots)
    gin = (P[ka] * a[:, None] + Q[ka]) + (P[kb] * b[:, None] + Q[kb])
    if c_real is not None:
        gin = gin + c_real
    S, H2 = len(ind) - 1, lstm.hidden_size
    lens = ind[1:] - ind[:-1]
    W = lstm.weight_hh_l0
    h, c = gin.new_zeros((S, H2)), gin.new_zeros((S, H2))
    pad = c_pad if c_pad is not None else gin.new_zeros(4 * H2)
    for t in range(L_):
        real = lens > t
        r = torch.where(real, ind[:-1] + t, torch.zeros_like(lens))
        g = torch.where(real[:, None], gin[r], pad.expand(S, -1)) + h @ W.t()
        i, f, gg, o = g.split(H2, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
    return h


@pytest.mark.parametrize("bias", [True, False])
def test_table_form_equals_nn_lstm_on_the_padded_batch_of_the_golden_join(bias):
    """over tests/golden/sjoin_float.npz (128 segments of 1-25 rows), float64: the forward within 1e-12 (measured on synthetic rows:
    6e-16), every parameter's gradient through the table form within 1e-9 of the largest entry of the reference form's (2.3e-15)"""
    g = np.load(f"{GOLDEN}/sjoin_float.npz")
    xz = torch.from_numpy(g["xz_ptr1"].astype(np.float64))
    ind = torch.from_numpy(g["ind_ptr1"].astype(np.int64))
    L_ = max(int((ind[1:] - ind[:-1]).max()), 1)
    H, H1, H2 = 24, 12, 16

    def nets():
        torch.manual_seed(5)
        embed = torch.nn.Sequential(torch.nn.Linear(1, H, bias=bias), torch.nn.ReLU(), torch.nn.Linear(H, H1, bias=bias)).double()
        lstm = torch.nn.LSTM(H1, H2, batch_first=True, bias=bias).double()
        with torch.no_grad():                   # the golden scores are small: spread the knots over them
            embed[0].weight.mul_(40.0)
        return embed, lstm
    ra, rb = nets(), nets()
    want, got = _reference(xz, ind, L_, *ra), _table_form(xz, ind, L_, *rb)
    assert float((got - want).detach().abs().max()) <= 1e-12
    w =torch.from_numpy(np.random.default_rng(2).standard_normal(tuple(want.shape)))
    (want * w).sum().backward()
    (got * w).sum().backward()
    for (n, pa), (_, pb) in zip([(n, p) for m in ra for n, p in m.named_parameters()], [(n, p) for m in rb for n, p in m.named_parameters()]):
        assert pb.grad is not None, n
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-9 * max(float(pa.grad.abs().max()), 1e-30), n

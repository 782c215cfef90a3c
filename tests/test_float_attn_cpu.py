"""CPU: the argument contract of the fused first model stage of the float encoders with attentional aggregation
(subgacc_sjoin_relu_attn / subgacc_sjoin_relu_attn_backward, spjoin.float_attn_stage) -- what the library refuses before it launches
anything, what float_attn_stage refuses before any device work -- and the identity the stage rests on, restated in NumPy over the golden
float join against torch autograd of the reference form.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_relu_attn_is_exported_at_abi_7(L):
    from surel_plus_amd import _lib
    for name in ("subgacc_sjoin_relu_attn", "subgacc_sjoin_relu_attn_backward"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert L.subgacc_abi_version() == 7


def _desc(here):
    """a mirrored F64 descriptor over packed rows that the library accepts up to its launch: B = 2 pairs (S = 4).  It is only ever
    passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_F64
    d.row_off, d.n_rows, d.max_len, d.S, d.pair_block = here, 4, 4, 4, 2
    d.ids = d.payload = d.own = d.flags = here
    return d


_DESC_REFUSALS = [
    (dict(payload_kind=0), b"F64"),                                        # SFPTR
    (dict(payload_kind=2), b"F64"),                                        # 32-bit keys
    (dict(row_off=None, row_len="here", row_stride=32), b"strided"),
    (dict(form=1), b"form"),
    (dict(form=2), b"form"),
    (dict(options=1), b"options"),                                         # OPT_SIZES
    (dict(options=2), b"options"),                                         # OPT_STAR
    (dict(pair_block=0), b"pair_block"),
    (dict(pair_block=-2), b"pair_block"),
    (dict(S=6), b"multiple of 2*pair_block"),
    (dict(own=None), b"own = NULL"),
    (dict(H=0), b"H = 0"),
    (dict(H=1025), b"H = 1025"),
    (dict(out_xz="here"), b"out_* and seg"),
    (dict(out_idx="here"), b"out_* and seg"),
    (dict(out_segid="here"), b"out_* and seg"),
    (dict(out_counts="here"), b"out_* and seg"),
    (dict(out_pairs="here"), b"out_* and seg"),
    (dict(out_mult="here"), b"out_* and seg"),
    (dict(out_cnt="here"), b"out_* and seg"),
    (dict(out_seg="here"), b"out_* and seg"),
    (dict(seg="here"), b"out_* and seg"),
    (dict(row_off=None, row_stride=9024), b"do not fit LDS"),             # headed rows the row form refuses too
]


def _call(L, name, change):
    """call `name` with the accepted descriptor and arguments, one change applied; (status, message)"""
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    if name == "subgacc_sjoin_relu_attn":
        keys = ("w1", "b1", "u", "H", "out_a", "out_max", "out_den")
    else:
        keys = ("w1", "b1", "u", "H", "g", "a", "max", "den", "out_dw", "out_db", "out_du")
    args = {k: (96 if k == "H" else here) for k in keys}
    for k, val in change.items():
        val = here if val == "here" else val
        if k in args:
            args[k] = val
        else:
            setattr(d, k, val)
    rc = getattr(L, name)(C.byref(d), *[args[k] for k in keys], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,cause", _DESC_REFUSALS + [
    (dict(w1=None), b"w1, b1, u and out_a"),
    (dict(b1=None), b"w1, b1, u and out_a"),
    (dict(u=None), b"w1, b1, u and out_a"),
    (dict(out_a=None), b"w1, b1, u and out_a"),
    (dict(out_max=None), b"out_max and out_den"),
    (dict(out_den=None), b"out_max and out_den"),
])
def test_relu_attn_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, "subgacc_sjoin_relu_attn", change)
    assert rc == _lib.ERR_BADARG
    assert b"sjoin_relu_attn:" in msg and cause in msg, msg


@pytest.mark.parametrize("change,cause", _DESC_REFUSALS + [
    (dict({k: None}), b"are required") for k in ("w1", "b1", "u", "g", "a", "max", "den", "out_dw", "out_db", "out_du")
])
def test_relu_attn_backward_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, "subgacc_sjoin_relu_attn_backward", change)
    assert rc == _lib.ERR_BADARG
    assert b"sjoin_relu_attn_backward:" in msg and cause in msg, msg


def test_relu_attn_refuses_a_foreign_descriptor(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    d.struct_bytes = 8
    assert L.subgacc_sjoin_relu_attn(C.byref(d), here, here, here, 96, here, None, None, None) == _lib.ERR_BADARG
    assert b"struct_bytes" in L.subgacc_last_error()
    assert L.subgacc_sjoin_relu_attn(None, here, here, here, 96, here, None, None, None) == _lib.ERR_BADARG
    assert L.subgacc_sjoin_relu_attn_backward(None, *([here] * 3), 96, *([here] * 7), None) == _lib.ERR_BADARG


def test_relu_mean_keeps_its_own_name_in_shared_refusals(L):
    """the checks shared with subgacc_sjoin_relu_attn still name sjoin_relu_mean"""
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    d.payload_kind = 0
    assert L.subgacc_sjoin_relu_mean(C.byref(d), here, here, 96, here, None, None, None) == _lib.ERR_BADARG
    assert L.subgacc_last_error().startswith(b"sjoin_relu_mean: ")


# ------------------------------------------------------------------------------------------------ float_attn_stage's refusals
@pytest.fixture
def no_device(monkeypatch):
    """every path from float_attn_stage to the library or a device raises"""
    from surel_plus_amd import _lib, spjoin

    def device_work(*a, **k):
        raise AssertionError("device work before the argument check")
    for name in ("lib", "join_fill", "stream_ptr", "check", "ptr", "_as_rows", "_as_spg", "_seg_and_flags", "sjoin", "gather"):
        monkeypatch.setattr(spjoin, name, device_work)
    for name in ("lib", "join_desc", "join_fill", "stream_ptr"):
        monkeypatch.setattr(_lib, name, device_work)
    return spjoin


def _mlp(d_in=1, H=8, act=torch.nn.ReLU, H2=4):
    return torch.nn.Sequential(torch.nn.Linear(d_in, H), act(), torch.nn.Linear(H, H2))


def _gate(H2=4):
    return torch.nn.Linear(H2, 1)


def _float_spg(dtype=torch.float64):
    from surel_plus_amd.spg import SpG
    indptr = torch.tensor([0, 2, 3, 3], dtype=torch.int64)
    data = torch.tensor([0.5, 0.25, 1.0], dtype=dtype) if dtype == torch.float64 else torch.tensor([1, 2, 1], dtype=torch.int32)
    return SpG(indptr, torch.tensor([0, 2, 1], dtype=torch.int32), data, max_len=2)


E = np.zeros((2, 3), np.int64)


def test_float_attn_stage_refuses_an_integer_store(no_device):
    with pytest.raises(TypeError, match="attn_stage"):
        no_device.float_attn_stage(E, _float_spg(torch.int32), _mlp(), _gate())


def test_float_attn_stage_refuses_a_strided_store(no_device):
    from types import SimpleNamespace
    from surel_plus_amd.spg import StridedSpG
    n, pitch = 3, 32
    ids = torch.zeros(n * pitch, dtype=torch.int32)
    sets = SimpleNamespace(strided=True, ids=ids, slot=ids.clone(), nsize=torch.zeros(n, dtype=torch.int32), stride=pitch, table=None,
                           capacity=0, num_walks=8, num_steps=2)
    with pytest.raises(TypeError, match="StridedSpG"):
        no_device.float_attn_stage(E, StridedSpG(sets, 10), _mlp(), _gate())


@pytest.mark.parametrize("embed", [
    _mlp(d_in=2),                                                   # Linear(2, H): not the float encoders' input_dim = 1
    _mlp(act=torch.nn.Tanh),                                        # another activation
    torch.nn.Linear(1, 8),                                          # not the three-layer MLP
    torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.ReLU(), torch.nn.Linear(8, 4), torch.nn.ReLU()),
])
def test_float_attn_stage_refuses_other_embed_modules(no_device, embed):
    with pytest.raises(TypeError, match="gather") as e:
        no_device.float_attn_stage(E, _float_spg(), embed, _gate())
    assert "float_attn_stage" in str(e.value) and "Sequential(Linear(1, H), ReLU(), Linear(H, H'))" in str(e.value)


@pytest.mark.parametrize("gate,value", [
    (torch.nn.Linear(4, 2), None),                                              # a gate of two outputs
    (torch.nn.Linear(5, 1), None),                                              # not H' inputs
    (torch.nn.Sequential(torch.nn.Linear(4, 1), torch.nn.Sigmoid()), None),     # more than one Linear
    (torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.ReLU(), torch.nn.Linear(4, 1)), None),
    (torch.nn.Identity(), None),
    (_gate(), torch.nn.Linear(5, 4)),                                           # a value net of other inputs
    (_gate(), torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.ReLU())),    # PyG's MLP with an activation is not one Linear
    (_gate(), torch.nn.Bilinear(4, 4, 4)),
])
def test_float_attn_stage_refuses_other_gate_and_value_modules(no_device, gate, value):
    with pytest.raises(TypeError, match="gather") as e:
        no_device.float_attn_stage(E, _float_spg(), _mlp(), gate, value)
    assert "float_attn_stage" in str(e.value)


@pytest.mark.parametrize("edge", [
    np.zeros((3, 4), np.int64),                 # not [2, B]
    np.zeros(4, np.int64),                      # 1-D
    np.zeros((2, 4), np.float32),               # float rows
    torch.zeros((2, 4), dtype=torch.float64),
    torch.zeros((2, 4), dtype=torch.bool),
    [[0, 1, 2], [0, 1]],                        # ragged
])
def test_float_attn_stage_refuses_a_malformed_edge(no_device, edge):
    with pytest.raises(ValueError, match=r"float_attn_stage: edge must be a \[2, B\] integer"):
        no_device.float_attn_stage(edge, _float_spg(), _mlp(), _gate())


def test_float_attn_stage_refuses_h_beyond_the_kernel(no_device):
    with pytest.raises(ValueError, match="1 <= H <= 1024"):
        no_device.float_attn_stage(E, _float_spg(), _mlp(H=1025), _gate())


# ------------------------------------------------------------------------------------------------ the identity, in NumPy
def _reference_form(xz, ind, embed, gate, val):
    """model.py:59-62,78-81 in torch float64 on the full xz: pe_embedding(xz).sum(-2), then AttentionalAggregation as PyG 2.2 computes
    it (softmax: exp(g - max) / (sum + 1e-16) per segment, then the weighted segment sum of nn(x))"""
    S = len(ind) - 1
    x = embed(xz).sum(dim=-2)
    seg = torch.repeat_interleave(torch.arange(S), torch.diff(ind))
    g = gate(x).reshape(-1)
    gmax = torch.full((S,), float("-inf"), dtype=g.dtype).scatter_reduce(0, seg, g.detach(), "amax")
    w = torch.exp(g - gmax[seg])
    den = torch.zeros(S, dtype=g.dtype).index_add_(0, seg, w)
    alpha = w / (den[seg] + 1e-16)
    v = val(x) if val is not None else x
    return torch.zeros((S, v.shape[-1]), dtype=g.dtype).index_add_(0, seg, alpha[:, None] * v)


@pytest.mark.parametrize("with_value", [False, True])
def test_restated_stage_equals_the_reference_form_on_the_golden_join(with_value):
    """out_j = (nn(W2 A_j + 2 b2)) [n_j > 0] with A_j = sum_t softmax_j(u . r)_t r_t, u = W2^T wg, and the backward sums of the header
    (dL/du = sum beta r, dL/dw1 = sum dr (a [ya > 0] + b [yb > 0]), dL/db1 = sum dr ([ya > 0] + [yb > 0])), in NumPy float64 over the
    reference's own xz / indptr of tests/golden/sjoin_float.npz, against torch autograd of the reference form"""
    g = np.load(f"{GOLDEN}/sjoin_float.npz")
    xz, ind = g["xz_ptr1"].astype(np.float64), g["ind_ptr1"].astype(np.int64)
    S = len(ind) - 1
    n = np.diff(ind)
    assert n.min() > 0
    H, H2, H3 = 96, 24, 12
    torch.manual_seed(0)
    embed = torch.nn.Sequential(torch.nn.Linear(1, H), torch.nn.ReLU(), torch.nn.Linear(H, H2)).double()
    gate = torch.nn.Linear(H2, 1).double()
    val = torch.nn.Linear(H2, H3).double() if with_value else None
    with torch.no_grad():                      # scores of the golden join are small: spread the pre-activations over both signs
        embed[0].weight.mul_(40.0)
        gate.weight.mul_(10.0)
    ref = _reference_form(torch.from_numpy(xz), torch.from_numpy(ind), embed, gate, val)
    Wt = np.random.default_rng(1).standard_normal(tuple(ref.shape))
    (ref * torch.from_numpy(Wt)).sum().backward()

    w1, b1 = embed[0].weight.detach().numpy().reshape(-1), embed[0].bias.detach().numpy()
    W2, b2 = embed[2].weight.detach().numpy(), embed[2].bias.detach().numpy()
    wg = gate.weight.detach().numpy().reshape(-1)
    segid = np.repeat(np.arange(S), n)
    ya, yb = xz[:, 0, :] * w1 + b1, xz[:, 1, :] * w1 + b1                 # [R, H]
    r = np.maximum(ya, 0) + np.maximum(yb, 0)
    u = W2.T @ wg
    l = r @ u
    m = np.full(S, -np.inf)
    np.maximum.at(m, segid, l)
    e = np.exp(l - m[segid])
    den = np.zeros(S)
    np.add.at(den, segid, e)
    alpha = e / den[segid]
    A = np.zeros((S, H))
    np.add.at(A, segid, alpha[:, None] * r)
    h = A @ W2.T + 2 * b2
    if with_value:
        Wf, bf = val.weight.detach().numpy(), val.bias.detach().numpy()
        h = h @ Wf.T + bf
    out = h * (n > 0)[:, None]
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-10, atol=1e-12)

    # the backward: G = dL/dA through the affine tail, then the three per-segment sums of the header, summed over the segments
    Gh = Wt * (n > 0)[:, None]
    if with_value:
        Gh = Gh @ Wf
    G = Gh @ W2                                                            # [S, H]
    beta = alpha * ((G[segid] * r).sum(1) - (G * A).sum(1)[segid])
    dr = alpha[:, None] * G[segid] + beta[:, None] * u
    du = (beta[:, None] * r).sum(0)
    dw1 = (dr * (xz[:, 0, :] * (ya > 0) + xz[:, 1, :] * (yb > 0))).sum(0)
    db1 = (dr * ((ya > 0) * 1.0 + (yb > 0))).sum(0)
    np.testing.assert_allclose(dw1, embed[0].weight.grad.numpy().reshape(-1), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(db1, embed[0].bias.grad.numpy(), rtol=1e-9, atol=1e-10)
    # torch's gate weight gradient is W2 du (the constant 2 b2 . wg + bg drops out of the softmax) and its bias gradient is zero
    np.testing.assert_allclose(W2 @ du, gate.weight.grad.numpy().reshape(-1), rtol=1e-9, atol=1e-10)
    assert abs(float(gate.bias.grad)) < 1e-10

"""CPU: the argument contract of the fused first model stage of the float encoders (subgacc_sjoin_relu_mean, spjoin.float_mean_stage)
-- what the library refuses before it launches anything, what float_mean_stage refuses before any device work -- and the identity the
stage rests on, restated in NumPy over the golden float join.  No GPU needed."""
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


def test_relu_mean_is_exported_at_abi_7(L):
    from surel_plus_amd import _lib
    assert "subgacc_sjoin_relu_mean" in _lib.SYMBOLS
    assert hasattr(L, "subgacc_sjoin_relu_mean")
    assert L.subgacc_abi_version() == 7


def _mean_desc(here):
    """a mirrored F64 descriptor over packed rows that the library accepts up to its launch: B = 2 pairs (S = 4).  It is only ever
    passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_F64
    d.row_off, d.n_rows, d.max_len, d.S, d.pair_block = here, 4, 4, 4, 2
    d.ids = d.payload = d.own = d.flags = here
    return d


@pytest.mark.parametrize("change,cause", [
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
    (dict(w1=None), b"w1, b1 and out_mean"),
    (dict(b1=None), b"w1, b1 and out_mean"),
    (dict(out_mean=None), b"w1, b1 and out_mean"),
    (dict(H=0), b"H = 0"),
    (dict(H=1025), b"H = 1025"),
    (dict(out_p=None), b"out_p and out_q"),
    (dict(out_q=None), b"out_p and out_q"),
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
])
def test_relu_mean_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _mean_desc(here)
    args = dict(w1=here, b1=here, H=96, out_mean=here, out_p=here, out_q=here)
    for name, val in change.items():
        val = here if val == "here" else val
        if name in args:
            args[name] = val
        else:
            setattr(d, name, val)
    rc = L.subgacc_sjoin_relu_mean(C.byref(d), args["w1"], args["b1"], args["H"], args["out_mean"], args["out_p"], args["out_q"], None)
    assert rc == _lib.ERR_BADARG
    msg = L.subgacc_last_error()
    assert b"sjoin_relu_mean" in msg and cause in msg, msg


def test_relu_mean_refuses_a_foreign_descriptor(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _mean_desc(here)
    d.struct_bytes = 8
    assert L.subgacc_sjoin_relu_mean(C.byref(d), here, here, 96, here, None, None, None) == _lib.ERR_BADARG
    assert b"struct_bytes" in L.subgacc_last_error()
    assert L.subgacc_sjoin_relu_mean(None, here, here, 96, here, None, None, None) == _lib.ERR_BADARG


# ------------------------------------------------------------------------------------------------ float_mean_stage's refusals
@pytest.fixture
def no_device(monkeypatch):
    """every path from float_mean_stage to the library or a device raises"""
    from surel_plus_amd import _lib, spjoin

    def device_work(*a, **k):
        raise AssertionError("device work before the argument check")
    for name in ("lib", "join_fill", "stream_ptr", "check", "ptr", "_as_rows", "_as_spg", "_seg_and_flags", "sjoin", "gather"):
        monkeypatch.setattr(spjoin, name, device_work)
    for name in ("lib", "join_desc", "join_fill", "stream_ptr"):
        monkeypatch.setattr(_lib, name, device_work)
    return spjoin


def _mlp(d_in=1, H=8, act=torch.nn.ReLU):
    return torch.nn.Sequential(torch.nn.Linear(d_in, H), act(), torch.nn.Linear(H, 4))


def _float_spg(dtype=torch.float64):
    from surel_plus_amd.spg import SpG
    indptr = torch.tensor([0, 2, 3, 3], dtype=torch.int64)
    data = torch.tensor([0.5, 0.25, 1.0], dtype=dtype) if dtype == torch.float64 else torch.tensor([1, 2, 1], dtype=torch.int32)
    return SpG(indptr, torch.tensor([0, 2, 1], dtype=torch.int32), data, max_len=2)


def test_float_mean_stage_refuses_an_integer_store(no_device):
    with pytest.raises(TypeError, match="mean_stage"):
        no_device.float_mean_stage(np.zeros((2, 3), np.int64), _float_spg(torch.int32), _mlp())


def test_float_mean_stage_refuses_a_strided_store(no_device):
    from types import SimpleNamespace
    from surel_plus_amd.spg import StridedSpG
    n, pitch = 3, 32
    ids = torch.zeros(n * pitch, dtype=torch.int32)
    sets = SimpleNamespace(strided=True, ids=ids, slot=ids.clone(), nsize=torch.zeros(n, dtype=torch.int32), stride=pitch, table=None,
                           capacity=0, num_walks=8, num_steps=2)
    with pytest.raises(TypeError, match="StridedSpG"):
        no_device.float_mean_stage(np.zeros((2, 3), np.int64), StridedSpG(sets, 10), _mlp())


@pytest.mark.parametrize("embed", [
    _mlp(d_in=2),                                                   # Linear(2, H): not the float encoders' input_dim = 1
    _mlp(act=torch.nn.Tanh),                                        # another activation
    torch.nn.Linear(1, 8),                                          # not the three-layer MLP
    torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.ReLU()),
    torch.nn.Sequential(torch.nn.Linear(1, 8), torch.nn.ReLU(), torch.nn.Linear(8, 4), torch.nn.ReLU()),
])
def test_float_mean_stage_refuses_other_modules(no_device, embed):
    with pytest.raises(TypeError, match="gather") as e:
        no_device.float_mean_stage(np.zeros((2, 3), np.int64), _float_spg(), embed)
    assert "Sequential(Linear(1, H), ReLU(), Linear(H, H'))" in str(e.value)


@pytest.mark.parametrize("edge", [
    np.zeros((3, 4), np.int64),                 # not [2, B]
    np.zeros(4, np.int64),                      # 1-D
    np.zeros((2, 4), np.float32),               # float rows
    torch.zeros((2, 4), dtype=torch.float64),
    torch.zeros((2, 4), dtype=torch.bool),
    [[0, 1, 2], [0, 1]],                        # ragged
])
def test_float_mean_stage_refuses_a_malformed_edge(no_device, edge):
    with pytest.raises(ValueError, match=r"\[2, B\] integer"):
        no_device.float_mean_stage(edge, _float_spg(), _mlp())


def test_float_mean_stage_refuses_h_beyond_the_kernel(no_device):
    with pytest.raises(ValueError, match="1 <= H <= 1024"):
        no_device.float_mean_stage(np.zeros((2, 3), np.int64), _float_spg(), _mlp(H=1025))


# ------------------------------------------------------------------------------------------------ the identity, in NumPy
def test_restated_stage_equals_the_reference_form_on_the_golden_join():
    """W2 M_j + 2 b2 (M_j = the mean over segment j's rows of relu(w1 a + b1) + relu(w1 b + b1)) == pe_embedding(xz).sum(-2) followed by
    the segment mean, over the reference's own xz / indptr of tests/golden/sjoin_float.npz (model.py:78-83), in float64"""
    g = np.load(f"{GOLDEN}/sjoin_float.npz")
    xz, ind = g["xz_ptr1"].astype(np.float64), g["ind_ptr1"]
    S, R = len(ind) - 1, xz.shape[0]
    n = np.diff(ind)
    assert n.max() > 0
    rng = np.random.default_rng(0)
    H, H2 = 96, 24
    w1, b1 = rng.standard_normal(H), rng.standard_normal(H) * 0.3
    W2, b2 = rng.standard_normal((H2, H)), rng.standard_normal(H2)
    segid = np.repeat(np.arange(S), n)
    # the reference form: x = pe(xz).sum(-2) over [R, 2, H'], then MeanAggregation(x, ptr) (empty segments: zero rows)
    pe = np.maximum(xz * w1 + b1, 0) @ W2.T + b2                   # [R, 2, H']
    x = pe.sum(axis=-2)
    ref = np.zeros((S, H2))
    np.add.at(ref, segid, x)
    ref /= np.maximum(n, 1)[:, None]
    # the restatement: per segment an H-vector M, one [S, H] x [H, H'] product
    act = np.maximum(xz[:, 0, :] * w1 + b1, 0) + np.maximum(xz[:, 1, :] * w1 + b1, 0)      # [R, H]
    M = np.zeros((S, H))
    np.add.at(M, segid, act)
    M /= np.maximum(n, 1)[:, None]
    out = (M @ W2.T + 2 * b2) * (n > 0)[:, None]
    assert R == ind[-1]
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12)
    # and the backward sums of the header: dL/dw1 = sum_j G_j P_j, dL/db1 = sum_j G_j Q_j for L = sum(out * Wt), G = dL/dM
    Wt = rng.standard_normal((S, H2))
    G = (Wt * (n > 0)[:, None]) @ W2
    mask_a, mask_b = (xz[:, 0, :] * w1 + b1) > 0, (xz[:, 1, :] * w1 + b1) > 0
    P, Q = np.zeros((S, H)), np.zeros((S, H))
    np.add.at(P, segid, xz[:, 0, :] * mask_a + xz[:, 1, :] * mask_b)
    np.add.at(Q, segid, mask_a * 1.0 + mask_b)
    P /= np.maximum(n, 1)[:, None]
    Q /= np.maximum(n, 1)[:, None]
    # the same gradients by the chain rule over the reference form's rows
    Gx = (Wt / np.maximum(n, 1)[:, None])[segid] @ W2                # dL/d(relu output) per row and slot, [R, H]
    gw1 = (Gx * (xz[:, 0, :] * mask_a + xz[:, 1, :] * mask_b)).sum(0)
    gb1 = (Gx * (mask_a * 1.0 + mask_b)).sum(0)
    np.testing.assert_allclose((G * P).sum(0), gw1, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose((G * Q).sum(0), gb1, rtol=1e-10, atol=1e-10)

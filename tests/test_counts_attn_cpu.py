"""CPU: the argument contract of the LP encoder's first stage with attentional aggregation fused with the count form of the join
(subgacc_sjoin_counts_attn / subgacc_sjoin_counts_attn_backward, spjoin.counts_attn_stage) -- what the library refuses before it
launches anything, what counts_attn_stage refuses before any device work -- and the identity the stage rests on, restated in NumPy over
the golden LP join against torch autograd of the reference form.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN

NAMES = ("subgacc_sjoin_counts_attn", "subgacc_sjoin_counts_attn_backward")


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_counts_attn_is_exported_at_abi_7(L):
    from surel_plus_amd import _lib
    for name in NAMES:
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert L.subgacc_abi_version() == 7


def _desc(here):
    """a mirrored count-form descriptor over packed rows that the library accepts up to its launch: B = 2 pairs (S = 4), T = 16.  It is
    only ever passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_COUNTS, _lib.JOIN_SFPTR
    d.row_off, d.n_rows, d.max_len, d.S, d.pair_block, d.table_rows = here, 4, 4, 4, 2, 16
    d.ids = d.payload = d.own = d.flags = here
    return d


_DESC_REFUSALS = [
    (dict(form=0), b"form"),                                               # ROWS
    (dict(form=2), b"form"),                                               # PAIRS
    (dict(options=1), b"options"),                                         # OPT_SIZES
    (dict(options=2), b"options"),                                         # OPT_STAR
    (dict(payload_kind=1), b"SFPTR"),                                      # F64
    (dict(payload_kind=2), b"SFPTR"),                                      # 32-bit keys
    (dict(payload_kind=3), b"SFPTR"),
    (dict(row_off=None, row_stride=32), b"packed rows"),                   # headed rows
    (dict(row_off=None, row_len="here", row_stride=32), b"packed rows"),   # strided rows
    (dict(row_len="here", row_stride=32), b"packed rows"),
    (dict(pair_block=0), b"pair_block"),
    (dict(pair_block=-2), b"pair_block"),
    (dict(S=6), b"multiple of 2*pair_block"),
    (dict(own=None), b"own = NULL"),
    (dict(table_rows=0), b"table_rows"),
    (dict(table_rows=-5), b"table_rows"),
    (dict(out_xz="here"), b"out_* and seg"),
    (dict(out_idx="here"), b"out_* and seg"),
    (dict(out_segid="here"), b"out_* and seg"),
    (dict(out_counts="here"), b"out_* and seg"),
    (dict(out_pairs="here"), b"out_* and seg"),
    (dict(out_mult="here"), b"out_* and seg"),
    (dict(out_cnt="here"), b"out_* and seg"),
    (dict(out_seg="here"), b"out_* and seg"),
    (dict(seg="here"), b"out_* and seg"),
    (dict(flags=None), b"null argument"),
    (dict(ids=None), b"null argument"),
    (dict(payload=None), b"null argument"),
]
_KEYS = {NAMES[0]: ("g", "out_w", "out_max", "out_den"), NAMES[1]: ("g", "dw", "w", "max", "den", "out_dg")}


def _call(L, name, change):
    """call `name` with the accepted descriptor and arguments, one change applied; (status, message)"""
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    args = {k: here for k in _KEYS[name]}
    for k, val in change.items():
        val = here if val == "here" else val
        if k in args:
            args[k] = val
        else:
            setattr(d, k, val)
    rc = getattr(L, name)(C.byref(d), *[args[k] for k in _KEYS[name]], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,cause", _DESC_REFUSALS + [
    (dict(g=None), b"g and out_w"),
    (dict(out_w=None), b"g and out_w"),
    (dict(out_max=None), b"out_max and out_den"),
    (dict(out_den=None), b"out_max and out_den"),
])
def test_counts_attn_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[0], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"sjoin_counts_attn: ") and cause in msg, msg


@pytest.mark.parametrize("change,cause", _DESC_REFUSALS + [
    (dict({k: None}), b"are required") for k in ("g", "dw", "w", "max", "den", "out_dg")
])
def test_counts_attn_backward_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[1], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"sjoin_counts_attn_backward: ") and cause in msg, msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("change", [dict(table_rows=30000), dict(max_len=8000), dict(max_len=2000, table_rows=15000)])
def test_counts_attn_refuses_what_lds_does_not_hold(L, name, change):
    """too many LP rows or too long rows for the kernel's LDS: SUBGACC_ERR_LDS, pointing to the pair form, before any launch"""
    from surel_plus_amd import _lib
    rc, msg = _call(L, name, change)
    assert rc == _lib.ERR_LDS
    assert b"LDS" in msg and b"attn_stage" in msg, msg


@pytest.mark.parametrize("name", NAMES)
def test_counts_attn_refuses_a_forward_whose_backward_lds_does_not_fit(L, name):
    """max_len 1,500 and 10,000 LP rows: the forward needs 4 (7 L + 2 T + 2 D + 8) = 146,032 B, the backward 4 (7 L + 2 T + 6 D + 8) =
    194,032 B of the 160 KiB.  A forward that keeps m / den is followed by the backward, so both refuse with SUBGACC_ERR_LDS before any
    launch -- not the backward alone, in the middle of a training step.  (The forward without out_max / out_den fits and would launch:
    the GPU suite runs it, test_gpu_stage_shapes.py.)"""
    from surel_plus_amd import _lib
    rc, msg = _call(L, name, dict(max_len=1500, table_rows=10000))
    assert rc == _lib.ERR_LDS
    assert b"LDS" in msg and b"attn_stage" in msg and b"194032" in msg, msg


@pytest.mark.parametrize("name", NAMES)
def test_counts_attn_refuses_a_foreign_descriptor(L, name):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    d.struct_bytes = 8
    n = len(_KEYS[name])
    assert getattr(L, name)(C.byref(d), *([here] * n), None) == _lib.ERR_BADARG
    assert b"struct_bytes" in L.subgacc_last_error()
    assert getattr(L, name)(None, *([here] * n), None) == _lib.ERR_BADARG
    assert b"null descriptor" in L.subgacc_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_counts_attn_accepts_an_empty_list_without_a_launch(L, name):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    d.S = 0
    assert getattr(L, name)(C.byref(d), *([here] * len(_KEYS[name])), None) == _lib.OK


# ------------------------------------------------------------------------------------------------ counts_attn_stage's refusals
@pytest.fixture
def no_device(monkeypatch):
    """every path from counts_attn_stage to the library or a device raises"""
    from surel_plus_amd import _lib, spjoin

    def device_work(*a, **k):
        raise AssertionError("device work before the argument check")
    for name in ("lib", "join_fill", "stream_ptr", "check", "ptr", "_as_rows", "_as_spg", "_seg_and_flags", "sjoin", "gather",
                 "gather_pairs", "gather_counts"):
        monkeypatch.setattr(spjoin, name, device_work)
    for name in ("lib", "join_desc", "join_fill", "stream_ptr"):
        monkeypatch.setattr(_lib, name, device_work)
    return spjoin


def _lp_spg(dtype=torch.int32, device="cpu"):
    from surel_plus_amd.spg import SpG
    indptr = torch.tensor([0, 2, 3, 3], dtype=torch.int64, device=device)
    data = torch.tensor([1, 2, 1], dtype=torch.int32, device=device) if dtype == torch.int32 else \
        torch.tensor([0.5, 0.25, 1.0], dtype=dtype, device=device)
    return SpG(indptr, torch.tensor([0, 2, 1], dtype=torch.int32, device=device), data, max_len=2, max_data=2)


E = np.zeros((2, 3), np.int64)
TABLE = torch.zeros((3, 3))


def _embed(H=8):
    return torch.nn.Sequential(torch.nn.Linear(3, H), torch.nn.ReLU(), torch.nn.Linear(H, H))


def test_counts_attn_stage_refuses_a_strided_store(no_device):
    from types import SimpleNamespace
    from surel_plus_amd.spg import StridedSpG
    n, pitch = 3, 32
    ids = torch.zeros(n * pitch, dtype=torch.int32)
    sets = SimpleNamespace(strided=True, ids=ids, slot=ids.clone(), nsize=torch.zeros(n, dtype=torch.int32), stride=pitch, table=None,
                           capacity=0, num_walks=8, num_steps=2)
    with pytest.raises(TypeError, match="counts_attn_stage needs a packed SFptr"):
        no_device.counts_attn_stage(E, StridedSpG(sets, 10), TABLE, _embed(), torch.nn.Linear(8, 1))


def test_counts_attn_stage_refuses_a_headed_store(no_device):
    from surel_plus_amd.spg import HeadedSpG
    z = HeadedSpG(torch.zeros(3 * 32, dtype=torch.int32), torch.zeros(3 * 32, dtype=torch.int32), 32, 3, 2, (3, 3), max_data=2)
    with pytest.raises(ValueError, match="counts_attn_stage joins the packed store"):
        no_device.counts_attn_stage(E, z, TABLE, _embed(), torch.nn.Linear(8, 1))


def test_counts_attn_stage_refuses_a_keyed_store(no_device):
    z = _lp_spg()
    z.keyrows = True
    with pytest.raises(TypeError, match=r"not a keyed\(\) one"):
        no_device.counts_attn_stage(E, z, TABLE, _embed(), torch.nn.Linear(8, 1))


def test_counts_attn_stage_points_a_float_store_to_float_attn_stage(no_device):
    with pytest.raises(TypeError, match="float_attn_stage"):
        no_device.counts_attn_stage(E, _lp_spg(torch.float64), TABLE, _embed(), torch.nn.Linear(8, 1))


def test_counts_attn_stage_refuses_a_scipy_matrix(no_device):
    with pytest.raises(TypeError, match="packed SFptr"):
        no_device.counts_attn_stage(E, np.zeros((3, 3)), TABLE, _embed(), torch.nn.Linear(8, 1))


@pytest.mark.parametrize("gate,value", [
    (torch.nn.Linear(8, 2), None),                                              # a gate of two outputs
    (torch.nn.Sequential(torch.nn.Linear(8, 1), torch.nn.Sigmoid()), None),     # more than one module
    (torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1)), None),
    (torch.nn.Identity(), None),
    (torch.nn.Linear(8, 1), torch.nn.Linear(5, 8)),                            # a value net of other inputs than the gate's
    (torch.nn.Linear(8, 1), torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU())),   # attn_stage's value_nn of the tests
    (torch.nn.Linear(8, 1), torch.nn.Bilinear(8, 8, 8)),
])
def test_counts_attn_stage_points_other_gate_and_value_modules_to_attn_stage(no_device, gate, value):
    with pytest.raises(TypeError, match=r"attn_stage\(edge, x, encode, embed, gate_nn, value_nn\)") as e:
        no_device.counts_attn_stage(E, _lp_spg(), TABLE, _embed(), gate, value)
    assert str(e.value).startswith("counts_attn_stage fuses ")


def test_float_attn_stage_keeps_its_message():
    """_one_linear's stage-name parameter defaults to float_attn_stage's message, word for word"""
    from surel_plus_amd.spjoin import _one_linear
    with pytest.raises(TypeError) as e:
        _one_linear(torch.nn.Identity(), "gate_nn", 4, 1)
    assert str(e.value) == ("float_attn_stage fuses gate_nn = Linear(4, 1) (or a Sequential of that one Linear; PyG's MLP([...]) as its "
                            ".lins[0]) only; for any other module use xz, ind = gather(edge, x) and the modules on xz")


@pytest.mark.parametrize("which", ["gate", "value", "embed"])
def test_counts_attn_stage_refuses_parameters_of_another_dtype(no_device, which):
    gate, val, embed = torch.nn.Linear(8, 1), torch.nn.Linear(8, 4), _embed()
    {"gate": gate, "value": val, "embed": embed}[which].double()
    with pytest.raises(ValueError, match="float32 parameters on the store's device"):
        no_device.counts_attn_stage(E, _lp_spg(), TABLE, embed, gate, val)


def test_counts_attn_stage_refuses_parameters_on_another_device(no_device):
    z = _lp_spg(device="meta")
    with pytest.raises(ValueError, match=r"store's device \(meta\)"):
        no_device.counts_attn_stage(E, z, TABLE, _embed(), torch.nn.Linear(8, 1))


@pytest.mark.parametrize("edge", [
    np.zeros((3, 4), np.int64),                 # not [2, B]
    np.zeros(4, np.int64),                      # 1-D
    np.zeros((2, 4), np.float32),               # float rows
    torch.zeros((2, 4), dtype=torch.bool),
    [[0, 1, 2], [0, 1]],                        # ragged
])
def test_counts_attn_stage_refuses_a_malformed_edge(no_device, edge):
    with pytest.raises(ValueError, match=r"counts_attn_stage: edge must be a \[2, B\] integer"):
        no_device.counts_attn_stage(edge, _lp_spg(), TABLE, _embed(), torch.nn.Linear(8, 1))


@pytest.mark.parametrize("edge", [np.array([[0, 3], [1, 2]]), np.array([[0, 1], [-1, 2]]), torch.tensor([[0, 1], [2, 7]])])
def test_counts_attn_stage_refuses_an_edge_out_of_range(no_device, edge):
    with pytest.raises(IndexError, match="row index out of range for an SpG with 3 rows"):
        no_device.counts_attn_stage(edge, _lp_spg(), TABLE, _embed(), torch.nn.Linear(8, 1))


@pytest.mark.parametrize("table", [torch.zeros(3), torch.zeros((0, 3)), torch.zeros((3, 3), dtype=torch.bool)])
def test_counts_attn_stage_refuses_a_malformed_table(no_device, table):
    with pytest.raises(ValueError, match="encode must be the"):
        no_device.counts_attn_stage(E, _lp_spg(), table, _embed(), torch.nn.Linear(8, 1))


# ------------------------------------------------------------------------------------------------ the identity, in NumPy
def _golden_pairs(g):
    """the index pairs (p, q) of gather()'s rows over tests/golden/sjoin_int.npz: for segment j the members of its own row in ascending
    id order, p = their SFptr+1, q = the partner row's value at the same id or 0 -- checked against the oracle's xz rows"""
    ip, ix, dat, edge = g["z_indptr"], g["z_indices"], g["z_data"], g["edge"]
    own, par = np.concatenate([edge[0], edge[1]]), np.concatenate([edge[1], edge[0]])
    P, Q, seg = [], [], []
    for j, (a, b) in enumerate(zip(own, par)):
        pb = dict(zip(ix[ip[b]:ip[b + 1]].tolist(), dat[ip[b]:ip[b + 1]].tolist()))
        order = np.argsort(ix[ip[a]:ip[a + 1]], kind="stable")
        for t in order:
            P.append(int(dat[ip[a] + t]))
            Q.append(pb.get(int(ix[ip[a] + t]), 0))
            seg.append(j)
    P, Q, seg = np.array(P), np.array(Q), np.array(seg)
    enc = g["encode"]
    np.testing.assert_array_equal(np.stack([enc[P], enc[Q]], 1), g["xz_ptr1"])
    np.testing.assert_array_equal(np.bincount(seg, minlength=len(own)), np.diff(g["ind_ptr1"]))
    return P, Q, seg, len(own)


@pytest.mark.parametrize("golden", ["sjoin_int.npz", "sjoin_int_emptyrows.npz"])
@pytest.mark.parametrize("with_value", [False, True])
def test_restated_stage_equals_the_reference_form_on_the_golden_join(golden, with_value):
    """out_j = nn(W[j] @ E) [n_j > 0] with W the softmax-weighted count rows, and the backward of include/subgacc.h (dW = dA E^T, kappa_j
    = sum_r W dW, beta_t = alpha_t (dW[p_t] + dW[q_t] - kappa_j), dg = sum_j sum_t beta_t ([p_t = r] + [q_t = r])) with the rest by the
    chain rule, in NumPy float64 over the oracle's own join of tests/golden/, against torch autograd of the reference form on its xz"""
    g = np.load(f"{GOLDEN}/{golden}")
    P, Q, segid, S = _golden_pairs(g)
    enc = g["encode"].astype(np.float64)
    T, k = enc.shape
    xz, ind = torch.from_numpy(g["xz_ptr1"].astype(np.float64)), torch.from_numpy(g["ind_ptr1"].astype(np.int64))
    H, H3 = 24, 12
    torch.manual_seed(0)
    embed = torch.nn.Linear(k, H).double()
    gate = torch.nn.Linear(H, 1).double()
    val = torch.nn.Linear(H, H3).double() if with_value else None
    with torch.no_grad():                      # spread the logits over a few units, so that the softmax is far from uniform
        gate.weight.mul_(8.0)
    x = embed(xz).sum(dim=-2)
    seg = torch.repeat_interleave(torch.arange(S), torch.diff(ind))
    gl = gate(x).reshape(-1)
    gmax = torch.full((S,), float("-inf"), dtype=gl.dtype).scatter_reduce(0, seg, gl.detach(), "amax")
    w = torch.exp(gl - gmax[seg])
    den_t = torch.zeros(S, dtype=gl.dtype).index_add_(0, seg, w)
    alpha_t = w / (den_t[seg] + 1e-16)
    v = val(x) if val is not None else x
    ref = torch.zeros((S, v.shape[-1]), dtype=gl.dtype).index_add_(0, seg, alpha_t[:, None] * v)
    Wt = np.random.default_rng(1).standard_normal(tuple(ref.shape))
    (ref * torch.from_numpy(Wt)).sum().backward()

    n = np.bincount(segid, minlength=S)
    Wl, bl = embed.weight.detach().numpy(), embed.bias.detach().numpy()
    wg = gate.weight.detach().numpy().reshape(-1)
    E = enc @ Wl.T + bl                                                   # [T, H]
    gt = E @ wg                                                           # the gate bias dropped
    lo = gt[P] + gt[Q]
    m = np.full(S, -np.inf)
    np.maximum.at(m, segid, lo)
    e = np.exp(lo - m[segid])
    den = np.zeros(S)
    np.add.at(den, segid, e)
    alpha = e / den[segid]
    W = np.zeros((S, T))
    np.add.at(W, (segid, P), alpha)
    np.add.at(W, (segid, Q), alpha)
    nz = n > 0
    np.testing.assert_allclose(W[nz].sum(1), 2.0, rtol=1e-12)
    assert not W[~nz].any()
    h = W @ E
    if with_value:
        Wv, bv = val.weight.detach().numpy(), val.bias.detach().numpy()
        h = h @ Wv.T + bv
    out = h * nz[:, None]
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-10, atol=1e-12)

    Gh = Wt * nz[:, None]
    dA = Gh @ Wv if with_value else Gh
    dW = dA @ E.T                                                         # [S, T]
    kappa = (W * dW).sum(1)
    beta = alpha * (dW[segid, P] + dW[segid, Q] - kappa[segid])
    dg = np.zeros(T)
    np.add.at(dg, P, beta)
    np.add.at(dg, Q, beta)
    dE = W.T @ dA + np.outer(dg, wg)
    np.testing.assert_allclose(dE.T @ enc, embed.weight.grad.numpy(), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(dE.sum(0), embed.bias.grad.numpy(), rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(E.T @ dg, gate.weight.grad.numpy().reshape(-1), rtol=1e-9, atol=1e-10)
    assert abs(float(gate.bias.grad)) < 1e-10
    if with_value:
        np.testing.assert_allclose(Gh.T @ (W @ E), val.weight.grad.numpy(), rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(Gh.sum(0), val.bias.grad.numpy(), rtol=1e-9, atol=1e-10)

"""CPU: the argument contract of the count form over the key rows of an on-demand step -- subgacc_keyrows_columns and
subgacc_sjoin_key_counts refuse every fault before they launch anything, with a message led by their name -- and what
StepBuffers(stage="counts") refuses before it touches a device.  No GPU needed."""
import ctypes as C
from types import SimpleNamespace

import pytest

NAMES = ("subgacc_keyrows_columns_workspace_bytes", "subgacc_keyrows_columns", "subgacc_sjoin_key_counts")


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_step_stage_entry_points_are_exported_at_abi_7(L):
    import re
    import os
    from surel_plus_amd import _lib
    txt = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "subgacc.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, txt)
    assert L.subgacc_abi_version() == 7
    assert C.sizeof(_lib.JoinDesc) == 248          # subgacc_join_desc keeps its layout


# ------------------------------------------------------------------------------------------------------ subgacc_keyrows_columns
def test_columns_workspace_is_the_set_of_keys(L):
    """a power of two >= 2 T words, at least 1,024; 0 for a T the call refuses"""
    assert L.subgacc_keyrows_columns_workspace_bytes(2) == 4 * 1024
    assert L.subgacc_keyrows_columns_workspace_bytes(512) == 4 * 1024
    assert L.subgacc_keyrows_columns_workspace_bytes(513) == 4 * 2048
    assert L.subgacc_keyrows_columns_workspace_bytes(2048) == 4 * 4096
    assert L.subgacc_keyrows_columns_workspace_bytes(16384) == 4 * 32768
    assert L.subgacc_keyrows_columns_workspace_bytes(16385) == 0
    assert L.subgacc_keyrows_columns_workspace_bytes(1) == 0


_COL_KEYS = ("row_keys", "nsize", "n", "stride", "num_walks", "num_steps", "table_rows", "out_ukeys", "out_count", "out_feat", "flags",
             "workspace", "workspace_bytes")


def _columns(L, **change):
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    a = dict(row_keys=here, nsize=here, n=4, stride=32, num_walks=200, num_steps=3, table_rows=16, out_ukeys=here, out_count=here,
             out_feat=here, flags=here, workspace=here, workspace_bytes=4096)
    a.update(change)
    rc = L.subgacc_keyrows_columns(*[a[k] for k in _COL_KEYS], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,status,cause", [
    (dict(table_rows=1), "ERR_BADARG", b"table_rows"),
    (dict(table_rows=0), "ERR_BADARG", b"table_rows"),
    (dict(table_rows=-3), "ERR_BADARG", b"table_rows"),
    (dict(table_rows=16385, workspace_bytes=1 << 20), "ERR_LDS", b"LDS"),
    (dict(n=-1), "ERR_BADARG", b"bad sizes"),
    (dict(stride=0), "ERR_BADARG", b"bad sizes"),
    (dict(stride=-32), "ERR_BADARG", b"bad sizes"),
    (dict(num_walks=0), "ERR_BADARG", b"num_walks"),
    (dict(num_steps=0), "ERR_BADARG", b"num_walks"),
    (dict(num_walks=200, num_steps=4), "ERR_BADARG", b"33 bits"),           # the paper's citation2 setting: a 64-bit key
    (dict(out_ukeys=None), "ERR_BADARG", b"null argument"),
    (dict(out_count=None), "ERR_BADARG", b"null argument"),
    (dict(out_feat=None), "ERR_BADARG", b"null argument"),
    (dict(flags=None), "ERR_BADARG", b"null argument"),
    (dict(workspace=None), "ERR_BADARG", b"null argument"),
    (dict(row_keys=None), "ERR_BADARG", b"null argument"),
    (dict(nsize=None), "ERR_BADARG", b"null argument"),
    (dict(workspace_bytes=4095), "ERR_WORKSPACE", b"workspace"),
    (dict(table_rows=2048), "ERR_WORKSPACE", b"16384 needed"),
])
def test_columns_refuses_before_any_launch(L, change, status, cause):
    from surel_plus_amd import _lib
    rc, msg = _columns(L, **change)
    assert rc == getattr(_lib, status)
    assert msg.startswith(b"keyrows_columns: ") and cause in msg, msg


def test_columns_refuses_a_key_that_has_no_width(L):
    """M*m+1 bits beyond 64: the status and message of subgacc_key_shift, as every entry point that takes (num_walks, num_steps)"""
    from surel_plus_amd import _lib
    rc, _ = _columns(L, num_walks=1 << 20, num_steps=4)
    assert rc == _lib.ERR_KEYWIDTH


# ----------------------------------------------------------------------------------------------------- subgacc_sjoin_key_counts
def _desc(here):
    """a mirrored descriptor over strided key rows that the library accepts up to its launch: B = 2 pairs (S = 4), T = 16.  It is only
    ever passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_COUNTS, _lib.JOIN_KEY32
    d.row_len, d.row_stride, d.n_rows, d.S, d.pair_block, d.table_rows = here, 32, 4, 4, 2, 16
    d.num_walks, d.num_steps = 200, 3
    d.ids = d.payload = d.own = d.flags = here
    return d


_KC_KEYS = ("ukeys", "n_keys", "out_counts", "out_len")


def _key_counts(L, change):
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    args = {k: here for k in _KC_KEYS}
    for k, val in change.items():
        val = here if val == "here" else val
        if k in args:
            args[k] = val
        else:
            setattr(d, k[2:] if k.startswith("d.") else k, val)      # "d.out_counts": the descriptor's field, not the argument
    rc = L.subgacc_sjoin_key_counts(C.byref(d), *[args[k] for k in _KC_KEYS], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,cause", [
    (dict(options=1), b"option"),                                           # OPT_SIZES
    (dict(options=2), b"option"),                                           # OPT_STAR
    (dict(payload_kind=0), b"KEY32"),                                       # SFptr
    (dict(payload_kind=1), b"KEY32"),                                       # F64
    (dict(payload_kind=3), b"KEY32"),                                       # 64-bit keys
    (dict(row_len=None, row_off="here"), b"strided key rows"),              # packed rows
    (dict(row_len=None), b"strided key rows"),                              # headed rows
    (dict(row_off="here"), b"exactly one of"),
    (dict(row_stride=0), b"row_stride"),
    (dict(row_stride=1 << 31), b"row_stride"),
    (dict(S=-4), b"none may be negative"),
    (dict(n_rows=-1), b"none may be negative"),
    (dict(pair_block=0), b"pair_block"),
    (dict(pair_block=-2), b"pair_block"),
    (dict(S=6), b"multiple of 2*pair_block"),
    (dict(own=None), b"own = NULL"),
    (dict(table_rows=1), b"table_rows"),
    (dict(table_rows=0), b"table_rows"),
    (dict(table_rows=-5), b"table_rows"),
    (dict(out_xz="here"), b"out_* and seg"),
    (dict(out_idx="here"), b"out_* and seg"),
    (dict(out_segid="here"), b"out_* and seg"),
    ({"d.out_counts": "here"}, b"out_* and seg"),                           # (the descriptor's out_counts: the entry point has its own)
    (dict(out_pairs="here"), b"out_* and seg"),
    (dict(out_mult="here"), b"out_* and seg"),
    (dict(out_cnt="here"), b"out_* and seg"),
    (dict(out_seg="here"), b"out_* and seg"),
    (dict(seg="here"), b"out_* and seg"),
    (dict(flags=None), b"null argument"),
    (dict(ids=None), b"null argument"),
    (dict(payload=None), b"null argument"),
    (dict(ukeys=None), b"are required"),
    (dict(n_keys=None), b"are required"),
])
def test_key_counts_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _key_counts(L, change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"sjoin_key_counts: ") and cause in msg, msg


def test_key_counts_refuses_a_null_output(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    rc = L.subgacc_sjoin_key_counts(C.byref(_desc(here)), here, here, None, here, None)
    assert rc == _lib.ERR_BADARG and L.subgacc_last_error().startswith(b"sjoin_key_counts: ukeys, n_keys and out_counts are required")
    rc = L.subgacc_sjoin_key_counts(None, here, here, here, here, None)
    assert rc == _lib.ERR_BADARG and L.subgacc_last_error().startswith(b"sjoin_key_counts: null descriptor")
    d = _desc(here)
    d.struct_bytes -= 8
    rc = L.subgacc_sjoin_key_counts(C.byref(d), here, here, here, here, None)
    assert rc == _lib.ERR_BADARG and b"struct_bytes" in L.subgacc_last_error()


@pytest.mark.parametrize("change", [dict(table_rows=14000), dict(row_stride=21000), dict(row_stride=8192, table_rows=9000)])
def test_key_counts_refuses_what_lds_does_not_hold(L, change):
    """8 row_stride + 12 T + 16 bytes beyond the 160 KiB of a CU: SUBGACC_ERR_LDS before any launch"""
    from surel_plus_amd import _lib
    rc, msg = _key_counts(L, change)
    assert rc == _lib.ERR_LDS
    assert msg.startswith(b"sjoin_key_counts: ") and b"LDS" in msg, msg


def test_key_counts_of_no_segments_is_a_no_op(L):
    """S = 0 launches nothing (host pointers, no device): SUBGACC_OK"""
    rc, _ = _key_counts(L, dict(S=0))
    assert rc == 0


# -------------------------------------------------------------------------------------------------------------------- Python
_NO_DEVICE = SimpleNamespace(device="cpu")       # nothing of it is looked at before the refusals


@pytest.mark.parametrize("kw,cause", [
    (dict(num_walks=200, num_steps=4), "key_rows_form == 64"),              # the paper's citation2 setting: 64-bit keys
    (dict(num_walks=128, num_steps=4), "key_rows_form == 64"),
    (dict(num_walks=300, num_steps=3), "no key-rows form"),
    (dict(key_rows=False), "key_rows=False"),
    (dict(batch=4), "batch=None"),
    (dict(table_rows=1), "table_rows"),
    (dict(table_rows=16385), "table_rows"),
    (dict(ptr=False), "ptr=False"),
    (dict(out=object()), "out="),
])
def test_step_buffers_refuse_the_count_stage_without_a_device(kw, cause):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match=cause):
        sp.StepBuffers(_NO_DEVICE, 8, stage="counts", **kw)
    with pytest.raises(ValueError, match="stage"):
        sp.StepBuffers(_NO_DEVICE, 8, stage="rows")


def test_the_step_calls_refuse_without_a_device():
    """the shape refusals of the calls that make their own buffers, and buffers made for another result"""
    import torch
    import surel_plus_amd as sp
    e, h = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_counts(_NO_DEVICE, e, num_walks=200, num_steps=4)
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_hmean_stage(_NO_DEVICE, h, torch.nn.Identity(), num_walks=200, num_steps=4)
    with pytest.raises(ValueError, match=r"\[2, B\]"):
        sp.sample_and_counts(_NO_DEVICE, h)
    with pytest.raises(ValueError, match=r"\[3, B\]"):
        sp.sample_and_hcounts(_NO_DEVICE, e)
    rows = SimpleNamespace(stage=None, triplets=False)       # StepBuffers of the row form
    with pytest.raises(ValueError, match="stage='counts'"):
        sp.sample_and_counts(_NO_DEVICE, e, buffers=rows)
    pairs = SimpleNamespace(stage="counts", triplets=False)
    with pytest.raises(ValueError, match="triplets=True"):
        sp.sample_and_hcounts(_NO_DEVICE, h, buffers=pairs)
    with pytest.raises(ValueError, match="sample_and_counts"):
        sp.sample_and_gather(_NO_DEVICE, e, buffers=SimpleNamespace(stage="counts", triplets=False, ptr=True))


def test_the_stage_gives_an_empty_segment_a_zero_row():
    """(C @ embed(table)) / sizes with a zero row of C and size 0: a zero row, not NaN; the other rows the weighted mean"""
    import torch
    from surel_plus_amd import spjoin
    C_ = torch.tensor([[1., 2., 1.], [0., 0., 0.], [3., 0., 1.], [0., 0., 0.]])
    sizes = torch.tensor([2, 0, 2, 0], dtype=torch.int32)
    table = torch.tensor([[0., 0.], [1., 0.5], [0., 0.25]])
    embed = torch.nn.Linear(2, 3)
    with torch.no_grad():
        embed.bias.fill_(0.5)
        out = spjoin._step_mean(C_, sizes, table, None, embed, 2)
        E = embed(table)
    assert out.shape == (2, 2, 3)
    flat = out.reshape(4, 3)
    assert not flat[1].any() and not flat[3].any()
    assert torch.allclose(flat[0], (E[0] + 2 * E[1] + E[2]) / 2) and torch.allclose(flat[2], (3 * E[0] + E[2]) / 2)

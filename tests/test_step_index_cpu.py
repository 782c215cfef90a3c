"""CPU: the argument contract of the index form over the key rows of an on-demand step -- subgacc_sjoin_key_index refuses every fault
before it launches anything, with a message led by its name; the LDS formula at its limit -- and what StepBuffers(stage="index"),
sample_and_index and sample_and_lstm_stage refuse before they touch a device.  No GPU needed."""
import ctypes as C
from types import SimpleNamespace

import pytest

NAME = "subgacc_sjoin_key_index"
LEAD = b"sjoin_key_index: "
_KEYS = ("ukeys", "n_keys", "seg", "out_idx", "out_len")
LDS = 160 * 1024


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_the_entry_point_is_declared_listed_and_exported_at_abi_7(L):
    import os
    import re
    import surel_plus_amd as sp
    from surel_plus_amd import _lib
    txt = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "subgacc.h")).read()
    assert NAME in _lib.SYMBOLS and hasattr(L, NAME)
    assert re.search(r"\bint %s\(const subgacc_join_desc \*d, const int32_t \*ukeys, const int64_t \*n_keys,\s*const int64_t \*seg,"
                     r"\s*int32_t \*out_idx, int32_t \*out_len, void \*stream\);" % NAME, txt)
    assert L.subgacc_abi_version() == 7 and "#define SUBGACC_ABI_VERSION 7" in txt
    assert C.sizeof(_lib.JoinDesc) == 248          # subgacc_join_desc keeps its layout
    assert callable(sp.sample_and_index) and callable(sp.sample_and_lstm_stage)


def _desc(here):
    """a mirrored descriptor over strided key rows that the library accepts up to its launch: B = 2 pairs (S = 4), T = 16.  It is only
    ever passed with one change the library refuses, or with S = 0 -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_KEY32
    d.row_len, d.row_stride, d.n_rows, d.S, d.pair_block, d.table_rows = here, 32, 4, 4, 2, 16
    d.num_walks, d.num_steps = 200, 3
    d.ids = d.payload = d.own = d.flags = here
    return d


def _call(L, change):
    """call the entry point with the accepted descriptor and arguments, the changes applied; (status, message)"""
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    args = {k: here for k in _KEYS}
    for k, val in change.items():
        val = here if val == "here" else val
        if k in args:
            args[k] = val
        else:
            setattr(d, k, val)
    rc = getattr(L, NAME)(C.byref(d), *[args[k] for k in _KEYS], None)
    return rc, L.subgacc_last_error()


# every refusal of subgacc_sjoin_key_counts (tests/test_step_stage_cpu.py), then the index form's own
_REFUSALS = [
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
    (dict(out_segid="here"), b"out_* and seg"),
    (dict(out_counts="here"), b"out_* and seg"),
    (dict(out_pairs="here"), b"out_* and seg"),
    (dict(out_mult="here"), b"out_* and seg"),
    (dict(out_cnt="here"), b"out_* and seg"),
    (dict(out_seg="here"), b"out_* and seg"),
    (dict(flags=None), b"null argument"),
    (dict(ids=None), b"null argument"),
    (dict(payload=None), b"null argument"),
    (dict(ukeys=None), b"are required"),
    (dict(n_keys=None), b"are required"),
    (dict(form=1), b"form ROWS"),                                           # COUNTS
    (dict(form=2), b"form ROWS"),                                           # PAIRS
    (dict(seg=None), b"seg and out_idx are required"),
    (dict(out_idx=None), b"seg and out_idx are required"),
    (dict(form=1, options=1), b"form ROWS"),                                # both wrong: the form is looked at before the options
]


@pytest.mark.parametrize("change,cause", _REFUSALS)
def test_refuses_before_anything_is_launched(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(LEAD) and cause in msg, msg


@pytest.mark.parametrize("field", ["out_idx", "seg"])
def test_refuses_the_descriptors_own_output_fields(L, field):
    """the descriptor's out_idx and seg FIELDS stay NULL (the call's arguments of the same names carry them): _call's `change` would
    set the argument, so the field is set here"""
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    setattr(d, field, here)
    rc = getattr(L, NAME)(C.byref(d), here, here, here, here, here, None)
    msg = L.subgacc_last_error()
    assert rc == _lib.ERR_BADARG and msg.startswith(LEAD) and b"out_* and seg" in msg, msg


def test_refuses_a_foreign_descriptor(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    args = [here] * len(_KEYS)
    rc = getattr(L, NAME)(None, *args, None)
    assert rc == _lib.ERR_BADARG and L.subgacc_last_error().startswith(LEAD + b"null descriptor")
    d = _desc(here)
    d.struct_bytes -= 8
    rc = getattr(L, NAME)(C.byref(d), *args, None)
    assert rc == _lib.ERR_BADARG and L.subgacc_last_error().startswith(LEAD) and b"struct_bytes" in L.subgacc_last_error()


def test_refuses_an_out_idx_that_is_not_8_byte_aligned(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    rc, msg = _call(L, dict(out_idx=C.addressof(buf) + 4))
    assert rc == _lib.ERR_BADARG and msg.startswith(LEAD) and b"8-byte aligned" in msg, msg


def test_an_empty_list_needs_neither_seg_nor_out_idx_nor_out_len(L):
    rc, msg = _call(L, dict(S=0, seg=None, out_idx=None, out_len=None))
    assert rc == 0, msg


def _need(stride, T):
    """the header's formula: 12 row_stride + 4 T bytes"""
    return 12 * stride + 4 * T


def test_the_lds_formula_at_its_limit(L):
    """row_stride = 608 (the cit2 step: 200 walks of 3 hops + 1, on whole lines).  S = 0 launches nothing, and the LDS need is refused
    before that: the last T accepted and the first refused."""
    from surel_plus_amd import _lib
    stride = 608
    last = (LDS - 12 * stride) // 4
    assert last == 39136 and _need(stride, last) <= LDS < _need(stride, last + 1)
    assert _need(stride, 2048) == 15488                                     # the figure the header quotes
    rc, msg = _call(L, dict(S=0, row_stride=stride, table_rows=last))
    assert rc == 0, msg
    rc, msg = _call(L, dict(S=0, row_stride=stride, table_rows=last + 1))
    assert rc == _lib.ERR_LDS
    assert msg.startswith(LEAD) and b"table_rows" in msg and b"row form" in msg, msg
    assert str(_need(stride, last + 1)).encode() in msg, msg
    # and along the other axis: T = 2,048, the longest row_stride
    last_stride = (LDS - 4 * 2048) // 12
    assert _need(last_stride, 2048) <= LDS < _need(last_stride + 1, 2048)
    assert _call(L, dict(S=0, row_stride=last_stride, table_rows=2048))[0] == 0
    rc, msg = _call(L, dict(S=0, row_stride=last_stride + 1, table_rows=2048))
    assert rc == _lib.ERR_LDS and msg.startswith(LEAD) and str(_need(last_stride + 1, 2048)).encode() in msg, msg
    # a refusal of the LDS comes with S > 0 too, before the launch
    rc, msg = _call(L, dict(table_rows=41000))
    assert rc == _lib.ERR_LDS and msg.startswith(LEAD), msg


def test_the_cit2_step_is_accepted(L):
    rc, msg = _call(L, dict(S=0, row_stride=608, table_rows=2048))
    assert rc == 0, msg


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
    (dict(triplets=True), "triplets=True"),
])
def test_step_buffers_refuse_the_index_stage_without_a_device(kw, cause):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match=cause) as err:
        sp.StepBuffers(_NO_DEVICE, 8, stage="index", **kw)
    assert "index" in str(err.value)


def test_an_unknown_stage_still_raises():
    import surel_plus_amd as sp
    for stage in ("rows", "lstm", "index ", "Index", ""):
        with pytest.raises(ValueError, match="stage"):
            sp.StepBuffers(_NO_DEVICE, 8, stage=stage)


def test_the_step_calls_refuse_without_a_device():
    """the shape refusals of the calls that make their own buffers, buffers made for another result, LSTMs the stage does not fuse"""
    import torch
    import surel_plus_amd as sp
    e, h = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[2, B\]"):
        sp.sample_and_index(_NO_DEVICE, h)
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_index(_NO_DEVICE, e, num_walks=200, num_steps=4)
    embed = torch.nn.Linear(4, 16)
    good = torch.nn.LSTM(16, 16, batch_first=True)
    for other in (SimpleNamespace(stage=None, triplets=False), SimpleNamespace(stage="counts", triplets=False),
                  SimpleNamespace(stage="counts_attn", triplets=False), SimpleNamespace(stage="index", triplets=True)):
        with pytest.raises(ValueError, match="stage='index'"):
            sp.sample_and_index(_NO_DEVICE, e, buffers=other)
        with pytest.raises(ValueError, match="stage='index'"):
            sp.sample_and_lstm_stage(SimpleNamespace(device=torch.device("cpu")), e, embed, good, buffers=other)
    index = SimpleNamespace(stage="index", triplets=False, ptr=True)
    with pytest.raises(ValueError, match="stage='counts'"):
        sp.sample_and_counts(_NO_DEVICE, e, buffers=index)
    with pytest.raises(ValueError, match="stage='counts_attn'"):
        sp.sample_and_attn_counts(_NO_DEVICE, e, lambda table: table.sum(1), buffers=index)
    with pytest.raises(ValueError, match="made for another result"):
        sp.sample_and_gather(_NO_DEVICE, e, buffers=index)
    general = "sample_and_gather"           # the general path the messages name: the row-form step and the modules on xz
    for bad in (torch.nn.LSTM(16, 16, batch_first=True, num_layers=2), torch.nn.LSTM(16, 16, batch_first=True, bidirectional=True),
                torch.nn.LSTM(16, 100, batch_first=True), torch.nn.LSTM(16, 16, batch_first=False),
                torch.nn.GRU(16, 16, batch_first=True)):
        with pytest.raises((TypeError, ValueError), match=general) as err:
            sp.sample_and_lstm_stage(_NO_DEVICE, e, embed, bad)
        assert "sample_and_lstm_stage" in str(err.value)

"""CPU: the argument contract of the attentional count form over the key rows of an on-demand step -- subgacc_sjoin_key_counts_attn and
its backward refuse every fault before they launch anything, with a message led by their name; the LDS formula at its limit -- and
what StepBuffers(stage="counts_attn") refuses before it touches a device.  No GPU needed."""
import ctypes as C
from types import SimpleNamespace

import pytest

NAMES = ("subgacc_sjoin_key_counts_attn", "subgacc_sjoin_key_counts_attn_backward")
LEAD = {NAMES[0]: b"sjoin_key_counts_attn: ", NAMES[1]: b"sjoin_key_counts_attn_backward: "}
_KEYS = {NAMES[0]: ("ukeys", "n_keys", "g", "out_w", "out_max", "out_den", "out_len"),
         NAMES[1]: ("ukeys", "n_keys", "g", "dw", "w", "max", "den", "out_dg")}
LDS = 160 * 1024


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_step_attn_entry_points_are_exported_at_abi_7(L):
    import os
    import re
    from surel_plus_amd import _lib
    txt = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "subgacc.h")).read()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert re.search(r"\b%s\(" % name, txt)
    assert L.subgacc_abi_version() == 7
    assert C.sizeof(_lib.JoinDesc) == 248          # subgacc_join_desc keeps its layout


def _desc(here):
    """a mirrored descriptor over strided key rows that the library accepts up to its launch: B = 2 pairs (S = 4), T = 16.  It is only
    ever passed with one change the library refuses, or with S = 0 -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_COUNTS, _lib.JOIN_KEY32
    d.row_len, d.row_stride, d.n_rows, d.S, d.pair_block, d.table_rows = here, 32, 4, 4, 2, 16
    d.num_walks, d.num_steps = 200, 3
    d.ids = d.payload = d.own = d.flags = here
    return d


def _call(L, name, change):
    """call `name` with the accepted descriptor and arguments, the changes applied; (status, message)"""
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


# every refusal of subgacc_sjoin_key_counts (tests/test_step_stage_cpu.py)
_KEY_COUNTS_REFUSALS = [
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
    (dict(out_counts="here"), b"out_* and seg"),
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
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("change,cause", _KEY_COUNTS_REFUSALS)
def test_refuses_what_key_counts_refuses(L, name, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, name, change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(LEAD[name]) and cause in msg, msg


@pytest.mark.parametrize("change,cause", [
    (dict(g=None), b"g and out_w are required"),
    (dict(out_w=None), b"g and out_w are required"),
    (dict(out_max=None), b"out_max and out_den go together"),
    (dict(out_den=None), b"out_max and out_den go together"),
])
def test_forward_refuses_its_own_arguments(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[0], change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(LEAD[NAMES[0]]) and cause in msg, msg


@pytest.mark.parametrize("arg", ["g", "dw", "w", "max", "den", "out_dg"])
def test_backward_refuses_a_null_argument(L, arg):
    from surel_plus_amd import _lib
    rc, msg = _call(L, NAMES[1], {arg: None})
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(LEAD[NAMES[1]]) and b"are required" in msg, msg


@pytest.mark.parametrize("name", NAMES)
def test_refuses_a_foreign_descriptor(L, name):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    args = [here] * len(_KEYS[name])
    rc = getattr(L, name)(None, *args, None)
    assert rc == _lib.ERR_BADARG and L.subgacc_last_error().startswith(LEAD[name] + b"null descriptor")
    d = _desc(here)
    d.struct_bytes -= 8
    rc = getattr(L, name)(C.byref(d), *args, None)
    assert rc == _lib.ERR_BADARG and L.subgacc_last_error().startswith(LEAD[name]) and b"struct_bytes" in L.subgacc_last_error()


def _need(stride, T, bwd):
    """the header's formula: 4 (7 row_stride + 3 T + 2 D + 7) bytes, D = min(2 row_stride, T); the backward: 6 D"""
    D = min(2 * stride, T)
    return 4 * (7 * stride + 3 * T + (6 if bwd else 2) * D + 7)


def test_the_lds_formula_at_its_limit(L):
    """row_stride = 608 (the cit2 step: 200 walks of 3 hops + 1, on whole lines).  S = 0 launches nothing, and the LDS need is refused
    before that: the last T accepted and the first refused, for the backward, for a forward that keeps m / den (the backward's need)
    and for a forward that does not (its own)."""
    from surel_plus_amd import _lib
    stride = 608
    last_bwd, last_fwd = 9800, 11421
    assert _need(stride, last_bwd, True) <= LDS < _need(stride, last_bwd + 1, True)
    assert _need(stride, last_fwd, False) <= LDS < _need(stride, last_fwd + 1, False)
    assert _need(stride, 2048, False) == 51356 and _need(stride, 2048, True) == 70812       # the figures the header quotes
    fwd_alone = dict(out_max=None, out_den=None)
    for name, extra, last, bwd in ((NAMES[1], {}, last_bwd, True), (NAMES[0], {}, last_bwd, True), (NAMES[0], fwd_alone, last_fwd, False)):
        rc, msg = _call(L, name, dict(S=0, row_stride=stride, table_rows=last, **extra))
        assert rc == 0, msg
        rc, msg = _call(L, name, dict(S=0, row_stride=stride, table_rows=last + 1, **extra))
        assert rc == _lib.ERR_LDS
        assert msg.startswith(LEAD[name]) and b"table_rows" in msg and b"row form" in msg, msg
        assert str(_need(stride, last + 1, bwd)).encode() in msg, msg


@pytest.mark.parametrize("name", NAMES)
def test_the_cit2_step_is_accepted(L, name):
    """row_stride = 608, T = 2,048, forward (keeping m / den) and backward: past every refusal (S = 0: nothing to launch)"""
    rc, msg = _call(L, name, dict(S=0, row_stride=608, table_rows=2048))
    assert rc == 0, msg


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("change", [dict(table_rows=14000), dict(row_stride=21000), dict(row_stride=4096, table_rows=9000)])
def test_refuses_what_lds_does_not_hold(L, name, change):
    from surel_plus_amd import _lib
    rc, msg = _call(L, name, change)
    assert rc == _lib.ERR_LDS
    assert msg.startswith(LEAD[name]) and b"LDS" in msg and b"table_rows" in msg and b"row form" in msg, msg


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
def test_step_buffers_refuse_the_attn_stage_without_a_device(kw, cause):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match=cause) as err:
        sp.StepBuffers(_NO_DEVICE, 8, stage="counts_attn", **kw)
    assert "counts_attn" in str(err.value)


def test_an_unknown_stage_still_raises():
    import surel_plus_amd as sp
    for stage in ("rows", "attn", "counts_attn ", ""):
        with pytest.raises(ValueError, match="stage"):
            sp.StepBuffers(_NO_DEVICE, 8, stage=stage)


def test_the_step_calls_refuse_without_a_device():
    """the shape refusals of the calls that make their own buffers, buffers made for another result, modules the stage does not fuse"""
    import torch
    import surel_plus_amd as sp
    e, h = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)
    gate = lambda table: table.sum(1)       # noqa: E731
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_attn_counts(_NO_DEVICE, e, gate, num_walks=200, num_steps=4)
    with pytest.raises(ValueError, match=r"\[2, B\]"):
        sp.sample_and_attn_counts(_NO_DEVICE, h, gate)
    for other in (SimpleNamespace(stage=None, triplets=False), SimpleNamespace(stage="counts", triplets=False)):
        with pytest.raises(ValueError, match="stage='counts_attn'"):
            sp.sample_and_attn_counts(_NO_DEVICE, e, gate, buffers=other)
    attn = SimpleNamespace(stage="counts_attn", triplets=False, ptr=True)
    with pytest.raises(ValueError, match="stage='counts'"):
        sp.sample_and_counts(_NO_DEVICE, e, buffers=attn)
    with pytest.raises(ValueError, match="made for another result"):
        sp.sample_and_gather(_NO_DEVICE, e, buffers=attn)
    embed, lin = torch.nn.Linear(4, 8), torch.nn.Linear(8, 1)
    with pytest.raises(TypeError, match="sample_and_attn_stage fuses gate_nn"):
        sp.sample_and_attn_stage(_NO_DEVICE, e, embed, torch.nn.Sequential(lin, torch.nn.ReLU()))
    with pytest.raises(TypeError, match="sample_and_attn_stage fuses value_nn"):
        sp.sample_and_attn_stage(_NO_DEVICE, e, embed, lin, torch.nn.Linear(7, 8))
    with pytest.raises(ValueError, match="float32 parameters"):
        sp.sample_and_attn_stage(_NO_DEVICE, e, embed, lin.double())

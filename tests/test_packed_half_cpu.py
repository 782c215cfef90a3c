"""CPU: the join over the step's packed rows written in a 16-bit type -- the seventh header and its binding, every fault
subgacc_sjoin_fill_packed_half refuses before it launches anything (return code, a message led by its name and naming the cause), and
what StepBuffers does with packed_half=True before it touches a device.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED_HALF_H = os.path.join(ROOT, "include", "subgacc_packed_half.h")
NAME = "subgacc_sjoin_fill_packed_half"


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_seventh_header_parses_and_adds_one_entry_point(L):
    from surel_plus_amd import _lib
    assert _lib.PACKED_HALF_HEADER == PACKED_HALF_H
    decls = _lib.parse_header(open(PACKED_HALF_H).read())
    assert list(decls) == [NAME] == list(_lib.PACKED_HALF_SYMBOLS) == list(_lib.PACKED_HALF_DECLS)
    ret, args = decls[NAME]
    assert ret == "int" and args == [("d", "const subgacc_join_desc *"), ("nesc", "const int32_t *"), ("num_nodes", "int64_t"),
                                     ("out_dtype", "int32_t"), ("out_rows", "void *"), ("stream", "void *")]
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.restype is C.c_int and len(fn.argtypes) == 6
    assert fn.argtypes[0] == C.POINTER(_lib.JoinDesc) and fn.argtypes[2:] == [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]


def test_the_other_headers_keep_their_entry_points(L):
    from surel_plus_amd import _lib
    assert len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7
    assert _lib.HALF_SYMBOLS == ("subgacc_sjoin_fill_half",) and _lib.HALF64_SYMBOLS == ("subgacc_sjoin_fill_half64",)
    assert (len(_lib.SMALL_SYMBOLS), len(_lib.PACKED_SYMBOLS), len(_lib.WIDE_SYMBOLS)) == (1, 4, 2)
    for syms in (_lib.SYMBOLS, _lib.HALF_SYMBOLS, _lib.SMALL_SYMBOLS, _lib.PACKED_SYMBOLS, _lib.WIDE_SYMBOLS, _lib.HALF64_SYMBOLS):
        assert NAME not in syms
    assert C.sizeof(_lib.JoinDesc) == 248


def test_build_watches_the_seventh_header_and_the_makefile_compiles_the_kernel():
    from surel_plus_amd import _lib
    assert "PACKED_HALF_HEADER" in inspect.getsource(_lib.build)
    mk = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "Makefile")).read()
    assert " sjoin_packed_half.hip " in mk and "subgacc_packed_half.h" in mk


# ------------------------------------------------------------------------------------------------ subgacc_sjoin_fill_packed_half
NODES = 1 << 20       # cb = 12, fb = 3 at three hops


def _desc(here, layout="strided"):
    """a mirrored descriptor over strided packed rows that the library accepts up to its launch: B = 2 pairs (S = 4), M = 200, 3 hops,
    a pitch of 608.  It is only ever passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_KEY32
    if layout == "packed":
        d.row_off, d.max_len = here, 32
    elif layout == "headed":
        d.row_stride = 608
    else:
        d.row_len, d.row_stride = here, 608
    d.n_rows, d.S, d.pair_block, d.num_walks, d.num_steps = 4, 4, 2, 200, 3
    d.ids = d.payload = d.own = d.flags = d.seg = here
    return d


def _fill(L, change=None, dtype=2, out="here", layout="strided", nesc="here", nodes=NODES):
    buf = (C.c_int64 * 64)()
    here = (C.addressof(buf) + 15) & ~15
    d = _desc(here, layout)
    for name, val in (change or {}).items():
        setattr(d, name, here if val == "here" else val)
    out = {"here": here, "odd": here + 8, None: None}[out]
    rc = L.subgacc_sjoin_fill_packed_half(C.byref(d), C.cast(here, C.POINTER(C.c_int32)) if nesc else None, nodes, dtype, out, None)
    return rc, L.subgacc_last_error()


REFUSALS = [
    pytest.param(dict(change=dict(form=1)), "ERR_BADARG", b"row form", id="count-form"),
    pytest.param(dict(change=dict(form=2)), "ERR_BADARG", b"row form", id="pair-form"),
    pytest.param(dict(change=dict(options=1)), "ERR_BADARG", b"no option bits", id="opt-sizes"),
    pytest.param(dict(change=dict(options=2)), "ERR_BADARG", b"no option bits", id="opt-star"),
    pytest.param(dict(change=dict(payload_kind=1)), "ERR_BADARG", b"payload_kind KEY32", id="payload-f64"),
    pytest.param(dict(change=dict(payload_kind=3)), "ERR_BADARG", b"payload_kind KEY32", id="payload-key64"),
    pytest.param(dict(change=dict(payload_kind=0)), "ERR_BADARG", b"payload_kind KEY32", id="payload-sfptr"),
    pytest.param(dict(layout="packed"), "ERR_BADARG", b"strided rows", id="packed-rows"),
    pytest.param(dict(layout="headed"), "ERR_BADARG", b"strided rows", id="headed-rows"),
    pytest.param(dict(change=dict(pair_block=0)), "ERR_BADARG", b"pair_block > 0", id="not-mirrored"),
    pytest.param(dict(change=dict(S=6)), "ERR_BADARG", b"multiple of 2*pair_block", id="S-not-whole-blocks"),
    pytest.param(dict(change=dict(out_xz="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_xz-set"),
    pytest.param(dict(change=dict(out_idx="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_idx-set"),
    pytest.param(dict(change=dict(out_segid="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_segid-set"),
    pytest.param(dict(change=dict(out_counts="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_counts-set"),
    pytest.param(dict(change=dict(out_pairs="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_pairs-set"),
    pytest.param(dict(change=dict(out_mult="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_mult-set"),
    pytest.param(dict(change=dict(out_cnt="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_cnt-set"),
    pytest.param(dict(change=dict(out_seg="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_seg-set"),
    pytest.param(dict(dtype=0), "ERR_BADARG", b"out_dtype = 0", id="dtype-0"),
    pytest.param(dict(dtype=3), "ERR_BADARG", b"out_dtype = 3", id="dtype-3"),
    pytest.param(dict(out=None), "ERR_BADARG", b"out_rows = NULL", id="null-out-rows"),
    pytest.param(dict(out="odd"), "ERR_BADARG", b"16-byte aligned", id="misaligned-out-rows"),
    pytest.param(dict(nesc=None), "ERR_BADARG", b"nesc = NULL", id="null-nesc"),
    pytest.param(dict(change=dict(seg=None)), "ERR_BADARG", b"seg = NULL", id="null-seg"),
    pytest.param(dict(change=dict(num_walks=3, num_steps=5)), "ERR_BADARG", b"2 to 4 hops", id="five-hops"),
    pytest.param(dict(change=dict(num_walks=200, num_steps=4)), "ERR_KEYWIDTH", b"do not fit 32 bits", id="keys-of-33-bits"),
    pytest.param(dict(change=dict(num_walks=2047, num_steps=3)), "ERR_KEYWIDTH", b"do not fit 32 bits", id="keys-of-34-bits"),
    pytest.param(dict(nodes=(1 << 22) + 1), "ERR_BADARG", b"3 bits a count", id="two-bits-a-count"),
    pytest.param(dict(nodes=1 << 31), "ERR_BADARG", b"3 bits a count", id="ids-of-31-bits"),
    pytest.param(dict(nodes=-1), "ERR_BADARG", b"num_nodes = -1", id="negative-num-nodes"),
    pytest.param(dict(change=dict(row_stride=1025)), "ERR_LDS", b"rows of 1025 members", id="pitch-1025"),
    pytest.param(dict(change=dict(flags=None)), "ERR_BADARG", b"null argument", id="null-flags"),
    pytest.param(dict(change=dict(ids=None)), "ERR_BADARG", b"null argument", id="null-ids"),
    pytest.param(dict(change=dict(payload=None)), "ERR_BADARG", b"null argument", id="null-payload"),
    pytest.param(dict(change=dict(own=None)), "ERR_BADARG", b"null argument", id="null-own"),
]


@pytest.mark.parametrize("how,status,cause", REFUSALS)
def test_fill_packed_half_refuses_before_any_launch(L, how, status, cause):
    from surel_plus_amd import _lib
    rc, msg = _fill(L, **how)
    assert rc == getattr(_lib, status), msg
    assert msg.startswith(b"sjoin_fill_packed_half: ") and cause in msg, msg


def test_the_refusals_are_those_of_the_two_calls_it_joins(L):
    """the descriptor's faults answer with subgacc_sjoin_fill_packed's status, the output's with subgacc_sjoin_fill_half's"""
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = (C.addressof(buf) + 15) & ~15
    nesc = C.cast(here, C.POINTER(C.c_int32))
    for change in (dict(form=1), dict(options=1), dict(payload_kind=3), dict(pair_block=0), dict(S=6), dict(num_walks=3, num_steps=5),
                   dict(num_walks=200, num_steps=4), dict(row_stride=1025)):
        d = _desc(here)
        d.out_xz = here
        for k, v in change.items():
            setattr(d, k, v)
        want = L.subgacc_sjoin_fill_packed(C.byref(d), nesc, NODES, None)
        assert want < 0 and _fill(L, change=change)[0] == want, change
    for how in (dict(dtype=0), dict(out=None), dict(out="odd"), dict(change=dict(out_idx="here"))):
        d = _desc(here)
        for k, v in how.get("change", {}).items():
            setattr(d, k, here)
        out = {"here": here, "odd": here + 8, None: None}[how.get("out", "here")]
        want = L.subgacc_sjoin_fill_half(C.byref(d), how.get("dtype", 2), out, None)
        assert want < 0 and _fill(L, **how)[0] == want, how
    assert _lib.ERR_BADARG < 0


@pytest.mark.parametrize("dtype", [1, 2])
def test_an_empty_list_launches_nothing(L, dtype):
    """S = 0: accepted without a device -- nothing is launched -- with and without the pointers a list would need; a pitch of 1,024 is
    within the limit"""
    assert _fill(L, change=dict(S=0), dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0, seg=None, own=None, flags=None, ids=None, payload=None), out=None, nesc=None, dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0, row_stride=1024), dtype=dtype)[0] == 0


# --------------------------------------------------------------------------------------------------------------- the Python layer
HALF = [torch.float16, torch.bfloat16]


def _graph(num_nodes=1 << 17, idx=torch.int32, **more):
    return SimpleNamespace(device="cpu", num_nodes=num_nodes, indptr=torch.zeros(1, dtype=idx), **more)


# what StepBuffers(packed_half=True) refuses: (keywords, the reason it names)
STEP_REFUSALS = [(dict(dtype=None), "dtype=None"), (dict(dtype=torch.float32), "dtype=torch.float32"),
                 (dict(packed_rows=False), "packed_rows=False"), (dict(ptr=False), "ptr=False"), (dict(triplets=True), "triplets=True"),
                 (dict(stage="counts"), "stage='counts'"), (dict(stage="index"), "stage='index'"), (dict(key_rows=False), "key_rows=False"),
                 (dict(batch=8), "batch="),
                 (dict(num_walks=200, num_steps=4), "no packed form"),           # 64-bit keys
                 (dict(num_walks=200, num_steps=4, wide_keys=True), "no packed form"),
                 (dict(num_walks=300, num_steps=3), "no packed form"),           # no key rows
                 (dict(num_walks=200, num_steps=2), "no packed form"),           # the one-wave form
                 (dict(graph=dict(num_nodes=(1 << 22) + 1)), "no packed form")]  # two bits a count


@pytest.mark.parametrize("dtype", HALF)
def test_step_buffers_refuse_the_keyword_before_any_device_work(dtype):
    """every refusal is a ValueError that names the keyword and the reason; the graph is a namespace without a device"""
    from surel_plus_amd import spjoin
    for kw, reason in STEP_REFUSALS:
        kw = {"num_walks": 200, "num_steps": 3, "dtype": dtype, **kw}
        g = _graph(**kw.pop("graph", {}))
        with pytest.raises(ValueError, match=re.escape(reason)) as e:
            spjoin.StepBuffers(g, 16, packed_half=True, **kw)
        assert str(e.value).startswith("StepBuffers(packed_half=True): "), (kw, str(e.value))
    with pytest.raises(ValueError, match="packed_half=True") as e:      # several at once: all are named
        spjoin.StepBuffers(_graph(), 16, packed_half=True, num_walks=200, num_steps=3, dtype=dtype, ptr=False, batch=8)
    assert "ptr=False" in str(e.value) and "batch=" in str(e.value)


@pytest.mark.parametrize("dtype", HALF)
def test_without_the_keyword_nothing_changes(dtype):
    """packed_rows=True beside a 16-bit dtype still raises, and the 16-bit refusals keep their words"""
    from surel_plus_amd import spjoin
    with pytest.raises(ValueError, match=re.escape(f"StepBuffers: dtype={dtype} (16-bit rows")):
        spjoin.StepBuffers(_graph(), 16, num_walks=200, num_steps=3, dtype=dtype, ptr=False)
    sb = inspect.signature(spjoin.StepBuffers.__init__).parameters
    assert sb["packed_half"].default is False and sb["packed_rows"].default is None and list(sb)[-1] == "packed_half"
    import surel_plus_amd as sp
    for name in ("sample_and_gather", "sjoin", "gather", "CapturedStep"):
        fn = getattr(spjoin, name, None) or getattr(sp, name)
        assert "packed_half" not in inspect.signature(fn).parameters, name
    src = inspect.getsource(spjoin.StepBuffers.__init__)
    assert '"a 16-bit dtype (without packed_half=True)": bool(self.half) and not packed_half' in src


def test_sample_and_gather_serves_such_buffers_with_todays_dtype_check():
    """buffers with .packed and .half pass the dtype check and are refused only for what a namespace is not; another dtype is
    refused as ever"""
    from surel_plus_amd import spjoin
    e = torch.zeros((2, 4), dtype=torch.int64)
    bufs = SimpleNamespace(half=2, half64=False, packed=True, dtype=torch.bfloat16)
    with pytest.raises(AttributeError):
        spjoin.sample_and_gather(_graph(), e, num_walks=200, num_steps=3, buffers=bufs, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        spjoin.sample_and_gather(_graph(), e, num_walks=200, num_steps=3, buffers=bufs, dtype=torch.float16)
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        spjoin.sample_and_gather(_graph(), e, num_walks=200, num_steps=3, buffers=bufs)

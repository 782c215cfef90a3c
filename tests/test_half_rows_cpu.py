"""CPU: the join's rows in a 16-bit type -- the second header and its binding, every fault subgacc_sjoin_fill_half refuses before it
launches anything (return code, a message led by its name), and what sjoin / gather / sample_and_gather / StepBuffers refuse of
dtype=torch.float16 / torch.bfloat16 before they touch a device.  No GPU needed."""
import ctypes as C
import importlib.util
import os
import re
import shutil
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_H = os.path.join(ROOT, "include", "subgacc_half.h")


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_second_header_parses_and_adds_one_entry_point(L):
    from surel_plus_amd import _lib
    decls = _lib.parse_header(open(HALF_H).read())
    assert list(decls) == ["subgacc_sjoin_fill_half"] == list(_lib.HALF_SYMBOLS)
    ret, args = decls["subgacc_sjoin_fill_half"]
    assert ret == "int" and args == [("d", "const subgacc_join_desc *"), ("out_dtype", "int32_t"), ("out_rows", "void *"),
                                     ("stream", "void *")]
    fn = L.subgacc_sjoin_fill_half                                   # AttributeError: the library does not export it
    assert fn.argtypes == [C.POINTER(_lib.JoinDesc), C.c_int32, C.c_void_p, C.c_void_p] and fn.restype is C.c_int
    text = open(HALF_H).read()
    assert re.search(r"^#define\s+SUBGACC_HALF_F16\s+1\b", text, re.M) and re.search(r"^#define\s+SUBGACC_HALF_BF16\s+2\b", text, re.M)
    assert (_lib.HALF_F16, _lib.HALF_BF16) == (1, 2)


def test_the_abi_of_the_first_header_keeps_its_size(L):
    from surel_plus_amd import _lib
    assert len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and "subgacc_sjoin_fill_half" not in _lib.SYMBOLS
    assert C.sizeof(_lib.JoinDesc) == 248


def test_a_missing_second_header_is_an_error_that_names_the_path(tmp_path):
    """a copy of _lib.py in a tree that has include/subgacc.h but not include/subgacc_half.h refuses to import"""
    (tmp_path / "pkg").mkdir()
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "subgacc.h"), str(tmp_path / "include" / "subgacc.h"))
    shutil.copy(os.path.join(ROOT, "surel_plus_amd", "_lib.py"), str(tmp_path / "pkg" / "_lib.py"))
    spec = importlib.util.spec_from_file_location("_lib_without_half_header", str(tmp_path / "pkg" / "_lib.py"))
    with pytest.raises(RuntimeError, match=re.escape(os.path.join(str(tmp_path), "include", "subgacc_half.h"))) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "SubgAccError"


# ---------------------------------------------------------------------------------------------------------- subgacc_sjoin_fill_half
def _desc(here, packed=False):
    """a mirrored descriptor over strided rows of 32-bit keys (packed: over packed rows) that the library accepts up to its launch:
    B = 2 pairs (S = 4), M = 200, 3 hops.  It is only ever passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_KEY32
    if packed:
        d.row_off, d.max_len = here, 32
    else:
        d.row_len, d.row_stride = here, 32
    d.n_rows, d.S, d.pair_block, d.num_walks, d.num_steps = 4, 4, 2, 200, 3
    d.ids = d.payload = d.own = d.flags = d.seg = here
    return d


def _sfptr(d, here, k=4):
    from surel_plus_amd import _lib
    d.payload_kind, d.table, d.table_rows, d.k = _lib.JOIN_SFPTR, here, 8, k


def _fill(L, change=None, dtype=2, out="here", packed=False, sfptr=None, null_desc=False):
    buf = (C.c_int64 * 64)()
    here = (C.addressof(buf) + 15) & ~15
    d = _desc(here, packed)
    if sfptr is not None:
        _sfptr(d, here, sfptr)
    for name, val in (change or {}).items():
        setattr(d, name, here if val == "here" else val)
    out = {"here": here, "odd": here + 8, None: None}[out]
    rc = L.subgacc_sjoin_fill_half(None if null_desc else C.byref(d), dtype, out, None)
    return rc, L.subgacc_last_error()


REFUSALS = [
    pytest.param(dict(null_desc=True), "ERR_BADARG", b"null descriptor", id="null-descriptor"),
    pytest.param(dict(change=dict(struct_bytes=240)), "ERR_BADARG", b"descriptor of 240 bytes", id="wrong-size-descriptor"),
    pytest.param(dict(change=dict(form=1)), "ERR_BADARG", b"form ROWS", id="count-form"),
    pytest.param(dict(change=dict(form=2), packed=True, sfptr=4), "ERR_BADARG", b"form ROWS", id="pair-form"),
    pytest.param(dict(change=dict(options=1)), "ERR_BADARG", b"no option", id="opt-sizes"),
    pytest.param(dict(change=dict(options=2), packed=True), "ERR_BADARG", b"no option", id="opt-star"),
    pytest.param(dict(change=dict(options=4)), "ERR_BADARG", b"no option", id="unknown-option"),
    pytest.param(dict(change=dict(payload_kind=1), packed=True), "ERR_BADARG", b"payload kind 1", id="payload-f64"),
    pytest.param(dict(change=dict(payload_kind=3)), "ERR_BADARG", b"payload kind 3", id="payload-key64"),
    pytest.param(dict(change=dict(row_len=None)), "ERR_BADARG", b"headed rows", id="headed-rows"),
    pytest.param(dict(sfptr=4), "ERR_BADARG", b"uniq_table", id="sfptr-over-strided-rows"),
    pytest.param(dict(sfptr=4, change=dict(uniq_table="here", uniq_capacity=64)), "ERR_BADARG", b"uniq_table", id="sfptr-slots-with-uniq-table"),
    pytest.param(dict(change=dict(pair_block=0)), "ERR_BADARG", b"pair_block > 0", id="not-mirrored"),
    pytest.param(dict(change=dict(pair_block=-2)), "ERR_BADARG", b"pair_block > 0", id="negative-pair-block"),
    pytest.param(dict(change=dict(S=6)), "ERR_BADARG", b"not a multiple of 2*pair_block", id="S-not-whole-blocks"),
    pytest.param(dict(change=dict(seg=None)), "ERR_BADARG", b"seg = NULL", id="null-seg"),
    pytest.param(dict(change=dict(out_xz="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_xz-set"),
    pytest.param(dict(change=dict(out_idx="here"), packed=True, sfptr=4), "ERR_BADARG", b"out_* fields must be NULL", id="out_idx-set"),
    pytest.param(dict(change=dict(out_segid="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_segid-set"),
    pytest.param(dict(change=dict(out_counts="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_counts-set"),
    pytest.param(dict(change=dict(out_pairs="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_pairs-set"),
    pytest.param(dict(change=dict(out_mult="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_mult-set"),
    pytest.param(dict(change=dict(out_cnt="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_cnt-set"),
    pytest.param(dict(change=dict(out_seg="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_seg-set"),
    pytest.param(dict(change=dict(num_walks=100, num_steps=5)), "ERR_KEYWIDTH", b"do not fit 32 bits", id="keys-wider-than-32-bits"),
    pytest.param(dict(change=dict(num_walks=3, num_steps=5)), "ERR_BADARG", b"k = 6", id="key-k-6"),
    pytest.param(dict(packed=True, sfptr=1), "ERR_BADARG", b"k = 1", id="table-k-1"),
    pytest.param(dict(packed=True, sfptr=6), "ERR_BADARG", b"k = 6", id="table-k-6"),
    pytest.param(dict(packed=True, sfptr=4, change=dict(table=None)), "ERR_BADARG", b"feature table", id="sfptr-without-table"),
    pytest.param(dict(dtype=0), "ERR_BADARG", b"out_dtype = 0", id="dtype-0"),
    pytest.param(dict(dtype=3), "ERR_BADARG", b"out_dtype = 3", id="dtype-3"),
    pytest.param(dict(out=None), "ERR_BADARG", b"out_rows = NULL", id="null-out-rows"),
    pytest.param(dict(out="odd"), "ERR_BADARG", b"16-byte aligned", id="misaligned-out-rows"),
    pytest.param(dict(change=dict(row_stride=14000)), "ERR_LDS", b"LDS", id="rows-beyond-lds"),
    pytest.param(dict(change=dict(max_len=14000), packed=True), "ERR_LDS", b"LDS", id="packed-rows-beyond-lds"),
    pytest.param(dict(change=dict(flags=None)), "ERR_BADARG", b"null argument", id="null-flags"),
    pytest.param(dict(change=dict(ids=None)), "ERR_BADARG", b"null argument", id="null-ids"),
    pytest.param(dict(change=dict(payload=None)), "ERR_BADARG", b"null argument", id="null-payload"),
    pytest.param(dict(change=dict(own=None)), "ERR_BADARG", b"own = NULL", id="null-own"),
]


@pytest.mark.parametrize("how,status,cause", REFUSALS)
def test_fill_half_refuses_before_any_launch(L, how, status, cause):
    from surel_plus_amd import _lib
    rc, msg = _fill(L, **how)
    assert rc == getattr(_lib, status), msg
    assert msg.startswith(b"sjoin_fill_half: ") and cause in msg, msg


@pytest.mark.parametrize("dtype", [1, 2])
def test_an_empty_list_launches_nothing(L, dtype):
    """S = 0: accepted without a device -- nothing is launched -- with and without the pointers a list would need"""
    assert _fill(L, change=dict(S=0), dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0, seg=None, own=None, flags=None, ids=None, payload=None), out=None, dtype=dtype)[0] == 0


# --------------------------------------------------------------------------------------------------------------- the Python layer
HALF = [torch.float16, torch.bfloat16]


def _graph(**more):
    return SimpleNamespace(device="cpu", **more)


def _rows():
    return torch.zeros(4, dtype=torch.int64)


@pytest.mark.parametrize("dtype", HALF)
def test_sjoin_refuses_what_the_half_rows_do_not_cover(dtype):
    from surel_plus_amd import spjoin
    from surel_plus_amd.spg import HeadedSpG
    store = _graph(payload_is_slot=False, data=torch.zeros(1, dtype=torch.int32))
    for kw, name in [(dict(ptr_mode=False), "ptr=False"), (dict(return_index=True), "return_index"), (dict(lazy=True), "lazy=True"),
                     (dict(star=True), "star=True"), (dict(pair_block=0), "pair_block")]:
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.sjoin(store, _rows(), None, **{"pair_block": 2, **kw}, dtype=dtype)
    headed = HeadedSpG.__new__(HeadedSpG)
    headed.device, headed.data = "cpu", torch.zeros(1, dtype=torch.int32)
    for x, name in [(headed, "HeadedSpG"), (_graph(payload_is_slot=False, data=torch.zeros(1, dtype=torch.float64)), "float64 store"),
                    (_graph(payload_is_slot=True, keyrows=True, key64=True), "64-bit keys"),
                    (_graph(payload_is_slot=True, keyrows=False), "key_rows=False")]:
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.sjoin(x, _rows(), None, pair_block=2, dtype=dtype)
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.gather(torch.zeros((2, 2), dtype=torch.int64), x, dtype=dtype)
    with pytest.raises(ValueError, match="dtype is None, torch.float32"):
        spjoin.sjoin(store, _rows(), None, pair_block=2, dtype=torch.float64)


@pytest.mark.parametrize("dtype", HALF)
def test_gather_refuses_segment_ids_and_the_lazy_form(dtype):
    from surel_plus_amd import spjoin
    store, e = _graph(payload_is_slot=False, data=torch.zeros(1, dtype=torch.int32)), torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=re.escape("ptr=False")):
        spjoin.gather(e, store, ptr=False, dtype=dtype)
    with pytest.raises(ValueError, match=re.escape("lazy=True")):
        spjoin.gather(e, store, lazy=True, out=torch.empty(8), dtype=dtype)
    import scipy.sparse as sps
    with pytest.raises(ValueError, match="float64 store"):             # (a SciPy matrix of float scores: refused before its upload)
        spjoin.gather(e, sps.csr_matrix((4, 4), dtype="float64"), dtype=dtype)


@pytest.mark.parametrize("dtype", HALF)
def test_step_buffers_refuse_what_the_half_rows_do_not_cover(dtype):
    from surel_plus_amd import spjoin
    for kw, name in [(dict(ptr=False), "ptr=False"), (dict(triplets=True), "triplets=True"), (dict(stage="counts"), "stage='counts'"),
                     (dict(key_rows=False), "key_rows=False"), (dict(num_walks=200, num_steps=4), "64-bit keys"),
                     (dict(num_walks=300, num_steps=3), "no key rows"), (dict(batch=8), "batch=")]:
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.StepBuffers(_graph(), 16, **kw, dtype=dtype)
    with pytest.raises(ValueError, match="dtype is None, torch.float32"):
        spjoin.StepBuffers(_graph(), 16, dtype=torch.int16)


@pytest.mark.parametrize("dtype", HALF)
def test_rand_r_buffers_on_a_graph_with_dead_ends_are_refused_as_ever(L, dtype):
    from surel_plus_amd import spjoin
    with pytest.raises(ValueError, match="dead ends"):
        spjoin.StepBuffers(_graph(_rand_r_dead_ends=True), 16, rng="rand_r", dtype=dtype)
    with pytest.raises(ValueError, match="dead ends"):
        spjoin.StepBuffers(_graph(_rand_r_dead_ends=True), 16, rng="rand_r")


@pytest.mark.parametrize("dtype", HALF)
def test_sample_and_gather_refuses_what_the_half_rows_do_not_cover(dtype):
    from surel_plus_amd import spjoin
    e = torch.zeros((2, 4), dtype=torch.int64)
    for kw, name in [(dict(ptr=False), "ptr=False"), (dict(lazy=True), "lazy=True"), (dict(key_rows=False), "key_rows=False"),
                     (dict(strided=False), "strided=False"), (dict(num_walks=200, num_steps=4), "64-bit keys"),
                     (dict(num_walks=1000, num_steps=3), "no key rows")]:
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.sample_and_gather(_graph(), e, **kw, dtype=dtype)
    # a step that passes buffers= asks for the dtype they were made with
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    for bufs, asked in [(SimpleNamespace(half=0, dtype=torch.float32), dtype), (SimpleNamespace(half=3 - HALF.index(dtype) - 1, dtype=other), dtype),
                        (SimpleNamespace(half=HALF.index(dtype) + 1, dtype=dtype), None),
                        (SimpleNamespace(half=HALF.index(dtype) + 1, dtype=dtype), torch.float32)]:
        with pytest.raises(ValueError, match="buffers= were made with dtype"):
            spjoin.sample_and_gather(_graph(), e, buffers=bufs, dtype=asked)


def test_only_the_four_row_form_calls_take_the_argument():
    """gather_many, gather_star, hgather, pgather, CapturedStep and CapturedJoin keep their signatures"""
    import inspect
    import surel_plus_amd as sp
    from surel_plus_amd import spjoin
    for fn in (spjoin.sjoin, spjoin.gather, spjoin.sample_and_gather, spjoin.StepBuffers.__init__):
        assert inspect.signature(fn).parameters["dtype"].default is None
    for name in ("gather_many", "gather_star", "hgather", "pgather", "CapturedStep", "CapturedJoin"):
        fn = getattr(spjoin, name, None) or getattr(sp, name)
        assert "dtype" not in inspect.signature(fn).parameters, name

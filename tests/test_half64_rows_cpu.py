"""CPU: the join's rows in a 16-bit type over 64-bit key rows -- the sixth header and its binding, every fault subgacc_sjoin_fill_half64
refuses before it launches anything (return code, a message led by its name and naming the cause), and what sjoin / gather /
sample_and_gather / StepBuffers do with wide_keys=True beside dtype=torch.float16 / torch.bfloat16 before they touch a device.
No GPU needed."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import shutil
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF64_H = os.path.join(ROOT, "include", "subgacc_half64.h")
NAME = "subgacc_sjoin_fill_half64"


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_sixth_header_parses_and_adds_one_entry_point(L):
    from surel_plus_amd import _lib
    assert _lib.HALF64_HEADER == HALF64_H
    decls = _lib.parse_header(open(HALF64_H).read())
    assert list(decls) == [NAME] == list(_lib.HALF64_SYMBOLS) == list(_lib.HALF64_DECLS)
    ret, args = decls[NAME]
    assert ret == "int" and args == [("d", "const subgacc_join_desc *"), ("out_dtype", "int32_t"), ("out_rows", "void *"),
                                     ("stream", "void *")]
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.argtypes == [C.POINTER(_lib.JoinDesc), C.c_int32, C.c_void_p, C.c_void_p] and fn.restype is C.c_int


def test_the_other_headers_keep_their_entry_points(L):
    from surel_plus_amd import _lib
    assert len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and NAME not in _lib.SYMBOLS
    assert _lib.HALF_SYMBOLS == ("subgacc_sjoin_fill_half",)
    assert (len(_lib.SMALL_SYMBOLS), len(_lib.PACKED_SYMBOLS), len(_lib.WIDE_SYMBOLS)) == (1, 4, 2)
    assert C.sizeof(_lib.JoinDesc) == 248


def test_a_missing_sixth_header_is_an_error_that_names_the_path(tmp_path):
    """a copy of _lib.py in a tree that has the five other headers but not include/subgacc_half64.h refuses to import"""
    (tmp_path / "pkg").mkdir()
    (tmp_path / "include").mkdir()
    for h in ("subgacc.h", "subgacc_half.h", "subgacc_small.h", "subgacc_packed.h", "subgacc_wide.h"):
        shutil.copy(os.path.join(ROOT, "include", h), str(tmp_path / "include" / h))
    shutil.copy(os.path.join(ROOT, "surel_plus_amd", "_lib.py"), str(tmp_path / "pkg" / "_lib.py"))
    spec = importlib.util.spec_from_file_location("_lib_without_half64_header", str(tmp_path / "pkg" / "_lib.py"))
    with pytest.raises(RuntimeError, match=re.escape(os.path.join(str(tmp_path), "include", "subgacc_half64.h"))) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "SubgAccError"


def test_build_watches_the_sixth_header():
    from surel_plus_amd import _lib
    assert "HALF64_HEADER" in inspect.getsource(_lib.build)


# -------------------------------------------------------------------------------------------------------- subgacc_sjoin_fill_half64
def _desc(here, layout="strided"):
    """a mirrored descriptor over strided rows of 64-bit keys that the library accepts up to its launch: B = 2 pairs (S = 4), M = 200,
    4 hops.  It is only ever passed with one change the library refuses -- its pointers are host memory."""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_KEY64
    if layout == "packed":
        d.row_off, d.max_len = here, 32
    elif layout == "headed":
        d.row_stride = 32
    else:
        d.row_len, d.row_stride = here, 32
    d.n_rows, d.S, d.pair_block, d.num_walks, d.num_steps = 4, 4, 2, 200, 4
    d.ids = d.payload = d.own = d.flags = d.seg = here
    return d


def _fill(L, change=None, dtype=2, out="here", layout="strided", null_desc=False):
    buf = (C.c_int64 * 64)()
    here = (C.addressof(buf) + 15) & ~15
    d = _desc(here, layout)
    for name, val in (change or {}).items():
        setattr(d, name, here if val == "here" else val)
    out = {"here": here, "odd": here + 8, None: None}[out]
    rc = L.subgacc_sjoin_fill_half64(None if null_desc else C.byref(d), dtype, out, None)
    return rc, L.subgacc_last_error()


REFUSALS = [
    pytest.param(dict(null_desc=True), "ERR_BADARG", b"null descriptor", id="null-descriptor"),
    pytest.param(dict(change=dict(struct_bytes=240)), "ERR_BADARG", b"descriptor of 240 bytes", id="wrong-size-descriptor"),
    pytest.param(dict(change=dict(row_off="here")), "ERR_BADARG", b"exactly one of row_off", id="two-row-layouts"),
    pytest.param(dict(change=dict(row_stride=0)), "ERR_BADARG", b"row_stride = 0", id="bad-row-stride"),
    pytest.param(dict(change=dict(S=-4)), "ERR_BADARG", b"none may be negative", id="negative-S"),
    pytest.param(dict(change=dict(n_rows=-1)), "ERR_BADARG", b"none may be negative", id="negative-n_rows"),
    pytest.param(dict(change=dict(max_len=-1)), "ERR_BADARG", b"none may be negative", id="negative-max_len"),
    pytest.param(dict(change=dict(form=1)), "ERR_BADARG", b"form ROWS", id="count-form"),
    pytest.param(dict(change=dict(form=2)), "ERR_BADARG", b"form ROWS", id="pair-form"),
    pytest.param(dict(change=dict(options=1)), "ERR_BADARG", b"no option", id="opt-sizes"),
    pytest.param(dict(change=dict(options=2)), "ERR_BADARG", b"no option", id="opt-star"),
    pytest.param(dict(change=dict(options=4)), "ERR_BADARG", b"no option", id="unknown-option"),
    pytest.param(dict(change=dict(payload_kind=0)), "ERR_BADARG", b"payload kind 0 (SFPTR", id="payload-sfptr"),
    pytest.param(dict(change=dict(payload_kind=1)), "ERR_BADARG", b"payload kind 1 (F64", id="payload-f64"),
    pytest.param(dict(change=dict(payload_kind=2)), "ERR_BADARG", b"payload kind 2 (KEY32", id="payload-key32"),
    pytest.param(dict(change=dict(payload_kind=2, num_walks=200, num_steps=3)), "ERR_BADARG", b"payload kind 2 (KEY32", id="payload-key32-narrow-shape"),
    pytest.param(dict(change=dict(payload_kind=7)), "ERR_BADARG", b"payload kind 7", id="payload-unknown"),
    pytest.param(dict(layout="packed"), "ERR_BADARG", b"strided rows", id="packed-rows"),
    pytest.param(dict(layout="headed"), "ERR_BADARG", b"strided rows", id="headed-rows"),
    pytest.param(dict(change=dict(pair_block=0)), "ERR_BADARG", b"pair_block > 0", id="not-mirrored"),
    pytest.param(dict(change=dict(pair_block=-2)), "ERR_BADARG", b"pair_block > 0", id="negative-pair-block"),
    pytest.param(dict(change=dict(S=6)), "ERR_BADARG", b"not a multiple of 2*pair_block", id="S-not-whole-blocks"),
    pytest.param(dict(change=dict(seg=None)), "ERR_BADARG", b"seg = NULL", id="null-seg"),
    pytest.param(dict(change=dict(out_xz="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_xz-set"),
    pytest.param(dict(change=dict(out_idx="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_idx-set"),
    pytest.param(dict(change=dict(out_segid="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_segid-set"),
    pytest.param(dict(change=dict(out_counts="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_counts-set"),
    pytest.param(dict(change=dict(out_pairs="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_pairs-set"),
    pytest.param(dict(change=dict(out_mult="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_mult-set"),
    pytest.param(dict(change=dict(out_cnt="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_cnt-set"),
    pytest.param(dict(change=dict(out_seg="here")), "ERR_BADARG", b"out_* fields must be NULL", id="out_seg-set"),
    pytest.param(dict(change=dict(num_walks=0)), "ERR_BADARG", b"must be positive", id="num_walks-0"),
    pytest.param(dict(change=dict(num_steps=0)), "ERR_BADARG", b"must be positive", id="num_steps-0"),
    pytest.param(dict(change=dict(num_walks=65535, num_steps=4)), "ERR_KEYWIDTH", b"do not fit 63 bits", id="keys-of-65-bits"),
    pytest.param(dict(change=dict(num_walks=2047, num_steps=6)), "ERR_KEYWIDTH", b"do not fit 63 bits", id="keys-of-67-bits"),
    pytest.param(dict(change=dict(num_walks=2 ** 21 - 2, num_steps=3)), "ERR_KEYWIDTH", b"do not fit 63 bits", id="keys-of-64-bits"),
    pytest.param(dict(change=dict(num_walks=3, num_steps=5)), "ERR_BADARG", b"k = 6", id="k-6"),
    pytest.param(dict(dtype=0), "ERR_BADARG", b"out_dtype = 0", id="dtype-0"),
    pytest.param(dict(dtype=3), "ERR_BADARG", b"out_dtype = 3", id="dtype-3"),
    pytest.param(dict(out=None), "ERR_BADARG", b"out_rows = NULL", id="null-out-rows"),
    pytest.param(dict(out="odd"), "ERR_BADARG", b"16-byte aligned", id="misaligned-out-rows"),
    pytest.param(dict(change=dict(row_stride=8193)), "ERR_LDS", b"LDS", id="rows-beyond-lds"),
    pytest.param(dict(change=dict(flags=None)), "ERR_BADARG", b"null argument", id="null-flags"),
    pytest.param(dict(change=dict(ids=None)), "ERR_BADARG", b"null argument", id="null-ids"),
    pytest.param(dict(change=dict(payload=None)), "ERR_BADARG", b"null argument", id="null-payload"),
    pytest.param(dict(change=dict(own=None)), "ERR_BADARG", b"own = NULL", id="null-own"),
]


@pytest.mark.parametrize("how,status,cause", REFUSALS)
def test_fill_half64_refuses_before_any_launch(L, how, status, cause):
    from surel_plus_amd import _lib
    rc, msg = _fill(L, **how)
    assert rc == getattr(_lib, status), msg
    assert msg.startswith(b"sjoin_fill_half64: ") and cause in msg, msg


@pytest.mark.parametrize("dtype", [1, 2])
def test_an_empty_list_launches_nothing(L, dtype):
    """S = 0: accepted without a device -- nothing is launched -- with and without the pointers a list would need; rows of exactly
    160 KiB of LDS (8,192 members of 20 bytes) are within the limit"""
    assert _fill(L, change=dict(S=0), dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0, seg=None, own=None, flags=None, ids=None, payload=None), out=None, dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0, row_stride=8192), dtype=dtype)[0] == 0


# --------------------------------------------------------------------------------------------------------------- the Python layer
HALF = [torch.float16, torch.bfloat16]


def _graph(**more):
    return SimpleNamespace(device="cpu", **more)


def _rows():
    return torch.zeros(4, dtype=torch.int64)


def _wide_store():
    return _graph(payload_is_slot=True, keyrows=True, key64=True)


@pytest.mark.parametrize("dtype", HALF)
def test_without_the_keyword_the_four_calls_refuse_the_shape_as_ever(dtype):
    from surel_plus_amd import spjoin
    e = torch.zeros((2, 4), dtype=torch.int64)
    words = re.escape(f"dtype={dtype} (16-bit rows: pairs with segment pointers over 32-bit LP keys or a packed SFptr store) does not go with ")
    with pytest.raises(ValueError, match="^sjoin: " + words + "64-bit keys$"):
        spjoin.sjoin(_wide_store(), _rows(), None, pair_block=2, dtype=dtype)
    with pytest.raises(ValueError, match="^gather: " + words + "64-bit keys$"):
        spjoin.gather(torch.zeros((2, 2), dtype=torch.int64), _wide_store(), dtype=dtype)
    shape = re.escape("num_walks = 200, num_steps = 4 (64-bit keys, or no key rows)") + "$"
    with pytest.raises(ValueError, match="^sample_and_gather: " + words + shape):
        spjoin.sample_and_gather(_graph(), e, num_walks=200, num_steps=4, dtype=dtype)
    with pytest.raises(ValueError, match="^StepBuffers: " + words + shape):
        spjoin.StepBuffers(_graph(), 16, num_walks=200, num_steps=4, dtype=dtype)
    with pytest.raises(ValueError, match="^StepBuffers: " + words + shape):
        spjoin.StepBuffers(_graph(), 16, num_walks=200, num_steps=4, dtype=dtype, wide_keys=False)


@pytest.mark.parametrize("dtype", HALF)
def test_with_the_keyword_sjoin_and_gather_refuse_what_stays_outside(dtype):
    from surel_plus_amd import spjoin
    from surel_plus_amd.spg import HeadedSpG
    for kw, name in [(dict(ptr_mode=False), "ptr=False"), (dict(return_index=True), "return_index"), (dict(lazy=True), "lazy=True"),
                     (dict(star=True), "star=True"), (dict(pair_block=0), "pair_block")]:
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.sjoin(_wide_store(), _rows(), None, **{"pair_block": 2, **kw}, dtype=dtype, wide_keys=True)
    headed = HeadedSpG.__new__(HeadedSpG)
    headed.device, headed.data = "cpu", torch.zeros(1, dtype=torch.int32)
    headed64 = HeadedSpG.__new__(HeadedSpG)
    headed64.device, headed64.data, headed64.key64 = "cpu", torch.zeros(1, dtype=torch.int64), True
    for x, name in [(headed, "HeadedSpG"), (headed64, "HeadedSpG"),
                    (_graph(payload_is_slot=False, data=torch.zeros(1, dtype=torch.float64)), "float64 store"),
                    (_graph(payload_is_slot=False, data=torch.zeros(1, dtype=torch.int64), key64=True), "64-bit keys"),
                    (_graph(payload_is_slot=True, keyrows=False), "key_rows=False")]:
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.sjoin(x, _rows(), None, pair_block=2, dtype=dtype, wide_keys=True)
        with pytest.raises(ValueError, match=re.escape(name)):
            spjoin.gather(torch.zeros((2, 2), dtype=torch.int64), x, dtype=dtype, wide_keys=True)
    e = torch.zeros((2, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=re.escape("ptr=False")):
        spjoin.gather(e, _wide_store(), ptr=False, dtype=dtype, wide_keys=True)
    with pytest.raises(ValueError, match=re.escape("lazy=True")):
        spjoin.gather(e, _wide_store(), lazy=True, out=torch.empty(8), dtype=dtype, wide_keys=True)
    with pytest.raises(ValueError, match="dtype is None, torch.float32"):
        spjoin.sjoin(_wide_store(), _rows(), None, pair_block=2, dtype=torch.float64, wide_keys=True)


STEP_REFUSALS = [(dict(ptr=False), "ptr=False"), (dict(triplets=True), "triplets=True"), (dict(stage="counts"), "stage='counts'"),
                 (dict(key_rows=False), "key_rows=False"), (dict(batch=8), "batch=")]
SHAPE_REFUSALS = [(dict(num_walks=205, num_steps=4), "no key rows"), (dict(num_walks=300, num_steps=3), "no key rows")]


@pytest.mark.parametrize("dtype", HALF)
def test_with_the_keyword_step_buffers_refuse_what_stays_outside(dtype):
    from surel_plus_amd import spjoin
    for kw, name in STEP_REFUSALS + SHAPE_REFUSALS:
        with pytest.raises(ValueError, match=re.escape(name)) as e:
            spjoin.StepBuffers(_graph(), 16, **{"num_walks": 200, "num_steps": 4, **kw}, dtype=dtype, wide_keys=True)
        assert str(e.value).startswith(f"StepBuffers: dtype={dtype} (16-bit rows")
    with pytest.raises(ValueError, match="dtype is None, torch.float32"):
        spjoin.StepBuffers(_graph(), 16, num_walks=200, num_steps=4, dtype=torch.int16, wide_keys=True)


@pytest.mark.parametrize("dtype", HALF)
def test_rand_r_buffers_on_a_graph_with_dead_ends_are_refused_as_ever(L, dtype):
    from surel_plus_amd import spjoin
    with pytest.raises(ValueError, match="dead ends"):
        spjoin.StepBuffers(_graph(_rand_r_dead_ends=True), 16, num_walks=200, num_steps=4, rng="rand_r", dtype=dtype, wide_keys=True)


@pytest.mark.parametrize("dtype", HALF)
def test_with_the_keyword_sample_and_gather_refuses_what_stays_outside(dtype):
    from surel_plus_amd import spjoin
    e = torch.zeros((2, 4), dtype=torch.int64)
    for kw, name in [(dict(ptr=False), "ptr=False"), (dict(lazy=True), "lazy=True"), (dict(key_rows=False), "key_rows=False"),
                     (dict(strided=False), "strided=False")] + SHAPE_REFUSALS:
        with pytest.raises(ValueError, match=re.escape(name)) as err:
            spjoin.sample_and_gather(_graph(), e, **{"num_walks": 200, "num_steps": 4, **kw}, dtype=dtype, wide_keys=True)
        assert str(err.value).startswith(f"sample_and_gather: dtype={dtype} (16-bit rows")


@pytest.mark.parametrize("dtype", HALF)
def test_buffers_of_another_half_or_wide_setting_are_refused(dtype):
    """before any device work: the graph and the buffers are plain namespaces"""
    from surel_plus_amd import spjoin
    e = torch.zeros((2, 4), dtype=torch.int64)
    code, other = HALF.index(dtype) + 1, HALF[1 - HALF.index(dtype)]
    wide = dict(num_walks=200, num_steps=4, wide_keys=True)
    for bufs, kw in [(SimpleNamespace(half=0, dtype=torch.float32), dict(dtype=dtype, **wide)),                       # f32 buffers
                     (SimpleNamespace(half=3 - code, dtype=other, half64=True), dict(dtype=dtype, **wide)),          # the other 16-bit type
                     (SimpleNamespace(half=code, dtype=dtype, half64=False), dict(dtype=dtype, **wide)),             # 32-bit-key buffers
                     (SimpleNamespace(half=code, dtype=dtype), dict(dtype=dtype, **wide)),
                     (SimpleNamespace(half=code, dtype=dtype, half64=True), dict(dtype=None, **wide)),               # an f32 call
                     (SimpleNamespace(half=code, dtype=dtype, half64=True), dict(dtype=torch.float32, **wide)),
                     (SimpleNamespace(half=code, dtype=dtype, half64=True), dict(dtype=dtype, num_walks=200, num_steps=3, wide_keys=True)),
                     (SimpleNamespace(half=code, dtype=dtype, half64=True), dict(dtype=dtype, num_walks=200, num_steps=3))]:
        with pytest.raises(ValueError, match="buffers= were made with dtype"):
            spjoin.sample_and_gather(_graph(), e, buffers=bufs, **kw)


@pytest.mark.parametrize("dtype", HALF)
def test_at_a_32_bit_shape_the_keyword_changes_no_refusal(dtype):
    """(200, 3): every refusal of tests/test_half_rows_cpu.py stands with wide_keys=True, word for word what it is without"""
    from surel_plus_amd import spjoin
    e = torch.zeros((2, 4), dtype=torch.int64)

    def said(fn, *a, **kw):
        with pytest.raises(ValueError) as err:
            fn(*a, **kw)
        return str(err.value)

    for kw, name in STEP_REFUSALS:
        a, b = (said(spjoin.StepBuffers, _graph(), 16, num_walks=200, num_steps=3, **kw, dtype=dtype, wide_keys=w) for w in (False, True))
        assert a == b and name in a
    for kw, name in [(dict(ptr=False), "ptr=False"), (dict(lazy=True), "lazy=True"), (dict(key_rows=False), "key_rows=False"),
                     (dict(strided=False), "strided=False")]:
        a, b = (said(spjoin.sample_and_gather, _graph(), e, num_walks=200, num_steps=3, **kw, dtype=dtype, wide_keys=w) for w in (False, True))
        assert a == b and name in a
    # buffers made without the keyword serve a call with it, and the other way round: the mismatch left is the dtype's
    bufs = SimpleNamespace(half=0, dtype=torch.float32)
    a, b = (said(spjoin.sample_and_gather, _graph(), e, num_walks=200, num_steps=3, buffers=bufs, dtype=dtype, wide_keys=w) for w in (False, True))
    assert a == b and "buffers= were made with dtype" in a and "wide_keys" not in a
    # the 32-bit-key buffers of such a call pass the check and are refused only for what a namespace is not
    ok = SimpleNamespace(half=HALF.index(dtype) + 1, dtype=dtype, half64=False)
    with pytest.raises(AttributeError):
        spjoin.sample_and_gather(_graph(), e, num_walks=200, num_steps=3, buffers=ok, dtype=dtype, wide_keys=True)


def test_the_signatures():
    """wide_keys=False follows dtype on the four row-form calls; in sample_and_gather it is a named keyword in front of **kw;
    gather_many, gather_star, hgather, pgather, CapturedStep and CapturedJoin keep their signatures"""
    import surel_plus_amd as sp
    from surel_plus_amd import spjoin
    for fn in (spjoin.sjoin, spjoin.gather, spjoin.sample_and_gather):
        names = list(inspect.signature(fn).parameters)
        p = inspect.signature(fn).parameters["wide_keys"]
        assert p.default is False and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        assert names[names.index("dtype") + 1] == "wide_keys", fn
    names = list(inspect.signature(spjoin.sample_and_gather).parameters)
    assert names[-2:] == ["wide_keys", "kw"]
    sb = inspect.signature(spjoin.StepBuffers.__init__).parameters
    assert sb["wide_keys"].default is False and sb["dtype"].default is None
    for name in ("gather_many", "gather_star", "hgather", "pgather", "CapturedStep", "CapturedJoin"):
        fn = getattr(spjoin, name, None) or getattr(sp, name)
        params = inspect.signature(fn).parameters
        assert "dtype" not in params and "wide_keys" not in params, name


def test_the_keyword_does_not_reach_the_sampler(monkeypatch):
    """the unbuffered sample_and_gather hands **kw to sample_spg: wide_keys is not among it"""
    from surel_plus_amd import spg, spjoin
    seen = {}

    def fake_sample_spg(csr, roots, **kw):
        seen.update(kw)
        raise RuntimeError("far enough")

    monkeypatch.setattr(spg, "sample_spg", fake_sample_spg)
    with pytest.raises(RuntimeError, match="far enough"):
        spjoin.sample_and_gather(_graph(), torch.zeros((2, 4), dtype=torch.int64), num_walks=200, num_steps=4, dtype=torch.bfloat16,
                                 wide_keys=True, bucket=0)
    assert "wide_keys" not in seen and seen["bucket"] == 0 and seen["num_walks"] == 200

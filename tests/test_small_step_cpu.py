"""CPU: the row-form step at the small walk shapes (small_rows=True) and the 16-bit row join with segment ids -- the eighth header and
its binding, every fault subgacc_sjoin_fill_half_ids refuses before it launches anything (return code, a message led by its name),
what StepBuffers / sample_and_gather / sample_and_hgather refuse of the keyword before they touch a device, that the keyword changes
nothing at a shape that is not small, and a NumPy restatement of "rows -> (xz.to(dtype), segid)" against a golden of the reference's
join.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import join_rows_edges as J
from test_half_rows_cpu import REFUSALS, _desc, _sfptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS_H = os.path.join(ROOT, "include", "subgacc_half_ids.h")
NAME = "subgacc_sjoin_fill_half_ids"
HALF = [torch.float16, torch.bfloat16]
SMALL = [(100, 2), (50, 1), (203, 1), (67, 3), (50, 4)]


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_eighth_header_parses_and_adds_one_entry_point(L):
    from surel_plus_amd import _lib
    decls = _lib.parse_header(open(IDS_H).read())
    assert list(decls) == [NAME] == list(_lib.HALF_IDS_SYMBOLS) and _lib.HALF_IDS_HEADER == IDS_H
    ret, args = decls[NAME]
    assert ret == "int" and args == [("d", "const subgacc_join_desc *"), ("out_dtype", "int32_t"), ("out_rows", "void *"),
                                     ("out_segid", "int64_t *"), ("stream", "void *")]
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.argtypes == [C.POINTER(_lib.JoinDesc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] and fn.restype is C.c_int
    assert NAME not in _lib.SYMBOLS and len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and L.subgacc_abi_version() == 7
    assert list(_lib.HALF_SYMBOLS) == ["subgacc_sjoin_fill_half"]    # the second header keeps its one entry point


def test_the_makefile_and_the_staleness_check_name_the_header():
    from surel_plus_amd import _lib
    make = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^build/%\.o:.*$", make, re.M).group(0)
    assert "../../include/subgacc_half_ids.h" in rule and "sjoin_half.hip" in re.search(r"^SRCS\s*:=.*$", make, re.M).group(0)
    assert "HALF_IDS_HEADER" in inspect.getsource(_lib.build)


# ------------------------------------------------------------------------------------------------------ subgacc_sjoin_fill_half_ids
def _fill(L, change=None, dtype=2, out="here", segid="here", packed=False, sfptr=None, null_desc=False):
    buf = (C.c_int64 * 64)()
    here = (C.addressof(buf) + 15) & ~15
    d = _desc(here, packed)
    if sfptr is not None:
        _sfptr(d, here, sfptr)
    for name, val in (change or {}).items():
        setattr(d, name, here if val == "here" else val)
    where = {"here": here, "odd": here + 8, None: None}
    rc = getattr(L, NAME)(None if null_desc else C.byref(d), dtype, where[out], where[segid], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("how,status,cause", REFUSALS + [
    pytest.param(dict(segid=None), "ERR_BADARG", b"out_segid = NULL", id="null-out-segid")])
def test_fill_half_ids_refuses_before_any_launch(L, how, status, cause):
    """every refusal of subgacc_sjoin_fill_half (tests/test_half_rows_cpu.py: REFUSALS), with this entry point's name in front, and
    out_segid = NULL"""
    from surel_plus_amd import _lib
    rc, msg = _fill(L, **how)
    assert rc == getattr(_lib, status), msg
    assert msg.startswith(b"sjoin_fill_half_ids: ") and cause in msg, msg


@pytest.mark.parametrize("dtype", [1, 2])
def test_an_empty_list_launches_nothing(L, dtype):
    """S = 0: accepted without a device, with and without the pointers a list would need -- out_segid among them"""
    assert _fill(L, change=dict(S=0), dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0, seg=None, own=None, flags=None, ids=None, payload=None), out=None, segid=None, dtype=dtype)[0] == 0
    assert _fill(L, change=dict(S=0), segid="odd", dtype=dtype)[0] == 0


# --------------------------------------------------------------------------------------------------------------- the Python layer
def _graph(**more):
    return SimpleNamespace(device="cpu", **more)


E = torch.zeros((2, 4), dtype=torch.int64)
H3 = torch.zeros((3, 4), dtype=torch.int64)


@pytest.mark.parametrize("M,m", SMALL)
def test_step_buffers_refuse_by_the_keywords_name(M, m):
    from surel_plus_amd import spjoin
    for kw, name in [(dict(key_rows=False), "key_rows=False"), (dict(packed_rows=True), "packed_rows=True"),
                     (dict(packed_half=True, dtype=torch.bfloat16), "packed_half=True"),
                     (dict(dtype=torch.float16, batch=8), "batch="), (dict(dtype=torch.bfloat16, batch=8), "batch=")]:
        with pytest.raises(ValueError, match=re.escape("small_rows=True")) as err:
            spjoin.StepBuffers(_graph(), 16, num_walks=M, num_steps=m, small_rows=True, **kw)
        assert name in str(err.value), (kw, str(err.value))


@pytest.mark.parametrize("M,m", SMALL)
def test_the_calls_refuse_by_the_keywords_name(M, m):
    from surel_plus_amd import spjoin
    shape = dict(num_walks=M, num_steps=m, small_rows=True)
    for kw, name in [(dict(key_rows=False), "key_rows=False"), (dict(packed_rows=True), "packed_rows=True"),
                     (dict(packed_half=True), "packed_half=True"), (dict(strided=False), "strided=False"),
                     (dict(dtype=torch.float16, lazy=True), "lazy=True"), (dict(dtype=torch.bfloat16, lazy=True), "lazy=True")]:
        with pytest.raises(ValueError, match=re.escape("small_rows=True")) as err:
            spjoin.sample_and_gather(_graph(), E, **shape, **kw)
        assert name in str(err.value), (kw, str(err.value))
    for kw, name in [(dict(key_rows=False), "key_rows=False"), (dict(packed_rows=True), "packed_rows=True"),
                     (dict(packed_half=True), "packed_half=True")]:
        with pytest.raises(ValueError, match=re.escape("small_rows=True")) as err:
            spjoin.sample_and_hgather(_graph(), H3, **shape, **kw)
        assert name in str(err.value), (kw, str(err.value))
    # buffers= made for the other route, either way round
    for bufs, small_rows in [(SimpleNamespace(half=0, small=False, stage=None), True), (SimpleNamespace(half=0, small=True, stage=None), False)]:
        with pytest.raises(ValueError, match=re.escape("small_rows=")):
            spjoin.sample_and_gather(_graph(), E, num_walks=M, num_steps=m, small_rows=small_rows, buffers=bufs)
        with pytest.raises(ValueError, match=re.escape("small_rows=")):
            spjoin.sample_and_hgather(_graph(), H3, num_walks=M, num_steps=m, small_rows=small_rows, buffers=bufs)
    # ... and for another dtype, as at every other shape
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        spjoin.sample_and_gather(_graph(), E, **shape, dtype=torch.bfloat16, ptr=False, buffers=SimpleNamespace(half=0, dtype=torch.float32))
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        spjoin.sample_and_hgather(_graph(), H3, **shape, dtype=torch.bfloat16, buffers=SimpleNamespace(half=0, dtype=torch.float32))


@pytest.mark.parametrize("dtype", HALF)
def test_half_rows_of_a_small_shape_need_the_keyword(dtype):
    """without small_rows=True every refusal of a 16-bit dtype at a small shape stands, and sample_and_hgather has 16-bit rows nowhere
    else"""
    from surel_plus_amd import spjoin
    for M, m in SMALL:
        with pytest.raises(ValueError, match="64-bit keys, or no key rows"):
            spjoin.StepBuffers(_graph(), 16, num_walks=M, num_steps=m, dtype=dtype)
        with pytest.raises(ValueError, match="64-bit keys, or no key rows"):
            spjoin.sample_and_gather(_graph(), E, num_walks=M, num_steps=m, dtype=dtype)
        with pytest.raises(ValueError, match="triplets"):
            spjoin.sample_and_hgather(_graph(), H3, num_walks=M, num_steps=m, dtype=dtype)
    with pytest.raises(ValueError, match="triplets"):
        spjoin.sample_and_hgather(_graph(), H3, num_walks=200, num_steps=3, dtype=dtype, small_rows=True)


@pytest.mark.parametrize("dtype", HALF)
def test_the_keyword_changes_nothing_at_200_3(dtype):
    """a shape of the fused-row kernel: the refusals tests/test_half_rows_cpu.py pins keep their words with the keyword"""
    from surel_plus_amd import sampler, spjoin
    assert not sampler.small_rows_form(200, 3) and sampler.key_rows_form(200, 3) == 32 and sampler.rows_kernel_takes(200, 3)
    assert sampler.walk_kernel_name(None, 200, 3, True) == "walk_rows_kernel"
    for kw, name in [(dict(ptr=False), "ptr=False"), (dict(triplets=True), "triplets=True"), (dict(stage="counts"), "stage='counts'"),
                     (dict(key_rows=False), "key_rows=False"), (dict(num_walks=200, num_steps=4), "64-bit keys"),
                     (dict(num_walks=300, num_steps=3), "no key rows"), (dict(batch=8), "batch=")]:
        with pytest.raises(ValueError, match=re.escape(name)) as err:
            spjoin.StepBuffers(_graph(), 16, **{"num_walks": 200, "num_steps": 3, **kw}, dtype=dtype, small_rows=True)
        assert str(err.value).startswith(f"StepBuffers: dtype={dtype} (16-bit rows") and "small_rows" not in str(err.value)
    for kw, name in [(dict(ptr=False), "ptr=False"), (dict(lazy=True), "lazy=True"), (dict(key_rows=False), "key_rows=False"),
                     (dict(strided=False), "strided=False")]:
        with pytest.raises(ValueError, match=re.escape(name)) as err:
            spjoin.sample_and_gather(_graph(), E, num_walks=200, num_steps=3, **kw, dtype=dtype, small_rows=True)
        assert "small_rows" not in str(err.value)
    # what the keyword refuses at a small shape is not refused by it here: these reach the device (a namespace has none)
    with pytest.raises(AttributeError):
        spjoin.StepBuffers(_graph(), 16, num_walks=200, num_steps=3, key_rows=False, small_rows=True)
    # buffers of the fused-row step are served with and without the keyword
    for small_rows in (False, True):
        with pytest.raises(AttributeError):
            spjoin.sample_and_gather(_graph(), E, num_walks=200, num_steps=3, small_rows=small_rows,
                                     buffers=SimpleNamespace(half=0, small=False, stage=None))


def test_the_keyword_is_opt_in_on_three_calls():
    import surel_plus_amd as sp
    from surel_plus_amd import spjoin
    for fn in (spjoin.StepBuffers.__init__, spjoin.sample_and_gather, spjoin.sample_and_hgather):
        assert inspect.signature(fn).parameters["small_rows"].default is False
    for name in ("sjoin", "gather", "hgather", "gather_many", "sample_and_gather_many", "sample_and_counts", "CapturedStep"):
        fn = getattr(spjoin, name, None) or getattr(sp, name)
        assert "small_rows" not in inspect.signature(fn).parameters, name


# ------------------------------------------------------------------------------------------- rows -> (xz.to(dtype), segid), restated
def half_rows_ref(r, dtype):
    """what subgacc_sjoin_fill_half_ids writes for the join `r` of join_rows_edges.join_rows_ref: the f32 rows rounded to nearest even
    as int16 words [R, 2, k], and the segment id of every row"""
    return torch.from_numpy(np.ascontiguousarray(r.xz)).to(dtype).view(torch.int16).numpy(), r.segid


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("name", ["sjoin_int.npz", "sjoin_int_emptyrows.npz"])
def test_the_restatement_reproduces_a_join_golden(name, dtype):
    """the reference's gather(ptr=False) of a golden: xz_ptr0 under .to(dtype) and ind_ptr0"""
    import oracle
    g = np.load(os.path.join(ROOT, "tests", "golden", name))
    rows = J.EdgeRows.from_packed(name, g["z_indptr"], g["z_indices"], g["z_data"].astype(np.int32), "sfptr")
    own, partner = oracle.pair_segments(g["edge"])
    r = J.join_rows_ref(rows, own, None, "sfptr", pair_block=g["edge"].shape[1], table=g["encode"])
    words, segid = half_rows_ref(r, dtype)
    assert r.flags3 == 0 and r.live.all()
    want = torch.from_numpy(g["xz_ptr0"]).to(dtype)
    assert words.shape == g["xz_ptr0"].shape and np.array_equal(words, want.view(torch.int16).numpy())
    assert np.array_equal(segid, g["ind_ptr0"]) and segid.dtype == np.int64
    # the rounding is not a truncation: the golden's rows round in both directions
    back = want.float().numpy()
    assert (back > g["xz_ptr0"]).any() and (back < g["xz_ptr0"]).any()
    # the ids are the pointers spread out: row r of segment j holds j
    assert np.array_equal(np.searchsorted(g["ind_ptr1"], np.arange(len(segid)), side="right") - 1, segid)

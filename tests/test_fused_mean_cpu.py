"""CPU: the mean first stage fused into the count join of an on-demand step -- the tenth header and its binding, every fault
subgacc_sjoin_key_mean refuses before it launches anything (return code, a message led by its name), what StepBuffers(stage="mean")
refuses before it touches a device, and the NumPy restatement of the kernel's summation chain (tests/fused_mean_ref.py) on
hand-built counts.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from fused_mean_ref import bound, fused_mean

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN_H = os.path.join(ROOT, "include", "subgacc_mean.h")
NAME = "subgacc_sjoin_key_mean"
PUBLIC = ("sample_and_fused_mean_stage", "sample_and_fused_hmean_stage", "sample_and_fused_mean_stage_star",
          "sample_and_fused_hmean_stage_star")


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_tenth_header_declares_exactly_the_one_name(L):
    from surel_plus_amd import _lib
    decls = _lib.parse_header(open(MEAN_H).read())
    assert list(decls) == [NAME] == list(_lib.MEAN_SYMBOLS) and _lib.MEAN_HEADER == MEAN_H
    ret, args = decls[NAME]
    assert ret == "int" and args == [("d", "const subgacc_join_desc *"), ("ukeys", "const int32_t *"), ("n_keys", "const int64_t *"),
                                     ("e", "const float *"), ("width", "int32_t"), ("out_mean", "float *"), ("out_len", "int32_t *"),
                                     ("stream", "void *")]
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.argtypes == [C.POINTER(_lib.JoinDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    # the C ABI and the nine other headers stay as they were
    assert NAME not in _lib.SYMBOLS and len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and L.subgacc_abi_version() == 7
    assert "subgacc_sjoin_key_counts" in _lib.SYMBOLS and list(_lib.STAR_SYMBOLS) == ["subgacc_step_prologue_star"]
    assert C.sizeof(_lib.JoinDesc) == 248


def test_the_symbol_is_exported_by_the_built_library(L):
    from surel_plus_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % NAME, out, re.M)


def test_the_header_states_the_chain_the_formula_and_its_reference_lines():
    txt = open(MEAN_H).read()
    for cite in ("model.py:78-83", "model_horder.py:56-57", "acc = acc + (float)c * e[x*width + h]", "max(size_j, 1)",
                 "max_len*8 + table_rows*12 + 16"):
        assert cite in txt, cite


def test_the_makefile_and_the_staleness_check_name_the_header_and_the_source():
    from surel_plus_amd import _lib
    make = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^build/%\.o:.*$", make, re.M).group(0)
    assert "../../include/subgacc_mean.h" in rule and "sjoin_mean.hip" in re.search(r"^SRCS\s*:=.*$", make, re.M).group(0)
    assert "MEAN_HEADER" in inspect.getsource(_lib.build)
    src = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "sjoin_mean.hip")).read()
    assert f'extern "C" int {NAME}(' in src and "sjoin_key_mean_kernel" in src
    assert "fmaf" not in src and "__builtin_fma" not in src         # a separate multiply and add: the chain is the result


def test_the_public_calls_are_exported():
    import surel_plus_amd as sp
    for name in PUBLIC:
        assert callable(getattr(sp, name)), name
        twin = getattr(sp, name.replace("_fused", ""))
        assert list(inspect.signature(getattr(sp, name)).parameters) == list(inspect.signature(twin).parameters), name


# ------------------------------------------------------------------------------------------------------- subgacc_sjoin_key_mean
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


_KM_KEYS = ("ukeys", "n_keys", "e", "width", "out_mean", "out_len")


def _key_mean(L, change):
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    args = {k: here for k in _KM_KEYS}
    args["width"] = 8
    for k, val in change.items():
        val = here if val == "here" else val
        if k in args:
            args[k] = val
        else:
            setattr(d, k[2:] if k.startswith("d.") else k, val)
    rc = getattr(L, NAME)(C.byref(d), *[args[k] for k in _KM_KEYS], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,cause", [
    (dict(options=1), b"option"),                                           # every refusal of subgacc_sjoin_key_counts ...
    (dict(options=2), b"option"),
    (dict(payload_kind=0), b"KEY32"),
    (dict(payload_kind=1), b"KEY32"),
    (dict(payload_kind=3), b"KEY32"),
    (dict(row_len=None, row_off="here"), b"strided key rows"),
    (dict(row_len=None), b"strided key rows"),
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
    (dict(ukeys=None), b"are required"),                                    # ... and its own
    (dict(n_keys=None), b"are required"),
    (dict(e=None), b"are required"),
    (dict(out_mean=None), b"are required"),
    (dict(width=0), b"width = 0"),
    (dict(width=-1), b"width = -1"),
    (dict(width=1025), b"width = 1025"),
])
def test_key_mean_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _key_mean(L, change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"sjoin_key_mean: ") and cause in msg, msg


def test_key_mean_refuses_in_the_order_of_the_count_form(L):
    """a descriptor fault is named before a NULL argument, a NULL argument before the width, the width before the LDS request"""
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    fn = getattr(L, NAME)
    assert fn(None, here, here, here, 8, here, here, None) == _lib.ERR_BADARG
    assert L.subgacc_last_error().startswith(b"sjoin_key_mean: null descriptor")
    d = _desc(here)
    d.struct_bytes -= 8
    assert fn(C.byref(d), here, here, here, 8, here, here, None) == _lib.ERR_BADARG and b"struct_bytes" in L.subgacc_last_error()
    rc, msg = _key_mean(L, dict(options=1, e=None, width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"option" in msg
    rc, msg = _key_mean(L, dict(e=None, width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"are required" in msg
    rc, msg = _key_mean(L, dict(width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"width" in msg
    rc, msg = _key_mean(L, dict(out_len=None, table_rows=14000))             # out_len is optional
    assert rc == _lib.ERR_LDS


@pytest.mark.parametrize("change", [dict(table_rows=14000), dict(row_stride=21000), dict(row_stride=8192, table_rows=9000)])
def test_key_mean_refuses_what_lds_does_not_hold(L, change):
    """8 row_stride + 12 T + 16 bytes beyond the 160 KiB of a CU: SUBGACC_ERR_LDS before any launch, naming table_rows"""
    from surel_plus_amd import _lib
    rc, msg = _key_mean(L, change)
    assert rc == _lib.ERR_LDS
    assert msg.startswith(b"sjoin_key_mean: ") and b"LDS" in msg and b"table_rows" in msg, msg


def test_key_mean_of_no_segments_is_a_no_op(L):
    """S = 0 launches nothing (host pointers, no device): SUBGACC_OK"""
    rc, _ = _key_mean(L, dict(S=0))
    assert rc == 0


# -------------------------------------------------------------------------------------------------------------------- Python
_NO_DEVICE = SimpleNamespace(device="cpu")       # nothing of it is looked at before the refusals


@pytest.mark.parametrize("kw,cause", [
    (dict(), "width"),                                                      # missing width
    (dict(width=0), "width"),
    (dict(width=1025), "width"),
    (dict(width=8, out=object()), "out="),
    (dict(width=8, ptr=False), "ptr=False"),
    (dict(width=8, num_walks=300, num_steps=3), "no key-rows form"),        # a shape without key rows
    (dict(width=8, num_walks=200, num_steps=4), "key_rows_form == 64"),     # 64-bit keys without wide_keys=True
    (dict(width=8, key_rows=False), "key_rows=False"),
    (dict(width=8, table_rows=1), "table_rows"),
    (dict(width=8, table_rows=16385), "table_rows"),
    (dict(width=8, table_rows=8193, num_walks=200, num_steps=4, wide_keys=True), "table_rows"),
    (dict(width=8, batch=4), "batch=None"),
])
def test_step_buffers_refuse_the_mean_stage_without_a_device(kw, cause):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match=cause):
        sp.StepBuffers(_NO_DEVICE, 8, stage="mean", **kw)


@pytest.mark.parametrize("stage", [None, "counts", "counts_attn", "index"])
def test_width_goes_with_the_mean_stage_alone(stage):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match="width"):
        sp.StepBuffers(_NO_DEVICE, 8, stage=stage, width=8)


def test_refusals_that_were_refusals_stay():
    import torch
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match="stage"):
        sp.StepBuffers(_NO_DEVICE, 8, stage="mean", width=8, dtype=torch.bfloat16)      # a 16-bit dtype beside a stage
    with pytest.raises(ValueError, match="star"):
        sp.StepBuffers(_NO_DEVICE, 8, stage="index", star=2)
    with pytest.raises(ValueError, match="stage"):
        sp.StepBuffers(_NO_DEVICE, 8, stage="rows")
    e, h = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"sample_and_fused_mean_stage: edge must be \[2, B\]"):
        sp.sample_and_fused_mean_stage(_NO_DEVICE, h, torch.nn.Identity())
    with pytest.raises(ValueError, match=r"\[3, B\]"):
        sp.sample_and_fused_hmean_stage(_NO_DEVICE, e, torch.nn.Identity())
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_fused_mean_stage(_NO_DEVICE, e, torch.nn.Identity(), num_walks=200, num_steps=4)
    counts = SimpleNamespace(stage="counts", triplets=False)                 # buffers made for another result
    with pytest.raises(ValueError, match="stage='mean'"):
        sp.sample_and_fused_mean_stage(_NO_DEVICE, e, torch.nn.Identity(), buffers=counts)


# ----------------------------------------------------------------------------------------------------- the restatement of the chain
def test_the_restatement_is_exact_on_integer_rows():
    """small whole numbers: every product and sum is exact in float32, so the chain IS (C @ E) / size"""
    Cm = np.array([[2, 0, 1, 0, 3], [0, 0, 0, 0, 0], [0, 4, 0, 0, 0], [1, 1, 1, 1, 1]])
    sizes = np.array([3, 0, 2, 5])
    E = np.arange(5 * 3, dtype=np.float32).reshape(5, 3) - 6.0
    want = (Cm.astype(np.float64) @ E.astype(np.float64)) / np.maximum(sizes, 1)[:, None]
    got = fused_mean(Cm, sizes, E)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert not got[1].any()                                             # an empty segment: a zero row
    assert np.array_equal(fused_mean(Cm, sizes, E, descending=True), got)
    E[1] = np.nan                                                       # a row whose count is zero is never looked at
    assert np.array_equal(fused_mean(Cm[:2], sizes[:2], E), got[:2])


def test_the_restatement_multiplies_adds_and_divides_in_float32_in_ascending_order():
    """2^24 + 1 + 1: ascending, each 1 is lost to the rounding of the add; descending, 1 + 1 = 2 survives -- other bits"""
    big = np.float32(2.0 ** 24)
    Cm = np.array([[1, 1, 1]])
    E = np.array([[big], [1.0], [1.0]], dtype=np.float32)
    up, down = fused_mean(Cm, [1], E), fused_mean(Cm, [1], E, descending=True)
    assert up[0, 0] == big and down[0, 0] == np.float32(2.0 ** 24 + 2) and up.view(np.uint32)[0, 0] != down.view(np.uint32)[0, 0]
    # the product is rounded before the add (no fused multiply-add): 3 * (1 + 2^-23) rounds to 3 + 2^-21 (a tie, to even); with
    # -3 behind it the chain gives 2^-21, a fused multiply-add would give the exact 3 * 2^-23
    E = np.array([[-3.0], [1.0 + 2.0 ** -23]], dtype=np.float32)
    got = fused_mean(np.array([[1, 3]]), [1], E)
    assert got[0, 0] == np.float32(2.0 ** -21) and got[0, 0] != np.float32(3 * 2.0 ** -23)
    # the division is one float32 division by max(size, 1)
    got = fused_mean(np.array([[1]]), [3], np.array([[1.0]], dtype=np.float32))
    assert got[0, 0] == np.float32(1.0) / np.float32(3.0)
    assert fused_mean(np.array([[1]]), [0], np.array([[5.0]], dtype=np.float32))[0, 0] == 5.0
    # and the derived bound holds for it
    rng = np.random.default_rng(0)
    Cm = rng.integers(0, 4, (6, 40)) * (rng.random((6, 40)) < 0.3)
    E = rng.standard_normal((40, 7)).astype(np.float32)
    sizes = np.maximum(Cm.sum(1) // 2, 1)
    exact = (Cm.astype(np.float64) @ E.astype(np.float64)) / sizes[:, None]
    assert (np.abs(fused_mean(Cm, sizes, E).astype(np.float64) - exact) <= bound(Cm, sizes, E)).all()

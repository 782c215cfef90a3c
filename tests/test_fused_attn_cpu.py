"""CPU: the attentional first stage fused into the attentional count join of an on-demand step -- the eleventh header and its
binding, every fault subgacc_sjoin_key_attn refuses before it launches anything (return code, a message led by its name), what
StepBuffers(stage="attn") refuses before it touches a device, and the NumPy restatement of the kernel's summation chain
(tests/fused_attn_ref.py) on hand-built weights.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from fused_attn_ref import bound, fused_attn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN_H = os.path.join(ROOT, "include", "subgacc_attn.h")
NAME = "subgacc_sjoin_key_attn"
PUBLIC = ("sample_and_fused_attn_stage", "sample_and_fused_attn_stage_star")


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_eleventh_header_declares_exactly_the_one_name(L):
    from surel_plus_amd import _lib
    decls = _lib.parse_header(open(ATTN_H).read())
    assert list(decls) == [NAME] == list(_lib.ATTN_SYMBOLS) and _lib.ATTN_HEADER == ATTN_H and _lib.ATTN_DECLS == decls
    ret, args = decls[NAME]
    assert ret == "int" and args == [("d", "const subgacc_join_desc *"), ("ukeys", "const int32_t *"), ("n_keys", "const int64_t *"),
                                     ("g", "const float *"), ("e", "const float *"), ("width", "int32_t"), ("out_a", "float *"),
                                     ("out_max", "float *"), ("out_den", "float *"), ("out_len", "int32_t *"), ("stream", "void *")]
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.argtypes == [C.POINTER(_lib.JoinDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int
    # the C ABI and the ten other headers stay as they were
    assert NAME not in _lib.SYMBOLS and len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and L.subgacc_abi_version() == 7
    assert "subgacc_sjoin_key_counts_attn" in _lib.SYMBOLS and list(_lib.MEAN_SYMBOLS) == ["subgacc_sjoin_key_mean"]
    assert C.sizeof(_lib.JoinDesc) == 248


def test_the_symbol_is_exported_by_the_built_library(L):
    from surel_plus_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT %s$" % NAME, out, re.M)


def test_the_header_states_the_chain_the_formula_and_its_reference_lines():
    txt = open(ATTN_H).read()
    for cite in ("model.py:59-62,78-81", "acc = acc + W[j, r] * e[r*width + h]", "not the bit pattern of +0.0f",
                 "4 * (7*max_len + 3*table_rows + 2*D + 7)", "D = min(2*max_len, table_rows)", "never a fused multiply-add"):
        assert cite in txt, cite


def test_the_makefile_and_the_staleness_check_name_the_header_and_the_source():
    from surel_plus_amd import _lib
    make = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^build/%\.o:.*$", make, re.M).group(0)
    assert "../../include/subgacc_attn.h" in rule and "sjoin_key_attn.hip" in re.search(r"^SRCS\s*:=.*$", make, re.M).group(0)
    assert "ATTN_HEADER" in inspect.getsource(_lib.build)
    src = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "sjoin_key_attn.hip")).read()
    assert f'extern "C" int {NAME}(' in src and "sjoin_key_attn_kernel" in src
    assert "counts_attn_body<false>" in src                         # the front is the unfused kernel's text, not a copy
    assert "fmaf" not in src and "__builtin_fma" not in src         # a separate multiply and add: the chain is the result


def test_the_public_calls_have_their_twins_signatures():
    import surel_plus_amd as sp
    for name in PUBLIC:
        assert callable(getattr(sp, name)), name
        twin = getattr(sp, name.replace("_fused", ""))
        assert list(inspect.signature(getattr(sp, name)).parameters) == list(inspect.signature(twin).parameters), name
        assert [p.default for p in inspect.signature(getattr(sp, name)).parameters.values()] == \
            [p.default for p in inspect.signature(twin).parameters.values()], name


# ------------------------------------------------------------------------------------------------------- subgacc_sjoin_key_attn
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


_KA_KEYS = ("ukeys", "n_keys", "g", "e", "width", "out_a", "out_max", "out_den", "out_len")


def _key_attn(L, change):
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _desc(here)
    args = {k: here for k in _KA_KEYS}
    args["width"] = 8
    for k, val in change.items():
        val = here if val == "here" else val
        if k in args:
            args[k] = val
        else:
            setattr(d, k, val)
    rc = getattr(L, NAME)(C.byref(d), *[args[k] for k in _KA_KEYS], None)
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
    (dict(g=None), b"are required"),
    (dict(e=None), b"are required"),
    (dict(out_a=None), b"are required"),
    (dict(out_max=None), b"out_max and out_den go together"),
    (dict(out_den=None), b"out_max and out_den go together"),
    (dict(width=0), b"width = 0"),
    (dict(width=-1), b"width = -1"),
    (dict(width=1025), b"width = 1025"),
])
def test_key_attn_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _key_attn(L, change)
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"sjoin_key_attn: ") and cause in msg, msg


def test_key_attn_refuses_in_the_order_of_the_count_form(L):
    """a descriptor fault is named before a NULL argument, a NULL argument before a lone out_max, that before the width, the width
    before the LDS request"""
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    fn = getattr(L, NAME)
    assert fn(None, here, here, here, here, 8, here, here, here, here, None) == _lib.ERR_BADARG
    assert L.subgacc_last_error().startswith(b"sjoin_key_attn: null descriptor")
    d = _desc(here)
    d.struct_bytes -= 8
    assert fn(C.byref(d), here, here, here, here, 8, here, here, here, here, None) == _lib.ERR_BADARG
    assert b"struct_bytes" in L.subgacc_last_error()
    rc, msg = _key_attn(L, dict(options=1, e=None, out_max=None, width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"option" in msg
    rc, msg = _key_attn(L, dict(e=None, out_max=None, width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"are required" in msg
    rc, msg = _key_attn(L, dict(out_max=None, width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"go together" in msg
    rc, msg = _key_attn(L, dict(width=0, table_rows=14000))
    assert rc == _lib.ERR_BADARG and b"width" in msg
    rc, msg = _key_attn(L, dict(out_len=None, table_rows=14000))             # out_len is optional
    assert rc == _lib.ERR_LDS
    rc, msg = _key_attn(L, dict(out_len=None, out_max=None, out_den=None, table_rows=14000))        # ... and so are m and den together
    assert rc == _lib.ERR_LDS


@pytest.mark.parametrize("change", [dict(table_rows=14000), dict(row_stride=21000), dict(row_stride=8192, table_rows=9000)])
def test_key_attn_refuses_what_lds_does_not_hold(L, change):
    """4 (7 row_stride + 3 T + 2 D + 7) bytes beyond the 160 KiB of a CU: SUBGACC_ERR_LDS before any launch, naming table_rows"""
    from surel_plus_amd import _lib
    rc, msg = _key_attn(L, change)
    assert rc == _lib.ERR_LDS
    assert msg.startswith(b"sjoin_key_attn: ") and b"LDS" in msg and b"table_rows" in msg, msg


def test_key_attn_checks_the_backward_s_lds_when_it_keeps_max_and_den(L):
    """row_stride = 544, T = 8,192: the forward's 4 (7*544 + 3*8192 + 2*1088 + 7) = 122,268 B fit, the backward's 139,676 B too; at
    T = 10,500 the forward's 149,964 B fit and the backward's 167,372 B do not -- refused only when out_max / out_den are kept"""
    from surel_plus_amd import _lib
    assert 4 * (7 * 544 + 3 * 10500 + 2 * 1088 + 7) <= 160 * 1024 < 4 * (7 * 544 + 3 * 10500 + 6 * 1088 + 7)
    rc, msg = _key_attn(L, dict(row_stride=544, table_rows=10500))
    assert rc == _lib.ERR_LDS and msg.startswith(b"sjoin_key_attn: ") and b"backward" in msg and b"table_rows" in msg, msg
    rc, _ = _key_attn(L, dict(row_stride=544, table_rows=10500, out_max=None, out_den=None, S=0))
    assert rc == 0


def test_key_attn_of_no_segments_is_a_no_op(L):
    """S = 0 launches nothing (host pointers, no device): SUBGACC_OK"""
    rc, _ = _key_attn(L, dict(S=0))
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
    (dict(width=8, batch=4), "batch=None"),
])
def test_step_buffers_refuse_the_attn_stage_without_a_device(kw, cause):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match=cause):
        sp.StepBuffers(_NO_DEVICE, 8, stage="attn", **kw)


def test_refusals_that_were_refusals_stay():
    import torch
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match="stage"):
        sp.StepBuffers(_NO_DEVICE, 8, stage="attn", width=8, dtype=torch.bfloat16)      # a 16-bit dtype beside a stage
    for stage in (None, "counts", "counts_attn", "index"):                               # width stays refused with the other stages
        with pytest.raises(ValueError, match="width"):
            sp.StepBuffers(_NO_DEVICE, 8, stage=stage, width=8)
    with pytest.raises(ValueError, match="stage"):
        sp.StepBuffers(_NO_DEVICE, 8, stage="rows")
    e, h = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)
    embed, gate = torch.nn.Linear(4, 8), torch.nn.Linear(8, 1)
    host = SimpleNamespace(device=torch.device("cpu"))                       # (the modules' parameters are compared with it)
    with pytest.raises(ValueError, match=r"sample_and_fused_attn_stage: edge must be \[2, B\]"):
        sp.sample_and_fused_attn_stage(host, h, embed, gate)
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        sp.sample_and_fused_attn_stage(host, e, embed, gate, num_walks=200, num_steps=4)
    with pytest.raises(TypeError, match="sample_and_fused_attn_stage fuses gate_nn"):      # (as its twin)
        sp.sample_and_fused_attn_stage(host, e, embed, torch.nn.Linear(8, 2))
    counts = SimpleNamespace(stage="counts_attn", triplets=False)            # buffers made for another result
    with pytest.raises(ValueError, match="stage='attn'"):
        sp.sample_and_fused_attn_stage(host, e, embed, gate, buffers=counts)


# ----------------------------------------------------------------------------------------------------- the restatement of the chain
def test_the_restatement_is_exact_on_small_whole_numbers():
    """small whole numbers: every product and sum is exact in float32, so the chain IS W @ E"""
    W = np.array([[2, 0, 1, 0, 3], [0, 0, 0, 0, 0], [0, 4, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=np.float32)
    E = np.arange(5 * 3, dtype=np.float32).reshape(5, 3) - 6.0
    want = W.astype(np.float64) @ E.astype(np.float64)
    got = fused_attn(W, E)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert not got[1].any()                                             # an empty segment: a zero row
    assert np.array_equal(fused_attn(W, E, descending=True), got)
    E[1] = np.nan                                                       # a row whose weight is zero is never looked at
    assert np.array_equal(fused_attn(W[:2], E), got[:2])
    Wn = W.copy()
    Wn[0, 1] = -0.0                                                     # only the bits of +0.0f are passed over: -0.0 * NaN shows
    assert np.isnan(fused_attn(Wn[:1], E)).all()


def test_the_restatement_multiplies_and_adds_in_float32_in_ascending_order():
    """2^24 + 1 + 1: ascending, each 1 is lost to the rounding of the add; descending, 1 + 1 = 2 survives -- other bits"""
    big = np.float32(2.0 ** 24)
    W = np.array([[1, 1, 1]], dtype=np.float32)
    E = np.array([[big], [1.0], [1.0]], dtype=np.float32)
    up, down = fused_attn(W, E), fused_attn(W, E, descending=True)
    assert up[0, 0] == big and down[0, 0] == np.float32(2.0 ** 24 + 2) and up.view(np.uint32)[0, 0] != down.view(np.uint32)[0, 0]
    # the product is rounded before the add (no fused multiply-add): 3 * (1 + 2^-23) rounds to 3 + 2^-21 (a tie, to even); with
    # -3 behind it the chain gives 2^-21, a fused multiply-add would give the exact 3 * 2^-23
    E = np.array([[-3.0], [1.0 + 2.0 ** -23]], dtype=np.float32)
    got = fused_attn(np.array([[1, 3]], dtype=np.float32), E)
    assert got[0, 0] == np.float32(2.0 ** -21) and got[0, 0] != np.float32(3 * 2.0 ** -23)
    # no division: a weight is taken as it stands
    assert fused_attn(np.array([[0.25]], dtype=np.float32), np.array([[5.0]], dtype=np.float32))[0, 0] == np.float32(1.25)
    # and the derived bound holds for it
    rng = np.random.default_rng(0)
    W = (rng.random((6, 40)) * (rng.random((6, 40)) < 0.3)).astype(np.float32)
    E = rng.standard_normal((40, 7)).astype(np.float32)
    exact = W.astype(np.float64) @ E.astype(np.float64)
    assert (np.abs(fused_attn(W, E).astype(np.float64) - exact) <= bound(W, E)).all()

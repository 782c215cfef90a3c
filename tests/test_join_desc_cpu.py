"""CPU: the descriptor refusals shared by every entry point that takes a subgacc_join_desc (include/subgacc.h) -- one table of descriptor
faults, each refused by all six entry points with SUBGACC_ERR_BADARG and a message led by the called entry point's name, before anything
is launched; and the mirrored-list faults, refused alike by the four fused stages.  No GPU needed."""
import ctypes as C

import pytest

_BUF = (C.c_int64 * 64)()
HERE = C.addressof(_BUF)               # any non-null pointer: nothing is read through it before a refusal


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def _f64_desc():
    """a mirrored F64 row-form join over packed rows, B = 2 pairs (S = 4)"""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_F64
    d.row_off, d.n_rows, d.max_len, d.S, d.pair_block = HERE, 4, 4, 4, 2
    d.ids = d.payload = d.own = d.flags = HERE
    return d


def _fill_desc():
    d = _f64_desc()
    d.seg = d.out_xz = HERE
    return d


def _counts_desc():
    from surel_plus_amd import _lib
    d = _f64_desc()
    d.form, d.payload_kind, d.table_rows = _lib.JOIN_COUNTS, _lib.JOIN_SFPTR, 16
    return d


# entry point -> (a descriptor it accepts up to its launch, its arguments behind the descriptor)
ENTRY = {
    "subgacc_sjoin_fill_v2": (_fill_desc, (None,)),
    "subgacc_sjoin_relu_mean": (_f64_desc, (HERE, HERE, 96, HERE, None, None, None)),
    "subgacc_sjoin_relu_attn": (_f64_desc, (HERE, HERE, HERE, 96, HERE, None, None, None)),
    "subgacc_sjoin_relu_attn_backward": (_f64_desc, (HERE, HERE, HERE, 96) + (HERE,) * 7 + (None,)),
    "subgacc_sjoin_counts_attn": (_counts_desc, (HERE, HERE, None, None, None)),
    "subgacc_sjoin_counts_attn_backward": (_counts_desc, (HERE,) * 6 + (None,)),
}
FUSED = [name for name in ENTRY if name != "subgacc_sjoin_fill_v2"]

DESC_FAULTS = [
    pytest.param(None, b"null descriptor", id="null-descriptor"),
    pytest.param(dict(struct_bytes=8), b"struct_bytes", id="foreign-struct_bytes"),
    pytest.param(dict(row_len=HERE, row_stride=32), b"exactly one", id="row_off-and-row_len"),
    pytest.param(dict(row_off=None), b"exactly one", id="no-layout"),
    pytest.param(dict(row_off=None, row_stride=1), b"row_stride = 1", id="headed-row_stride-1"),
    pytest.param(dict(row_off=None, row_stride=1 << 31), b"row_stride = 2147483648", id="headed-row_stride-2^31"),
    pytest.param(dict(row_off=None, row_len=HERE, row_stride=1 << 31), b"row_stride = 2147483648", id="strided-row_stride-2^31"),
    pytest.param(dict(S=-4), b"bad arguments", id="negative-S"),
    pytest.param(dict(n_rows=-1), b"bad arguments", id="negative-n_rows"),
    pytest.param(dict(max_len=-1), b"bad arguments", id="negative-max_len"),
]

MIRROR_FAULTS = [
    pytest.param(dict(pair_block=0), b"pair_block", id="pair_block-0"),
    pytest.param(dict(pair_block=-2), b"pair_block", id="pair_block-negative"),
    pytest.param(dict(S=6), b"multiple of 2*pair_block", id="S-not-a-multiple"),
    pytest.param(dict(own=None), b"own = NULL", id="own-NULL"),
]


def _refusal(L, name, change):
    """call `name` with its accepted descriptor, `change` applied (None: no descriptor at all); (status, message)"""
    make, args = ENTRY[name]
    d = None
    if change is not None:
        d = make()
        for field, val in change.items():
            setattr(d, field, val)
    rc = getattr(L, name)(C.byref(d) if d is not None else None, *args)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,cause", DESC_FAULTS)
@pytest.mark.parametrize("name", list(ENTRY))
def test_every_descriptor_entry_point_refuses_a_faulty_descriptor(L, name, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _refusal(L, name, change)
    assert rc == _lib.ERR_BADARG, (rc, msg)
    assert msg.startswith(name[len("subgacc_"):].encode() + b": ") and cause in msg, msg


@pytest.mark.parametrize("change,cause", MIRROR_FAULTS)
@pytest.mark.parametrize("name", FUSED)
def test_every_fused_stage_refuses_a_list_that_is_not_mirrored(L, name, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _refusal(L, name, change)
    assert rc == _lib.ERR_BADARG, (rc, msg)
    assert msg.startswith(name[len("subgacc_"):].encode() + b": ") and cause in msg, msg

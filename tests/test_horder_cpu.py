"""CPU: the library side of the on-demand triplet step (sample_and_hgather) -- the dedup prologue that knows roles is declared,
exported and refuses every bad argument before it launches anything; subgacc_sjoin_fill_v2 takes out_segid with the strided rows of
an on-demand step; the new calls are exported by the package.  No GPU needed: every call here returns before its first launch."""
import ctypes as C
import os
import re

import pytest

_BUF = (C.c_int64 * 64)()
HERE = C.addressof(_BUF)               # any non-null pointer: nothing is read through it before a refusal
NAME = "subgacc_step_prologue_dedup_roles"


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def _roles_args(L, **change):
    """the arguments of a triplet prologue (B = 4: n = 12 roots, r = 3, s = 4) that passes every check, `change` applied"""
    n = change.get("n", 12)
    a = dict(table=None, capacity=0, zero_words=HERE, n_zero=4, edge=HERE, roots=HERE, own=HERE, worklist=HERE, row_len=HERE, n=n,
             B=4, r=3, s=4, workspace=HERE, workspace_bytes=L.subgacc_step_dedup_workspace_bytes(n), n_distinct=HERE, stream=None)
    a.update(change)
    return tuple(a.values())


def test_roles_prologue_is_declared_and_exported(L):
    from surel_plus_amd import _lib
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "subgacc.h")
    txt = open(header).read()
    assert re.search(r"\bint %s\(" % NAME, txt) and NAME in _lib.SYMBOLS and hasattr(L, NAME)
    assert "subgacc_step_prologue_dedup(" in txt and "subgacc_step_prologue_dedup" in _lib.SYMBOLS      # the pair form stays
    assert L.subgacc_abi_version() == 7           # additions only


ROLE_FAULTS = [
    pytest.param(dict(edge=None), "ERR_BADARG", b"null argument", id="edge-NULL"),
    pytest.param(dict(roots=None), "ERR_BADARG", b"null argument", id="roots-NULL"),
    pytest.param(dict(own=None), "ERR_BADARG", b"null argument", id="own-NULL"),
    pytest.param(dict(worklist=None), "ERR_BADARG", b"null argument", id="worklist-NULL"),
    pytest.param(dict(row_len=None), "ERR_BADARG", b"null argument", id="row_len-NULL"),
    pytest.param(dict(n_distinct=None), "ERR_BADARG", b"null argument", id="n_distinct-NULL"),
    pytest.param(dict(zero_words=None), "ERR_BADARG", b"null argument", id="zero_words-NULL-with-n_zero"),
    pytest.param(dict(table=HERE, capacity=1000), "ERR_BADARG", b"power of two", id="capacity-not-a-power-of-two"),
    pytest.param(dict(n=11), "ERR_BADARG", b"r*B", id="n-not-r*B"),
    pytest.param(dict(n=8), "ERR_BADARG", b"r*B", id="n-is-2B-with-r-3"),
    pytest.param(dict(B=0, n=0), "ERR_BADARG", b"r*B", id="B-0"),
    pytest.param(dict(r=4, n=16), "ERR_BADARG", b"not implemented", id="r-4"),
    pytest.param(dict(r=1, n=4), "ERR_BADARG", b"not implemented", id="r-1"),
    pytest.param(dict(s=3), "ERR_BADARG", b"not implemented", id="s-3-with-r-3"),
    pytest.param(dict(r=2, s=4, n=8), "ERR_BADARG", b"not implemented", id="s-4-with-r-2"),
    pytest.param(dict(workspace=None), "ERR_WORKSPACE", b"workspace too small", id="workspace-NULL"),
    pytest.param(dict(workspace_bytes=64), "ERR_WORKSPACE", b"workspace too small", id="workspace-too-small"),
]


@pytest.mark.parametrize("change,status,cause", ROLE_FAULTS)
def test_roles_prologue_refuses_before_launching(L, change, status, cause):
    from surel_plus_amd import _lib
    rc = getattr(L, NAME)(*_roles_args(L, **change))
    msg = L.subgacc_last_error()
    assert rc == getattr(_lib, status), (rc, msg)
    assert msg.startswith(NAME[len("subgacc_"):].encode() + b": ") and cause in msg, msg


def _strided_key_desc(kind, S=0):
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, kind
    d.row_len, d.row_stride, d.n_rows, d.S, d.pair_block = HERE, 320, 8, S, 4
    d.ids = d.payload = d.own = d.flags = d.seg = d.out_xz = HERE
    d.num_walks, d.num_steps = 100, 3
    return d


def test_fill_takes_segment_ids_with_the_strided_rows_of_an_on_demand_step(L):
    """KEY32 rows of M = 100, 3 hops, an empty list: with out_segid the call is accepted like the one without (it was refused with
    "keys of strided rows -- a transient batch -- are joined with segment pointers"); KEY64 over packed rows stays refused"""
    from surel_plus_amd import _lib
    for kind in (_lib.JOIN_KEY32, _lib.JOIN_SFPTR):
        d = _strided_key_desc(kind)
        assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.OK, L.subgacc_last_error()
        d.out_segid = HERE
        assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.OK, L.subgacc_last_error()
    d = _strided_key_desc(_lib.JOIN_KEY64)
    d.num_walks, d.num_steps, d.out_segid = 200, 4, HERE
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.OK, L.subgacc_last_error()
    d.row_len, d.row_stride, d.row_off = None, 0, HERE              # the same keys over packed rows
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG
    assert L.subgacc_last_error().startswith(b"sjoin_fill_v2: ") and b"64-bit keys" in L.subgacc_last_error()


def test_the_package_exports_the_higher_order_calls():
    import surel_plus_amd as sp
    for name in ("hgather_counts", "hmean_stage", "sample_and_hgather"):
        assert callable(getattr(sp, name)), name
    import inspect
    assert inspect.signature(sp.sample_and_gather).parameters["ptr"].default is True
    assert inspect.signature(sp.StepBuffers.__init__).parameters["ptr"].default is True
    assert inspect.signature(sp.StepBuffers.__init__).parameters["triplets"].default is False
    sig = inspect.signature(sp.sample_and_hgather)
    assert list(sig.parameters)[:2] == ["csr", "hedge"] and sig.parameters["rng"].default == "philox"

"""CPU: the argument contract of the star join (SUBGACC_JOIN_OPT_STAR, spjoin.gather_star) -- what the library refuses before it
launches anything, and what gather_star refuses before any device work.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def _star_desc(here):
    """a star descriptor over packed rows that the library accepts up to its first launch: P = 2 sources, K = 2 targets each"""
    from surel_plus_amd import _lib
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.payload_kind, d.options = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_SFPTR, _lib.JOIN_OPT_STAR
    d.row_off, d.n_rows, d.max_len, d.S, d.pair_block = here, 4, 4, 8, 2
    d.ids = d.payload = d.own = d.partner = d.seg = d.flags = d.out_xz = d.table = here
    d.table_rows, d.k = 4, 3
    return d


def test_star_option_is_known(L):
    from surel_plus_amd import _lib
    assert _lib.JOIN_OPT_STAR == 2
    assert "subgacc_sjoin_star_sizes" in _lib.SYMBOLS
    assert L.subgacc_abi_version() == 7


@pytest.mark.parametrize("change,cause", [
    (dict(form=1), b"row form"),                                   # the count form
    (dict(form=2), b"row form"),                                   # the pair form
    (dict(row_off=None, row_len="here", row_stride=32), b"strided"),
    (dict(payload_kind=3, row_off=None, row_stride=32), b"64-bit keys"),
    (dict(pair_block=0), b"pair_block"),
    (dict(pair_block=-2), b"pair_block"),
    (dict(S=6), b"S = 2*P*K"),
    (dict(partner=None), b"partner = NULL"),
    (dict(own=None), b"own = NULL"),
    (dict(out_idx="here"), b"out_idx"),
])
def test_fill_v2_refuses_what_the_star_form_does_not_join(L, change, cause):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _star_desc(here)
    for name, val in change.items():
        setattr(d, name, here if val == "here" else val)
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG
    msg = L.subgacc_last_error()
    assert b"star option" in msg and cause in msg, msg
    # with OPT_SIZES as well (the one-launch size pass): refused before the size pass, too
    d.options = _lib.JOIN_OPT_STAR | _lib.JOIN_OPT_SIZES
    d.seg, d.out_seg = None, here
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG
    assert cause in L.subgacc_last_error()


def test_star_sizes_argument_errors(L):
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    ws = L.subgacc_sjoin_workspace_bytes(8)
    assert L.subgacc_sjoin_star_sizes(here, 4, here, None, 2, 2, here, None, here, ws, None) == _lib.ERR_BADARG
    assert b"null argument" in L.subgacc_last_error()
    assert L.subgacc_sjoin_star_sizes(here, 4, here, here, -1, 2, here, None, here, ws, None) == _lib.ERR_BADARG
    assert L.subgacc_sjoin_star_sizes(here, 4, here, here, 1 << 20, 1 << 12, here, None, here, ws, None) == _lib.ERR_BADARG
    assert b"2^31" in L.subgacc_last_error()
    assert L.subgacc_sjoin_star_sizes(here, 4, here, here, 2, 2, here, None, here, 8, None) == _lib.ERR_WORKSPACE


@pytest.fixture
def no_device(monkeypatch):
    """every path from gather_star to the library or a device raises"""
    from surel_plus_amd import spjoin

    def device_work(*a, **k):
        raise AssertionError("device work before the argument check")
    for name in ("lib", "join_fill", "stream_ptr", "check", "_as_rows", "_as_spg", "_seg_and_flags", "sjoin", "gather"):
        monkeypatch.setattr(spjoin, name, device_work)
    return spjoin


def test_gather_star_refuses_a_strided_store(no_device):
    from types import SimpleNamespace
    import surel_plus_amd as sp
    from surel_plus_amd.spg import StridedSpG
    n, pitch = 3, 32
    ids = torch.zeros(n * pitch, dtype=torch.int32)
    sets = SimpleNamespace(strided=True, ids=ids, slot=ids.clone(), nsize=torch.zeros(n, dtype=torch.int32), stride=pitch, table=None,
                           capacity=0, num_walks=8, num_steps=2)
    with pytest.raises(ValueError, match="HeadedSpG") as e:
        sp.gather_star(np.arange(2), np.zeros((2, 3), np.int64), StridedSpG(sets, 10), "cuda")
    assert "SpG" in str(e.value) and "float" in str(e.value)


@pytest.mark.parametrize("source,targets,exc,match", [
    (np.arange(2), [[0, 1, 2], [0, 1]], ValueError, "rectangular|ragged"),         # ragged targets
    (np.arange(3), np.zeros((2, 4), np.int64), ValueError, "2 rows for 3 sources"),  # P mismatch
    (np.arange(2), np.zeros(4, np.int64), ValueError, "2-D"),                        # targets not [P, K]
    (np.zeros((2, 1), np.int64), np.zeros((2, 4), np.int64), ValueError, "1-D"),     # source not [P]
    (np.arange(2.0), np.zeros((2, 4), np.int64), TypeError, "integer"),              # float source
    (torch.arange(2.0), torch.zeros((2, 4), dtype=torch.int64), TypeError, "integer"),
    (np.arange(2), np.zeros((2, 4), np.float32), TypeError, "integer"),              # float targets
])
def test_gather_star_argument_errors(no_device, source, targets, exc, match):
    import surel_plus_amd as sp
    z = object()        # never looked at: the arguments are refused first
    with pytest.raises(exc, match=match):
        sp.gather_star(source, targets, z, "cuda")

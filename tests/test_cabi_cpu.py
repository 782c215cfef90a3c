"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/subgacc.h declares.
No compute call is made here (there is no GPU in the build container)."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


def test_header_symbols_are_exported(L):
    from surel_plus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "subgacc.h")).read()
    declared = set(re.findall(r"\b(subgacc_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"subgacc_status"}
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(L, name), name


def test_abi_version_and_argument_errors(L):
    from surel_plus_amd import _lib
    assert L.subgacc_abi_version() == 7           # 7: headed rows, the per-form join entry points of ABI 1-5 gone; 6: subgacc_sjoin_fill_v2 (one descriptor for every form of the join); 5: 64-bit key rows (4-hop walks); 2: row / node counts in the join and rng_positions entry points (bounds); 3: hop records in the walk cfg; 4: batched registration of key rows
    assert L.subgacc_key_shift(200, 3) == 8            # SHIFT = 32-clz(M), subg_acc.c:903
    assert L.subgacc_key_shift(100, 4) == 7
    assert L.subgacc_key_shift(200, 8) == _lib.ERR_KEYWIDTH   # 8*8+1 > 64 (subg_acc.c:905-915)
    with pytest.raises(AssertionError, match="hasing key"):
        _lib.check(L.subgacc_key_shift(200, 8))
    assert L.subgacc_key_shift(0, 3) == _lib.ERR_BADARG
    with pytest.raises(TypeError, match="Input parsing error"):
        _lib.check(L.subgacc_key_shift(0, 3))
    assert L.subgacc_scan_workspace_bytes(10) > 0
    assert L.subgacc_uniq_table_bytes(1024) == 1024 * 20


def test_no_cpu_fallback():
    """Without a GPU the product path must fail loudly (never route through the oracle)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import numpy as np
    import surel_plus_amd as sp
    with pytest.raises(sp.SubgAccError, match="no HIP device"):
        sp.gset_sampler(np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.arange(2))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "surel_plus_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "oracle/" not in txt, f


def test_join_descriptor_layout_matches_the_header(tmp_path, L):
    """struct subgacc_join_desc (ABI 6) as gcc lays it out from include/subgacc.h == the ctypes mirror, field by field: a binding
    that disagrees about one offset would hand the kernels a wrong pointer.  And the entry point refuses a descriptor of another
    size or with neither / both row layouts before anything is launched (no GPU needed for that)."""
    import ctypes as C
    import subprocess
    from surel_plus_amd import _lib
    names = [f[0] for f in _lib.JoinDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "subgacc.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(subgacc_join_desc));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(subgacc_join_desc, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(src), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == C.sizeof(_lib.JoinDesc)
    assert out[1:] == [getattr(_lib.JoinDesc, n).offset for n in names]
    # ... and struct subgacc_walk_cfg (row_pitch joined it this round)
    wnames = [f[0] for f in _lib.WalkCfg._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "subgacc.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(subgacc_walk_cfg));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(subgacc_walk_cfg, {n}));\n' for n in wnames) + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", str(src), "-I" + os.path.join(ROOT, "include"), "-o", str(exe)])
    wout = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert wout[0] == C.sizeof(_lib.WalkCfg) and wout[1:] == [getattr(_lib.WalkCfg, n).offset for n in wnames]
    d = _lib.JoinDesc()
    d.struct_bytes = 8
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG
    assert b"descriptor" in L.subgacc_last_error()
    d.struct_bytes = C.sizeof(_lib.JoinDesc)
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG          # neither row_off nor row_len
    assert L.subgacc_sjoin_fill_v2(None, None) == _lib.ERR_BADARG
    # SUBGACC_JOIN_OPT_SIZES (the whole join in one call): what it refuses before it launches anything
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d.row_off, d.n_rows, d.S, d.pair_block = here, 4, 4, 2
    d.options = 2                                                               # an option bit this library does not know
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG and b"option" in L.subgacc_last_error()
    d.options = _lib.JOIN_OPT_SIZES
    d.form = _lib.JOIN_COUNTS
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG          # the row form only
    d.form = _lib.JOIN_ROWS
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG          # no out_seg
    d.out_seg, d.seg = here, here
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG          # seg next to out_seg
    d.seg, d.own = None, here
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_WORKSPACE       # (no output: the size pass alone) no state
    # (round 6: with an output, what the FILL would refuse is refused before the size pass has written out_seg / host_tail)
    d.out_xz = here
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG and b"null argument" in L.subgacc_last_error()
    d.ids = d.payload = d.flags = here
    d.payload_kind = 9
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG and b"payload kind" in L.subgacc_last_error()
    d.payload_kind = _lib.JOIN_KEY64                                            # 64-bit keys are the payload of STRIDED / HEADED rows
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG and b"row layout" in L.subgacc_last_error()
    d.payload_kind = _lib.JOIN_SFPTR
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_WORKSPACE       # no state
    # ABI 7, headed rows: neither row_off nor row_len, a row_stride -- and not two layouts at once
    d.row_len, d.row_stride = here, 32
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG and b"exactly one" in L.subgacc_last_error()
    d.row_off = d.row_len = None
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_WORKSPACE       # headed rows: accepted up to the missing state
    d.row_stride = 1
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG          # a headed row needs a slot behind its length
    d.row_off, d.row_stride = here, 0
    d.size_state, d.size_state_bytes = here, 8
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_WORKSPACE       # a state too small
    assert L.subgacc_sjoin_workspace_bytes(4) >= 64 + 8 and L.subgacc_sjoin_workspace_bytes(1 << 22) >= 64 + 8 * (1 << 12)


def test_headed_sizes_only_call_needs_ids(L):
    """Headed rows keep their lengths in `ids`, and the one-launch size pass reads them: the sizes-only call (OPT_SIZES, no output)
    with S > 0 and ids = NULL is refused before anything is launched, naming `ids` (it used to reach the state check)."""
    import ctypes as C
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    d = _lib.JoinDesc()
    d.struct_bytes, d.form, d.options = C.sizeof(_lib.JoinDesc), _lib.JOIN_ROWS, _lib.JOIN_OPT_SIZES
    d.row_stride, d.n_rows, d.S, d.pair_block = 32, 4, 4, 2
    d.own, d.out_seg = here, here
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_BADARG
    assert b"ids" in L.subgacc_last_error()
    d.ids = here                                                                # with ids: on to the missing state, as before
    assert L.subgacc_sjoin_fill_v2(C.byref(d), None) == _lib.ERR_WORKSPACE


def test_walk_entry_points_refuse_before_launching(L):
    """Each of the six subgacc_walk_* entry points refuses an argument fault before anything is launched (no GPU needed): one fault
    per call, its return code and a piece of subgacc_last_error()'s text."""
    import ctypes as C
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)               # any non-null pointer: nothing is read through it before the refusal

    def cfg(M=100, m=3, **kw):            # philox, set_sampler order, no bucket: every entry point accepts it
        c = _lib.WalkCfg(M, m, -1, _lib.RNG_PHILOX, 111413, 1, _lib.ORDER_WALK_MAJOR, 1, 0, 0, None, 0, 0, None, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    graph = (here, here, 10)              # indptr, indices, num_nodes

    def sets(c=None, num_nodes=10, query=here, n=4, rng=(None, None), keys=here, walks=None, flags=here):
        return L.subgacc_walk_sets(c or cfg(), here, here, num_nodes, query, n, *rng, here, keys, here, walks, flags, None)

    def spg(c=None, root_base=0, table=here, cap=1024, ids=here, slot=here):
        return L.subgacc_walk_spg(c or cfg(), *graph, here, 4, root_base, None, None, table, cap, ids, slot, here, here, None)

    def sparse(c=None, wl=here, nwl=here):
        return L.subgacc_walk_spg_sparse(c or cfg(), *graph, here, 4, wl, nwl, here, 1024, here, here, here, here, None)

    def listed(c=None, wl=here, nwl=here):
        return L.subgacc_walk_spg_list(c or cfg(), *graph, here, 4, None, None, wl, nwl, here, 1024, here, here, here, here, None)

    def keys64(c=None, keys=here, flags=here):
        return L.subgacc_walk_keyrows64(c or cfg(200, 4), *graph, here, 4, None, None, here, here, here, keys, here, flags, None)

    def tags(c=None, work_cap=0, table=here, cap=1024, flags=here):
        return L.subgacc_walk_tags(c or cfg(), *graph, here, 4, 0, None, None, here, here, work_cap, table, cap, flags, None)

    cases = [
        (lambda: sets(keys=None), _lib.ERR_BADARG, b"null set_keys"),
        (lambda: sets(flags=None), _lib.ERR_BADARG, b"null argument"),
        (lambda: sets(n=-1), _lib.ERR_BADARG, b"negative size"),
        (lambda: sets(cfg(rng_mode=7)), _lib.ERR_BADARG, b"unknown rng_mode"),
        (lambda: sets(cfg(200, 8)), _lib.ERR_KEYWIDTH, b"hasing key"),
        (lambda: sets(cfg(emit_walks=1)), _lib.ERR_BADARG, b"emit_walks without a walks buffer"),
        (lambda: sets(cfg(rng_mode=_lib.RNG_RAND_R)), _lib.ERR_BADARG, b"RAND_R mode needs rng_pos"),
        (lambda: sets(query=None), _lib.ERR_BADARG, b"null query"),
        (lambda: sets(num_nodes=0), _lib.ERR_BADARG, b"a graph without nodes"),
        (lambda: sets(cfg(row_pitch=10)), _lib.ERR_BADARG, b"row_pitch 10 < the row capacity 301"),
        (lambda: sets(cfg(hop_records=here, rec_id_bits=40, rec_beg_bits=30)), _lib.ERR_BADARG, b"hop records with field widths 40 / 30"),
        (lambda: spg(slot=None), _lib.ERR_BADARG, b"null row_slot"),
        (lambda: spg(cfg(emit_walks=1)), _lib.ERR_BADARG, b"walk_spg: set_sampler order only, no raw walks"),
        (lambda: spg(cfg(order=_lib.ORDER_STEP_MAJOR)), _lib.ERR_BADARG, b"walk_spg: set_sampler order only"),
        (lambda: spg(ids=None), _lib.ERR_BADARG, b"null argument"),
        (lambda: spg(cfg(256, 4)), _lib.ERR_LDS, b"needs a per-root table above 1024 slots"),
        (lambda: spg(cap=1000), _lib.ERR_BADARG, b"power-of-two table"),
        (lambda: spg(root_base=-1), _lib.ERR_BADARG, b"power-of-two table"),
        (lambda: sparse(cfg(rng_mode=_lib.RNG_RAND_R)), _lib.ERR_BADARG, b"Philox mode"),
        (lambda: sparse(nwl=None), _lib.ERR_BADARG, b"a work list without its length"),
        (lambda: listed(wl=None), _lib.ERR_BADARG, b"null row_slot / work list / length"),
        (lambda: listed(cfg(emit_walks=1)), _lib.ERR_BADARG, b"walk_spg_list: set_sampler order only, no raw walks"),
        (lambda: keys64(cfg(100, 3)), _lib.ERR_BADARG, b"fit 32 bits"),
        (lambda: keys64(cfg(200, 4, bucket=50)), _lib.ERR_BADARG, b"no bucket"),
        (lambda: keys64(keys=None), _lib.ERR_BADARG, b"null row_keys"),
        (lambda: keys64(flags=None), _lib.ERR_BADARG, b"null argument"),
        (lambda: tags(table=None), _lib.ERR_BADARG, b"needs a work list, its length and a table"),
        (lambda: tags(work_cap=-1), _lib.ERR_BADARG, b"needs a work list, its length and a table"),
        (lambda: tags(cfg(bucket=50)), _lib.ERR_BADARG, b"walk_tags: set_sampler order, no raw walks, no bucket"),
        (lambda: tags(flags=None), _lib.ERR_BADARG, b"null argument"),
        (lambda: tags(cap=1000), _lib.ERR_BADARG, b"power-of-two table"),
    ]
    for i, (call, want, text) in enumerate(cases):
        rc = call()
        assert rc == want and text in L.subgacc_last_error(), (i, rc, L.subgacc_last_error())

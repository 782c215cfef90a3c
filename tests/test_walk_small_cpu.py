"""CPU: key rows for the small walk shapes -- the third header and its binding, the host predicate small_rows_form beside the four
predicates it must not move, every fault subgacc_walk_keyrows_small refuses before it launches anything (return code, a message led
by its name), and the shapes the on-demand stages accept and refuse.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_H = os.path.join(ROOT, "include", "subgacc_small.h")
NAME = "subgacc_walk_keyrows_small"


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_third_header_declares_one_entry_point_and_the_library_exports_it(L):
    from surel_plus_amd import _lib
    text = open(SMALL_H).read()
    decls = _lib.parse_header(text)
    assert list(decls) == [NAME] == list(_lib.SMALL_SYMBOLS) == list(_lib.SMALL_DECLS)
    ret, args = decls[NAME]
    assert ret == "int" and args == [
        ("cfg", "const subgacc_walk_cfg *"), ("indptr", "const void *"), ("indices", "const int32_t *"), ("num_nodes", "int64_t"),
        ("query", "const int32_t *"), ("n", "int64_t"), ("rng_pos", "const uint32_t *"), ("rng_seed", "const uint32_t *"),
        ("worklist", "const int32_t *"), ("n_work", "const int64_t *"), ("row_ids", "int32_t *"), ("row_keys", "int32_t *"),
        ("nsize", "int32_t *"), ("flags", "int32_t *"), ("stream", "void *")]
    # the mirror of subgacc_walk_keyrows64, with 32-bit keys
    big = [(n, "int32_t *" if n == "row_keys" else t) for n, t in _lib.DECLS["subgacc_walk_keyrows64"][1]]
    assert args == big
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.restype is C.c_int and fn.argtypes == [C.POINTER(_lib.WalkCfg), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64] + \
        [C.c_void_p] * 9
    assert "subg_acc.c:742-846, 900-955" in text                     # the reference lines it replaces
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert NAME in names


def test_the_other_two_headers_keep_their_entry_points(L):
    from surel_plus_amd import _lib
    assert len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and NAME not in _lib.SYMBOLS
    assert _lib.HALF_SYMBOLS == ("subgacc_sjoin_fill_half",)
    assert os.path.basename(_lib.SMALL_HEADER) == "subgacc_small.h"


# ----------------------------------------------------------------------------------------------------------------- the predicates
def _slots(q):
    t = 64
    while t < q + q // 4 + 1:
        t <<= 1
    return t


def test_the_slot_arithmetic_at_its_edges():
    assert [_slots(q) for q in (51, 52, 102, 103, 204, 205)] == [64, 128, 128, 256, 256, 512]


def test_small_rows_form_is_the_written_out_rule():
    from surel_plus_amd.sampler import key_rows_form, small_rows_form
    most = {1: 203, 2: 101, 3: 67, 4: 50}                            # the largest M of every hop count: M * m + 1 <= 204
    for m in range(1, 7):
        for M in range(1, 301):
            want = m in most and M <= most[m]
            assert bool(small_rows_form(M, m)) == want, (M, m)
            assert want == (1 <= m <= 4 and _slots(M * m + 1) in (64, 128, 256)), (M, m)
            assert not (want and key_rows_form(M, m) != 0), (M, m)
            if want:
                assert m * int(M).bit_length() + 1 <= 25             # the key's bits
    assert not small_rows_form(0, 1) and not small_rows_form(10, 0)


# What the four predicates of the fused-row kernel returned for M = 1 .. 300 and m = 1 .. 6 before the one-wave kernel existed, as
# runs: (the first M of the run, the value).  Generated once from that code; the predicates must not move.
_G, _R, _P, _S = "walk_sets_kernel<SPG>", "walk_rows_kernel", "walk_pipe_kernel", "walk_sets_kernel"
_NONE = dict(form=((1, 0),), ok=((1, False),), takes=((1, False),), name_fused=((1, _G),))
BEFORE = {
    1: _NONE,
    2: dict(form=((1, 0), (102, 32), (257, 0)), ok=((1, False), (102, True), (257, False)), takes=((1, False), (102, True), (257, False)),
            name_fused=((1, _G), (102, _R), (257, _G))),
    3: dict(form=((1, 0), (68, 32), (257, 0)), ok=((1, False), (68, True), (257, False)), takes=((1, False), (68, True), (257, False)),
            name_fused=((1, _G), (68, _R), (257, _G))),
    4: dict(form=((1, 0), (51, 32), (128, 64), (205, 0)), ok=((1, False), (51, True), (128, False)), takes=((1, False), (51, True), (205, False)),
            name_fused=((1, _G), (51, _R), (205, _G))),
    5: _NONE,
    6: _NONE,
}
BEFORE_SETS = ((1, _P), (257, _S))          # walk_kernel_name(fused_rows=False), every m; rows_kernel_takes with a bucket: never


def _run_value(runs, M):
    return [v for start, v in runs if start <= M][-1]


def test_the_four_predicates_return_what_they_returned():
    from surel_plus_amd import sampler
    for m in range(1, 7):
        for M in range(1, 301):
            b = BEFORE[m]
            assert sampler.key_rows_form(M, m) == _run_value(b["form"], M), (M, m)
            assert sampler.key_rows_ok(M, m) is _run_value(b["ok"], M), (M, m)
            assert sampler.rows_kernel_takes(M, m) is _run_value(b["takes"], M), (M, m)
            assert sampler.rows_kernel_takes(M, m, 64) is False, (M, m)
            assert sampler.walk_kernel_name(None, M, m, True) == _run_value(b["name_fused"], M), (M, m)
            assert sampler.walk_kernel_name(None, M, m, False) == _run_value(BEFORE_SETS, M), (M, m)


# ------------------------------------------------------------------------------------------------------ subgacc_walk_keyrows_small
def _call(L, cfg=None, null_cfg=False, n=4, num_nodes=10, null=(), work="none"):
    """one call whose pointers are host memory: it is only ever made with something the library refuses before it launches"""
    from surel_plus_amd import _lib
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    c = dict(num_walks=100, num_steps=2, bucket=-1, rng_mode=_lib.RNG_PHILOX, seed=1, first_hop_wo=1, order=_lib.ORDER_WALK_MAJOR,
             cap_root_degree=1, indptr64=0, emit_walks=0, hop_records=None, rec_id_bits=0, rec_beg_bits=0, walk_pos=None, row_pitch=0)
    c.update(cfg or {})
    if c["walk_pos"] == "here":
        c["walk_pos"] = here
    wc = _lib.WalkCfg(*[c[f] for f, _ in _lib.WalkCfg._fields_])
    p = {k: (None if k in null else here) for k in ("indptr", "indices", "query", "rng_pos", "rng_seed", "row_ids", "row_keys", "nsize", "flags")}
    wl, nw = {"none": (None, None), "both": (here, here), "list": (here, None), "length": (None, here)}[work]
    rc = getattr(L, NAME)(None if null_cfg else C.byref(wc), p["indptr"], p["indices"], num_nodes, p["query"], n, p["rng_pos"],
                          p["rng_seed"], wl, nw, p["row_ids"], p["row_keys"], p["nsize"], p["flags"], None)
    assert not any(buf), "a refused call wrote something"
    return rc, L.subgacc_last_error()


def _shape(M, m):
    return dict(cfg=dict(num_walks=M, num_steps=m))


REFUSALS = [
    pytest.param(dict(null_cfg=True), b"null cfg", id="null-cfg"),
    pytest.param(_shape(102, 2), b"subgacc_walk_spg", id="512-slots-2-hops"),
    pytest.param(_shape(68, 3), b"subgacc_walk_spg", id="512-slots-3-hops"),
    pytest.param(_shape(51, 4), b"subgacc_walk_spg", id="512-slots-4-hops"),
    pytest.param(_shape(200, 3), b"subgacc_walk_spg", id="1024-slots"),
    pytest.param(_shape(204, 1), b"not a small shape", id="one-hop-204-walks"),
    pytest.param(_shape(256, 1), b"not a small shape", id="one-hop-256-walks"),
    pytest.param(_shape(10, 5), b"not a small shape", id="five-hops"),
    pytest.param(_shape(300, 3), b"not a small shape", id="more-than-256-walks"),
    pytest.param(_shape(0, 2), b"must be positive", id="no-walks"),
    pytest.param(_shape(10, 0), b"must be positive", id="no-hops"),
    pytest.param(dict(cfg=dict(bucket=200)), b"bucket of 200 truncates", id="truncating-bucket"),
    pytest.param(dict(cfg=dict(order=1)), b"set_sampler order", id="step-major-order"),
    pytest.param(dict(cfg=dict(emit_walks=1)), b"no raw walks", id="emit-walks"),
    pytest.param(dict(cfg=dict(first_hop_wo=0)), b"first hop without replacement", id="first-hop-with-replacement"),
    pytest.param(dict(cfg=dict(walk_pos="here", rng_mode=0)), b"walk_pos", id="walk-pos"),
    pytest.param(dict(cfg=dict(rng_mode=2)), b"unknown rng_mode 2", id="unknown-rng"),
    pytest.param(dict(work="list"), b"work list without its length", id="list-without-length"),
    pytest.param(dict(work="length"), b"work list without its length", id="length-without-list"),
    pytest.param(dict(null=("row_ids",)), b"null argument", id="null-row-ids"),
    pytest.param(dict(null=("row_keys",)), b"null argument", id="null-row-keys"),
    pytest.param(dict(null=("nsize",)), b"null argument", id="null-nsize"),
    pytest.param(dict(null=("flags",)), b"null argument", id="null-flags"),
    pytest.param(dict(null=("indptr",)), b"null argument", id="null-indptr"),
    pytest.param(dict(null=("query",)), b"null argument", id="null-query"),
    pytest.param(dict(cfg=dict(rng_mode=0), null=("rng_pos",)), b"rng_pos/rng_seed", id="rand_r-without-positions"),
    pytest.param(dict(num_nodes=0), b"graph without nodes", id="no-nodes"),
    pytest.param(dict(cfg=dict(row_pitch=200)), b"row_pitch 200 < the row capacity 201", id="pitch-below-Q"),
    pytest.param(dict(n=-1), b"negative size", id="negative-n"),
    pytest.param(dict(num_nodes=-1), b"negative size", id="negative-num-nodes"),
]


@pytest.mark.parametrize("how,cause", REFUSALS)
def test_walk_keyrows_small_refuses_before_any_launch(L, how, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, **how)
    assert rc == _lib.ERR_BADARG, msg
    assert msg.startswith(b"walk_keyrows_small: ") and cause in msg, msg


def test_no_roots_launch_nothing(L):
    """n = 0: accepted without a device, with and without the pointers a batch would need; a bucket that does not truncate is no bucket"""
    assert _call(L, n=0)[0] == 0
    assert _call(L, n=0, null=("indptr", "indices", "query", "row_ids", "row_keys", "nsize", "flags"))[0] == 0
    assert _call(L, n=0, cfg=dict(bucket=201, row_pitch=224), work="both")[0] == 0
    for M, m in [(50, 1), (203, 1), (101, 2), (67, 3), (50, 4), (1, 1)]:
        assert _call(L, n=0, **_shape(M, m))[0] == 0, (M, m)


# ----------------------------------------------------------------------------------------------------------- the stages' shapes
@pytest.mark.parametrize("M,m", [(100, 2), (50, 1), (101, 2), (67, 3), (50, 4), (203, 1)])
def test_the_stages_accept_the_small_shapes(M, m):
    from surel_plus_amd import spjoin
    assert spjoin._counts_stage_shape("stage", M, m, True, 2048) is None


@pytest.mark.parametrize("M,m,why", [(300, 3, "no key-rows form"), (204, 1, "no key-rows form"), (100, 5, "no key-rows form"),
                                     (200, 4, "64-bit keys (key_rows_form == 64)")])
def test_the_stages_still_refuse_the_other_shapes(M, m, why):
    from surel_plus_amd import spjoin
    with pytest.raises(ValueError) as e:
        spjoin._counts_stage_shape("stage", M, m, True, 2048)
    assert str(e.value) == f"stage needs 32-bit LP keys: num_walks = {M}, num_steps = {m} has {why}"
    with pytest.raises(ValueError, match="key_rows=False has none"):
        spjoin._counts_stage_shape("stage", 100, 2, False, 2048)


def test_half_rows_stay_the_row_form_steps():
    """StepBuffers(dtype=) at a small shape is refused before it touches a device, as at every shape without 32-bit key rows of the
    fused-row kernel"""
    import torch
    from types import SimpleNamespace
    from surel_plus_amd import spjoin
    with pytest.raises(ValueError, match="no key rows"):
        spjoin.StepBuffers(SimpleNamespace(device="cpu"), 16, num_walks=100, num_steps=2, dtype=torch.bfloat16)

"""CPU: the on-demand step for one source against K targets -- the ninth header and its binding, every fault
subgacc_step_prologue_star refuses before it launches anything (return code, a message led by its name), the (P, K) segment lists
against the lists of the expanded edge tensor mapped to first-occurrence rows in NumPy, and what StepBuffers(star=K) refuses before
it touches a device.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAR_H = os.path.join(ROOT, "include", "subgacc_star.h")
NAME = "subgacc_step_prologue_star"
PUBLIC = ("sample_and_gather_star", "sample_and_hgather_star", "sample_and_counts_star", "sample_and_mean_stage_star",
          "sample_and_attn_counts_star", "sample_and_attn_stage_star", "sample_and_hcounts_star", "sample_and_hmean_stage_star")


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_ninth_header_parses_and_adds_one_entry_point(L):
    from surel_plus_amd import _lib
    decls = _lib.parse_header(open(STAR_H).read())
    assert list(decls) == [NAME] == list(_lib.STAR_SYMBOLS) and _lib.STAR_HEADER == STAR_H
    ret, args = decls[NAME]
    assert ret == "int" and args == [("uniq_table", "void *"), ("capacity", "int64_t"), ("zero_words", "int64_t *"), ("n_zero", "int64_t"),
                                     ("heads", "const int64_t *"), ("n_heads", "int64_t"), ("tails", "const int64_t *"),
                                     ("n_tails", "int64_t"), ("roots", "int32_t *"), ("stream", "void *")]
    fn = getattr(L, NAME)                                            # AttributeError: the library does not export it
    assert fn.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                           C.c_void_p] and fn.restype is C.c_int
    # the C ABI and the eight other headers stay as they were
    assert NAME not in _lib.SYMBOLS and len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and L.subgacc_abi_version() == 7
    assert "subgacc_step_prologue" in _lib.SYMBOLS and list(_lib.HALF_IDS_SYMBOLS) == ["subgacc_sjoin_fill_half_ids"]
    assert list(_lib.SMALL_SYMBOLS) == ["subgacc_walk_keyrows_small"]


def test_the_header_cites_the_reference_lines_it_serves():
    txt = open(STAR_H).read()
    for cite in ("utils.py:93-95", "train.py:246-280", "dataloader.py:265-275", "train.py:283-317"):
        assert cite in txt, cite


def test_the_makefile_and_the_staleness_check_name_the_header():
    from surel_plus_amd import _lib
    make = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^build/%\.o:.*$", make, re.M).group(0)
    assert "../../include/subgacc_star.h" in rule and "walk_prep.hip" in re.search(r"^SRCS\s*:=.*$", make, re.M).group(0)
    assert "STAR_HEADER" in inspect.getsource(_lib.build)
    src = open(os.path.join(ROOT, "surel_plus_amd", "csrc", "walk_prep.hip")).read()
    assert f'extern "C" int {NAME}(' in src and "step_prologue_star_kernel" in src


# -------------------------------------------------------------------------------------------------------- subgacc_step_prologue_star
def _call(L, table=None, capacity=0, zero="here", n_zero=4, heads="here", n_heads=3, tails="here", n_tails=5, roots="here"):
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    where = {"here": here, None: None}
    rc = getattr(L, NAME)(where[table], capacity, where[zero], n_zero, where[heads], n_heads, where[tails], n_tails, where[roots], None)
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("how,cause", [
    pytest.param(dict(roots=None), b"null argument", id="null-roots"),
    pytest.param(dict(roots=None, n_heads=0), b"null argument", id="null-roots-tails-only"),
    pytest.param(dict(roots=None, n_tails=0), b"null argument", id="null-roots-heads-only"),
    pytest.param(dict(heads=None), b"null argument", id="null-heads"),
    pytest.param(dict(tails=None), b"null argument", id="null-tails"),
    pytest.param(dict(zero=None), b"null argument", id="null-zero-words"),
    pytest.param(dict(zero=None, n_zero=1, n_heads=0, n_tails=0, heads=None, tails=None, roots=None), b"null argument", id="null-zero-words-alone"),
    pytest.param(dict(n_heads=-1), b"negative count", id="negative-heads"),
    pytest.param(dict(n_tails=-1), b"negative count", id="negative-tails"),
    pytest.param(dict(n_zero=-1), b"negative count", id="negative-zero-words"),
    pytest.param(dict(n_heads=1 << 29, n_tails=1 << 29), b"below 2^30", id="2^30-roots"),
    pytest.param(dict(n_heads=1 << 30, n_tails=0), b"below 2^30", id="2^30-heads"),
    pytest.param(dict(n_heads=1, n_tails=(1 << 30) - 1), b"below 2^30", id="2^30-tails"),
    pytest.param(dict(n_heads=1 << 62, n_tails=1 << 62), b"below 2^30", id="a-sum-that-would-wrap"),
    pytest.param(dict(n_zero=1 << 30), b"below 2^30", id="2^30-status-words"),
    pytest.param(dict(table="here", capacity=0), b"power of two", id="capacity-0"),
    pytest.param(dict(table="here", capacity=1000), b"power of two", id="capacity-1000"),
    pytest.param(dict(table="here", capacity=-8), b"power of two", id="capacity-negative"),
    pytest.param(dict(table="here", capacity=1 << 31), b"power of two", id="capacity-2^31")])
def test_the_prologue_refuses_before_any_launch(L, how, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, **how)
    assert rc == _lib.ERR_BADARG, msg
    assert msg.startswith(b"step_prologue_star: ") and cause in msg, msg


def test_nothing_to_do_launches_nothing(L):
    """no table, no words, no roots: accepted without a device, with and without the pointers"""
    assert _call(L, n_zero=0, n_heads=0, n_tails=0)[0] == 0
    assert _call(L, zero=None, n_zero=0, heads=None, n_heads=0, tails=None, n_tails=0, roots=None)[0] == 0
    assert _call(L, capacity=12345, n_zero=0, n_heads=0, n_tails=0)[0] == 0          # (without a table the capacity is not looked at)


# ------------------------------------------------------------------------------------------------------------- the segment lists
def _first_occurrence_rows(labels):
    """every entry's row when each distinct label gets one row, numbered in the order of first occurrence"""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)]


@pytest.mark.parametrize("P,K", [(1, 1), (1, 7), (3, 1), (5, 13), (64, 33), (2, 1024), (3, 683)])
def test_the_pair_lists_are_the_expanded_lists_on_first_occurrence_rows(P, K):
    """the expanded batch [source.repeat_interleave(K) | targets.view(-1)] with every position labelled by what stands there (source j,
    target i): gather's lists over it are own = the rows of [left | right] and partner = the rows of [right | left]"""
    from surel_plus_amd import spjoin
    B = P * K
    left = np.repeat(np.arange(P), K)                 # label: source j
    right = P + np.arange(B)                          # label: target i (every position its own: a repeated id is walked again)
    rows = _first_occurrence_rows(np.concatenate([left, right]))
    own, partner = spjoin._star_segments(P, K)
    assert own.dtype == partner.dtype == torch.int64 and own.shape == partner.shape == (2 * B,)
    assert np.array_equal(own.numpy(), rows) and np.array_equal(partner.numpy(), np.concatenate([rows[B:], rows[:B]]))
    assert int(own.max()) == P + B - 1 and len(np.unique(own.numpy())) == P + B
    # the issue's closed form
    i = np.arange(B)
    assert np.array_equal(own.numpy(), np.concatenate([i // K, P + i]))


@pytest.mark.parametrize("P,K", [(1, 1), (1, 7), (3, 1), (5, 13), (64, 33), (2, 1024), (3, 683)])
def test_the_triplet_list_is_the_expanded_list_on_first_occurrence_rows(P, K):
    """[u.repeat_interleave(K) | v.repeat_interleave(K) | w.view(-1)] labelled u_j, v_j, w_i: hgather's own list is the rows of
    [U | W | V | W], its partner list is left to the kernels (mirrored)"""
    from surel_plus_amd import spjoin
    B = P * K
    u, v, w = np.repeat(np.arange(P), K), P + np.repeat(np.arange(P), K), 2 * P + np.arange(B)
    rows = _first_occurrence_rows(np.concatenate([u, v, w]))
    ru, rv, rw = rows[:B], rows[B:2 * B], rows[2 * B:]
    own, partner = spjoin._star_segments(P, K, triplets=True)
    assert partner is None and own.dtype == torch.int64 and own.shape == (4 * B,)
    assert np.array_equal(own.numpy(), np.concatenate([ru, rw, rv, rw]))
    assert int(own.max()) == 2 * P + B - 1 and len(np.unique(own.numpy())) == 2 * P + B
    i = np.arange(B)
    assert np.array_equal(own.numpy(), np.concatenate([i // K, 2 * P + i, P + i // K, 2 * P + i]))


def test_an_empty_star_has_empty_lists():
    from surel_plus_amd import spjoin
    for P, K in [(0, 5), (4, 0)]:
        own, partner = spjoin._star_segments(P, K)
        assert own.numel() == partner.numel() == 0 and spjoin._star_segments(P, K, triplets=True)[0].numel() == 0


# --------------------------------------------------------------------------------------------------------------- the Python layer
def _graph(**more):
    return SimpleNamespace(device="cpu", **more)


@pytest.mark.parametrize("triplets", [False, True])
def test_step_buffers_refuse_by_the_keywords_name(triplets):
    from surel_plus_amd import spjoin
    for pairs, kw, name in [(16, dict(star=4, batch=8), "batch="), (16, dict(star=4, batch=16), "batch="),
                            (16, dict(star=4, dedup_roots=True), "dedup_roots=True"),
                            (16, dict(star=4, rng="rand_r"), "rng='rand_r'"),
                            (16, dict(star=4, stage="index", table_rows=64), "stage='index'"),
                            (16, dict(star=0), "K = 0"), (16, dict(star=-3), "K = -3"),
                            (16, dict(star=5), "a multiple of K = 5"), (7, dict(star=2), "a multiple of K = 2")]:
        with pytest.raises(ValueError, match=re.escape("star=")) as err:
            spjoin.StepBuffers(_graph(), pairs, triplets=triplets, **kw)
        assert name in str(err.value) and str(err.value).startswith("StepBuffers(star="), (kw, str(err.value))
    # what star does not refuse reaches the device (a namespace has none)
    with pytest.raises(AttributeError):
        spjoin.StepBuffers(_graph(), 16, triplets=triplets, star=4)


def test_without_the_keyword_nothing_changes():
    from surel_plus_amd import spjoin
    assert inspect.signature(spjoin.StepBuffers.__init__).parameters["star"].default is None
    with pytest.raises(ValueError, match="root dedup works on one batch") as err:       # today's refusal, today's words
        spjoin.StepBuffers(_graph(), 16, batch=8, dedup_roots=True)
    assert "star" not in str(err.value)
    # gather_star's refusal of a strided store stays
    assert "not a StridedSpG" in inspect.getsource(spjoin.gather_star)


def test_the_public_functions_are_exported_and_check_their_input_on_the_host():
    import surel_plus_amd as sp
    from surel_plus_amd import spjoin
    for name in PUBLIC:
        assert getattr(sp, name) is getattr(spjoin, name)
        prm = inspect.signature(getattr(sp, name)).parameters
        assert "dedup_roots" not in prm and "rng" not in prm and "buffers" in prm, name
    src, tg = np.arange(3), np.zeros((3, 4), dtype=np.int64)
    for fn in (sp.sample_and_gather_star, sp.sample_and_counts_star):
        with pytest.raises(ValueError, match="targets has 2 rows for 3 sources"):
            fn(_graph(), src, tg[:2])
        with pytest.raises(ValueError, match="targets must be 2-D"):
            fn(_graph(), src, tg.reshape(-1))
        with pytest.raises(TypeError, match="integer"):
            fn(_graph(), src, tg.astype(np.float32))
    for fn in (sp.sample_and_hgather_star, sp.sample_and_hcounts_star):
        with pytest.raises(ValueError, match=re.escape("uv must be [2, P]")):
            fn(_graph(), np.zeros((3, 3), dtype=np.int64), tg)
        with pytest.raises(ValueError, match="targets has 2 rows for 3 sources"):
            fn(_graph(), np.zeros((2, 3), dtype=np.int64), tg[:2])


def test_buffers_of_another_geometry_are_refused():
    import surel_plus_amd as sp
    src, tg = np.arange(3), np.zeros((3, 4), dtype=np.int64)
    base = dict(star=4, B=12, triplets=False, stage=None, ptr=True, M=200, m=3, half=0, half64=False, small=False, order=None, dtype=torch.float32)
    for change in (dict(star=0), dict(star=3), dict(B=16), dict(triplets=True), dict(stage="counts"), dict(ptr=False), dict(M=100)):
        with pytest.raises(ValueError, match="another geometry"):
            sp.sample_and_gather_star(_graph(), src, tg, buffers=SimpleNamespace(**{**base, **change}))
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather_star(_graph(), src, tg, dtype=torch.bfloat16, buffers=SimpleNamespace(**base))
    with pytest.raises(ValueError, match="another geometry"):
        sp.sample_and_hgather_star(_graph(), np.zeros((2, 3), dtype=np.int64), tg, buffers=SimpleNamespace(**base))
    stage = {**base, "stage": "counts", "dedup": False, "T": 64, "wide": False}
    for change in (dict(star=0), dict(star=2), dict(B=8), dict(triplets=True), dict(stage="counts_attn")):
        with pytest.raises(ValueError, match="buffers= must be StepBuffers"):
            sp.sample_and_counts_star(_graph(), src, tg, buffers=SimpleNamespace(**{**stage, **change}))
    # ... and star buffers under the plain stage call
    with pytest.raises(ValueError, match="buffers= must be StepBuffers"):
        sp.sample_and_counts(_graph(), np.zeros((2, 12), dtype=np.int64), buffers=SimpleNamespace(**stage))

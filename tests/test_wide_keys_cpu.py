"""CPU: the on-demand stages over 64-bit key rows -- the NumPy restatements of tests/wide_keys.py against the oracle's LP rows of a
4-hop sample, the fifth header and its binding, every fault subgacc_keyrows_columns64 refuses before it launches anything, and what
the Python side admits and refuses with and without wide_keys=True.  No GPU needed."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import wide_keys as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_H = os.path.join(ROOT, "include", "subgacc_wide.h")
NAMES = ["subgacc_keyrows_columns64_workspace_bytes", "subgacc_keyrows_columns64"]
_NO_DEVICE = SimpleNamespace(device="cpu")       # nothing of it is looked at before the refusals


@pytest.fixture(scope="module")
def L():
    from surel_plus_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------- the restatements
def test_the_shapes_of_the_tests_have_33_and_61_bits():
    assert W.shift_of(200) == 8 and W.key_bits(200, 4) == 33
    assert W.shift_of(30000) == 15 and W.key_bits(30000, 4) == 61
    assert W.shift_of(128) == 8 and W.shift_of(204) == 8 and W.shift_of(127) == 7
    for M in (200, 30000):
        keys = W.edge_keys(M, 4)
        lead = 1 << (4 * W.shift_of(M))
        assert keys[1] == keys[0] | lead and keys[0] & lead == 0                       # the lead bit alone
        assert keys[2] - keys[0] == 1 << (3 * W.shift_of(M)) and keys[3] - keys[0] == 1  # the top count alone, the low word alone
        assert max(keys) == keys[4] and keys[4].bit_length() == W.key_bits(M, 4)
        assert len({k & 0xFFFFFFFF for k in keys}) < len(keys)                          # a truncation to 32 bits merges keys
    k200 = W.edge_keys(200, 4)
    assert k200[0] & 0xFFFFFFFF == k200[1] & 0xFFFFFFFF                                 # 33 bits: the lead is all a truncation loses


def test_feature_rows_unpack_what_pack_packed():
    for M in (128, 200, 204, 30000):
        rng = np.random.default_rng(M)
        counts = rng.integers(0, M + 1, (300, 4))
        lead = rng.integers(0, 2, 300)
        keys = np.array([W.pack(c, l, M) for c, l in zip(counts, lead)], dtype=np.uint64)
        f = W.feature_rows(keys, M, 4)
        want = np.concatenate([(lead * M)[:, None], counts], 1).astype(np.float32) / np.float32(M)
        assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), want.astype(np.float32).view(np.uint32))
        # the 32-bit restatement of the 3-hop tests, on keys that fit it
    small = np.array([W.pack(c, 0, 200) for c in np.random.default_rng(1).integers(0, 201, (50, 3))], dtype=np.uint64)
    s = 8
    cols = [np.zeros(50, np.float32)] + [((small >> np.uint64((3 - j) * s)) & np.uint64(255)).astype(np.float32) for j in (1, 2, 3)]
    assert np.array_equal(W.feature_rows(small, 200, 3), np.stack(cols, 1) / np.float32(200))


def test_the_mix_restated_twice_agrees_and_spreads():
    keys = W.lp_keys(5000, 3, 30000, 4)
    h = W.mix(keys)
    assert all(int(h[i]) == W.mix_int(int(keys[i])) for i in range(0, 5000, 97))
    home = W.lds_home(keys)
    assert home.min() >= 0 and home.max() < 4096 and len(np.unique(home)) > 2500        # 5,000 balls, 4,096 bins: ~2,900 occupied
    # keys that differ only above bit 31 do not share a home by construction
    a, b = W.edge_keys(30000, 4)[:2]
    assert W.mix_int(a) != W.mix_int(b)
    crowd, slot = W.same_home_keys(40, 9, 200, 4)
    assert len(np.unique(crowd)) == 40 > W.PROBES and (W.lds_home(crowd) == slot).all()


def test_columns_restated_on_a_hand_made_case():
    M, hops, stride = 200, 4, 8
    k = np.array([W.pack([1, 0, 0, 0], 0, M), W.pack([0, 0, 0, 2], 1, M), W.pack([0, 0, 0, 2], 0, M)], dtype=np.uint64)
    assert k[1] > k[0] > k[2] and int(k[1]) & 0xFFFFFFFF == int(k[2])                   # equal low words
    keys = np.full((3, stride), W.POISON64, dtype=np.uint64)
    keys[0, :3], keys[2, :2] = [k[0], k[1], k[2]], [k[1], k[1]]
    lens = np.array([3, 0, 2])
    c, u64, u, feat, cols, over = W.columns(keys, lens, 5, M, hops)
    assert c == 3 and not over and u64.tolist() == [k[2], k[0], k[1], 0] and u.tolist() == [1, 2, 3, 0]
    assert cols[0, :3].tolist() == [2, 3, 1] and cols[2, :2].tolist() == [3, 3]
    assert (cols[1] == W.POISON32).all() and (cols[0, 3:] == W.POISON32).all() and (cols[2, 2:] == W.POISON32).all()
    assert not feat[0].any() and not feat[4].any() and feat[3, 0] == 1.0 and feat[1, 4] == np.float32(2) / np.float32(200)
    c, u64, u, feat, cols, over = W.columns(keys, lens, 3, M, hops)                     # one key too many: the largest is dropped
    assert c == 2 and over and u64.tolist() == [k[2], k[0]] and cols[0, :3].tolist() == [2, 0, 1] and cols[2, :2].tolist() == [0, 0]
    c, u64, u, feat, cols, over = W.columns(keys, np.array([100, 0, 0]), 5, M, hops)    # a length beyond the stride is clamped
    assert c == 4 and W.POISON64 in u64.tolist()


def _graph():
    """the graph of test_gpu_horder.World, built without its device store"""
    from test_gpu_horder import World
    return World(SimpleNamespace(DeviceCSR=lambda *a: None))


def test_restatements_against_the_oracle_rows_of_a_4_hop_sample():
    """the oracle's distinct LP rows (enc) of every node's 4-hop set at M = 200 and M = 128, packed as subg_acc.c:936-955 packs them:
    as many keys as rows, feature_rows(sorted keys) are the rows / M, and their number fits the 8,191 columns of a wide step"""
    import oracle
    w = _graph()
    for M, want in ((200, 7398), (128, 5074)):
        nsize, remap, enc, raw = oracle.gset_sampler(w.indptr, w.indices, np.arange(w.N), num_walks=M, num_steps=4, seed=5, rng="philox",
                                                     debug=True)
        c = len(enc)
        print(f"M = {M}, 4 hops: {c} distinct LP rows over {w.N} roots, {len(raw)} members")
        assert c == want and c + 1 <= W.MAX_T
        assert enc.min() >= 0 and enc.max() <= M and set(np.unique(enc[:, 0])) <= {0, M}
        keys = np.array([W.pack(r[1:], r[0] != 0, M) for r in enc], dtype=np.uint64)
        assert len(np.unique(keys)) == c and int(keys.max()).bit_length() == 33
        order = np.argsort(keys)
        f = W.feature_rows(keys[order], M, 4)
        assert np.array_equal(f.view(np.uint32), (enc[order].astype(np.float32) / np.float32(M)).view(np.uint32))
        member = np.array([W.pack(r[1:], r[0] != 0, M) for r in raw[:: max(len(raw) // 20000, 1)]], dtype=np.uint64)
        assert np.isin(member, keys).all()
        if M == 200:        # the members as two rows of a step: every column is the rank + 1 of its key
            rows = np.full((2, len(member)), W.POISON64, dtype=np.uint64)
            rows[0], rows[1, :100] = member, member[:100]
            cc, u64, u, feat, cols, over = W.columns(rows, np.array([len(member), 100]), c + 1, M, 4)
            assert not over and cc == len(np.unique(member)) and np.array_equal(u64[cols[0] - 1], member)
            assert np.array_equal(cols[1, :100], cols[0, :100]) and (cols[1, 100:] == W.POISON32).all()


# ------------------------------------------------------------------------------------------------------- the header and its binding
def test_the_fifth_header_declares_two_entry_points_and_the_library_exports_them(L):
    from surel_plus_amd import _lib
    decls = _lib.parse_header(open(WIDE_H).read())
    assert list(decls) == NAMES == list(_lib.WIDE_SYMBOLS) == list(_lib.WIDE_DECLS)
    assert decls[NAMES[0]] == ("size_t", [("table_rows", "int64_t")])
    ret, args = decls[NAMES[1]]
    assert ret == "int" and args == [
        ("row_keys", "const int64_t *"), ("nsize", "const int32_t *"), ("n", "int64_t"), ("stride", "int32_t"), ("num_walks", "int32_t"),
        ("num_steps", "int32_t"), ("table_rows", "int64_t"), ("out_ukeys64", "int64_t *"), ("out_ukeys", "int32_t *"),
        ("out_count", "int64_t *"), ("out_feat", "float *"), ("out_cols", "int32_t *"), ("flags", "int32_t *"), ("workspace", "void *"),
        ("workspace_bytes", "size_t"), ("stream", "void *")]
    # subgacc_keyrows_columns with 64-bit rows, the 64-bit key list and the surrogate plane
    narrow = [a for a in args if a[0] not in ("out_ukeys64", "out_cols")]
    assert [(n, "const int32_t *" if n == "row_keys" else t) for n, t in narrow] == _lib.DECLS["subgacc_keyrows_columns"][1]
    assert len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7 and not set(NAMES) & set(_lib.SYMBOLS)
    assert os.path.basename(_lib.WIDE_HEADER) == "subgacc_wide.h"
    fn = getattr(L, NAMES[1])                                        # AttributeError: the library does not export it
    assert fn.restype is C.c_int and getattr(L, NAMES[0]).restype is C.c_size_t
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    assert all(n in names for n in NAMES)


def test_workspace_bytes(L):
    f = L.subgacc_keyrows_columns64_workspace_bytes
    assert [f(t) for t in (0, 1, 8193, 1 << 40, -3)] == [0] * 5
    assert f(2) == 1024 * 8 == f(512) and f(513) == 2048 * 8 and f(4096) == 8192 * 8 and f(4097) == 16384 * 8 == f(8192) == 128 * 1024
    assert all(f(t) == W.set_slots(t) * 8 for t in (2, 300, 1030, 5001, 8192))


# ------------------------------------------------------------------------------------------------------- the entry point's refusals
def _call(L, **change):
    """subgacc_keyrows_columns64 with host pointers: every case is refused before a launch"""
    buf = (C.c_int64 * 64)()
    here = C.addressof(buf)
    a = dict(row_keys=here, nsize=here, n=4, stride=8, num_walks=200, num_steps=4, table_rows=16, out_ukeys64=here, out_ukeys=here,
             out_count=here, out_feat=here, out_cols=here, flags=here, workspace=here, workspace_bytes=1 << 20, stream=None)
    a.update(change)
    rc = L.subgacc_keyrows_columns64(*[a[k] for k in ("row_keys", "nsize", "n", "stride", "num_walks", "num_steps", "table_rows",
                                                      "out_ukeys64", "out_ukeys", "out_count", "out_feat", "out_cols", "flags",
                                                      "workspace", "workspace_bytes", "stream")])
    return rc, L.subgacc_last_error()


@pytest.mark.parametrize("change,cause", [
    (dict(n=-1), b"bad sizes"), (dict(n=1 << 40), b"bad sizes"), (dict(stride=0), b"bad sizes"),
    (dict(table_rows=1), b"table_rows = 1"), (dict(table_rows=0), b"table_rows = 0"),
    (dict(out_ukeys64=None), b"null argument (out_ukeys64"), (dict(out_ukeys=None), b"null argument (out_ukeys64"),
    (dict(out_count=None), b"null argument (out_ukeys64"), (dict(out_feat=None), b"null argument (out_ukeys64"),
    (dict(flags=None), b"null argument (out_ukeys64"), (dict(workspace=None), b"null argument (out_ukeys64"),
    (dict(row_keys=None), b"null argument (row_keys"), (dict(nsize=None), b"null argument (row_keys"),
    (dict(out_cols=None), b"null argument (row_keys"),
    (dict(num_walks=0), b"num_walks = 0"), (dict(num_steps=0), b"num_steps = 0"),
    (dict(num_walks=100, num_steps=9), b"64 bits > 63"),                # 9 * 7 + 1
    (dict(num_walks=30000, num_steps=5), None),                         # 76 bits: subgacc_key_shift's own refusal
])
def test_columns64_refuses_before_any_launch(L, change, cause):
    from surel_plus_amd import _lib
    rc, msg = _call(L, **change)
    if cause is None:
        assert rc == _lib.ERR_KEYWIDTH
        return
    assert rc == _lib.ERR_BADARG
    assert msg.startswith(b"keyrows_columns64: ") and cause in msg, msg


def test_columns64_refuses_what_lds_and_the_workspace_do_not_hold(L):
    from surel_plus_amd import _lib
    rc, msg = _call(L, table_rows=8193)
    assert rc == _lib.ERR_LDS and msg.startswith(b"keyrows_columns64: table_rows = 8193") and b"LDS" in msg and b"8192" in msg
    rc, msg = _call(L, table_rows=8192, workspace_bytes=128 * 1024 - 1)
    assert rc == _lib.ERR_WORKSPACE and msg.startswith(b"keyrows_columns64: workspace of 131071 bytes, 131072 needed")
    rc, msg = _call(L, table_rows=16, workspace_bytes=8191)
    assert rc == _lib.ERR_WORKSPACE
    # the order: table_rows before the null arguments, the null arguments before the shape, the shape before the workspace
    assert _call(L, table_rows=1, out_feat=None)[1].startswith(b"keyrows_columns64: table_rows")
    assert _call(L, table_rows=8193, out_feat=None)[0] == _lib.ERR_LDS
    assert _call(L, num_walks=0, out_feat=None)[1].startswith(b"keyrows_columns64: null argument")
    assert _call(L, num_walks=100, num_steps=9, workspace_bytes=0)[0] == _lib.ERR_BADARG


# -------------------------------------------------------------------------------------------------------------------- Python
def test_counts_stage_shape_with_and_without_wide_keys():
    from surel_plus_amd import spjoin
    assert spjoin.COUNTS_MAX_TABLE_ROWS_WIDE == 8192 == W.MAX_T
    assert spjoin._counts_stage_shape("stage", 200, 4, True, 2048, True) is None
    for M in (128, 204):
        assert spjoin._counts_stage_shape("stage", M, 4, True, 8192, True) is None
    with pytest.raises(ValueError, match=r"stage needs 32-bit LP keys: num_walks = 200, num_steps = 4 has 64-bit keys \(key_rows_form == 64\)"):
        spjoin._counts_stage_shape("stage", 200, 4, True, 2048)
    with pytest.raises(ValueError, match="key_rows_form == 64"):
        spjoin._counts_stage_shape("stage", 200, 4, True, 2048, False)
    for T in (8193, 16384, 1):
        with pytest.raises(ValueError, match=f"table_rows = {T}"):
            spjoin._counts_stage_shape("stage", 200, 4, True, T, True)
    # nothing changes at the other shapes: 32-bit rows keep their 16,384, a shape without key rows stays refused
    assert spjoin._counts_stage_shape("stage", 200, 3, True, 16384, True) is None
    assert spjoin._counts_stage_shape("stage", 127, 4, True, 16384, True) is None
    assert spjoin._counts_stage_shape("stage", 50, 4, True, 16384, True) is None             # a small shape
    with pytest.raises(ValueError, match="no key-rows form"):
        spjoin._counts_stage_shape("stage", 300, 3, True, 2048, True)
    with pytest.raises(ValueError, match="no key-rows form"):
        spjoin._counts_stage_shape("stage", 205, 4, True, 2048, True)
    with pytest.raises(ValueError, match="key_rows=False"):
        spjoin._counts_stage_shape("stage", 200, 4, False, 2048, True)


@pytest.mark.parametrize("stage", ["counts", "counts_attn", "index"])
def test_step_buffers_refuse_without_a_device(stage):
    import surel_plus_amd as sp
    with pytest.raises(ValueError, match="key_rows_form == 64"):                             # the default: as ever
        sp.StepBuffers(_NO_DEVICE, 8, num_walks=200, num_steps=4, stage=stage)
    with pytest.raises(ValueError, match="table_rows = 8193"):
        sp.StepBuffers(_NO_DEVICE, 8, num_walks=200, num_steps=4, stage=stage, table_rows=8193, wide_keys=True)
    with pytest.raises(ValueError, match="key_rows=False"):
        sp.StepBuffers(_NO_DEVICE, 8, num_walks=200, num_steps=4, stage=stage, key_rows=False, wide_keys=True)
    with pytest.raises(ValueError, match="batch=None"):
        sp.StepBuffers(_NO_DEVICE, 8, num_walks=200, num_steps=4, stage=stage, batch=4, wide_keys=True)


def test_the_eight_calls_take_the_keyword_and_refuse_without_a_device():
    import inspect
    import torch
    import surel_plus_amd as sp
    e, h = torch.zeros((2, 4), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64)
    ident, lin = torch.nn.Identity(), torch.nn.Linear(5, 1)
    lstm = torch.nn.LSTM(5, 16, batch_first=True)
    calls = {"sample_and_counts": (e,), "sample_and_hcounts": (h,), "sample_and_mean_stage": (e, ident), "sample_and_hmean_stage": (h, ident),
             "sample_and_attn_counts": (e, lambda t: t[:, 0]), "sample_and_attn_stage": (e, ident, lin), "sample_and_index": (e,),
             "sample_and_lstm_stage": (e, ident, lstm)}
    nodev = SimpleNamespace(device=torch.device("cpu"))     # (the model stages compare their modules' device with it first)
    for name, args in calls.items():
        f = getattr(sp, name)
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "wide_keys" and p["wide_keys"].default is False, name
        assert inspect.signature(sp.StepBuffers.__init__).parameters["wide_keys"].default is False
        with pytest.raises(ValueError, match="key_rows_form == 64"):                         # the pinned refusal, by default
            f(nodev, *args, num_walks=200, num_steps=4)
        with pytest.raises(ValueError, match="table_rows = 8193"):
            f(nodev, *args, num_walks=200, num_steps=4, table_rows=8193, wide_keys=True)
        with pytest.raises(ValueError, match="no key-rows form"):
            f(nodev, *args, num_walks=300, num_steps=3, wide_keys=True)


def test_buffers_made_with_another_setting_are_refused():
    """with buffers= the buffers' own setting holds: wide buffers meet a call without the keyword at a 64-bit shape (and the reverse)"""
    import torch
    import surel_plus_amd as sp
    e = torch.zeros((2, 4), dtype=torch.int64)
    for wide in (True, False):
        bufs = SimpleNamespace(stage="counts", triplets=False, dedup=False, M=200, m=4, T=64, order=None, wide=wide)
        with pytest.raises(ValueError, match="buffers= serves the step its StepBuffers were made for"):
            sp.sample_and_counts(_NO_DEVICE, e, num_walks=200, num_steps=4, buffers=bufs, wide_keys=not wide)

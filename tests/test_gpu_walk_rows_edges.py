"""GPU (MI355X): the fused-row walk (csrc/walk_rows.hip: walk_rows_kernel behind launch_walk_rows) driven through the C ABI at every
edge of its dispatch, of the root's degree and of the epilogues' sorts, with the graphs and shapes of tests/walk_rows_edges.py --
tests/test_walk_rows_edges_cpu.py shows on the host that every case reaches the branch it is here for.

The reference is the oracle's (nsize, remap, enc) of the same batch, computed once per (graph, shape, rng) and shared; every comparison
is bit for bit.  Every output is poisoned before the launch and stands between two poisoned guards: the guards, the tail of every
row behind its last member and the words between a row's capacity and the pitch must come back untouched."""
import functools

import numpy as np
import pytest
import torch

import walk_rows_edges as W
from gpu_helpers import sp  # noqa: F401
from walk_rows_edges import GUARD, NO_ROOT, POISON

pytestmark = pytest.mark.gpu

SEED = 13
CAP = 4096                   # slots of the table of distinct LP rows (a few hundred rows per batch)
EMPTY_KEY = np.uint64(2 ** 64 - 1)
RNGS = ("rand_r", "philox")
NARROW = (24, 32)            # id and row-begin bits of the narrow hop records: 8 bits are left for the degree


# --------------------------------------------------------------------------------------------------------------------- plumbing
def _L():
    from surel_plus_amd import _lib
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype, init=None):
    """n words of poison (or `init`) between two poisoned guards: (whole buffer, the n words)"""
    whole = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device="cuda")
    view = whole[GUARD: GUARD + n]
    if init is not None:
        view.copy_(_dev(init).view(dtype))
    return whole, view


def _back(whole, n):
    """the n words as NumPy, after the guards in front and behind were seen untouched"""
    h = whole.cpu().numpy()
    assert (h[:GUARD] == POISON).all() and (h[GUARD + n:] == POISON).all(), "a guard word was written"
    return h[GUARD: GUARD + n]


@functools.lru_cache(maxsize=2)
def _graphs(kind, M, m):
    """{(idx64, records): DeviceCSR} of one graph: int32 and int64 row offsets; no hop records, the records that go with the offsets
    (8 bytes | 16 bytes) and -- int32 offsets -- 8-byte records whose degree field is so narrow that hubs take the escape path"""
    from surel_plus_amd.sampler import DeviceCSR
    g = W.graph(kind, M, m)
    out = {}
    for idx64 in (False, True):
        ip = g["indptr"].astype(np.int64) if idx64 else g["indptr"]
        for rec in (False, True) + (() if idx64 else ("narrow",)):
            csr = DeviceCSR(ip, g["indices"])
            r = csr.hop_records(force=bool(rec), bits=NARROW if rec == "narrow" else None)
            assert (r is None) == (rec is False) and (r is None or (r[1] == 0) == idx64)
            out[(idx64, rec)] = csr
    return out


def _launch(csr, q, M, m, rng, form, pitch=0, work=None, n_work=None, work_cap=0, entry=None, bucket=-1, cap_root=True, check=True):
    """one walk through the C ABI into poisoned, guarded outputs.  form: table | keys32 | keys64; entry: None (subgacc_walk_spg /
    subgacc_walk_keyrows64), "sparse" or "list".  -> dict(rc, ids [n, P], pay [n, P], nsize [n], flags [4], table keys, ukeys)"""
    from surel_plus_amd import sampler
    L = _L()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n = len(q)
    Q = M * m + 1
    stride = bucket if bucket > 0 else Q
    P = pitch if pitch > 0 else stride
    d_q = _dev(np.asarray(q, dtype=np.int32))
    cfg = sampler.make_cfg(csr, M, m, bucket, SEED, rng, cap_root_degree=cap_root, row_pitch=pitch)
    rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st) if entry != "sparse" else (None, None)
    w_ids, ids = _guarded(n * P, torch.int32)
    w_pay, pay = _guarded(n * P, torch.int64 if form == "keys64" else torch.int32)
    w_ns, nsize = _guarded(n, torch.int32)
    w_fl, flags = _guarded(4, torch.int32, np.zeros(4, np.int32))
    table, tab = None, (None, 0)
    if form == "table":
        nbytes = lib.subgacc_uniq_table_bytes(CAP)
        table = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        L.check(lib.subgacc_uniq_reset(ptr(table), CAP, st))
        tab = (ptr(table), CAP)
    d_wl = _dev(np.asarray(work, dtype=np.int32)) if work is not None else None
    d_nw = _dev(np.array([n_work], dtype=np.int64)) if work is not None else None
    g = (cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n)
    rows = (ptr(ids), ptr(pay), ptr(nsize), ptr(flags), st)
    if form == "keys64":
        assert entry in (None, "sparse")
        rc = lib.subgacc_walk_keyrows64(*g, ptr(rp), ptr(rs), ptr(d_wl), ptr(d_nw), *rows)
    elif entry == "sparse":
        rc = lib.subgacc_walk_spg_sparse(*g, ptr(d_wl), ptr(d_nw), *tab, *rows)
    elif entry == "list":
        rc = lib.subgacc_walk_spg_list(*g, ptr(rp), ptr(rs), ptr(d_wl), ptr(d_nw), *tab, *rows)
    else:
        rc = lib.subgacc_walk_spg(*g, 0, ptr(rp), ptr(rs), *tab, *rows)
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    out = dict(rc=rc, P=P, n=n, form=form)
    if table is not None and rc == 0:
        ukeys = torch.full((CAP,), -1, dtype=torch.int64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.subgacc_uniq_number_workspace_bytes(CAP, 0), dtype=torch.uint8, device="cuda")
        L.check(lib.subgacc_uniq_number(ptr(table), CAP, None, 0, ptr(ukeys), CAP, ptr(count), CAP, ptr(ws), ws.numel(), st))
        t = table.cpu().numpy()
        assert (t[nbytes:] == 0xA5).all(), "bytes behind the table were written"
        out["tkeys"] = t[: 8 * CAP].view(np.uint64)
        out["ukeys"] = ukeys.cpu().numpy().view(np.uint64)[: int(count.item())]
    out.update(ids=_back(w_ids, n * P).reshape(n, P), pay=_back(w_pay, n * P).reshape(n, P), nsize=_back(w_ns, n), flags=_back(w_fl, 4))
    return out


def _check(got, exp, listed=None, empty=(), flags=(0, 0, 0, 0), numbering=True, what=""):
    """the rows `listed` (default: all) equal the oracle's -- ids, and the payload: the LP key itself, or the slot of a table whose key
    column holds it; rows in `empty` have nsize 0 and nothing else; every other row and every word behind a row's last member is
    poison; the table's numbering is the oracle's first-occurrence numbering of the listed rows"""
    n, P, form = got["n"], got["P"], got["form"]
    listed = np.arange(n) if listed is None else np.asarray(listed, dtype=np.int64)
    want_ns = np.full(n, POISON, dtype=np.int32)
    want_ns[listed] = exp["nsize"][listed]
    want_ns[list(empty)] = 0
    assert got["flags"].tolist() == list(flags), (what, got["flags"].tolist())
    assert np.array_equal(got["nsize"], want_ns), (what, np.nonzero(got["nsize"] != want_ns)[0][:8])
    lens = exp["nsize"][listed].astype(np.int64)
    assert lens.max(initial=0) <= P
    r = np.repeat(listed, lens)
    c = np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    src = np.repeat(exp["off"][listed], lens) + c
    want_ids = np.full((n, P), POISON, dtype=np.int32)
    want_ids[r, c] = exp["ids"][src]
    assert np.array_equal(got["ids"], want_ids), (what, "ids", np.nonzero((got["ids"] != want_ids).any(axis=1))[0][:8])
    member = np.zeros((n, P), dtype=bool)
    member[r, c] = True
    assert (got["pay"][~member] == POISON).all(), (what, "a payload word behind a row's end was written")
    keys = exp["keys"][src]
    if form == "table":
        slot = got["pay"][r, c]
        assert (slot >= 0).all() and (slot < CAP).all() and np.array_equal(got["tkeys"][slot], keys), (what, "slots")
        if numbering:
            assert np.array_equal(got["ukeys"], W.numbering_of(exp, listed)), (what, "numbering")
            assert int((got["tkeys"] != EMPTY_KEY).sum()) == len(got["ukeys"])
    elif form == "keys32":
        assert np.array_equal(got["pay"][r, c], keys.astype(np.uint32).view(np.int32)), (what, "keys")
    else:
        assert np.array_equal(got["pay"][r, c].view(np.uint64), keys), (what, "keys")


def _tags_only(csr, q, M, m, rng, pitch):
    """the batched registration of a kept store: 32-bit key rows, their keys registered with coarse tags, the candidates walked again
    by the table form for their exact first-visit tags (subgacc_walk_tags), the table numbered -> (the key rows, the distinct keys)"""
    from surel_plus_amd import sampler
    L = _L()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n = len(q)
    rows = _launch(csr, q, M, m, rng, "keys32", pitch)
    P = rows["P"]
    d_q = _dev(np.asarray(q, dtype=np.int32))
    cfg = sampler.make_cfg(csr, M, m, -1, SEED, rng, row_pitch=pitch)
    rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st)
    nbytes = lib.subgacc_uniq_table_bytes(CAP)
    table = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(lib.subgacc_uniq_reset(ptr(table), CAP, st))
    d_keys, d_ns = _dev(rows["pay"].reshape(-1)), _dev(rows["nsize"])
    ccap = lib.subgacc_keyrows_cand_capacity(n)
    w_cand, cand = _guarded(ccap, torch.int32)
    ncand = torch.zeros(1, dtype=torch.int64, device="cuda")
    w_fl, flags = _guarded(4, torch.int32, np.zeros(4, np.int32))
    L.check(lib.subgacc_keyrows_register(ptr(d_keys), ptr(d_ns), n, P, 0, ptr(table), CAP, ptr(cand), ccap, ptr(ncand), ptr(flags), st))
    nc = int(ncand.item())
    assert 1 <= nc <= n
    L.check(lib.subgacc_walk_tags(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, 0, ptr(rp), ptr(rs), ptr(cand),
                                  ptr(ncand), nc, ptr(table), CAP, ptr(flags), st))
    ukeys = torch.full((CAP,), -1, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.subgacc_uniq_number_workspace_bytes(CAP, 0), dtype=torch.uint8, device="cuda")
    L.check(lib.subgacc_uniq_number(ptr(table), CAP, None, 0, ptr(ukeys), CAP, ptr(count), CAP, ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    assert (table.cpu().numpy()[nbytes:] == 0xA5).all() and not _back(w_fl, 4).any()
    _back(w_cand, ccap)
    return rows, ukeys.cpu().numpy().view(np.uint64)[: int(count.item())], nc


def _each(M, m, form):
    """(idx64, records, pitch) of every launch of one form at one shape"""
    return [(i, r, p) for f, i, r in W.launches(M, m) if f == form for p in W.pitches(M * m + 1)]


# -------------------------------------------------------------------------------------------- 1. every shape of the shape table
@pytest.mark.parametrize("m,M", W.SHAPES)
def test_table_form_at_every_shape(sp, m, M):
    """the table form (fused, numbered) of every shape of the shape table on the edge graph: rows, slots and the first-occurrence
    numbering against the oracle -- int32 and int64 row offsets, no records / records / narrow records, both store pitches, both RNGs"""
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    seen = set()
    for rng in RNGS:
        exp = W.expected_rows("edge", M, m, rng, SEED)
        for idx64, rec, pitch in _each(M, m, "table"):
            got = _launch(csrs[(idx64, rec)], g["batch"], M, m, rng, "table", pitch)
            _check(got, exp, what=(rng, idx64, rec, pitch))
            assert np.array_equal(got["ukeys"], exp["ukeys"])
            seen.add(W.variant(M, m, "table", idx64, bool(rec)))
    print(f"M = {M}, m = {m}: rows = {len(g['batch'])}, largest set = {int(exp['nsize'].max())}, instantiations = {sorted(seen)}")


@pytest.mark.parametrize("m,M", W.SHAPES)
def test_key_rows_at_every_shape(sp, m, M):
    """32-bit key rows (64-bit from M = 128 at four hops): ids and every member's LP key against the oracle, the same crossing"""
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    form = W.forms_of(M, m)[1]
    seen = set()
    for rng in RNGS:
        exp = W.expected_rows("edge", M, m, rng, SEED)
        for idx64, rec, pitch in _each(M, m, form):
            _check(_launch(csrs[(idx64, rec)], g["batch"], M, m, rng, form, pitch), exp, what=(rng, idx64, rec, pitch))
            seen.add(W.variant(M, m, form, idx64, bool(rec)))
    print(f"M = {M}, m = {m}: {form}, wide rows at pitches {[p for p in W.pitches(M * m + 1) if W.wide_rows(p, M * m + 1)]}, "
          f"instantiations = {sorted(seen)}")


@pytest.mark.parametrize("m,M", [s for s in W.SHAPES if "tags" in W.forms_of(s[1], s[0])])
def test_tags_only_at_every_shape(sp, m, M):
    """the batched registration path: key rows registered, candidates walked again with tags only -- the numbering is the oracle's"""
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    for rng in RNGS:
        exp = W.expected_rows("edge", M, m, rng, SEED)
        for idx64, rec, pitch in _each(M, m, "tags"):
            if pitch == W.pitches(M * m + 1)[-1] and len(W.pitches(M * m + 1)) == 3:
                continue                                 # (tags write no row: the default and the line pitch are the two tag units)
            rows, ukeys, nc = _tags_only(csrs[(idx64, rec)], g["batch"], M, m, rng, pitch)
            _check(rows, exp, what=("tags", rng, idx64, rec, pitch))
            assert np.array_equal(ukeys, exp["ukeys"]), (rng, idx64, rec, pitch)
    print(f"M = {M}, m = {m}: {len(exp['ukeys'])} distinct LP rows, {nc} candidate roots of {len(g['batch'])}")


# ------------------------------------------------------------------------------------------------------------- 2. work lists
@pytest.mark.parametrize("m,M", W.WORKLIST_SHAPES)
def test_work_lists(sp, m, M):
    """subgacc_walk_spg_sparse, subgacc_walk_spg_list and the list of subgacc_walk_keyrows64 on a 512-slot, a 1,024-slot and a 64-bit
    shape: *n_work = 0, 1 and n, a list in reverse order, a list of some rows, the NULL-list form with SUBGACC_NO_ROOT rows; listed
    rows equal the oracle, the others keep their poison.  work_cap < n: subgacc_walk_tags, below"""
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    q = g["batch"]
    n = len(q)
    exp = W.expected_rows("edge", M, m, "philox", SEED)
    kform = W.forms_of(M, m)[1]
    some = np.random.default_rng(M).permutation(n)[: n // 3]
    lists = [("none", np.arange(n), 0), ("one", np.array([n - 2] + list(range(n - 1))), 1), ("all", np.arange(n), n),
             ("reverse", np.arange(n)[::-1], n), ("some", some, len(some)), ("longer", np.arange(n), n + 5)]
    for idx64 in (False, True):
        csr = csrs[(idx64, True)]
        for name, wl, nw in lists:
            listed = wl[: min(nw, n)]
            for form, entry in (("table", "sparse"), ("table", "list"), (kform, "sparse")):
                got = _launch(csr, q, M, m, "philox", form, 0, work=wl, n_work=nw, entry=entry)
                _check(got, exp, listed=listed, what=(name, form, entry, idx64))
        # the NULL-list form: rows whose root is SUBGACC_NO_ROOT get nsize = 0 and nothing else
        holes = np.arange(n) % 3 == 1
        qh = np.where(holes, NO_ROOT, q).astype(np.int32)
        for form in ("table", kform):
            got = _launch(csr, qh, M, m, "philox", form, W.pitches(M * m + 1)[1], entry="sparse")
            _check(got, exp, listed=np.nonzero(~holes)[0], empty=np.nonzero(holes)[0], what=("holes", form, idx64))
        # a work list that names rows without a root
        got = _launch(csr, qh, M, m, "philox", "table", 0, work=np.arange(n), n_work=n, entry="sparse")
        _check(got, exp, listed=np.nonzero(~holes)[0], empty=np.nonzero(holes)[0], what=("holes on a list", idx64))
    print(f"M = {M}, m = {m}: {n} rows, lists {[(a, c) for a, _, c in lists]}")


@pytest.mark.parametrize("m,M", [s for s in W.WORKLIST_SHAPES if "tags" in W.forms_of(s[1], s[0])])
def test_walk_tags_with_a_short_launch(sp, m, M):
    """subgacc_walk_tags with work_cap < n: a list that fits runs in a grid of work_cap blocks and numbers like the oracle; a longer list
    raises flags[3] |= 32 and stays inside the launch"""
    from surel_plus_amd import sampler
    L = _L()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    g, csr = W.edge_graph(M, m), _graphs("edge", M, m)[(False, False)]
    q = g["batch"]
    n = len(q)
    exp = W.expected_rows("edge", M, m, "philox", SEED)
    d_q = _dev(q)
    cfg = sampler.make_cfg(csr, M, m, -1, SEED, "philox")
    for nw, cap, flag in ((40, 48, 0), (40, 40, 0), (n, 0, 0), (41, 40, 32)):
        nbytes = lib.subgacc_uniq_table_bytes(CAP)
        table = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        L.check(lib.subgacc_uniq_reset(ptr(table), CAP, st))
        wl = np.arange(n)[::-1][:nw].copy()
        w_wl, d_wl = _guarded(nw, torch.int32, wl.astype(np.int32))
        d_nw = _dev(np.array([nw], dtype=np.int64))
        w_fl, flags = _guarded(4, torch.int32, np.zeros(4, np.int32))
        L.check(lib.subgacc_walk_tags(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, 0, None, None, ptr(d_wl),
                                      ptr(d_nw), cap, ptr(table), CAP, ptr(flags), st))
        ukeys = torch.full((CAP,), -1, dtype=torch.int64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.subgacc_uniq_number_workspace_bytes(CAP, 0), dtype=torch.uint8, device="cuda")
        L.check(lib.subgacc_uniq_number(ptr(table), CAP, None, 0, ptr(ukeys), CAP, ptr(count), CAP, ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        fl = _back(w_fl, 4)
        print(f"walk_tags: *n_work = {nw}, work_cap = {cap}, flags = {fl.tolist()}, distinct rows = {int(count.item())}")
        assert fl.tolist() == [0, 0, 0, flag] and (table.cpu().numpy()[nbytes:] == 0xA5).all()
        if not flag:
            assert np.array_equal(ukeys.cpu().numpy().view(np.uint64)[: int(count.item())], W.numbering_of(exp, wl))
        else:       # the launch covered the first work_cap / 8 * 8 list entries at most: a subset of the listed rows' keys
            assert set(ukeys.cpu().numpy().view(np.uint64)[: int(count.item())].tolist()) <= set(W.numbering_of(exp, wl).tolist())


# ------------------------------------------------------------------------------------------------------- 3. roots of the batch
@pytest.mark.parametrize("m,M", W.WORKLIST_SHAPES)
def test_roots_outside_the_graph(sp, m, M):
    """include/subgacc.h: a root outside [0, num_nodes) is never looked up -- its set is empty (nsize 0, nothing else written) and
    flags[3] |= 16; the rows around it are the oracle's.  num_nodes, num_nodes + 5, 2^31 - 1, -1, -7 between the first and the last node
    id and repeated roots (the oracle never sees the bad ones: Philox sets are functions of seed and root)"""
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    q = g["batch"].copy()
    n, N = len(q), g["num_nodes"]
    exp = W.expected_rows("edge", M, m, "philox", SEED)
    bad = {3: N, 4: N + 5, 70: 2 ** 31 - 1, n - 9: -1, n - 1: -7}
    for i, v in bad.items():
        q[i] = v
    good = np.array([i for i in range(n) if i not in bad])
    assert {0, N - 1} <= set(q[good].tolist())
    for form in W.forms_of(M, m)[:2]:
        for idx64 in (False, True):
            got = _launch(csrs[(idx64, False)], q, M, m, "philox", form, 0)
            _check(got, exp, listed=good, empty=list(bad), flags=(0, 0, 0, 16), what=(form, idx64))
    got = _launch(csrs[(False, False)], q, M, m, "philox", "table", 0, work=np.arange(n)[::-1], n_work=n, entry="sparse")
    _check(got, exp, listed=good, empty=list(bad), flags=(0, 0, 0, 16), what="sparse")


@pytest.mark.parametrize("m,M", W.WORKLIST_SHAPES)
def test_symmetric_version_of_the_edge_graph(sp, m, M):
    """the same batch on the symmetrised graph (what the reference's loader makes): hubs among the reached nodes, a root without
    edges where the lone self loop was; both RNGs, table form and key rows, narrow records"""
    g, csrs = W.symmetric_edge_graph(M, m), _graphs("sym", M, m)
    for rng in RNGS:
        exp = W.expected_rows("sym", M, m, rng, SEED)
        for form in W.forms_of(M, m)[:2]:
            for idx64, rec in ((False, "narrow"), (True, True), (False, False)):
                got = _launch(csrs[(idx64, rec)], g["batch"], M, m, rng, form, W.pitches(M * m + 1)[idx64])
                _check(got, exp, what=(rng, form, idx64, rec))


# ---------------------------------------------------------------------------------------------------------------- 4. dead ends
@pytest.mark.parametrize("m,M", [(2, 204), (3, 256), (4, 128)])
def test_dead_ends(sp, m, M):
    """walks that stop after hop 1 .. m - 1, dead ends whose rows begin at nnz, the owner of the last adjacency entry as a root:
    Philox through the fused-row kernel in every form, with and without records; rand_r through the replayed stream, as
    test_rand_r_on_directed_graphs_matches_the_sequential_stream does"""
    import oracle
    g, csrs = W.dead_ends(M, m), _graphs("dead", M, m)
    exp = W.expected_rows("dead", M, m, "philox", SEED)
    for form in W.forms_of(M, m)[:2]:
        for idx64, rec, pitch in _each(M, m, form):
            _check(_launch(csrs[(idx64, rec)], g["batch"], M, m, "philox", form, pitch), exp, what=(form, idx64, rec, pitch))
    o_ns, o_remap, o_enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng="rand_r")
    oi, ox, od = oracle.spg_build(o_ns, o_remap)
    z, sets = sp.sample_spg(csrs[(False, False)], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng="rand_r", fused=True)
    assert csrs[(False, False)]._rand_r_dead_ends
    assert np.array_equal(z.indptr.cpu().numpy(), oi) and np.array_equal(z.indices[: z.nnz].cpu().numpy(), ox)
    assert np.array_equal(z.data[: z.nnz].cpu().numpy(), od) and np.array_equal(sets.enc_int16().cpu().numpy(), o_enc)
    # the kernel itself reports the dead end under rand_r (flags[0] & 1) and stays inside its arrays
    got = _launch(csrs[(True, True)], g["batch"], M, m, "rand_r", "table", 0)
    assert got["flags"].tolist() == [1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ 5. hub_cap
def test_root_degree_cap(sp):
    """roots of degree 1,000,000 and 1,000,001: with cap_root_degree the second one draws from its first 1,000,000 neighbours like the
    reference (the oracle); without it the root of 1,000,000 is unchanged and the other one's row is what the general kernel
    (subgacc_walk_sets, another implementation of the same first hop) gives"""
    from surel_plus_amd import sampler
    L = _L()
    M, m = 200, 3
    g, csrs = W.hub_cap(), _graphs("hub", M, m)
    q = g["batch"]
    n = len(q)
    for rng in RNGS:
        exp = W.expected_rows("hub", M, m, rng, SEED)
        for form in ("table", "keys32"):
            for idx64 in (False, True):
                _check(_launch(csrs[(idx64, False)], q, M, m, rng, form, 0), exp, what=(rng, form, idx64))
    exp = W.expected_rows("hub", M, m, "philox", SEED)
    csr = csrs[(False, False)]
    got = _launch(csr, q, M, m, "philox", "keys32", 0, cap_root=False)
    same = np.nonzero(q != 1)[0]
    _check(dict(got, nsize=np.where(q == 1, POISON, got["nsize"]), ids=np.where((q == 1)[:, None], POISON, got["ids"]),
                pay=np.where((q == 1)[:, None], POISON, got["pay"])), exp, listed=same, what="uncapped, the other roots")
    # the uncapped root through the general kernel: ids in first-visit order + 64-bit keys
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    Q = M * m + 1
    cfg = sampler.make_cfg(csr, M, m, -1, SEED, "philox", cap_root_degree=False, records=False)
    d_q = _dev(q)
    ids = torch.full((n * Q,), POISON, dtype=torch.int32, device="cuda")
    keys = torch.zeros(n * Q, dtype=torch.int64, device="cuda")
    nsize = torch.zeros(n, dtype=torch.int32, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    L.check(lib.subgacc_walk_sets(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, None, None, ptr(ids), ptr(keys),
                                  ptr(nsize), None, ptr(flags), st))
    torch.cuda.synchronize()
    h_ids, h_keys, h_ns = ids.cpu().numpy().reshape(n, Q), keys.cpu().numpy().reshape(n, Q), nsize.cpu().numpy()
    assert np.array_equal(h_ns, got["nsize"])
    differs = False
    for i in np.nonzero(q == 1)[0]:
        k = h_ns[i]
        order = np.argsort(h_ids[i, :k])
        assert np.array_equal(got["ids"][i, :k], h_ids[i, :k][order])
        assert np.array_equal(got["pay"][i, :k], h_keys[i, :k][order].astype(np.uint32).view(np.int32))
        assert (got["ids"][i, k:] == POISON).all()
        differs |= not np.array_equal(got["ids"][i, :k], W.row_of(exp, i)[:k]) or k != exp["nsize"][i]
    assert differs, "1,000,001 neighbours drew like 1,000,000"


# --------------------------------------------------------------------------------------------------- 6. the dispatch neighbours
@pytest.mark.parametrize("m,M", W.GENERAL)
def test_general_kernel_takes_the_neighbouring_shapes(sp, m, M):
    """Q = 203 and 202 (a 256-slot table), M = 257 and m = 5 go to walk_sets_kernel<SPG>: the same rows, slots and numbering against
    the same oracle on the edge graph (degree_ladder, self_loop and the rest), at both pitches"""
    from surel_plus_amd import sampler
    assert sampler.walk_kernel_name(None, M, m, True) == "walk_sets_kernel<SPG>" and W.variant(M, m, "table") is None
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    for rng in RNGS:
        exp = W.expected_rows("edge", M, m, rng, SEED)
        for idx64 in (False, True):
            for pitch in W.pitches(M * m + 1)[:2]:
                _check(_launch(csrs[(idx64, False)], g["batch"], M, m, rng, "table", pitch), exp, what=(rng, idx64, pitch))
    # key rows and the selecting work list are the fused-row kernel's alone: refused, nothing written
    L = _L()
    for form, entry in (("keys32", None), ("table", "sparse")):
        got = _launch(csrs[(False, False)], g["batch"], M, m, "philox", form, 0, entry=entry, check=False,
                      **({"work": np.arange(4), "n_work": 4} if entry else {}))
        assert got["rc"] == L.ERR_BADARG and (got["ids"] == POISON).all() and (got["nsize"] == POISON).all() and not got["flags"].any()


def test_a_truncating_bucket_goes_to_the_general_kernel(sp):
    """an otherwise served shape (M = 102, m = 2) with bucket = 50: walk_sets_kernel<SPG>, rows cut like the oracle's"""
    import oracle
    M, m, bucket = 102, 2, 50
    assert W.outcome(M, m, "table", bucket=bucket) == "walk_sets_kernel<SPG>"
    g, csr = W.edge_graph(M, m), _graphs("edge", M, m)[(False, False)]
    for rng in RNGS:
        o_ns, o_remap, o_enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, bucket=bucket,
                                                   seed=SEED, rng=rng)
        oi, ox, od = oracle.spg_build(o_ns, o_remap)
        z, sets = sp.sample_spg(csr, g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng, bucket=bucket, fused=True)
        assert int(o_ns.max()) == bucket
        assert np.array_equal(z.indptr.cpu().numpy(), oi) and np.array_equal(z.indices[: z.nnz].cpu().numpy(), ox)
        assert np.array_equal(z.data[: z.nnz].cpu().numpy(), od) and np.array_equal(sets.enc_int16().cpu().numpy(), o_enc)


def test_the_first_refused_shape(sp):
    """M = 205, m = 4 (Q = 821, a 2,048-slot table): SUBGACC_ERR_LDS from every fused entry point, nothing written; sample_spg falls
    back to the general pipeline and gives the oracle's store"""
    import oracle
    m, M = W.REFUSED
    L = _L()
    g, csrs = W.edge_graph(M, m), _graphs("edge", M, m)
    for form, entry in (("table", None), ("keys64", None), ("table", "sparse")):
        got = _launch(csrs[(False, False)], g["batch"], M, m, "philox", form, 0, entry=entry, check=False)
        assert got["rc"] == L.ERR_LDS and (got["ids"] == POISON).all() and (got["nsize"] == POISON).all() and not got["flags"].any()
    with pytest.raises(ValueError, match="subgacc_walk_sets"):
        L.check(got["rc"])
    for rng in RNGS:
        o_ns, o_remap, o_enc = oracle.gset_sampler(g["indptr"], g["indices"], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng)
        oi, ox, od = oracle.spg_build(o_ns, o_remap)
        z, sets = sp.sample_spg(csrs[(True, False)], g["batch"], num_walks=M, num_steps=m, seed=SEED, rng=rng, fused=True)
        assert np.array_equal(z.indptr.cpu().numpy(), oi) and np.array_equal(z.indices[: z.nnz].cpu().numpy(), ox)
        assert np.array_equal(z.data[: z.nnz].cpu().numpy(), od) and np.array_equal(sets.enc_int16().cpu().numpy(), o_enc)

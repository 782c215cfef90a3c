"""GPU (MI355X): the step's key rows as one word per member (include/subgacc_packed.h) -- the walk's packed store, the kernel that
unpacks such rows, the packed join and the step that runs on them, each against what the two planes of today give, bit for bit.
The graphs, shapes and hand-made rows are those of tests/packed_rows.py; tests/test_packed_rows_cpu.py shows on the host that every
case reaches the branch it is here for.  Every output is poisoned before the launch and stands between two poisoned guards."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import packed_rows as P
import walk_rows_edges as W
from gpu_helpers import _load, sp  # noqa: F401
from walk_rows_edges import NO_ROOT, POISON

pytestmark = pytest.mark.gpu

SEED = P.SEED
RNGS = ("rand_r", "philox")


# --------------------------------------------------------------------------------------------------------------------- plumbing
@functools.lru_cache(maxsize=2)
def _graphs(M, m):
    """{(idx64, records): DeviceCSR} of the walk graph of one shape"""
    from surel_plus_amd.sampler import DeviceCSR
    g = P.walk_graph(M, m)
    out = {}
    for idx64 in (False, True):
        ip = g["indptr"].astype(np.int64) if idx64 else g["indptr"]
        for rec in (False, True):
            csr = DeviceCSR(ip, g["indices"])
            r = csr.hop_records(force=rec)
            assert (r is None) == (not rec)
            out[(idx64, rec)] = csr
    return out


def _launch_packed(csr, q, M, m, rng, pitch=0, work=None, n_work=None, selects=0, check=True):
    """subgacc_walk_keyrows_packed into poisoned, guarded planes, then subgacc_unpack_packed_rows into two more ->
    dict(rc, words [n, P], esc [n, P], nsize, nesc, flags, ids [n, P], pay [n, P] (the unpacked planes), uflags)"""
    from surel_plus_amd import sampler
    L = P.lib_module()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n = len(q)
    Pw = pitch if pitch > 0 else M * m + 1
    d_q = P.dev(np.asarray(q, dtype=np.int32))
    cfg = sampler.make_cfg(csr, M, m, -1, SEED, rng, row_pitch=pitch)
    rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st) if not (work is not None and selects) else (None, None)
    w_wd, words = P.guarded(n * Pw, torch.int32)
    w_es, esc = P.guarded(n * Pw, torch.int32)
    w_ns, nsize = P.guarded(n, torch.int32)
    w_ne, nesc = P.guarded(n, torch.int32)
    w_fl, flags = P.guarded(4, torch.int32, np.zeros(4, np.int32))
    d_wl = P.dev(np.asarray(work, dtype=np.int32)) if work is not None else None
    d_nw = P.dev(np.array([n_work], dtype=np.int64)) if work is not None else None
    rc = lib.subgacc_walk_keyrows_packed(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, ptr(rp), ptr(rs), ptr(d_wl),
                                         ptr(d_nw), selects, ptr(words), ptr(esc), ptr(nsize), ptr(nesc), ptr(flags), st)
    torch.cuda.synchronize()
    if check:
        L.check(rc)
    out = dict(rc=rc, P=Pw, n=n, words=P.back(w_wd, n * Pw).reshape(n, Pw), esc=P.back(w_es, n * Pw).reshape(n, Pw),
               nsize=P.back(w_ns, n), nesc=P.back(w_ne, n), flags=P.back(w_fl, 4))
    if rc != 0:
        return out
    # rows the walk passed over keep their poison in nsize / nesc: the unpack kernel is given what a step's buffers hold there, zeros
    d_ns = P.dev(np.where(out["nsize"] == POISON, 0, out["nsize"]).astype(np.int32))
    d_ne = P.dev(np.where(out["nesc"] == POISON, 0, out["nesc"]).astype(np.int32))
    w_id, ids = P.guarded(n * Pw, torch.int32)
    w_ky, keys = P.guarded(n * Pw, torch.int32)
    w_uf, uflags = P.guarded(4, torch.int32, np.zeros(4, np.int32))
    L.check(lib.subgacc_unpack_packed_rows(ptr(words), ptr(esc), ptr(d_ns), ptr(d_ne), n, Pw, csr.num_nodes, M, m, ptr(ids), ptr(keys),
                                           ptr(uflags), st))
    torch.cuda.synchronize()
    out.update(ids=P.back(w_id, n * Pw).reshape(n, Pw), pay=P.back(w_ky, n * Pw).reshape(n, Pw), uflags=P.back(w_uf, 4))
    return out


def _same_rows(got, ref, M, m, num_nodes, what):
    """the packed launch against the launch of subgacc_walk_spg(uniq_table = NULL) / _sparse / _list with the same arguments: flags and
    nsize (poison where the walk passed a row over) equal; the unpacked planes equal the reference's word for word, poison behind
    every row included; the words and the escape lists are the reference's rows packed by the restatement, with poison behind a
    row's last word and behind its last escape; nesc is the length of the list (poison where nsize is)"""
    cb, fb = P.fmt(num_nodes, m)
    assert got["flags"].tolist() == ref["flags"].tolist(), (what, got["flags"].tolist(), ref["flags"].tolist())
    assert not got["uflags"].any(), (what, got["uflags"].tolist())
    assert np.array_equal(got["nsize"], ref["nsize"]), (what, "nsize")
    assert np.array_equal(got["ids"], ref["ids"]), (what, "ids", np.nonzero((got["ids"] != ref["ids"]).any(axis=1))[0][:8])
    assert np.array_equal(got["pay"], ref["pay"]), (what, "keys", np.nonzero((got["pay"] != ref["pay"]).any(axis=1))[0][:8])
    n, Pw = got["n"], got["P"]
    want_w = np.full((n, Pw), POISON, np.int32)
    want_e = np.full((n, Pw), POISON, np.int32)
    want_ne = np.full(n, POISON, np.int32)
    for i in range(n):
        ns = ref["nsize"][i]
        if ns == POISON:
            continue
        words, lst = P.pack_row(ref["ids"][i, :ns], ref["pay"][i, :ns].view(np.uint32), M, m, cb, fb)
        want_w[i, :ns], want_e[i, :len(lst)], want_ne[i] = words.view(np.int32), lst.view(np.int32), len(lst)
    assert np.array_equal(got["nesc"], want_ne), (what, "nesc", np.nonzero(got["nesc"] != want_ne)[0][:8])
    assert np.array_equal(got["words"], want_w), (what, "words", np.nonzero((got["words"] != want_w).any(axis=1))[0][:8])
    assert np.array_equal(got["esc"], want_e), (what, "escape lists", np.nonzero((got["esc"] != want_e).any(axis=1))[0][:8])
    return want_ne


# ------------------------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("m,M", P.SHAPES)
def test_packed_rows_unpack_to_the_key_rows(sp, m, M):
    """every instantiation of the packed store on the walk graph of its shape: int32 and int64 row offsets, with and without hop
    records, the default pitch (one member per lane and store) and a pitch of whole lines (four), both RNGs"""
    g, csrs = P.walk_graph(M, m), _graphs(M, m)
    Q, N = M * m + 1, g["num_nodes"]
    seen = set()
    for rng in RNGS:
        for idx64 in (False, True):
            if not P.eligible(N, M, m, idx64):
                continue
            for rec, pitch in ((False, 0), (True, W.pitches(Q)[1]), (False, W.pitches(Q)[1])):
                csr = csrs[(idx64, rec)]
                ref = P.launch_keys32(csr, g["batch"], M, m, rng, pitch)
                got = _launch_packed(csr, g["batch"], M, m, rng, pitch)
                ne = _same_rows(got, ref, M, m, N, (rng, idx64, rec, pitch))
                seen.add((idx64, rec) + W.variant(M, m, "keys32", idx64, rec)[:3])
    print(f"M = {M}, m = {m}: {len(g['batch'])} rows, escapes per row up to {int(ne.max())}, {int((ne == 0).sum())} rows without, "
          f"instantiations (idx64, records, MH, SPL, NT) = {sorted(seen)}")


def test_the_one_wave_shape_is_refused(sp):
    """2 hops, 512 slots, int32 offsets: one wave per root, no packed store -- SUBGACC_ERR_BADARG, nothing written; so are 64-bit keys
    and a graph whose ids leave fewer than three bits a count"""
    L = P.lib_module()
    for (m, M), (gm, gM) in (((2, 204), (2, 204)), ((4, 128), (4, 127))):        # (the shape, the shape whose graph it runs on)
        csr = _graphs(gM, gm)[(False, False)]
        q = P.walk_graph(gM, gm)["batch"][:16]
        got = _launch_packed(csr, q, M, m, "philox", check=False)
        assert got["rc"] == L.ERR_BADARG, (m, M)
        assert (got["words"] == POISON).all() and (got["esc"] == POISON).all() and (got["nsize"] == POISON).all()
        assert (got["nesc"] == POISON).all() and not got["flags"].any()
    from surel_plus_amd.sampler import DeviceCSR
    N = (1 << 22) + 1                               # 23-bit ids: fb = 2 at three hops
    csr = DeviceCSR(np.minimum(np.arange(N + 1), 1).astype(np.int32), np.zeros(1, np.int32))        # one edge, 0 -> 0
    got = _launch_packed(csr, np.zeros(8, np.int32), 200, 3, "philox", check=False)
    assert got["rc"] == L.ERR_BADARG and (got["words"] == POISON).all() and (got["nsize"] == POISON).all()


@pytest.mark.parametrize("m,M", [(3, 200), (4, 102)])
def test_packed_rows_with_work_lists_and_bad_roots(sp, m, M):
    """the selecting list (subgacc_walk_spg_sparse's) and the ordering one (subgacc_walk_spg_list's) with *n_work = 0, 1 and n, a list
    in reverse, rows without a root on a list and without one, roots outside the graph: the listed rows equal the two-plane
    launch, the others keep their poison (nesc as nsize: 0 for a row without a root or with a root outside the graph)"""
    g, csrs = P.walk_graph(M, m), _graphs(M, m)
    q, N = g["batch"], g["num_nodes"]
    n = len(q)
    pitch = W.pitches(M * m + 1)[1]
    csr = csrs[(False, True)]
    lists = [("none", np.arange(n), 0), ("one", np.array([n - 2] + list(range(n - 1))), 1), ("all", np.arange(n), n),
             ("reverse", np.arange(n)[::-1], n)]
    for name, wl, nw in lists:
        for selects, entry in ((1, "sparse"), (0, "list")):
            if entry == "list" and nw != n:
                continue                            # (an order names every row)
            ref = P.launch_keys32(csr, q, M, m, "philox", pitch, work=wl, n_work=nw, entry=entry)
            got = _launch_packed(csr, q, M, m, "philox", pitch, work=wl, n_work=nw, selects=selects)
            _same_rows(got, ref, M, m, N, (name, entry))
    ref = P.launch_keys32(csr, q, M, m, "rand_r", 0, work=np.arange(n)[::-1], n_work=n, entry="list")
    _same_rows(_launch_packed(csr, q, M, m, "rand_r", 0, work=np.arange(n)[::-1], n_work=n, selects=0), ref, M, m, N, "rand_r list")
    holes = np.arange(n) % 3 == 1
    qh = np.where(holes, NO_ROOT, q).astype(np.int32)
    for work in (None, np.arange(n)):
        kw = dict(work=work, n_work=n) if work is not None else {}
        ref = P.launch_keys32(csr, qh, M, m, "philox", pitch, entry="sparse", **kw)
        got = _launch_packed(csr, qh, M, m, "philox", pitch, selects=1, **kw)
        ne = _same_rows(got, ref, M, m, N, ("holes", work is not None))
        assert (got["nsize"][holes] == 0).all() and (ne[holes] == 0).all()
    bad = {3: N, 4: N + 5, 70: 2 ** 31 - 1, n - 9: -1, n - 1: -7}
    qb = q.copy()
    for i, v in bad.items():
        qb[i] = v
    for idx64 in (False, True):
        ref = P.launch_keys32(csrs[(idx64, False)], qb, M, m, "philox", 0)
        got = _launch_packed(csrs[(idx64, False)], qb, M, m, "philox", 0)
        ne = _same_rows(got, ref, M, m, N, ("bad roots", idx64))
        assert got["flags"].tolist() == [0, 0, 0, 16] and all(got["nsize"][i] == 0 and ne[i] == 0 for i in bad)


# ------------------------------------------------------------------------------------------------------------------------- join
def _join(M, m, N, pitch, rows, pairs, nesc_edit=None, key_edit=None):
    """subgacc_sjoin_fill_packed over the packed `rows` against subgacc_sjoin_fill_v2 over their two planes, the same mirrored list of
    `pairs` [2, B] -> (packed xz, two-plane xz, packed flags, two-plane flags), the outputs between poisoned guards.  nesc_edit
    {row: value} corrupts the packed rows' nesc; key_edit {row: members} zeroes those members' keys in the two planes"""
    L = P.lib_module()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    cb, fb = rows["cb"], rows["fb"]
    n = len(rows["ids"])
    ids = np.full((n, pitch), POISON, np.int32)
    keys = np.full((n, pitch), POISON, np.int32)
    words = np.full((n, pitch), POISON, np.int32)
    esc = np.full((n, pitch), POISON, np.int32)
    nsize, nesc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, (ri, rk) in enumerate(zip(rows["ids"], rows["keys"])):
        ns = len(ri)
        w, lst = P.pack_row(ri, rk, M, m, cb, fb)
        k2 = rk.copy()
        if key_edit and i in key_edit:
            k2[key_edit[i]] = 0
        ids[i, :ns], keys[i, :ns], words[i, :ns], esc[i, :len(lst)] = ri.astype(np.int32), k2.view(np.int32), w.view(np.int32), lst.view(np.int32)
        nsize[i], nesc[i] = ns, len(lst)
    for i, v in (nesc_edit or {}).items():
        nesc[i] = v
    B = pairs.shape[1]
    own = P.dev(np.concatenate([pairs[0], pairs[1]]).astype(np.int64))
    partner = P.dev(np.concatenate([pairs[1], pairs[0]]).astype(np.int64))
    S = 2 * B
    d_ns = P.dev(nsize)
    seg = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(lib.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device="cuda")
    f0 = torch.zeros(4, dtype=torch.int32, device="cuda")
    L.check(lib.subgacc_sjoin_sizes_rows(ptr(d_ns), n, ptr(own), ptr(partner), S, ptr(seg), ptr(f0), ptr(ws), ws.numel(), st))
    R = int(seg[-1].item())
    k = m + 1
    outs, flags = [], []
    for packed in (True, False):
        w_xz, xz = P.guarded(max(R, 1) * 2 * k, torch.int32)
        w_fl, fl = P.guarded(4, torch.int32, np.zeros(4, np.int32))
        planes = (P.dev(words.reshape(-1)), P.dev(esc.reshape(-1))) if packed else (P.dev(ids.reshape(-1)), P.dev(keys.reshape(-1)))
        d = L.join_desc(L.JOIN_ROWS, L.JOIN_KEY32, row_len=d_ns, n_rows=n, row_stride=pitch, ids=planes[0], payload=planes[1], own=own,
                        partner=partner, S=S, seg=seg, pair_block=B, flags=fl, num_walks=M, num_steps=m, out_xz=xz)
        if packed:
            d_ne = P.dev(nesc)
            L.check(lib.subgacc_sjoin_fill_packed(ctypes.byref(d), ptr(d_ne), N, st))
        else:
            L.check(lib.subgacc_sjoin_fill_v2(ctypes.byref(d), st))
        torch.cuda.synchronize()
        outs.append(P.back(w_xz, max(R, 1) * 2 * k)[: R * 2 * k].copy())
        flags.append(P.back(w_fl, 4).tolist())
    return outs[0], outs[1], flags[0], flags[1], R


@pytest.mark.parametrize("m,M,N,pitch", P.JOIN_SHAPES)
def test_packed_join_equals_the_join_of_the_unpacked_rows(sp, m, M, N, pitch):
    """every ordered pair of the hand-made rows -- (u, u), an empty row on either side, S longer than T and T longer than S, nt at
    63 | 64 | 65 and 255 | 256 | 257, hits whose S member, T member, both or neither escape, a row without escapes, one of escapes
    only, one with more escapes than the join stages -- as two workgroups per pair (a batch of up to 1,024 pairs) and as one"""
    rows = P.join_rows(M, m, N, pitch)
    n = len(rows["ids"])
    for count in (n * n, 1100):
        got, want, fl, fl0, R = _join(M, m, N, pitch, rows, P.join_pairs(n, count))
        assert fl == [0, 0, 0, 0] and fl0 == [0, 0, 0, 0], (count, fl, fl0)
        assert R > 0 and np.array_equal(got, want), (count, np.nonzero(got != want)[0][:8])
    print(f"M = {M}, m = {m}, {N} nodes (cb = {rows['cb']}, fb = {rows['fb']}), pitch {pitch}: {n} rows, {R} rows of xz")


def test_packed_join_flags_a_corrupted_escape_count(sp):
    """nesc above the list: the row's keys are all there (the ranks stay inside the real list), xz is the two planes', and
    flags[3] & 2 says that the length is not the row's number of escapes.  nesc below the list (and: negative, beyond the pitch):
    the escapes at and beyond it are never dereferenced -- they read as key 0, flags[3] & 2 -- and xz is that of the two planes
    with exactly those keys zeroed."""
    m, M, N, pitch = P.JOIN_SHAPES[0]
    rows = P.join_rows(M, m, N, pitch)
    n = len(rows["ids"])
    at = {name: i for i, name in enumerate(rows["names"])}
    pairs = P.join_pairs(n, n * n)
    esc = [np.nonzero(P.codes(k, M, m, rows["cb"], rows["fb"])[1])[0] for k in rows["keys"]]
    i_all, i_many = at["all"], at["many"]
    got, want, fl, fl0, _ = _join(M, m, N, pitch, rows, pairs, nesc_edit={i_all: len(esc[i_all]) + 3})
    assert fl == [0, 0, 0, 2] and fl0 == [0, 0, 0, 0] and np.array_equal(got, want)
    for cut in (10, 0, -5):
        got, want, fl, fl0, _ = _join(M, m, N, pitch, rows, pairs, nesc_edit={i_many: cut}, key_edit={i_many: esc[i_many][max(cut, 0):]})
        assert fl == [0, 0, 0, 2] and fl0 == [0, 0, 0, 0] and np.array_equal(got, want), cut
    got, want, fl, fl0, _ = _join(M, m, N, pitch, rows, pairs, nesc_edit={i_many: pitch + 7})
    assert fl == [0, 0, 0, 2] and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------- step
def _golden_graph():
    g = _load("gset_collablike_s1.npz")
    return g["indptr"].astype(np.int32), g["indices"].astype(np.int32)


def _zsf(enc, M):
    """Z_SF as main.py:174 makes it: the zero row, then counts / num_walks (a store's payload is SFptr + 1)"""
    return np.concatenate([np.zeros((1, enc.shape[1]), np.float32), enc.astype(np.float32) / np.float32(M)])


@functools.lru_cache(maxsize=None)
def _oracle_store(M, m, seed, rng):
    import oracle
    ptr_, idx = _golden_graph()
    N = len(ptr_) - 1
    nsize, remap, enc = oracle.gset_sampler(ptr_, idx, np.arange(N), num_walks=M, num_steps=m, seed=seed, rng=rng, nthreads=8 if rng == "philox" else 1)
    return oracle.spg_build(nsize, remap), _zsf(enc, M)


@pytest.mark.parametrize("dedup,order", [(False, False), (True, False), (False, True), (True, True)])
def test_packed_step_equals_the_unpacked_step_and_the_oracle(sp, dedup, order):
    """sample_and_gather(buffers=) on a golden graph, M = 200 and 3 hops: the library's choice is the packed path; (xz, indptr) equal
    those of packed_rows=False and the oracle's gather over the oracle's store, with root dedup and with order=; the step's sets show
    today's rows -- sets.ids / sets.slot, StridedSpG(sets).to_csr() -- and the step itself allocated no unpacked plane"""
    import oracle
    from surel_plus_amd.spg import StridedSpG
    M, m, B, seed = 200, 3, 192, 21
    ptr_, idx = _golden_graph()
    N = len(ptr_) - 1
    csr = sp.DeviceCSR(ptr_, idx)
    assert sp.sampler.packed_rows_form(N, M, m) == P.fmt(N, m)
    rs = np.random.default_rng(3)
    e = rs.integers(0, N, (2, B))
    e[1, :8] = e[0, :8]                      # (u, u)
    e[:, 8:40] = e[:, 40:72]                 # repeated endpoints
    edge = torch.from_numpy(e).cuda()
    lo = sp.sampler.locality_order(csr) if order else None
    kw = dict(num_walks=M, num_steps=m, dedup_roots=dedup, order=lo)
    bp = sp.StepBuffers(csr, B, **kw)
    bu = sp.StepBuffers(csr, B, packed_rows=False, **kw)
    assert bp.packed and not bu.packed and sp.StepBuffers(csr, B, packed_rows=True, **kw).packed
    call = dict(num_walks=M, num_steps=m, seed=seed, rng="philox", dedup_roots=dedup)
    xz_p, ind_p, sets_p = sp.sample_and_gather(csr, edge, buffers=bp, **call)
    xz_u, ind_u, sets_u = sp.sample_and_gather(csr, edge, buffers=bu, **call)
    sets_p.resolve(), sets_u.resolve()
    R = int(ind_u[-1].item())
    assert torch.equal(ind_p, ind_u) and torch.equal(xz_p[:R], xz_u[:R])
    assert bp._unpacked is None, "the step unpacked its rows"
    spg, table = _oracle_store(M, m, seed, "philox")
    oxz, oind = oracle.gather(e, spg, ptr=True, encode=table)
    assert np.array_equal(ind_p.cpu().numpy(), oind) and np.array_equal(xz_p[:R].cpu().numpy(), oxz)
    # what looks at the rows sees today's rows
    ns = bu.nsize.cpu().numpy()
    assert np.array_equal(bp.nsize.cpu().numpy(), ns)
    live = (np.arange(bu.stride)[None, :] < ns[:, None]).reshape(-1)
    for a, b in ((sets_p.ids, sets_u.ids), (sets_p.slot, sets_u.slot), (bp.ids, bu.ids), (bp.slot, bu.slot)):
        assert np.array_equal(a.cpu().numpy()[live], b.cpu().numpy()[live])
    assert bp._unpacked is not None and not bp._unpack_flags.any()
    zp, zu = StridedSpG(sets_p, N).to_csr(), StridedSpG(sets_u, N).to_csr()
    for name in ("indptr", "indices", "data"):
        assert torch.equal(getattr(zp, name), getattr(zu, name)), name
    assert sets_p.X == sets_u.X and sets_p.c == sets_u.c
    print(f"dedup = {dedup}, order = {order}: {R} rows of xz, walk order {sets_p.walk_order!r}, {int(bp.nesc.cpu().numpy()[ns > 0].sum())} escapes in "
          f"{int(ns.sum())} members")


def test_packed_step_in_rand_r_mode_and_captured(sp):
    """rand_r: the packed step equals the unpacked one and the oracle's sequential stream.  CapturedStep: the captured graph holds the
    packed step; replays with new batches equal the oracle, and the sets of a replay show that replay's rows"""
    import oracle
    M, m, B, seed = 200, 3, 96, 21
    ptr_, idx = _golden_graph()
    N = len(ptr_) - 1
    csr = sp.DeviceCSR(ptr_, idx)
    e = np.random.default_rng(4).integers(0, N, (2, B))
    edge = torch.from_numpy(e).cuda()
    bp = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, rng="rand_r")
    bu = sp.StepBuffers(csr, B, num_walks=M, num_steps=m, rng="rand_r", packed_rows=False)
    assert bp.packed
    xz_p, ind_p, s_p = sp.sample_and_gather(csr, edge, num_walks=M, num_steps=m, seed=seed, rng="rand_r", buffers=bp)
    xz_u, ind_u, s_u = sp.sample_and_gather(csr, edge, num_walks=M, num_steps=m, seed=seed, rng="rand_r", buffers=bu)
    s_p.resolve(), s_u.resolve()
    R = int(ind_u[-1].item())
    assert torch.equal(ind_p, ind_u) and torch.equal(xz_p[:R], xz_u[:R])
    nsize, remap, enc = oracle.gset_sampler(ptr_, idx, e.reshape(-1), num_walks=M, num_steps=m, seed=seed, rng="rand_r")
    oxz, oind = oracle.gather(np.stack([np.arange(B), np.arange(B, 2 * B)]), oracle.spg_build(nsize, remap), ptr=True,
                              encode=_zsf(enc, M))
    assert np.array_equal(ind_p.cpu().numpy(), oind) and np.array_equal(xz_p[:R].cpu().numpy(), oxz)
    cap = sp.CapturedStep(csr, B, num_walks=M, num_steps=m, seed=seed, rng="philox")
    assert cap._kw["buffers"].packed
    spg, table = _oracle_store(M, m, seed, "philox")
    for rep in range(2):
        e2 = np.random.default_rng(50 + rep).integers(0, N, (2, B))
        xz, ind = cap(torch.from_numpy(e2).cuda()).finish()
        oxz, oind = oracle.gather(e2, spg, ptr=True, encode=table)
        assert np.array_equal(ind.cpu().numpy(), oind) and np.array_equal(xz.cpu().numpy(), oxz), rep
        ids = cap.sets.ids.cpu().numpy().reshape(2 * B, -1)
        for j in (0, B, 2 * B - 1):
            r = e2.reshape(-1)[j]
            assert np.array_equal(ids[j, : spg[0][r + 1] - spg[0][r]], spg[1][spg[0][r]: spg[0][r + 1]]), (rep, j)


def test_packed_rows_keyword_refuses_what_has_no_packed_form(sp):
    """packed_rows=True raises ValueError for a shape or a form that is not eligible; None quietly keeps the two planes there"""
    ptr_, idx = _golden_graph()
    csr = sp.DeviceCSR(ptr_, idx)
    for kw in (dict(num_steps=2), dict(num_walks=200, num_steps=4), dict(ptr=False), dict(batch=16), dict(stage="counts"), dict(key_rows=False),
               dict(dtype=torch.bfloat16), dict(triplets=True)):
        kw = {"num_walks": 200, "num_steps": 3, **kw}
        with pytest.raises(ValueError, match="packed_rows=True"):
            sp.StepBuffers(csr, 64, packed_rows=True, **kw)
        assert not sp.StepBuffers(csr, 64, **kw).packed

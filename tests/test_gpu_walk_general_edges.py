"""GPU (MI355X): the three kernels that serve every walk walk_rows_kernel declines -- walk_sets_kernel, walk_sets_kernel<SPG>
(csrc/walk.hip) and the persistent walk_pipe_kernel (csrc/walk_pipe.hip) -- and subgacc_compact_sets, driven through the C ABI at
their table, bucket, LDS, walk-loop and pipeline edges with the graphs and shapes of tests/walk_general_edges.py;
tests/test_walk_general_edges_cpu.py shows on the host that every case reaches the branch it is here for.

The references are the oracle's: gset_sampler (sets in first-visit order, LP rows, numbering) and walk_sampler (raw walks, step-major
sets); where walks are emitted a plain-Python recount of the set from them stands beside.  Everything is integer and compared bit
for bit.  Every output is poisoned before the launch and stands between two poisoned guards: the guards and the words
[nsize[i], pitch) of every row must come back untouched."""
import numpy as np
import pytest
import torch

import walk_general_edges as G
import walk_rows_edges as W
from gpu_helpers import sp  # noqa: F401
from test_gpu_walk_rows_edges import CAP, _L, _back, _check, _dev, _guarded
from walk_general_edges import NO_ROOT, POISON, RNGS

pytestmark = pytest.mark.gpu

SEED = 13
POISON64 = np.int64(POISON).astype(np.int64).view(np.uint64)


# --------------------------------------------------------------------------------------------------------------------- plumbing
def _csr(g, idx64=False):
    from surel_plus_amd.sampler import DeviceCSR
    return DeviceCSR(g["indptr"].astype(np.int64) if idx64 else g["indptr"], g["indices"])


def _cfg(csr, M, m, rng, bucket=-1, pitch=0, order="walk", wo=True, emit=False):
    from surel_plus_amd import _lib, sampler
    return sampler.make_cfg(csr, M, m, bucket, SEED, rng, first_hop_wo=wo,
                            order=_lib.ORDER_WALK_MAJOR if order == "walk" else _lib.ORDER_STEP_MAJOR, emit_walks=emit, records=False,
                            row_pitch=pitch)


def _sets(csr, q, M, m, rng, bucket=-1, pitch=0, order="walk", wo=True, emit=False, replay=False):
    """subgacc_walk_sets into poisoned, guarded outputs -> dict(ids [n, P], keys [n, P] uint64, nsize, flags, walks [n, M, m + 1]).
    replay: the stream positions of every walk from subgacc_rng_replay (cfg.walk_pos), else subgacc_rng_positions under rand_r"""
    from surel_plus_amd import sampler
    L = _L()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n = len(q)
    stride = bucket if bucket > 0 else M * m + 1
    P = pitch if pitch > 0 else stride
    d_q = _dev(np.asarray(q, dtype=np.int32))
    cfg = _cfg(csr, M, m, rng, bucket, pitch, order, wo, emit)
    if replay:
        rp, rs = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        w_wp, wp = _guarded(n * M, torch.int32)
        L.check(lib.subgacc_rng_replay(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, 1, 0, ptr(rp), ptr(rs), ptr(wp), st))
        cfg.walk_pos = wp.data_ptr()
    else:
        rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st)
    w_ids, ids = _guarded(n * P, torch.int32)
    w_keys, keys = _guarded(n * P, torch.int64)
    w_ns, nsize = _guarded(n, torch.int32)
    w_fl, flags = _guarded(4, torch.int32, np.zeros(4, np.int32))
    w_wk, walks = _guarded(n * M * (m + 1), torch.int32) if emit else (None, None)
    L.check(lib.subgacc_walk_sets(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, ptr(rp), ptr(rs), ptr(ids), ptr(keys),
                                  ptr(nsize), ptr(walks), ptr(flags), st))
    torch.cuda.synchronize()
    if replay:
        _back(w_wp, n * M)
    return dict(n=n, P=P, ids=_back(w_ids, n * P).reshape(n, P), keys=_back(w_keys, n * P).view(np.uint64).reshape(n, P),
                nsize=_back(w_ns, n), flags=_back(w_fl, 4), walks=_back(w_wk, n * M * (m + 1)).reshape(n, M, m + 1) if emit else None)


def _want(n, P, nsize, ids, keys):
    """the rows as the outputs must hold them: members in front, poison behind"""
    nsize = np.asarray(nsize).astype(np.int64)
    assert nsize.max(initial=0) <= P and nsize.sum() == len(ids) == len(keys)
    r = np.repeat(np.arange(n), nsize)
    c = np.arange(nsize.sum()) - np.repeat(np.cumsum(nsize) - nsize, nsize)
    w_ids = np.full((n, P), POISON, dtype=np.int32)
    w_keys = np.full((n, P), POISON64, dtype=np.uint64)
    w_ids[r, c], w_keys[r, c] = ids, keys
    return w_ids, w_keys


def _flags(q, N, dead=0, cut=0):
    q = np.asarray(q).astype(np.int64)
    return [dead, cut, 0, 16 if (~G.in_graph(q, N) & (q != NO_ROOT)).any() else 0]


def _same_sets(got, nsize, ids, keys, flags, what):
    n, P = got["n"], got["P"]
    assert got["flags"].tolist() == list(flags), (what, got["flags"].tolist(), flags)
    assert np.array_equal(got["nsize"], nsize), (what, "nsize", np.nonzero(got["nsize"] != nsize)[0][:8])
    w_ids, w_keys = _want(n, P, nsize, ids, keys)
    assert np.array_equal(got["ids"], w_ids), (what, "ids", np.nonzero((got["ids"] != w_ids).any(axis=1))[0][:8])
    assert np.array_equal(got["keys"], w_keys), (what, "keys", np.nonzero((got["keys"] != w_keys).any(axis=1))[0][:8])


def _same_as_reference(got, ref, q, N, what, dead=0, cut=None):
    cut = int(ref.get("cut", 0)) if cut is None else cut
    _same_sets(got, ref["nsize"], ref["ids"], ref["keys"], _flags(q, N, dead, cut), what)


def _bitwise(a, b, what):
    """two launches of the same query wrote the same words: rows, poison, sizes and flags"""
    for k in ("ids", "keys", "nsize", "flags"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _reference(g, q, M, m, rng, bucket=-1):
    ref = G.reference(g, q, M, m, rng, SEED, bucket)
    if bucket > 0:
        ref["cut"] = int((G.reference(g, q, M, m, rng, SEED)["nsize"] > bucket).sum())
    return ref


def _check_walks(got, g, q, M, m, rng, order, bucket=-1, wo=True, rows=None):
    """the emitted walks are the oracle's; the rows of roots outside the graph keep their poison; the set recounted in plain Python
    from the GPU's own walks (first-visit order under `order`, landing counts per step) is what the kernel wrote next to them"""
    wr = G.walk_reference(g, q, M, m, rng, SEED, first_hop_wo=wo)
    good = wr["good"]
    assert np.array_equal(got["walks"][good], wr["walks"]), "walks"
    assert (got["walks"][~good] == POISON).all()
    rows = np.nonzero(good)[0] if rows is None else np.asarray([r for r in rows if good[r]])
    ns, ids, keys, _ = G.recount(got["walks"][rows], M, m, order, bucket)
    at = 0
    for r, k in zip(rows, ns):
        assert got["nsize"][r] == k and np.array_equal(got["ids"][r, :k], ids[at: at + k]) and np.array_equal(got["keys"][r, :k], keys[at: at + k]), r
        at += k


def _general_vs_oracle(g, q, M, m, emit, recount_rows=None, widths=(False, True)):
    """walk_sets_kernel on one query: both RNGs, both offset widths under Philox -- sets against oracle.gset_sampler, walks against
    oracle.walk_sampler and the recount"""
    assert G.kernel_for(M, m, emit_walks=emit) == "walk_sets_kernel"
    N = g["num_nodes"]
    for rng in RNGS:
        ref = _reference(g, q, M, m, rng)
        for idx64 in (widths if rng == "philox" else widths[:1]):
            got = _sets(_csr(g, idx64), q, M, m, rng, emit=emit)
            _same_as_reference(got, ref, q, N, (M, m, rng, idx64))
            if emit:
                _check_walks(got, g, q, M, m, rng, "walk", rows=recount_rows)
    return ref


# ----------------------------------------------------------------------------------------------- A. walk_sets_kernel, sets form
@pytest.mark.parametrize("pair", G.TABLE_PAIRS, ids=lambda p: f"Q{p[0][0] * p[0][1] + 1}")
def test_sets_on_both_sides_of_a_table_doubling(sp, pair):
    """Q = 51|52 .. 819|820: a set of exactly Q members in a table at its highest load (linear probing wraps at the last slot), one
    and two members, the ladder of root degrees -- raw walks emitted, so every shape runs walk_sets_kernel"""
    for M, m in pair:
        g = G.edge_graph(M, m)
        special = np.concatenate([g["rows"][k] for k in ("full", "shuffled", "self_loop", "isolated", "small", "run")])
        ref = _general_vs_oracle(g, g["batch"], M, m, True, recount_rows=special)
        print(f"M = {M}, m = {m}: T = {G.table_size_for(M * m + 1)}, rows = {len(g['batch'])}, largest set = {int(ref['nsize'].max())}")
        assert ref["nsize"].max() == M * m + 1


@pytest.mark.parametrize("pair", G.BITMAP_PAIRS, ids=lambda p: f"Q{p[0][0] * p[0][1] + 1}")
def test_sets_at_the_rank_bitmap_words(sp, pair):
    """Q = 32|33 and 64|65: first-visit numbers 31, 32, 33 on both sides of a bitmap word"""
    for M, m in pair:
        g = G.edge_graph(M, m)
        _general_vs_oracle(g, g["batch"], M, m, True)


@pytest.mark.parametrize("M,m", G.TRIP_SHAPES)
def test_sets_walk_loop_trips(sp, M, m):
    """M = 255|256|257 and 511|512|513: one, two and three walks per lane; roots of degree M - 1, M, M + 1 and 2M (the `w % rdeg`
    pick, the first shuffled degree, the Fisher-Yates chain across a lane's second and third walk)"""
    g = G.edge_graph(M, m)
    lad = g["rows"]["ladder"]
    picked = [lad[d] for d in (0, 1, M - 1, M, M + 1, M + 2)] + [lad[-2], lad[-1]] + g["rows"]["full"].tolist() + g["rows"]["shuffled"].tolist()
    _general_vs_oracle(g, g["batch"], M, m, True, recount_rows=picked, widths=(False,))
    if M > 256:                                         # ... and without raw walks: the launch the sampler makes at M > 256
        _general_vs_oracle(g, g["batch"], M, m, False, widths=(True,))


@pytest.mark.parametrize("M,m", G.LDS_SHAPES)
def test_sets_on_both_sides_of_the_dynamic_lds_switch(sp, M, m):
    """T = 2,048 (below 64 KiB), T = 4,096 (the hipFuncSetAttribute path) and T = 8,192 (140 KiB): a few dozen roots"""
    g = G.edge_graph(M, m, ladder=False)
    ref = _general_vs_oracle(g, g["batch"], M, m, False)
    print(f"M = {M}, m = {m}: {G.lds_of(M, m)} B of LDS, attribute = {G.needs_attribute(M, m)}, largest set = {int(ref['nsize'].max())}")
    assert ref["nsize"].max() == M * m + 1


def test_sets_buckets_around_a_set_and_around_q(sp):
    """bucket in {1, 2, ns - 1, ns, ns + 1, Q - 1, Q, Q + 1} for a tree of ns = Q - 5 members: nsize = min(ns, bucket), the first
    `bucket` members in first-visit order with the oracle's counts, flags[1] = the roots cut, rows at i * bucket -- the general
    kernel (raw walks) and the pipe"""
    M, m = G.BUCKET_SHAPE
    Q = M * m + 1
    g = G.edge_graph(M, m)
    q, N = g["batch"], g["num_nodes"]
    row = g["rows"]["short5"][0]
    for rng in RNGS:
        full = _reference(g, q, M, m, rng)
        ns = int(full["nsize"][row])
        for bucket in G.buckets_for(Q, ns):
            ref = _reference(g, q, M, m, rng, bucket)
            assert ref["cut"] == (full["nsize"] > bucket).sum() and ref["nsize"][row] == min(ns, bucket)
            gen = _sets(_csr(g), q, M, m, rng, bucket=bucket, emit=True)
            _same_as_reference(gen, ref, q, N, ("general", rng, bucket))
            _check_walks(gen, g, q, M, m, rng, "walk", bucket)
            pipe = _sets(_csr(g, True), q, M, m, rng, bucket=bucket)
            _same_as_reference(pipe, ref, q, N, ("pipe", rng, bucket))
            _bitwise(pipe, gen, (rng, bucket))


def test_sets_orders_and_plain_first_hops(sp):
    """walk-major against oracle.gset_sampler, step-major with raw walks against oracle.walk_sampler, on a graph where the two
    orders differ; the plain first hop (first_hop_wo = 0) in both orders and both RNGs against walk_sampler and the recount of its
    walks"""
    M, m = G.ORDER_SHAPE
    g = G.dense_graph(40, 4, 1)
    q, N = g["batch"], g["num_nodes"]
    for rng in RNGS:
        for idx64 in (False, True):
            csr = _csr(g, idx64)
            ref = _reference(g, q, M, m, rng)
            got = _sets(csr, q, M, m, rng, emit=True)
            _same_as_reference(got, ref, q, N, ("walk-major", rng))
            _check_walks(got, g, q, M, m, rng, "walk")
            for wo in (True, False):
                wr = G.walk_reference(g, q, M, m, rng, SEED, first_hop_wo=wo)
                got = _sets(csr, q, M, m, rng, order="step", wo=wo, emit=True)
                _same_sets(got, wr["nsize"], wr["ids"], wr["keys"], [0, 0, 0, 0], ("step-major", rng, wo))
                _check_walks(got, g, q, M, m, rng, "step", wo=wo)
            wr = G.walk_reference(g, q, M, m, rng, SEED, first_hop_wo=False)
            ns, ids, keys, _ = G.recount(wr["walks"], M, m, "walk")
            got = _sets(csr, q, M, m, rng, wo=False)                     # no raw walks: the plain first hop alone leaves the pipe
            _same_sets(got, ns, ids, keys, [0, 0, 0, 0], ("walk-major, plain first hop", rng))
            for bucket in (3, 7):
                ns, ids, keys, tot = G.recount(wr["walks"], M, m, "step", bucket)
                got = _sets(csr, q, M, m, rng, bucket=bucket, order="step", wo=False, emit=True)
                _same_sets(got, ns, ids, keys, [0, int((tot > bucket).sum()), 0, 0], ("step-major bucket", rng, bucket))


@pytest.mark.parametrize("M,m", G.DEAD_SHAPES)
def test_sets_rand_r_replay_over_dead_ends(sp, M, m):
    """rand_r over W.dead_ends: the first launch (positions from the degrees) reports flags[0] & 1; with subgacc_rng_replay's walk
    positions the general kernel -- the only reader of walk_pos -- gives the oracle's sets exactly"""
    g = W.dead_ends(M, m)
    q, N = g["batch"], g["num_nodes"]
    ref = _reference(g, q, M, m, "rand_r")
    for idx64 in (False, True):
        csr = _csr(g, idx64)
        first = _sets(csr, q, M, m, "rand_r")
        assert first["flags"].tolist() == [1, 0, 0, 0] and np.array_equal(first["nsize"] > 0, np.ones(len(q), bool))
        got = _sets(csr, q, M, m, "rand_r", replay=True)
        _same_as_reference(got, ref, q, N, (M, m, idx64))
        got = _sets(csr, q, M, m, "rand_r", replay=True, emit=True)
        _same_as_reference(got, ref, q, N, (M, m, idx64, "walks"))
        _check_walks(got, g, q, M, m, "rand_r", "walk", rows=range(0, len(q), 9))
    _same_as_reference(_sets(_csr(g), q, M, m, "philox"), _reference(g, q, M, m, "philox"), q, N, "philox")


@pytest.mark.parametrize("M,m", G.ROOT_SHAPES)
def test_sets_roots_outside_the_graph(sp, M, m):
    """-1, N, INT32_MAX and SUBGACC_NO_ROOT between an isolated root, a lone self loop, id 0 and id N - 1, and n = 1: a root outside
    the graph gives nsize = 0, flags[3] & 16 and an untouched row (include/subgacc.h), SUBGACC_NO_ROOT the same without the flag --
    in walk_sets_kernel and, at M = 4, two hops, in walk_pipe_kernel"""
    g = G.edge_graph(M, m)
    N = g["num_nodes"]
    base = g["batch"]
    q = np.concatenate([[-1], base[:7], [N], base[7:], [G.INT32_MAX, NO_ROOT], base[::-1], [NO_ROOT, -7]]).astype(np.int32)
    queries = [q, np.where(G.in_graph(q, N), q, NO_ROOT).astype(np.int32)] + [np.array([v], dtype=np.int32) for v in (-1, N, NO_ROOT, 0, N - 1)]
    piped = G.kernel_for(M, m) == "walk_pipe_kernel"
    for qq in queries:
        for rng in RNGS:
            ref = _reference(g, qq, M, m, rng)
            assert (ref["nsize"][~ref["good"]] == 0).all()
            for idx64 in (False, True):
                csr = _csr(g, idx64)
                gen = _sets(csr, qq, M, m, rng, emit=True)
                _same_as_reference(gen, ref, qq, N, ("general", rng, idx64, len(qq)))
                _check_walks(gen, g, qq, M, m, rng, "walk")
                if piped:
                    pipe = _sets(csr, qq, M, m, rng)
                    _same_as_reference(pipe, ref, qq, N, ("pipe", rng, idx64, len(qq)))
                    _bitwise(pipe, gen, (rng, idx64, len(qq)))
    assert _flags(queries[1], N) == [0, 0, 0, 0] and _flags(q, N)[3] == 16


# ---------------------------------------------------------------------------------- B. walk_sets_kernel<SPG>: fused rows
def _spg(csr, q, M, m, rng, pitch=0, bucket=-1, root_base=0):
    """subgacc_walk_spg with a table of distinct rows into poisoned, guarded outputs, numbered afterwards: the dict _check reads"""
    from surel_plus_amd import sampler
    L = _L()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n = len(q)
    stride = bucket if bucket > 0 else M * m + 1
    P = pitch if pitch > 0 else stride
    d_q = _dev(np.asarray(q, dtype=np.int32))
    cfg = sampler.make_cfg(csr, M, m, bucket, SEED, rng, records=False, row_pitch=pitch)
    rp, rs = sampler._rng_positions(lib, cfg, csr, d_q, n, 1, 0, st)
    w_ids, ids = _guarded(n * P, torch.int32)
    w_pay, pay = _guarded(n * P, torch.int32)
    w_ns, nsize = _guarded(n, torch.int32)
    w_fl, flags = _guarded(4, torch.int32, np.zeros(4, np.int32))
    nbytes = lib.subgacc_uniq_table_bytes(CAP)
    table = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(lib.subgacc_uniq_reset(ptr(table), CAP, st))
    L.check(lib.subgacc_walk_spg(cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(d_q), n, root_base, ptr(rp), ptr(rs), ptr(table),
                                 CAP, ptr(ids), ptr(pay), ptr(nsize), ptr(flags), st))
    ukeys = torch.full((CAP,), -1, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.subgacc_uniq_number_workspace_bytes(CAP, 0), dtype=torch.uint8, device="cuda")
    L.check(lib.subgacc_uniq_number(ptr(table), CAP, None, 0, ptr(ukeys), CAP, ptr(count), CAP, ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    t = table.cpu().numpy()
    assert (t[nbytes:] == 0xA5).all(), "bytes behind the table were written"
    return dict(n=n, P=P, form="table", tkeys=t[: 8 * CAP].view(np.uint64), ukeys=ukeys.cpu().numpy().view(np.uint64)[: int(count.item())],
                ids=_back(w_ids, n * P).reshape(n, P), pay=_back(w_pay, n * P).reshape(n, P), nsize=_back(w_ns, n), flags=_back(w_fl, 4))


def _spg_vs_oracle(g, q, M, m, buckets, pitches=None, widths=(False, True)):
    Q = M * m + 1
    for bucket in buckets:
        assert G.kernel_for(M, m, "table", bucket=bucket) == "walk_sets_kernel<SPG>"
        stride = bucket if bucket > 0 else Q
        for rng in RNGS:
            ref = _reference(g, q, M, m, rng, bucket)
            exp = G.as_rows(ref, M, m)
            for k, idx64 in enumerate(widths if rng == "philox" else widths[:1]):
                for pitch in (pitches or (0, (stride + 32) // 32 * 32)):          # row_pitch == stride and > stride
                    got = _spg(_csr(g, idx64), q, M, m, rng, pitch, bucket, root_base=0 if pitch == 0 else 1000 + k)
                    _check(got, exp, flags=(0, ref.get("cut", 0), 0, 0), what=(M, m, rng, idx64, pitch, bucket))
                    assert np.array_equal(got["ukeys"], exp["ukeys"])


@pytest.mark.parametrize("M,m", [s for s in G.SPG_SHAPES if s not in G.FOLD_SHAPES])
def test_spg_rows_from_the_general_kernel(sp, M, m):
    """the fused rows of the shapes launch_walk_rows declines, in both forms of the epilogue on the same graph: without a bucket (the
    fold table over inv, no ranking) and with a truncating one (ranking, the fold table behind inv; bucket = ns - 1, ns, ns + 1 of the
    tree of Q - 5 members).  Sets of 1 .. 5 members, runs at id 0 and N - 1, the full set past B = min(T / 4, 256), 12 | 13 | 24
    members in one level-1 bucket (M = 60), staged on both sides at Q = 682 | 683; both pitches, root_base > 0 with the wide one"""
    Q = M * m + 1
    crowd = (M, m) == G.CROWD_SHAPE
    g = G.edge_graph(M, m, crowd=crowd)
    big = M > 300
    _spg_vs_oracle(g, g["batch"], M, m, (-1,), widths=(False,) if big else (False, True))
    _spg_vs_oracle(g, g["batch"], M, m, (Q - 6, Q - 5, Q - 4), pitches=(0,), widths=(True,) if big else (False, True))


@pytest.mark.parametrize("M,m", G.FOLD_SHAPES)
def test_spg_fold_table_overflow(sp, M, m):
    """sets of more than kSpgFold distinct LP rows (dense graph): keys that find no slot in 16 probes go straight to the HBM table --
    with the fold table over inv and, bucket 160, behind it"""
    g = G.fold_graph(M, m)
    _spg_vs_oracle(g, g["batch"], M, m, (-1, 160))
    e = G.edge_graph(M, m)
    _spg_vs_oracle(e, e["batch"], M, m, (-1,), pitches=(0,), widths=(False,))


def test_spg_unstaged_row_write_with_a_bucket(sp):
    """T = 256: bucket 170 | 171 on both sides of stride <= (2T - 2) / 3 -- the row assembled in LDS, and written straight from
    the ranking loop"""
    M, m = G.STAGED_BUCKET
    g = G.edge_graph(M, m)
    _spg_vs_oracle(g, g["batch"], M, m, G.staged_edge(256))


# ------------------------------------------------------------------------------------------------------ C. walk_pipe_kernel
def _pipe_vs_both(g, q, M, m, rng, idx64, bucket=-1, ref=None, dead=0, oracle_too=True):
    assert G.kernel_for(M, m, bucket=bucket) == "walk_pipe_kernel" and G.kernel_for(M, m, bucket=bucket, emit_walks=True) == "walk_sets_kernel"
    csr = _csr(g, idx64)
    pipe = _sets(csr, q, M, m, rng, bucket=bucket)
    gen = _sets(csr, q, M, m, rng, bucket=bucket, emit=True)
    if oracle_too:
        ref = ref or _reference(g, q, M, m, rng, bucket)
        _same_as_reference(pipe, ref, q, g["num_nodes"], ("pipe", M, m, rng, idx64, bucket), dead=dead)
    _bitwise(pipe, gen, (M, m, rng, idx64, bucket))
    return pipe


def test_pipe_every_hop_count_rng_and_offset_width(sp):
    """all 24 instantiations of a product build: 1 .. 6 hops x rand_r | Philox x int32 | int64 row offsets, at M = 4"""
    for M, m, rng, idx64 in G.pipe_launches():
        g = G.edge_graph(M, m)
        _pipe_vs_both(g, g["batch"], M, m, rng, idx64)


@pytest.mark.parametrize("M,m", G.PIPE_WALKS)
def test_pipe_walker_mask(sp, M, m):
    """M = 1, 63, 64, 65, 255, 256 walkers of 256 lanes (M = 257 leaves the pipe: test_sets_walk_loop_trips)"""
    g = G.edge_graph(M, m)
    for rng in RNGS:
        _pipe_vs_both(g, g["batch"], M, m, rng, rng == "philox")


@pytest.mark.parametrize("rng", RNGS)
def test_pipe_grid_edges(sp, rng):
    """n = 1, 2, 256c - 1, 256c, 256c + 1 and 2 * 256c + 1 for every c = 1..8 the occupancy query may yield: one root short of the
    grid, the grid, one, every and one more than every workgroup with a second root.  Sets are prefixes of one oracle run (Philox:
    functions of the root; rand_r: one sequential stream)"""
    M, m = G.GRID_SHAPE
    g = G.edge_graph(M, m)
    base = np.random.default_rng(5).permutation(g["batch"])
    q = np.resize(base, max(G.GRID_NS)).astype(np.int32)
    whole = _reference(g, q, M, m, rng)
    for n in G.GRID_NS:
        ref = dict(nsize=whole["nsize"][:n], ids=whole["ids"][: whole["off"][n]], keys=whole["keys"][: whole["off"][n]])
        _pipe_vs_both(g, q[:n], M, m, rng, n % 2 == 0, ref=ref)


def test_pipe_root_kind_transitions(sp):
    """one workgroup's sequence of roots (i, i + G, i + 2G, ..) meets every ordered pair of kinds -- ordinary, shuffled, isolated,
    outside the graph, SUBGACC_NO_ROOT, truncated, full, dead ends, self loop -- for every grid G = 256c: the LDS tables must come
    back clean from each.  Without a bucket (full sets) and with one of 5 (truncated sets); under Philox a root that stands twice
    has identical rows; rand_r meets dead ends here, so it is compared with walk_sets_kernel alone"""
    M, m = G.GRID_SHAPE
    g, pools = G.transition_graph()
    q, kind = G.transition_query()
    for bucket in (-1, G.TRANSITION_BUCKET):
        for idx64 in (False, True):
            pipe = _pipe_vs_both(g, q, M, m, "philox", idx64, bucket=bucket)
            assert pipe["flags"][3] == 16 and (pipe["flags"][1] > 0) == (bucket > 0)
            order = np.argsort(q, kind="stable")
            for a, b in zip(order[:-1], order[1:]):
                if q[a] == q[b]:
                    assert pipe["nsize"][a] == pipe["nsize"][b] and np.array_equal(pipe["ids"][a], pipe["ids"][b]) and \
                        np.array_equal(pipe["keys"][a], pipe["keys"][b])
        _pipe_vs_both(g, q, M, m, "rand_r", False, bucket=bucket, oracle_too=False)
    # ... and the same transitions without the dead-end roots, rand_r against the oracle
    live = q[kind != G.KINDS.index("dead_end")]
    _pipe_vs_both(g, live, M, m, "rand_r", True)


# -------------------------------------------------------------------------------------------------- D. subgacc_compact_sets
@pytest.mark.parametrize("n", (1, 3, 4, 5))
def test_compact_sets(sp, n):
    """the strided -> packed copy with and without the table of distinct rows: sizes 0, 63, 64, 65 and a set of 300 distinct keys (a
    wave's 256-slot fold table overflows: those keys go straight to HBM and are found again by probing); every member's slot holds
    its key and subgacc_uniq_number numbers the keys by first occurrence in the packed array"""
    L = _L()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    c = G.compact_case(n)
    e_ids, e_keys, e_ukeys = G.compact_expected(c)
    X = len(e_ids)
    src = [_dev(c["ids"].reshape(-1)), _dev(c["keys"].reshape(-1).view(np.int64)), _dev(c["nsize"]), _dev(c["row_off"])]
    for insert in (False, True):
        w_ids, ids = _guarded(X, torch.int32)
        w_keys, keys = _guarded(X, torch.int64)
        w_slot, slot = _guarded(X, torch.int32)
        w_fl, flags = _guarded(4, torch.int32, np.zeros(4, np.int32))
        nbytes = lib.subgacc_uniq_table_bytes(CAP)
        table = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        L.check(lib.subgacc_uniq_reset(ptr(table), CAP, st))
        L.check(lib.subgacc_compact_sets(*[ptr(t) for t in src], n, c["stride"], ptr(ids), ptr(keys), ptr(table) if insert else None,
                                         CAP if insert else 0, 0, ptr(slot) if insert else None, ptr(flags) if insert else None, st))
        torch.cuda.synchronize()
        assert np.array_equal(_back(w_ids, X), e_ids) and np.array_equal(_back(w_keys, X).view(np.uint64), e_keys)
        assert not _back(w_fl, 4).any()
        h_slot = _back(w_slot, X)
        if not insert:
            assert (h_slot == POISON).all()
            continue
        ukeys = torch.full((CAP,), -1, dtype=torch.int64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.subgacc_uniq_number_workspace_bytes(CAP, 0), dtype=torch.uint8, device="cuda")
        L.check(lib.subgacc_uniq_number(ptr(table), CAP, None, 0, ptr(ukeys), CAP, ptr(count), CAP, ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        t = table.cpu().numpy()
        assert (t[nbytes:] == 0xA5).all()
        tkeys = t[: 8 * CAP].view(np.uint64)
        assert (h_slot >= 0).all() and (h_slot < CAP).all() and np.array_equal(tkeys[h_slot], e_keys)
        assert np.array_equal(ukeys.cpu().numpy().view(np.uint64)[: int(count.item())], e_ukeys)

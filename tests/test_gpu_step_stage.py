"""GPU (MI355X): the LP encoder's mean first stage on the on-demand step -- the columns of a step's LP keys (subgacc_keyrows_columns),
the count form over strided key rows (subgacc_sjoin_key_counts), sample_and_counts / sample_and_hcounts against gather_counts /
hgather_counts over the all-nodes store, one result whatever the route, the stage against the reference form, and the captured step.
Counts, sizes, keys and feature rows are compared bit for bit; the model stage with the tolerances
test_mean_stage_trains_like_the_reference_first_stage states."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import sp  # noqa: F401
from test_gpu_horder import M, World

pytestmark = pytest.mark.gpu

NT = 256                    # lanes of a workgroup of the count kernel; its register trips hold 2 * NT members of the searched row
STRIDE = 544                # words between two rows (a multiple of 32); one row fills it
LENS = (0, 1, NT - 1, NT, NT + 1, 2 * NT - 1, 2 * NT, 2 * NT + 1, STRIDE)
HOPS = 3
SHIFT = 8                   # 32 - clz(200)
POISON = 0x7FFFFFFF         # what stands behind a row's members: never read
GUARD = 64


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


# ------------------------------------------------------------------------------------------------------------- synthetic key rows
def _lp_keys(count, seed, M=M, hops=HOPS, shift=SHIFT):
    """`count` distinct valid LP keys of (M, hops): `hops` counts of `shift` bits (three of 8), some with the root's LEAD bit"""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < count:
        c = rng.integers(0, M + 1, hops)
        k = 0
        for v in c:
            k = (k << shift) | int(v)
        if rng.integers(0, 4) == 0:
            k |= 1 << (hops * shift)
        if k:
            keys.add(k)
    return np.array(sorted(keys), dtype=np.uint32)


class Rows:
    """strided key rows built on the host: ids ascend inside a row, keys are drawn from `keyset`; every key of the set occurs.
    Without `lens`: the rows of LENS, a disjoint pair and a fully overlapping pair, each row joined with itself and its neighbour.
    With `lens`: one row of random ids (below `id_space`) per entry, `stride` words apart; `pairs = (a, b)` replaces the list of
    every row with itself and with its neighbour; `distinct`: a row no longer than the key set holds no key twice (before the keys
    that make every key of the set stand somewhere are laid over the rows' first members)."""

    def __init__(self, keyset, seed, lens=None, stride=STRIDE, pairs=None, distinct=False, id_space=4000):
        rng = np.random.default_rng(seed)
        self.keyset, self.stride = keyset, stride
        rows = []
        for L in (LENS if lens is None else lens):
            rows.append(np.sort(rng.choice(id_space, L, replace=False)))
        if lens is None:
            rows.append(np.arange(0, 600, 2))                    # disjoint ids: even against odd
            rows.append(np.arange(1, 601, 2))
            same = np.sort(rng.choice(4000, 2 * NT + 1, replace=False))
            rows += [same, same.copy()]                          # full overlap: the same ids, other keys
        self.n = len(rows)
        self.ids = np.full((self.n, stride), -1, dtype=np.int32)
        self.keys = np.full((self.n, stride), POISON, dtype=np.uint32)
        self.len = np.array([len(r) for r in rows], dtype=np.int32)
        at = 0
        for i, r in enumerate(rows):
            self.ids[i, : len(r)] = r
            if distinct and len(r) <= len(keyset):
                k = rng.permutation(keyset)[: len(r)]
            else:
                k = keyset[rng.integers(0, len(keyset), len(r))]
            take = min(len(r), len(keyset) - at)              # every key of the set stands somewhere
            k[:take] = keyset[at: at + take]
            at += take
            self.keys[i, : len(r)] = k
        assert at == len(keyset)
        if pairs is not None:
            a, b = pairs
        elif lens is not None:
            a = list(range(self.n)) + list(range(self.n))
            b = list(range(self.n)) + [(i + 1) % self.n for i in range(self.n)]
        else:
            e, o, x = len(LENS), len(LENS) + 1, len(LENS) + 2
            a = list(range(self.n)) + list(range(self.n)) + [e, x, 0, 0]
            b = list(range(self.n)) + [(i + 1) % self.n for i in range(self.n)] + [o, x + 1, 0, len(LENS) - 1]
        self.a, self.b = np.array(a), np.array(b)            # with itself, with its neighbour, disjoint, full overlap, empty rows

    @classmethod
    def of(cls, keys, lens):
        """rows given as arrays (keys [n, stride] uint32, lens [n]) for the columns pass alone: no ids, no segment list"""
        self = cls.__new__(cls)
        self.n, self.stride = keys.shape
        self.keys, self.len, self.ids = keys, lens.astype(np.int32), None
        return self

    def device(self):
        ids = None if self.ids is None else torch.from_numpy(self.ids.reshape(-1)).cuda()
        return ids, torch.from_numpy(self.keys.view(np.int32).reshape(-1)).cuda(), torch.from_numpy(self.len).cuda()

    def present(self):
        return np.unique(np.concatenate([self.keys[i, : self.len[i]] for i in range(self.n)]))

    def counts(self, ukeys, T):
        """NumPy restatement of the count form: own = [a | b], partner = [b | a]; a feature slot whose key is outside `ukeys` is not counted"""
        col = {int(k): i + 1 for i, k in enumerate(ukeys)}
        own, par = np.concatenate([self.a, self.b]), np.concatenate([self.b, self.a])
        out = np.zeros((len(own), T), dtype=np.float32)
        missing = False
        for j, (ra, rb) in enumerate(zip(own, par)):
            pos = {int(v): t for t, v in enumerate(self.ids[rb, : self.len[rb]])}
            for t in range(self.len[ra]):
                p = col.get(int(self.keys[ra, t]), -1)
                hit = pos.get(int(self.ids[ra, t]))
                q = 0 if hit is None else col.get(int(self.keys[rb, hit]), -1)
                missing |= p < 0 or q < 0
                if p >= 0:
                    out[j, p] += 1
                if q >= 0:
                    out[j, q] += 1
        return out, self.len[own], missing


def _guarded(n, dtype, fill):
    """n elements with GUARD more behind them"""
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def _workspace(nbytes):
    """a zeroed columns workspace of nbytes with GUARD bytes of 0x5A behind it"""
    ws = torch.zeros(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0x5A
    return ws


def _columns(sp, rows, T, M=M, hops=HOPS, ws=None):
    """the columns pass over `rows`; `ws`: a _workspace() of the caller's (at least as large as T needs), given to the call whole"""
    from surel_plus_amd import _lib
    L = _lib.lib()
    ids, keys, nsize = rows.device()
    ukeys, count = _guarded(T - 1, torch.int32, -7), _guarded(1, torch.int64, -7)
    feat = _guarded(T * (hops + 1), torch.float32, -7.0)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    nbytes = L.subgacc_keyrows_columns_workspace_bytes(T)
    if ws is None:
        ws = _workspace(nbytes)
    else:
        assert ws.numel() - GUARD >= nbytes
        nbytes = ws.numel() - GUARD
    _lib.check(L.subgacc_keyrows_columns(_lib.ptr(keys), _lib.ptr(nsize), rows.n, rows.stride, M, hops, T, _lib.ptr(ukeys),
                                         _lib.ptr(count), _lib.ptr(feat), _lib.ptr(flags), _lib.ptr(ws), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((ukeys[T - 1:] == -7).all()) and bool((count[1:] == -7).all()) and bool((feat[T * (hops + 1):] == -7.0).all())
    assert bool((ws[:nbytes] == 0).all()) and bool((ws[nbytes:] == 0x5A).all())       # the workspace is left zeroed, its guard alone
    return ukeys[: T - 1], count[:1], feat[: T * (hops + 1)].view(T, hops + 1), flags


def _key_counts(sp, rows, ukeys, count, T, partner=False, want_len=True, M=M, hops=HOPS):
    from surel_plus_amd import _lib
    L = _lib.lib()
    ids, keys, nsize = rows.device()
    own = torch.from_numpy(np.concatenate([rows.a, rows.b])).cuda()
    par = torch.from_numpy(np.concatenate([rows.b, rows.a])).cuda() if partner else None
    S = own.numel()
    out, olen = _guarded(S * T, torch.float32, -7.0), _guarded(S, torch.int32, -7)
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    d = _lib.join_desc(_lib.JOIN_COUNTS, _lib.JOIN_KEY32, row_len=nsize, n_rows=rows.n, row_stride=rows.stride, ids=ids, payload=keys,
                       own=own, partner=par, S=S, pair_block=S // 2, table_rows=T, num_walks=M, num_steps=hops, flags=flags)
    _lib.check(L.subgacc_sjoin_key_counts(C.byref(d), _lib.ptr(ukeys), _lib.ptr(count), _lib.ptr(out), _lib.ptr(olen) if want_len else None,
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((out[S * T:] == -7.0).all()) and bool((olen[S:] == -7).all())
    return out[: S * T].view(S, T).cpu().numpy(), olen[:S].cpu().numpy(), flags.cpu().numpy()


def _feature_rows(keys, M=M, hops=HOPS, shift=SHIFT):
    """NumPy restatement of subgacc_unpack_lp(out_f32): float32 divisions by float32(M)"""
    k = keys.astype(np.uint64)
    cols = [np.where((k >> (hops * shift)) & 1, np.float32(M), np.float32(0))]
    cols += [((k >> ((hops - j) * shift)) & ((1 << shift) - 1)).astype(np.float32) for j in range(1, hops + 1)]
    return (np.stack(cols, 1).astype(np.float32) / np.float32(M)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("nkeys,T", [pytest.param(1, 2, id="one-key"), pytest.param(1, 40, id="one-key-wide"),
                                     pytest.param(15, 16, id="T-1-keys"), pytest.param(299, 300, id="299-keys"),
                                     pytest.param(700, 1030, id="700-keys-T1030")])
def test_columns_and_counts_equal_their_numpy_restatement(sp, nkeys, T):
    """row lengths 0, 1, NT-1, NT, NT+1, 2 NT-1, 2 NT, 2 NT+1 and a row that fills row_stride; a row with itself, disjoint ids, full
    overlap, an empty row; one key (every LDS atomic of a block on one address) and exactly T-1 keys"""
    from surel_plus_amd import _lib
    rows = Rows(_lp_keys(nkeys, 11 + nkeys), seed=nkeys)
    present = rows.present()
    assert len(present) == nkeys and np.array_equal(present, rows.keyset)
    ukeys, count, feat, flags = _columns(sp, rows, T)
    assert int(count) == nkeys and not flags.any()
    got = ukeys.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:nkeys], present) and not got[nkeys:].any()
    # feat: row 0 zero, rows 1 .. c the keys unpacked as subgacc_unpack_lp does it (bit for bit), rows past c zero
    f = feat.cpu().numpy()
    ref = torch.empty((nkeys + 1, HOPS + 1), dtype=torch.float32, device="cuda")
    k64 = torch.from_numpy(present.astype(np.int64)).cuda()
    _lib.check(_lib.lib().subgacc_unpack_lp(_lib.ptr(k64), nkeys, None, M, HOPS, None, None, _lib.ptr(ref), 1, _lib.stream_ptr()))
    assert np.array_equal(f[: nkeys + 1].view(np.uint32), ref.cpu().numpy().view(np.uint32))
    assert np.array_equal(f[1: nkeys + 1].view(np.uint32), _feature_rows(present).view(np.uint32))
    assert not f[0].any() and not f[nkeys + 1:].any()
    want, want_len, missing = rows.counts(present, T)
    assert not missing
    for partner in (False, True):
        out, olen, fl = _key_counts(sp, rows, ukeys, count, T, partner=partner)
        assert not fl.any()
        assert np.array_equal(out, want) and np.array_equal(olen, want_len)
        assert not out[:, nkeys + 1:].any()
    out, _, _ = _key_counts(sp, rows, ukeys, count, T, want_len=False)        # out_len is optional
    assert np.array_equal(out, want)
    # an empty segment is a zero row of C with size 0, and the stage's algebra on these very (C, sizes) gives it a zero row -- with an
    # embedding whose value on the zero feature row is not zero -- and every other segment a row that is not zero
    from surel_plus_amd import spjoin
    empty = np.flatnonzero(want_len == 0)
    assert empty.size and not out[empty].any()
    torch.manual_seed(2)
    embed = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8)).cuda()
    with torch.no_grad():
        assert bool(embed(feat[:1]).abs().sum() > 0)
        x = spjoin._step_mean(torch.from_numpy(out).cuda(), torch.from_numpy(want_len).cuda(), feat, None, embed, 2)
    x = x.reshape(len(want_len), 8).cpu().numpy()
    assert x.shape[0] == out.shape[0] and np.isfinite(x).all()
    assert not x[empty].any() and x[want_len > 0].any(1).all()
    # every member counts twice (its own LP row; its partner's, or column 0)
    assert np.array_equal(out.sum(1), 2.0 * want_len)


# ------------------------------------------------------------------------------------------------------ 2. too many distinct rows
def test_more_distinct_rows_than_columns(sp, world):
    """T-1 one less than the keys present: flags[2] & 1, the count clamped, the smallest T-1 keys kept, every guard untouched; the count
    kernel then meets keys that are not in its list: flags[3] & 2, those members not counted, nothing out of bounds"""
    from surel_plus_amd import _lib
    nkeys = 40
    rows = Rows(_lp_keys(nkeys, 3), seed=5)
    T = nkeys                                   # T - 1 = 39 columns for 40 keys
    ukeys, count, feat, flags = _columns(sp, rows, T)       # (_columns checks the guards)
    assert int(flags[2]) & 1 and int(count) == T - 1
    kept = ukeys.cpu().numpy().view(np.uint32)
    assert np.array_equal(kept, rows.present()[: T - 1])
    assert np.array_equal(feat.cpu().numpy()[1:].view(np.uint32), _feature_rows(kept).view(np.uint32))
    want, want_len, missing = rows.counts(kept, T)
    assert missing
    out, olen, fl = _key_counts(sp, rows, ukeys, count, T)
    assert int(fl[3]) & 2 and np.array_equal(out, want) and np.array_equal(olen, want_len)
    # the buffered step: nothing is read back, sets.resolve() raises and names table_rows
    bufs = sp.StepBuffers(world.csr, 64, num_walks=M, num_steps=HOPS, stage="counts", table_rows=8)
    _, _, _, sets = sp.sample_and_counts(world.csr, world.pairs(64, 1), num_walks=M, num_steps=HOPS, seed=5, buffers=bufs)
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        sets.resolve()
    x = sp.sample_and_mean_stage(world.csr, world.pairs(64, 1), torch.nn.Linear(HOPS + 1, 4).cuda(), num_walks=M, num_steps=HOPS, seed=5,
                                 buffers=bufs)
    assert x.shape == (2, 64, 4)
    with pytest.raises(_lib.SubgAccError, match="table_rows"):      # the stage returns the tensor alone: the step is checked here
        bufs.sets.resolve()
    with pytest.raises(_lib.SubgAccError, match="table_rows"):
        sp.sample_and_counts(world.csr, world.pairs(64, 1), num_walks=M, num_steps=HOPS, seed=5, table_rows=8)


# ------------------------------------------------------------------------------------------------------ 3. against the tested path
def _dicts(Cm, table):
    """per segment {feature row as bytes: count} over the columns that occur"""
    Cm, table = Cm.cpu().numpy(), np.ascontiguousarray(table.cpu().numpy())
    rowb = [table[p].tobytes() for p in range(table.shape[0])]
    out = []
    for j in range(Cm.shape[0]):
        d = {}
        for p in np.flatnonzero(Cm[j]):
            assert rowb[p] not in d
            d[rowb[p]] = float(Cm[j, p])
        out.append(d)
    return out


@pytest.mark.parametrize("hops", [2, 3])
def test_pair_counts_equal_gather_counts_over_the_store(sp, world, hops):
    """sample_and_counts against gather_counts(edge, z, rows) over the all-nodes store of the same seed with sets.feature_table(): per
    segment the same {feature row: count}, the same sizes.  table_rows is the store's own row count: the reference path alone decides
    that no overflow occurs.  The batch holds the isolated root, the hubs, every star centre, u == v."""
    z, table, lens = world.store(hops)
    T = table.shape[0]
    e = world.pairs(300, 1)
    en = e.cpu().numpy()
    assert (en[0] == en[1]).any() and all((en == s).any() for s in world.special)
    Cr, sizes_r = sp.gather_counts(e, z, T)
    Cm, sizes, tab, sets = sp.sample_and_counts(world.csr, e, num_walks=M, num_steps=hops, seed=5, table_rows=T)
    assert Cm.shape == (600, T) and tab.shape == table.shape and sizes.dtype == torch.int32
    assert torch.equal(sizes.to(torch.int64), sizes_r) and np.array_equal(sizes.cpu().numpy(), lens[en.reshape(-1)])
    assert _dicts(Cm, tab) == _dicts(Cr, table)
    # without table_rows: exactly one column per distinct LP row of the batch, the same counts
    Cf, sizes_f, tab_f, _ = sp.sample_and_counts(world.csr, e, num_walks=M, num_steps=hops, seed=5)
    c = tab_f.shape[0] - 1
    assert 1 <= c <= T - 1 and Cf.shape == (600, c + 1) and bool((Cf.sum(0) > 0).all())
    assert torch.equal(Cf, Cm[:, : c + 1]) and not bool(Cm[:, c + 1:].any()) and torch.equal(tab_f, tab[: c + 1])
    assert torch.equal(sizes_f, sizes)


@pytest.mark.parametrize("hops", [2, 3])
def test_triplet_counts_equal_hgather_counts_over_the_store(sp, world, hops):
    """the same for triplets against hgather_counts: u == v, u == w, u == v == w and every special root in every role"""
    z, table, lens = world.store(hops)
    T = table.shape[0]
    h = world.triplets(128, 3)
    hn = h.cpu().numpy()
    u, v, w = hn
    assert ((u == v) & (u != w)).any() and ((u == w) & (u != v)).any() and ((u == v) & (v == w)).any()
    assert all((hn[role] == s).any() for role in range(3) for s in world.special)
    Cr, sizes_r = sp.hgather_counts(h, z, T)
    for dedup in (False, True):
        Cm, sizes, tab, sets = sp.sample_and_hcounts(world.csr, h, num_walks=M, num_steps=hops, seed=5, table_rows=T, dedup_roots=dedup)
        assert Cm.shape == (512, T)
        assert torch.equal(sizes.to(torch.int64), sizes_r)
        assert _dicts(Cm, tab) == _dicts(Cr, table)


# ------------------------------------------------------------------------------------------------------ 4. one result whatever the route
def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_one_result_whatever_the_route(sp, world):
    csr, B, T = world.csr, 300, 1024
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    want1 = sp.sample_and_counts(csr, e1, table_rows=T, **kw)
    want2 = sp.sample_and_counts(csr, e2, table_rows=T, **kw)
    assert not torch.equal(want1[0], want2[0])
    assert _same(sp.sample_and_counts(csr, e1, table_rows=T, **kw), want1)                       # two runs
    assert _same(sp.sample_and_counts(csr, e1, table_rows=T, dedup_roots=True, **kw), want1)
    order = sp.locality_order(csr)
    assert _same(sp.sample_and_counts(csr, e1, table_rows=T, order=order, **kw), want1)
    for dedup, ordr in ((False, None), (True, None), (False, order), (True, order)):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=dedup, order=ordr, stage="counts", table_rows=T)
        assert bufs.out is None and bufs.segid is None and bufs.counts.shape == (2 * B, T)
        for e, want in ((e1, want1), (e2, want2), (e1, want1)):             # a second step on the same buffers gives ITS batch
            got = sp.sample_and_counts(csr, e, buffers=bufs, dedup_roots=dedup, order=ordr, **kw)
            assert got[0].data_ptr() == bufs.counts.data_ptr() and got[2].data_ptr() == bufs.feat.data_ptr()
            assert bufs.sets is got[3]
            got[3].prefetch().resolve()
            assert got[3].extra is None                  # no row form ran: there is no row count to report
            assert _same(got, want)
    h = world.triplets(128, 3)
    hwant = sp.sample_and_hcounts(csr, h, table_rows=T, **kw)
    hb = sp.StepBuffers(csr, 128, num_walks=M, num_steps=HOPS, triplets=True, dedup_roots=True, stage="counts", table_rows=T)
    for _ in range(2):
        got = sp.sample_and_hcounts(csr, h, buffers=hb, dedup_roots=True, **kw)
        got[3].resolve()
        assert _same(got, hwant)


# ------------------------------------------------------------------------------------------------------------------ 5. the stage
def _reference_stage(mlp, xz, seg, S, H, blocks):
    x = mlp(xz).sum(dim=-2)
    n = seg[1:] - seg[:-1]
    ids = torch.repeat_interleave(torch.arange(S, device="cuda"), n)
    return (torch.zeros(S, H, device="cuda").index_add_(0, ids, x) / n.clamp(min=1)[:, None]).view(blocks, -1, H)


@pytest.mark.parametrize("triplets", [False, True], ids=["pairs", "triplets"])
def test_stage_trains_like_the_reference_first_stage(sp, world, triplets):
    """sample_and_mean_stage / sample_and_hmean_stage against pe_embedding(xz).sum(-2) + mean aggregation (model.py:78-83,
    model_horder.py:56-57) on the (xz, ind) of sample_and_gather / sample_and_hgather for the same seed: forward and every parameter
    gradient, with the tolerances test_mean_stage_trains_like_the_reference_first_stage states (forward rtol 1e-4, atol 1e-5; gradients
    1e-4 of their largest entry)."""
    csr, H = world.csr, 16
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    torch.manual_seed(1)
    mlp_a = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, 16), torch.nn.ReLU(), torch.nn.Linear(16, H)).cuda()
    mlp_b.load_state_dict(mlp_a.state_dict())
    if triplets:
        B, blocks = 128, 4
        h = world.triplets(B, 3)
        fused = sp.sample_and_hmean_stage(csr, h, mlp_a, **kw)
        xz, ids, _ = sp.sample_and_hgather(csr, h, **kw)
        seg = ids.seg_pointers
    else:
        B, blocks = 300, 2
        e = world.pairs(B, 1)
        fused = sp.sample_and_mean_stage(csr, e, mlp_a, **kw)
        xz, seg, _ = sp.sample_and_gather(csr, e, **kw)
    assert fused.shape == (blocks, B, H) and torch.is_tensor(fused)
    w = torch.randn(blocks, B, H, device="cuda")
    (fused * w).sum().backward()
    ref = _reference_stage(mlp_b, xz, seg, blocks * B, H, blocks)
    (ref * w).sum().backward()
    assert torch.allclose(fused, ref, rtol=1e-4, atol=1e-5)
    for pa, pb in zip(mlp_a.parameters(), mlp_b.parameters()):
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-4 * float(pb.grad.abs().max()) + 1e-6


# ------------------------------------------------------------------------------------------------------------------ 6. capture
def test_captured_step_replays_another_batch(sp, world):
    """the buffered step with stage="counts" under torch.cuda.graph on one stream; replayed with a second batch copied into the static
    edge tensor it equals the eager result of that batch bit for bit"""
    csr, B, T = world.csr, 300, 1024
    kw = dict(num_walks=M, num_steps=HOPS, seed=5)
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    want2 = sp.sample_and_counts(csr, e2, table_rows=T, dedup_roots=True, **kw)
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, dedup_roots=True, stage="counts", table_rows=T)
    static = e1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                   # lazy code-object loads and cached segment lists, uncaptured
        sp.sample_and_counts(csr, static, buffers=bufs, dedup_roots=True, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = sp.sample_and_counts(csr, static, buffers=bufs, dedup_roots=True, **kw)
    static.copy_(e2)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(got, want2)
    assert int(bufs.status[2]) == int((want2[0].sum(0) > 0).sum()) - 1 and not int(bufs.status[1])

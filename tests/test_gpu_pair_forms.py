"""GPU (MI355X): what the count form, the pair form and the count form with attention (csrc/sjoin_forms.hip: sjoin_counts_kernel,
sjoin_pairs_kernel, sjoin_counts_attn_kernel) decide about a workgroup's mirrored pair before they join it -- which segment is whose
mirror, which row is the shorter one, and the three refusals: past the list, a list that is not mirrored (flags[3] & 4), a row longer
than the descriptor's max_len (flags[3] & 1).  A hand-made store of 16 rows (lengths 0, 1, 7 and 8 = max_len among them) over a table
of 8 LP rows; six pairs: longer row first, shorter row first, equal lengths, an empty row on either side, (u, u).  The count and the
pair form against the oracle's join bit for bit, the attention form's W against the pair form's rows through a float64 softmax at
test_gpu_counts_attn.py's tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import surel_plus_amd as spm
from gpu_helpers import _oracle_counts, sp  # noqa: F401
from surel_plus_amd import _lib, spjoin
from surel_plus_amd._lib import JOIN_COUNTS, JOIN_PAIRS, JOIN_SFPTR, check, join_fill, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

N, T, MAX_LEN = 16, 8, 8
LENS = [8, 7, 0, 1, 8, 3, 5, 1, 0, 2, 4, 6, 7, 8, 3, 5]
# (longer, shorter), (shorter, longer), equal lengths, (empty, .), (., empty), (u, u)
EDGE = np.array([[0, 3, 0, 2, 6, 13],
                 [5, 1, 4, 12, 8, 13]], np.int64)
B = EDGE.shape[1]
FITS_7 = [1, 3, 4]                  # the pairs whose rows both have at most 7 members
# segment j of the list in two mirrored blocks of 3 pairs, [u0 u1 u2 | v0 v1 v2 | u3 u4 u5 | v3 v4 v5], in the one-block list
BLOCKS_OF_3 = [0, 1, 2, 6, 7, 8, 3, 4, 5, 9, 10, 11]
W_TOL = 1e-5                        # test_w_is_the_softmax_weighted_count_of_the_index_pairs


@pytest.fixture(scope="module")
def store(sp):
    """(z, its row fields for a descriptor, the host arrays for the oracle): tests/test_gpu_stage_shapes.py's _lp_store with the row
    lengths given -- sorted, unique ids over a span of 14, SFptr in [1, T)"""
    rs = np.random.default_rng(8)
    indptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    ids = np.concatenate([np.sort(rs.choice(14, n, replace=False)) for n in LENS]).astype(np.int32)
    data = rs.integers(1, T, ids.size).astype(np.int32)
    z = spm.SpG(torch.from_numpy(indptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(data).cuda(), max_len=MAX_LEN,
                shape=(N, 14))
    assert {0, 1, MAX_LEN - 1, MAX_LEN} <= set(LENS) and max(LENS) == MAX_LEN
    return z, z.join_rows()[1], (indptr, ids, data)


def _lists(blocks_of_3=False):
    u, v = torch.from_numpy(EDGE[0]).cuda(), torch.from_numpy(EDGE[1]).cuda()
    if blocks_of_3:
        return torch.cat([u[:3], v[:3], u[3:], v[3:]]).contiguous(), torch.cat([v[:3], u[:3], v[3:], u[3:]]).contiguous(), 3
    return torch.cat([u, v]).contiguous(), torch.cat([v, u]).contiguous(), B


def _both_segments(pairs):
    return [j for p in pairs for j in (p, p + B)]


# ------------------------------------------------------------------------------------------------ the three forms, status unchecked
def _count_form(rows, own, partner, pb):
    out = torch.full((own.numel(), T), -1.0, dtype=torch.float32, device="cuda")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda")
    join_fill(JOIN_COUNTS, JOIN_SFPTR, **rows, own=own, partner=partner, S=own.numel(), pair_block=pb, table_rows=T, out_counts=out,
              flags=flags)
    return out.cpu().numpy(), int(flags[3].item())


def _pair_form(rows, own, partner, pb):
    """-> per segment its (pa, pb, multiplicity) rows sorted, and the status word"""
    S, L, st = own.numel(), lib(), stream_ptr()
    seg, flags = spjoin._seg_and_flags(S, own.device)
    ws = torch.empty(L.subgacc_sjoin_workspace_bytes(S), dtype=torch.uint8, device="cuda")
    check(L.subgacc_sjoin_sizes(ptr(rows["row_off"]), rows["n_rows"], ptr(own), ptr(partner), S, ptr(seg), ptr(flags), ptr(ws), ws.numel(),
                                st))
    R = int(seg[S].item())
    pairs = torch.zeros((R, 2), dtype=torch.int32, device="cuda")
    mult = torch.zeros(R, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    join_fill(JOIN_PAIRS, JOIN_SFPTR, st, **rows, own=own, partner=partner, S=S, seg=seg, pair_block=pb, out_pairs=pairs, out_mult=mult,
              out_cnt=cnt, flags=flags)
    seg, cnt, pairs, mult = (t.cpu().numpy() for t in (seg, cnt, pairs, mult))
    out = []
    for j in range(S):
        r = np.column_stack([pairs[seg[j]:seg[j] + cnt[j]], mult[seg[j]:seg[j] + cnt[j]]])
        out.append(r[np.lexsort((r[:, 1], r[:, 0]))])
    return out, int(flags[3].item())


class _AttnJoin(spjoin._CountsAttnJoin):
    """the stage's own join object with descriptor fields of the test's choosing (partner, pair_block, max_len)"""

    def __init__(self, z, rows, own, n_pairs, **fields):
        super().__init__(z, rows, own, n_pairs, T)
        self.fields = fields

    def desc(self):
        f = dict(self.rows, own=self.own, S=2 * self.B, pair_block=self.B, table_rows=self.T, flags=self.flags)
        f.update(self.fields)
        return _lib.join_desc(JOIN_COUNTS, JOIN_SFPTR, **f)


def _g():
    return torch.randn(T, device="cuda", generator=torch.Generator("cuda").manual_seed(3))


def _w_from_pair_rows(segments, g):
    """W [S, T] in float64 from every segment's distinct pairs and multiplicities: alpha = softmax of g[p] + g[q] over the segment's rows"""
    g = g.double().cpu().numpy()
    W = np.zeros((len(segments), T))
    for j, r in enumerate(segments):
        if len(r) == 0:
            continue
        lo = g[r[:, 0]] + g[r[:, 1]]
        e = r[:, 2] * np.exp(lo - lo.max())
        alpha = e / e.sum()
        np.add.at(W[j], r[:, 0], alpha)
        np.add.at(W[j], r[:, 1], alpha)
    return W


# ------------------------------------------------------------------------------------------------ the reference, computed once
@pytest.fixture(scope="module")
def truth(store):
    """the oracle's count rows C [2B, T] and per segment its sorted (pa, pb, multiplicity) rows"""
    z, rows, host = store
    C, sizes = _oracle_counts(host, EDGE, T)
    own, partner = oracle.pair_segments(EDGE)
    oseg, opairs = oracle.sjoin(*host, own, partner)
    want = []
    for j in range(2 * B):
        p, m = np.unique(opairs[oseg[j]:oseg[j + 1]], axis=0, return_counts=True)
        want.append(np.column_stack([p, m]).astype(np.int32).reshape(-1, 3))
    assert list(sizes) == [LENS[r] for r in np.concatenate([EDGE[0], EDGE[1]])]
    return C, want


def _same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("blocks_of_3", [False, True])
def test_count_and_pair_forms_equal_the_oracle(store, truth, blocks_of_3):
    z, rows, host = store
    C, want = truth
    own, partner, pb = _lists(blocks_of_3)
    order = BLOCKS_OF_3 if blocks_of_3 else list(range(2 * B))
    got_c, st_c = _count_form(rows, own, partner, pb)
    got_p, st_p = _pair_form(rows, own, partner, pb)
    assert st_c == 0 and st_p == 0
    assert np.array_equal(got_c, C[order])
    assert _same_rows(got_p, [want[j] for j in order])


@pytest.mark.parametrize("blocks_of_3", [False, True])
def test_attention_form_equals_the_softmax_of_the_pair_rows(store, blocks_of_3):
    z, rows, host = store
    own, partner, pb = _lists(blocks_of_3)
    g = _g()
    segments, st_p = _pair_form(rows, own, partner, pb)
    W, mx, den = _AttnJoin(z, rows, own, B, pair_block=pb).forward(g, True)
    assert st_p == 0
    want = _w_from_pair_rows(segments, g)
    assert float(np.abs(W.double().cpu().numpy() - want).max()) <= W_TOL
    n = np.array([LENS[r] for r in own.cpu().numpy()])
    assert not bool(W[torch.from_numpy(n == 0).cuda()].any())
    assert float((W.double().sum(1).cpu().numpy()[n > 0] - 2).max()) <= W_TOL


def test_a_list_that_is_not_mirrored_is_refused(store):
    z, rows, host = store
    own, partner, pb = _lists()
    assert _count_form(rows, own, own, pb)[1] & 4
    assert _pair_form(rows, own, own, pb)[1] & 4
    j = _AttnJoin(z, rows, own, B, partner=own)
    j.forward(_g(), False)
    assert int(j.flags[3].item()) & 4


def test_a_row_longer_than_max_len_is_refused_and_the_other_pairs_are_joined(store, truth):
    z, rows, host = store
    C, want = truth
    own, partner, pb = _lists()
    short = dict(rows, max_len=MAX_LEN - 1)
    keep = _both_segments(FITS_7)
    got_c, st_c = _count_form(short, own, partner, pb)
    assert st_c & 1 and np.array_equal(got_c[keep], C[keep])
    got_p, st_p = _pair_form(short, own, partner, pb)
    assert st_p & 1 and _same_rows([got_p[j] for j in keep], [want[j] for j in keep])
    g = _g()
    j = _AttnJoin(z, short, own, B)
    with pytest.raises(_lib.SubgAccError, match="SpG row longer than SpG.max_len"):
        j.forward(g, False)
    assert int(j.flags[3].item()) & 1
    W = torch.zeros((2 * B, T), dtype=torch.float32, device="cuda")
    d = j.desc()
    check(lib().subgacc_sjoin_counts_attn(ctypes.byref(d), ptr(g), ptr(W), ptr(None), ptr(None), stream_ptr()))
    full = _AttnJoin(z, rows, own, B).forward(g, False)[0]
    assert torch.equal(W[keep], full[keep])

"""GPU (MI355X): the join's rows in fp16 / bf16 (subgacc_sjoin_fill_half, include/subgacc_half.h; sjoin / gather / sample_and_gather /
StepBuffers with dtype=).  Every reference is the f32 row form (subgacc_sjoin_fill_v2, the f32 Python path) followed by torch's
.to(dtype); the rows are compared bit for bit (view(torch.int16)), segment pointers and status words exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import sp  # noqa: F401
from test_gpu_horder import M, World
from test_gpu_step_stage import LENS, STRIDE, Rows, _lp_keys

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
# (num_walks, hops): k = 3, 4, 5 -- rows of 12, 16 and 20 bytes
SHAPES = [pytest.param(200, 2, id="k3"), pytest.param(200, 3, id="k4"), pytest.param(100, 4, id="k5")]
RIM = 64                    # int16 words of poison in front of and behind the output (128 bytes: the rows stay 16-byte aligned)
BEHIND = 40                 # rows of poison behind row R
POISON = 0x7C7C


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------- 1, 2. the kernel through the C ABI
class KeyJoin:
    """one mirrored list over synthetic strided key rows: the size pass once, then the f32 fill and the 16-bit fill over the same
    rows and the same seg, each with status words of its own that the size pass has written first"""

    def __init__(self, rows, num_walks, hops, partner):
        from surel_plus_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.ids, self.keys, self.nsize = rows.device()
        self.own = torch.from_numpy(np.concatenate([rows.a, rows.b])).cuda()
        self.par = torch.from_numpy(np.concatenate([rows.b, rows.a])).cuda() if partner else None
        self.S, self.k, self.rows, self.M, self.hops = self.own.numel(), hops + 1, rows, num_walks, hops

    def sizes(self):
        _lib, L = self.lib, self.L
        seg = torch.full((self.S + 1,), -1, dtype=torch.int64, device="cuda")
        flags = torch.zeros(4, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(self.S), 8), dtype=torch.uint8, device="cuda")
        _lib.check(L.subgacc_sjoin_sizes_rows(_lib.ptr(self.nsize), self.rows.n, _lib.ptr(self.own), _lib.ptr(self.par), self.S, _lib.ptr(seg),
                                              _lib.ptr(flags), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
        return seg, flags

    def fields(self, seg, flags):
        return dict(row_len=self.nsize, n_rows=self.rows.n, row_stride=self.rows.stride, ids=self.ids, payload=self.keys, own=self.own,
                    partner=self.par, S=self.S, seg=seg, pair_block=self.S // 2, flags=flags, num_walks=self.M, num_steps=self.hops)

    def f32(self):
        seg, flags = self.sizes()
        R = int(seg[-1].item())
        xz = torch.full((R, 2, self.k), -7.0, dtype=torch.float32, device="cuda")
        self.lib.join_fill(self.lib.JOIN_ROWS, self.lib.JOIN_KEY32, out_xz=xz, **self.fields(seg, flags))
        torch.cuda.synchronize()
        return xz, seg, flags

    def half(self, dtype):
        """-> (rows [R, 2, k] of dtype, seg, flags); the rims and the rows behind R are checked here"""
        _lib = self.lib
        seg, flags = self.sizes()
        R = int(seg[-1].item())
        n = R * 2 * self.k
        buf = torch.full((RIM + n + BEHIND * 2 * self.k + RIM,), POISON, dtype=torch.int16, device="cuda")
        out = buf[RIM:]
        assert out.data_ptr() % 16 == 0
        d = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY32, **self.fields(seg, flags))
        code = {torch.float16: _lib.HALF_F16, torch.bfloat16: _lib.HALF_BF16}[dtype]
        _lib.check(self.L.subgacc_sjoin_fill_half(C.byref(d), code, _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((buf[:RIM] == POISON).all()) and bool((buf[RIM + n:] == POISON).all())      # nothing outside the R rows
        return buf[RIM: RIM + n].view(dtype).view(R, 2, self.k), seg, flags


# both types with the partner list derived from the mirror (gather's form), one of them with the list given as well
@pytest.mark.parametrize("dtype,partner", [pytest.param(torch.bfloat16, False, id="bf16"), pytest.param(torch.float16, False, id="fp16"),
                                           pytest.param(torch.bfloat16, True, id="bf16-partner-given")])
@pytest.mark.parametrize("num_walks,hops", SHAPES)
def test_kernel_equals_the_f32_fill_rounded(sp, num_walks, hops, dtype, partner):
    """rows of LENS (0, 1, 255 .. 513, a full stride), a disjoint and a fully overlapping pair, every row with itself and with its
    neighbour: bit for bit the f32 rows .to(dtype), flags zero, nothing written outside the R rows, the same bits on a second call"""
    keyset = _lp_keys(300, 11 + hops, M=num_walks, hops=hops, shift=int(num_walks).bit_length())
    j = KeyJoin(Rows(keyset, 23 + hops), num_walks, hops, partner)
    ref, rseg, rflags = j.f32()
    assert ref.shape[0] == int(j.rows.len[np.concatenate([j.rows.a, j.rows.b])].sum()) > 2 * sum(LENS) and STRIDE in j.rows.len
    want = ref.to(dtype)
    # the reference values round in both directions and some are exact: a kernel that truncates cannot pass
    back = want.float()
    assert bool((back > ref).any()) and bool((back < ref).any()) and bool(((back == ref) & (ref > 0) & (ref < 1)).any())
    got, seg, flags = j.half(dtype)
    assert torch.equal(seg, rseg)
    assert _same_bits(got, want)
    assert not flags.any() and not rflags.any()
    again, _, _ = j.half(dtype)
    assert _same_bits(again, want)


EDGE_LENS = (0, 1, 127, 128, 129, 255, 256, 257, 511, 512, 513, STRIDE)


@pytest.mark.parametrize("pairs", [pytest.param(2048, id="2048-pairs-256-lanes"), pytest.param(2049, id="2049-pairs-128-lanes")])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks,hops", SHAPES)
def test_both_workgroup_sizes(sp, num_walks, hops, dtype, pairs):
    """a batch of at most 2,048 pairs takes 256 lanes per pair, a larger one 128 (csrc/sjoin_half.hip: half_threads); either prefetches
    512 members of the searched row, in two trips or in four: rows at every trip's edge and beyond the last, each with itself and
    with its neighbour, the list repeated up to the number of pairs"""
    keyset = _lp_keys(200, 31 + hops, M=num_walks, hops=hops, shift=int(num_walks).bit_length())
    base = Rows(keyset, 41 + hops, lens=EDGE_LENS)
    reps = -(-pairs // len(base.a))
    rows = Rows(keyset, 41 + hops, lens=EDGE_LENS, pairs=(np.tile(base.a, reps)[:pairs], np.tile(base.b, reps)[:pairs]))
    j = KeyJoin(rows, num_walks, hops, False)
    assert j.S == 2 * pairs
    ref, rseg, rflags = j.f32()
    got, seg, flags = j.half(dtype)
    assert torch.equal(seg, rseg) and not flags.any() and not rflags.any()
    assert _same_bits(got, ref.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks,hops", SHAPES)
def test_a_row_outside_the_store_is_an_empty_row(sp, num_walks, hops, dtype):
    """one pair whose second row number is n_rows: the same status words, the same seg and the same rows as the f32 call on that list"""
    keyset = _lp_keys(40, 5, M=num_walks, hops=hops, shift=int(num_walks).bit_length())
    rows = Rows(keyset, 6, lens=(70, 300, 9), pairs=([0, 1, 2], [1, 3, 2]))
    assert rows.n == 3
    j = KeyJoin(rows, num_walks, hops, False)
    ref, rseg, rflags = j.f32()
    got, seg, flags = j.half(dtype)
    assert int(rflags[3].item()) & 16 and torch.equal(flags, rflags) and torch.equal(seg, rseg)
    assert ref.shape[0] == 70 + 300 + 9 + 300 + 0 + 9
    assert _same_bits(got, ref.to(dtype))


# ------------------------------------------------------------------------------------------------------------- 3. resident stores
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hops", [2, 3])
def test_gather_over_resident_stores(sp, world, hops, dtype):
    """the packed SFptr store with its Z_SF table and the same store keyed: the isolated root, hubs, star centres and u == v"""
    z, table, _ = world.store(hops)
    e = world.pairs(300, 1)
    ref, rind = sp.gather(e, z, encode=table)
    want = ref.to(dtype)
    enc = torch.round(table.double() * M).to(torch.int64)              # the integer LP rows: Z_SF is count / M, column 0 = M / M
    zk = z.keyed(enc, M)
    kref, kind = sp.gather(e, zk, encode=zk.slot_table())
    assert torch.equal(kref, ref) and torch.equal(kind, rind)
    for store, encode in ((z, table), (zk, zk.slot_table())):
        xz, ind = sp.gather(e, store, encode=encode, dtype=dtype)
        assert xz.dtype == dtype and torch.equal(ind, rind) and _same_bits(xz, want)
        buf = torch.full((want.numel() + 64,), -3.0, dtype=dtype, device="cuda")
        bxz, bind = sp.gather(e, store, encode=encode, out=buf, dtype=dtype)
        assert bxz.data_ptr() == buf.data_ptr() and torch.equal(bind, rind) and _same_bits(bxz, want)
        assert bool((buf[want.numel():] == -3.0).all())
        with pytest.raises(ValueError, match="out= must be a contiguous"):          # out= is a tensor of the dtype
            sp.gather(e, store, encode=encode, out=torch.empty(want.numel(), dtype=torch.float32, device="cuda"), dtype=dtype)
    # dtype=torch.float32 is today's path
    fxz, find = sp.gather(e, z, encode=table, dtype=torch.float32)
    assert torch.equal(fxz, ref) and torch.equal(find, rind)


# ------------------------------------------------------------------------------------------------------------ 4. the on-demand step
@pytest.mark.parametrize("dedup", [False, True], ids=["all-roots", "dedup-roots"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_on_demand_step(sp, world, dtype, dedup):
    csr, B = world.csr, 300
    e1, e2 = world.pairs(B, 1), world.pairs(B, 2)
    kw = dict(num_walks=M, num_steps=3, seed=5, dedup_roots=dedup)
    refs = [sp.sample_and_gather(csr, e, **kw)[:2] for e in (e1, e2)]
    xz, ind, _ = sp.sample_and_gather(csr, e1, dtype=dtype, **kw)
    assert xz.dtype == dtype and torch.equal(ind, refs[0][1]) and _same_bits(xz, refs[0][0].to(dtype))
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=3, dedup_roots=dedup, dtype=dtype)
    plain = sp.StepBuffers(csr, B, num_walks=M, num_steps=3, dedup_roots=dedup)
    assert bufs.out.dtype == dtype and plain.out.dtype == torch.float32
    assert 2 * bufs.out.numel() * bufs.out.element_size() == plain.out.numel() * plain.out.element_size()
    for e, (rxz, rind) in zip((e1, e2), refs):                      # a second batch through the same buffers
        bxz, bind, sets = sp.sample_and_gather(csr, e, buffers=bufs, dtype=dtype, **kw)
        sets.resolve()
        R = int(bind[-1].item())
        assert bxz.dtype == dtype and bxz.data_ptr() == bufs.out.data_ptr()
        assert torch.equal(bind, rind) and R == rxz.shape[0] and _same_bits(bxz[:R], rxz.to(dtype))
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, e1, buffers=bufs, **kw)
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, e1, buffers=plain, dtype=dtype, **kw)

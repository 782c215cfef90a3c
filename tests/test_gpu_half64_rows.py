"""GPU (MI355X): the join's rows in fp16 / bf16 over 64-bit key rows (subgacc_sjoin_fill_half64, include/subgacc_half64.h; sjoin /
gather / sample_and_gather / StepBuffers with dtype= and wide_keys=True).  Every reference is the f32 row form over the same rows
(subgacc_sjoin_fill_v2 with payload KEY64, the f32 Python path) followed by torch's .to(dtype); the rows are compared bit for bit
(view(torch.int16)), segment pointers and all four status words exactly.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_helpers import sp  # noqa: F401
from test_gpu_horder import World

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")]
STRIDE = 544                # int32 / int64 words between two rows (a multiple of 32); one row fills it
# every edge of the two prefetch trips of a workgroup's 256 lanes and of its 64-lane waves below them, beyond the last trip (512
# members), the empty row and a full stride
LENS = (0, 1, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, STRIDE)
# (num_walks, hops) -> k = hops + 1, shift = bit_length(num_walks), key bits = hops * shift + 1
SHAPES = [pytest.param(200, 4, id="M200-k5-33bits"), pytest.param(128, 4, id="M128-k5-33bits"), pytest.param(204, 4, id="M204-k5-33bits"),
          pytest.param(32767, 4, id="M32767-k5-61bits-division"), pytest.param(2047, 3, id="M2047-k4-34bits"),
          pytest.param(65535, 2, id="M65535-k3-33bits"), pytest.param(100, 4, id="M100-k5-29bits-narrow-key-stored-wide")]
# one shape per k specialisation of the launcher (k = 2: one hop, whose key never needs more than 32 bits -- stored wide)
K_SHAPES = [pytest.param(65535, 1, id="k2"), pytest.param(65535, 2, id="k3"), pytest.param(2047, 3, id="k4"), pytest.param(200, 4, id="k5")]
RIM = 64                    # int16 words of poison in front of and behind the output (128 bytes: the rows stay 16-byte aligned)
BEHIND = 40                 # rows of poison behind row R
POISON = 0x7C7C
KEY_POISON = 0x7FFFFFFF7FFFFFFF      # what stands behind a row's members: never read
UNWRITTEN = -7.0            # what the f32 reference buffer holds where the fill wrote nothing


def _shift(num_walks):
    return int(num_walks).bit_length()


def lp_keys64(count, seed, M, hops):
    """`count` distinct valid LP keys of (M, hops) as uint64: `hops` counts of `shift` bits, a quarter of them with the root's LEAD bit at
    hops * shift; among them the key of all counts M with the lead bit (every field full), M // 2 and M // 4 in every field (exact in
    either 16-bit type when M is a multiple of four) and the key whose only count is a 1 in the top field"""
    rng = np.random.default_rng(seed)
    shift = _shift(M)

    def pack(counts, lead):
        k = 0
        for v in counts:
            k = (k << shift) | int(v)
        return k | (int(lead) << (hops * shift))

    keys = {pack([M] * hops, True), pack([M // 2] * hops, False), pack([M // 4] * hops, False), pack([1] + [0] * (hops - 1), False)}
    while len(keys) < count:
        k = pack(rng.integers(0, M + 1, hops), rng.integers(0, 4) == 0)
        if k:
            keys.add(k)
    return np.array(sorted(keys), dtype=np.uint64)


class Rows64:
    """strided rows of 64-bit keys built on the host: ids (int32) ascend inside a row, keys (int64) are drawn from `keyset` and every
    key of the set stands somewhere.  One row of random ids per entry of `lens`; with extras=True a disjoint pair (even against odd
    ids) and a fully overlapping pair (the same ids, other keys) follow.  The list (a, b): every row with itself and with its
    neighbour, the two extra pairs, and the empty row with itself and with the longest row -- or `pairs`."""

    def __init__(self, keyset, seed, lens=LENS, stride=STRIDE, pairs=None, extras=True):
        rng = np.random.default_rng(seed)
        self.stride = stride
        rows = [np.sort(rng.choice(4000, L, replace=False)) for L in lens]
        if extras:
            rows += [np.arange(0, 600, 2), np.arange(1, 601, 2)]
            same = np.sort(rng.choice(4000, 513, replace=False))
            rows += [same, same.copy()]
        self.n = len(rows)
        self.ids = np.full((self.n, stride), -1, dtype=np.int32)
        self.keys = np.full((self.n, stride), KEY_POISON, dtype=np.uint64)
        self.len = np.array([len(r) for r in rows], dtype=np.int32)
        at = 0
        for i, r in enumerate(rows):
            k = keyset[rng.integers(0, len(keyset), len(r))]
            take = min(len(r), len(keyset) - at)
            k[:take] = keyset[at: at + take]
            at += take
            self.ids[i, : len(r)], self.keys[i, : len(r)] = r, k
        assert at == len(keyset)
        if pairs is not None:
            a, b = pairs
        else:
            a = list(range(self.n)) + list(range(self.n))
            b = list(range(self.n)) + [(i + 1) % self.n for i in range(self.n)]
            if extras:
                e = len(lens)
                a, b = a + [e, e + 2, 0, 0], b + [e + 1, e + 3, 0, int(np.argmax(self.len))]
        self.a, self.b = np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)

    def device(self):
        return (torch.from_numpy(self.ids.reshape(-1)).cuda(), torch.from_numpy(self.keys.view(np.int64).reshape(-1)).cuda(),
                torch.from_numpy(self.len).cuda())


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


class KeyJoin64:
    """one mirrored list over synthetic strided rows of 64-bit keys: the size pass once per call, then the f32 fill (KEY64) or the 16-bit
    fill over the same rows and the same seg, each with status words of its own that the size pass has written first"""

    def __init__(self, rows, num_walks, hops, partner):
        from surel_plus_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.ids, self.keys, self.nsize = rows.device()
        self.own = torch.from_numpy(np.concatenate([rows.a, rows.b])).cuda()
        if partner is True:
            partner = np.concatenate([rows.b, rows.a])
        self.par = None if partner is False else torch.from_numpy(partner).cuda()
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
        xz = torch.full((R, 2, self.k), UNWRITTEN, dtype=torch.float32, device="cuda")
        self.lib.join_fill(self.lib.JOIN_ROWS, self.lib.JOIN_KEY64, out_xz=xz, **self.fields(seg, flags))
        torch.cuda.synchronize()
        return xz, seg, flags

    def half(self, dtype):
        """-> (rows [R, 2, k] as int16 bits, seg, flags); the rims and the rows behind R are checked here"""
        _lib = self.lib
        seg, flags = self.sizes()
        R = int(seg[-1].item())
        n = R * 2 * self.k
        buf = torch.full((RIM + n + BEHIND * 2 * self.k + RIM,), POISON, dtype=torch.int16, device="cuda")
        out = buf[RIM:]
        assert out.data_ptr() % 16 == 0
        d = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY64, **self.fields(seg, flags))
        code = {torch.float16: _lib.HALF_F16, torch.bfloat16: _lib.HALF_BF16}[dtype]
        _lib.check(self.L.subgacc_sjoin_fill_half64(C.byref(d), code, _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert bool((buf[:RIM] == POISON).all()) and bool((buf[RIM + n:] == POISON).all())      # nothing outside the R rows
        return buf[RIM: RIM + n].view(R, 2, self.k), seg, flags


def _bits(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------- 1. the kernel through the C ABI
def _check_keys(keyset, num_walks, hops):
    """what the key set must hold for a kernel that looks at 32 bits, drops the top field or the lead bit to fail"""
    shift, mask = _shift(num_walks), (1 << _shift(num_walks)) - 1
    ks = [int(k) for k in keyset]
    bits = hops * shift + 1
    assert any(k >= 1 << 32 for k in ks) == (bits > 32)                   # (a key of 29 bits stored wide has none)
    assert any((k >> ((hops - 1) * shift)) & mask for k in ks)            # the top count field
    assert any((k >> (hops * shift)) & 1 for k in ks) and not all((k >> (hops * shift)) & 1 for k in ks)      # the lead bit
    assert all(k < 1 << bits and all(((k >> (c * shift)) & mask) <= num_walks for c in range(hops)) for k in ks)


@pytest.mark.parametrize("partner", [pytest.param(False, id="partner-from-mirror"), pytest.param(True, id="partner-given")])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks,hops", SHAPES)
def test_kernel_equals_the_f32_fill_rounded(sp, num_walks, hops, dtype, partner):
    """rows of LENS, a disjoint and a fully overlapping pair, every row with itself and with its neighbour: bit for bit the f32 rows
    .to(dtype), flags zero, nothing written outside the R rows, the same bits on a second call"""
    keyset = lp_keys64(300, 11 + hops, num_walks, hops)
    _check_keys(keyset, num_walks, hops)
    j = KeyJoin64(Rows64(keyset, 23 + hops), num_walks, hops, partner)
    ref, rseg, rflags = j.f32()
    assert ref.shape[0] == int(j.rows.len[np.concatenate([j.rows.a, j.rows.b])].sum()) > 2 * sum(LENS) and STRIDE in j.rows.len
    assert not bool((ref == UNWRITTEN).any())
    want = ref.to(dtype)
    # the reference values round in both directions and some are exact: a kernel that truncates cannot pass.  (Strictly inside (0, 1)
    # a count over num_walks is exact in 16 bits only where it is a short dyadic fraction -- M // 4 and M // 2 over a num_walks that is
    # a multiple of four; an odd num_walks divides no such count, there the exact values are the flag and the full count, 1.0)
    # Two shapes cannot round both ways, by arithmetic.  num_walks = 128: every count / 128 has at most eight significant bits and is
    # exact in either type.  num_walks = 2047 in fp16 (11 significant bits): c / 2047 = (c / 2048)(1 + 1/2047) with c / 2048 exact, and
    # the excess c / 2047 of a count in [2^j, 2^(j+1)) is between a half and a whole unit 2^(j-10) of its last place: always up.
    back = want.float()
    if num_walks == 128:
        assert bool((back == ref).all())
    else:
        assert bool((back > ref).any()) and (bool((back < ref).any()) or (num_walks == 2047 and dtype == torch.float16))
    assert bool(((back == ref) & (ref > 0)).any())
    assert num_walks % 4 or bool(((back == ref) & (ref > 0) & (ref < 1)).any())
    got, seg, flags = j.half(dtype)
    assert torch.equal(seg, rseg)
    assert torch.equal(got, _bits(want))
    assert not flags.any() and not rflags.any()
    again, _, _ = j.half(dtype)
    assert torch.equal(again, _bits(want))


# ------------------------------------------------------------------------------------- 2. every dispatch branch of the launcher
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks,hops", K_SHAPES)
def test_every_row_width(sp, num_walks, hops, dtype, pairs=2049):
    """the launcher's only choice is the kernel of k = 2 .. 5 and of the type (csrc/sjoin_half64.hip: launch_half64; one workgroup size
    at every batch): each of the eight over a batch of more pairs than the chip holds workgroups at once.  The kernel prefetches 512
    members of the searched row in two trips: rows at every trip's edge and beyond the last, each with itself and with its neighbour,
    the list repeated up to the number of pairs"""
    keyset = lp_keys64(200, 31 + hops, num_walks, hops)
    base = Rows64(keyset, 41 + hops, extras=False)
    reps = -(-pairs // len(base.a))
    rows = Rows64(keyset, 41 + hops, extras=False, pairs=(np.tile(base.a, reps)[:pairs], np.tile(base.b, reps)[:pairs]))
    j = KeyJoin64(rows, num_walks, hops, False)
    assert j.S == 2 * pairs
    ref, rseg, rflags = j.f32()
    got, seg, flags = j.half(dtype)
    assert torch.equal(seg, rseg) and not flags.any() and not rflags.any()
    assert not bool((ref == UNWRITTEN).any()) and torch.equal(got, _bits(ref.to(dtype)))


# ----------------------------------------------------------------------------------------------------------- 3. the status words
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks,hops", K_SHAPES)
def test_a_row_outside_the_store_is_an_empty_row(sp, num_walks, hops, dtype):
    """one pair whose second row number is n_rows: the same status words, the same seg and the same rows as the f32 call on that list"""
    keyset = lp_keys64(40, 5, num_walks, hops)
    rows = Rows64(keyset, 6, lens=(70, 300, 9), extras=False, pairs=([0, 1, 2], [1, 3, 2]))
    assert rows.n == 3
    j = KeyJoin64(rows, num_walks, hops, False)
    ref, rseg, rflags = j.f32()
    got, seg, flags = j.half(dtype)
    assert int(rflags[3].item()) & 16 and torch.equal(flags, rflags) and torch.equal(seg, rseg)
    assert ref.shape[0] == 70 + 300 + 9 + 300 + 0 + 9
    assert torch.equal(got, _bits(ref.to(dtype)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks,hops", K_SHAPES)
def test_a_list_that_is_not_mirrored_sets_bit_4_and_skips_the_pair(sp, num_walks, hops, dtype):
    """a partner list given with one entry of the second block changed: that pair is skipped by the f32 fill and by the 16-bit fill --
    neither writes its two segments' rows -- the status words and seg are the same, and so is every other row"""
    keyset = lp_keys64(40, 7, num_walks, hops)
    rows = Rows64(keyset, 8, lens=(70, 300, 9, 130), extras=False, pairs=([0, 1, 2, 3], [1, 2, 3, 0]))
    partner = np.concatenate([rows.b, rows.a])
    P, broken = 4, 1
    partner[P + broken] = 3                      # the mirror of pair 1 = (1, 2) should name row 1
    j = KeyJoin64(rows, num_walks, hops, partner)
    ref, rseg, rflags = j.f32()
    got, seg, flags = j.half(dtype)
    assert int(rflags[3].item()) & 4 and torch.equal(flags, rflags) and torch.equal(seg, rseg)
    s = rseg.tolist()
    skipped = torch.zeros(ref.shape[0], dtype=torch.bool, device="cuda")
    for jj in (broken, P + broken):
        assert s[jj + 1] > s[jj]
        skipped[s[jj]: s[jj + 1]] = True
    assert bool((ref[skipped] == UNWRITTEN).all()) and not bool((ref[~skipped] == UNWRITTEN).any())
    assert bool((got[skipped] == POISON).all())
    assert torch.equal(got[~skipped], _bits(ref[~skipped].to(dtype)))


# ------------------------------------------------------------------------------------------------------------ 4. the on-demand step
B = 64
WIDE_M = [pytest.param(128, id="M128"), pytest.param(200, id="M200"), pytest.param(204, id="M204")]


@pytest.fixture(scope="module")
def world(sp):
    return World(sp)


def _with_out_edges(world, e):
    """the pairs with every endpoint that has no out-edge replaced by hub 0 (the rand_r stream of a buffered step has no dead ends)"""
    deg = torch.from_numpy(np.diff(world.indptr)).cuda()
    return torch.where(deg[e] > 0, e, torch.zeros_like(e))


VARIANTS = [pytest.param("plain", id="plain"), pytest.param("dedup", id="dedup-roots"), pytest.param("order", id="locality-order"),
            pytest.param("rand_r", id="rand_r"), pytest.param("out", id="out-given")]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks", WIDE_M)
def test_the_buffered_step(sp, world, num_walks, dtype, variant):
    """StepBuffers(dtype=, wide_keys=True) + sample_and_gather(buffers=) against the f32 buffered step of the same settings: the same
    indptr, the f32 rows .to(dtype) bit for bit -- two consecutive steps with different seeds on one set of buffers"""
    csr, k = world.csr, 5
    made = dict(num_walks=num_walks, num_steps=4)
    call = dict(made)
    if variant == "dedup":
        made["dedup_roots"] = call["dedup_roots"] = True
    if variant == "order":
        made["order"] = sp.locality_order(csr)
    if variant == "rand_r":
        made["rng"] = call["rng"] = "rand_r"
    worst = 2 * B * (num_walks * 4 + 1) * 2 * k
    outs = {}
    if variant == "out":
        outs = {"f32": torch.full((worst + 64,), -3.0, dtype=torch.float32, device="cuda"),
                "half": torch.full((worst + 64,), -3.0, dtype=dtype, device="cuda")}
    plain = sp.StepBuffers(csr, B, **made, out=outs.get("f32"))
    bufs = sp.StepBuffers(csr, B, **made, dtype=dtype, wide_keys=True, out=outs.get("half"))
    assert bufs.out.element_size() == 2 and bufs.out.dtype == dtype and bufs.slot.dtype == torch.int64 and plain.slot.dtype == torch.int64
    assert bufs.half64 and not bufs.wide and not plain.half64 and bufs.key64
    assert 2 * bufs.out.numel() * bufs.out.element_size() == plain.out.numel() * plain.out.element_size()
    for seed, pseed in ((5, 1), (6, 2)):
        e = world.pairs(B, pseed)
        if variant == "rand_r":
            e = _with_out_edges(world, e)
        rxz, rind, rsets = sp.sample_and_gather(csr, e, buffers=plain, seed=seed, **call)
        rsets.resolve()
        bxz, bind, sets = sp.sample_and_gather(csr, e, buffers=bufs, seed=seed, dtype=dtype, wide_keys=True, **call)
        sets.resolve()
        R = int(bind[-1].item())
        assert bxz.dtype == dtype and bxz.data_ptr() == bufs.out.data_ptr() and R > 0
        assert torch.equal(bind, rind) and _same_bits(bxz[:R], rxz[:R].to(dtype))
        assert torch.equal(bufs.status, plain.status)
    if variant == "out":
        assert bufs.out.data_ptr() == outs["half"].data_ptr() and bool((outs["half"][worst:] == -3.0).all())
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, e, buffers=bufs, seed=5, **call)
    with pytest.raises(ValueError, match="buffers= were made with dtype"):
        sp.sample_and_gather(csr, e, buffers=plain, seed=5, dtype=dtype, wide_keys=True, **call)


@pytest.mark.parametrize("dedup", [False, True], ids=["all-roots", "dedup-roots"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_walks", WIDE_M)
def test_the_unbuffered_step(sp, world, num_walks, dtype, dedup):
    """sample_and_gather(dtype=, wide_keys=True) without buffers -- through sjoin, and with dedup_roots=True through gather -- gives the
    bits of the f32 call .to(dtype), with the same indptr; out= is a buffer of the dtype"""
    csr = world.csr
    e = world.pairs(B, 3)
    kw = dict(num_walks=num_walks, num_steps=4, seed=5, dedup_roots=dedup)
    rxz, rind, _ = sp.sample_and_gather(csr, e, **kw)
    xz, ind, _ = sp.sample_and_gather(csr, e, dtype=dtype, wide_keys=True, **kw)
    assert xz.dtype == dtype and xz.shape == rxz.shape and rxz.shape[0] > 0
    assert torch.equal(ind, rind) and _same_bits(xz, rxz.to(dtype))
    buf = torch.full((rxz.numel() + 64,), -3.0, dtype=dtype, device="cuda")
    oxz, oind, _ = sp.sample_and_gather(csr, e, dtype=dtype, wide_keys=True, out=buf, **kw)
    assert oxz.data_ptr() == buf.data_ptr() and torch.equal(oind, rind) and _same_bits(oxz, rxz.to(dtype))
    assert bool((buf[rxz.numel():] == -3.0).all())
    with pytest.raises(ValueError, match="64-bit keys"):
        sp.sample_and_gather(csr, e, dtype=dtype, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_at_a_32_bit_shape_the_keyword_changes_nothing(sp, world, dtype):
    """(200, 3): with wide_keys=True the buffered and the unbuffered step give what they give without it, bit for bit, and buffers
    made with or without the keyword serve either call"""
    csr = world.csr
    e = world.pairs(B, 4)
    kw = dict(num_walks=200, num_steps=3, seed=5)
    xz, ind, _ = sp.sample_and_gather(csr, e, dtype=dtype, **kw)
    wxz, wind, _ = sp.sample_and_gather(csr, e, dtype=dtype, wide_keys=True, **kw)
    assert torch.equal(ind, wind) and _same_bits(xz, wxz)
    with_kw = sp.StepBuffers(csr, B, num_walks=200, num_steps=3, dtype=dtype, wide_keys=True)
    without = sp.StepBuffers(csr, B, num_walks=200, num_steps=3, dtype=dtype)
    assert not with_kw.half64 and not with_kw.wide and with_kw.slot.dtype == torch.int32
    for bufs, asked in ((with_kw, False), (with_kw, True), (without, True)):
        bxz, bind, sets = sp.sample_and_gather(csr, e, buffers=bufs, dtype=dtype, wide_keys=asked, **kw)
        sets.resolve()
        R = int(bind[-1].item())
        assert torch.equal(bind, ind) and _same_bits(bxz[:R], xz)

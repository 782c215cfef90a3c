"""Hand-made packed rows for sjoin_packhalf_kernel (csrc/sjoin_packed_half.hip) beyond those of tests/packed_rows.py, and the plumbing
that runs subgacc_sjoin_fill_packed_half beside its two references over the same descriptor: subgacc_sjoin_fill_packed (f32, rounded by
torch) and subgacc_sjoin_fill_half over the rows unpacked by subgacc_unpack_packed_rows.  tests/test_gpu_packed_half.py drives it.

The rows added here sit on what the packed-half kernel decides by itself:
  lengths    127 | 128 | 129, 511 | 512 | 513, 639 | 640 | 641 and the pitch -- the ends of a register trip of 128 lanes, of four and of
             five trips, and the full row slot -- where the pitch holds them
  escapes    0, 1, 63, 64, 65 (the 64 staged keys and the first one loaded from memory) and every member; an escape as the first and
             as the last member of a 64-member chunk (the ballot's lanes 0 and 63, the chunk bases)
  quotients  one row whose hop-1 count runs over 0 .. M: every quotient c / M a key can hold is rounded once in each 16-bit type"""
import ctypes
import functools

import numpy as np

import packed_rows as P
import walk_rows_edges as W

POISON = W.POISON
EDGE_LENGTHS = (127, 128, 129, 511, 512, 513, 639, 640, 641)
ESC_COUNTS = (0, 1, 63, 64, 65)


def _keys(rs, n, M, m, fb, esc):
    """n keys whose counts all fit fb bits, except at the members `esc` (bool [n]): one count of those is 2^fb .. M"""
    s = W.key_shift(M)
    f = np.zeros((n, m + 1), np.int64)
    f[:, 0] = rs.integers(0, 2, n)
    f[:, 1:] = rs.integers(0, 1 << fb, (n, m))
    f[:, 1] = np.maximum(f[:, 1], 1)
    f[:, m] &= ~1                                  # (never the code of all ones: only `esc` escapes)
    col = rs.integers(1, m + 1, n)
    idx = np.nonzero(esc)[0]
    f[idx, col[idx]] = rs.integers(1 << fb, min(M, (1 << s) - 1) + 1, len(idx))
    return P.key_of(f, M, m)


@functools.lru_cache(maxsize=None)
def edge_rows(M, m, num_nodes, pitch):
    """dict(ids, keys, names, cb, fb): the rows of P.join_rows followed by the rows described above, over one small universe of ids"""
    base = P.join_rows(M, m, num_nodes, pitch)
    cb, fb = base["cb"], base["fb"]
    rs = np.random.default_rng([M, m, pitch, 7])
    universe = np.sort(rs.choice(num_nodes, int(1.5 * pitch), replace=False)).astype(np.int64)
    ids, keys, names = list(base["ids"]), list(base["keys"]), list(base["names"])

    def add(name, n, esc):
        ids.append(np.sort(rs.choice(universe, n, replace=False)))
        keys.append(_keys(rs, n, M, m, fb, esc))
        names.append(name)

    for n in [x for x in EDGE_LENGTHS if x <= pitch] + [pitch]:
        add(f"edge{n}", n, rs.random(n) < 0.1)
    n = min(200, pitch)
    for e in ESC_COUNTS:
        esc = np.zeros(n, bool)
        esc[rs.choice(n, e, replace=False)] = True
        add(f"esc{e}", n, esc)
    add("esc_all", n, np.ones(n, bool))
    esc = np.zeros(n, bool)
    esc[[0, 63, 64, 127, 128, n - 1]] = True      # first and last member of a chunk
    add("esc_chunk_ends", n, esc)
    # the quotients row: hop 1 counts 0 .. M (most of them escape)
    n = M + 1
    assert n <= pitch
    s = W.key_shift(M)
    f = np.zeros((n, m + 1), np.int64)
    f[:, 0] = np.arange(n) % 2
    f[:, 1] = np.arange(n)
    f[:, 2:] = rs.integers(0, 1 << fb, (n, m - 1))
    assert M < (1 << s)
    ids.append(np.sort(rs.choice(universe, n, replace=False)))
    keys.append(P.key_of(f, M, m))
    names.append("quotients")
    return dict(ids=[np.asarray(i, np.int64) for i in ids], keys=keys, names=names, cb=cb, fb=fb)


def planes(rows, M, m, pitch):
    """the packed planes of `rows` as NumPy: dict(words [n, pitch], esc [n, pitch], nsize [n], nesc [n]); unwritten words are poison"""
    n = len(rows["ids"])
    words = np.full((n, pitch), POISON, np.int32)
    esc = np.full((n, pitch), POISON, np.int32)
    nsize, nesc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, (ri, rk) in enumerate(zip(rows["ids"], rows["keys"])):
        w, lst = P.pack_row(ri, rk, M, m, rows["cb"], rows["fb"])
        words[i, :len(ri)], esc[i, :len(lst)] = w.view(np.int32), lst.view(np.int32)
        nsize[i], nesc[i] = len(ri), len(lst)
    return dict(words=words, esc=esc, nsize=nsize, nesc=nesc)


def join(M, m, N, pitch, pl, pairs, dtype, nesc_edit=None, nsize_edit=None, partner_edit=None, seg_shift=0, via_half=True):
    """subgacc_sjoin_fill_packed_half over the planes `pl` and the mirrored list of `pairs` [2, B], beside its references, every output
    poisoned between poisoned guards.  seg_shift: every segment begins that many output rows later (the rows in front stay poison).
    nesc_edit / nsize_edit {row: value}; partner_edit {segment: row} breaks the mirror.
    -> dict(got, want [rows, k] int32 on the device: want = the f32 packed join's rows under torch's .to(dtype), poison where that
       join wrote nothing; half = subgacc_sjoin_fill_half over the unpacked rows or None; flags, flags32, flags_half; R)"""
    import torch
    L = P.lib_module()
    lib, ptr, st = L.lib(), L.ptr, L.stream_ptr()
    n, k = len(pl["nsize"]), m + 1
    nsize, nesc = pl["nsize"].copy(), pl["nesc"].copy()
    for i, v in (nsize_edit or {}).items():
        nsize[i] = v
    for i, v in (nesc_edit or {}).items():
        nesc[i] = v
    B = pairs.shape[1]
    S = 2 * B
    own_h, partner_h = np.concatenate([pairs[0], pairs[1]]).astype(np.int64), np.concatenate([pairs[1], pairs[0]]).astype(np.int64)
    for j, v in (partner_edit or {}).items():
        partner_h[j] = v
    own, partner = P.dev(own_h), P.dev(partner_h)
    d_ns, d_ne = P.dev(nsize), P.dev(nesc)
    d_words, d_esc = P.dev(pl["words"].reshape(-1)), P.dev(pl["esc"].reshape(-1))
    seg = torch.zeros(S + 1, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(lib.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device="cuda")
    f0 = torch.zeros(4, dtype=torch.int32, device="cuda")
    L.check(lib.subgacc_sjoin_sizes_rows(ptr(d_ns), n, ptr(own), ptr(partner), S, ptr(seg), ptr(f0), ptr(ws), ws.numel(), st))
    R = int(seg[-1].item())
    seg = seg + seg_shift
    rows_out = max(R + seg_shift, 1)
    code = {torch.float16: L.HALF_F16, torch.bfloat16: L.HALF_BF16}[dtype]
    common = dict(row_len=d_ns, n_rows=n, row_stride=pitch, own=own, partner=partner, S=S, seg=seg, pair_block=B, num_walks=M, num_steps=m)

    def guarded_flags():
        return P.guarded(4, torch.int32, np.zeros(4, np.int32))

    def check_guards(whole, nwords, what):
        assert bool((whole[:W.GUARD] == POISON).all()) and bool((whole[W.GUARD + nwords:] == POISON).all()), f"{what}: a guard word was written"

    # the f32 packed join -> want
    w32, x32 = P.guarded(rows_out * 2 * k, torch.int32)
    wf32, fl32 = guarded_flags()
    d = L.join_desc(L.JOIN_ROWS, L.JOIN_KEY32, ids=d_words, payload=d_esc, flags=fl32, out_xz=x32, **common)
    L.check(lib.subgacc_sjoin_fill_packed(ctypes.byref(d), ptr(d_ne), N, st))
    # the packed join in 16 bits -> got
    wgot, got = P.guarded(rows_out * k, torch.int32)
    wfl, fl = guarded_flags()
    d = L.join_desc(L.JOIN_ROWS, L.JOIN_KEY32, ids=d_words, payload=d_esc, flags=fl, **common)
    L.check(lib.subgacc_sjoin_fill_packed_half(ctypes.byref(d), ptr(d_ne), N, code, ptr(got), st))
    half, flh = None, None
    if via_half:    # the two planes, unpacked by the library, through the two-plane half join
        u_ids = torch.full((n * pitch,), POISON, dtype=torch.int32, device="cuda")
        u_keys = torch.full((n * pitch,), POISON, dtype=torch.int32, device="cuda")
        fu = torch.zeros(4, dtype=torch.int32, device="cuda")
        L.check(lib.subgacc_unpack_packed_rows(ptr(d_words), ptr(d_esc), ptr(d_ns), ptr(d_ne), n, pitch, N, M, m, ptr(u_ids), ptr(u_keys),
                                               ptr(fu), st))
        whalf, half = P.guarded(rows_out * k, torch.int32)
        wflh, flh = guarded_flags()
        d = L.join_desc(L.JOIN_ROWS, L.JOIN_KEY32, ids=u_ids, payload=u_keys, flags=flh, **common)
        L.check(lib.subgacc_sjoin_fill_half(ctypes.byref(d), code, ptr(half), st))
    torch.cuda.synchronize()
    check_guards(w32, rows_out * 2 * k, "f32 packed join")
    check_guards(wgot, rows_out * k, "packed half join")
    x = x32.view(rows_out, 2 * k)
    written = x != POISON
    assert bool((written.all(dim=1) | ~written.any(dim=1)).all()), "the f32 packed join left a row half written"
    want = torch.where(written.all(dim=1, keepdim=True), x.view(torch.float32).to(dtype).view(torch.int32), torch.full_like(x[:, :k], POISON))
    out = dict(got=got.view(rows_out, k), want=want, half=None, R=R, written=written.all(dim=1), flags=fl.tolist(), flags32=fl32.tolist(),
               x32=x.view(torch.float32))
    if via_half:
        check_guards(whalf, rows_out * k, "two-plane half join")
        out["half"], out["flags_half"] = half.view(rows_out, k), flh.tolist()
    return out


def first_difference(a, b):
    import torch
    bad = torch.nonzero((a != b).any(dim=1))[:4].flatten().tolist()
    return [(r, a[r].tolist(), b[r].tolist()) for r in bad]

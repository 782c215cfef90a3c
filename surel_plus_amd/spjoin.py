"""SpJoin on the GPU: drop-ins for train.py's gather / bgather / pgather / hgather.

Reference: train.py:13-45 (gather), :48-72 (hgather), :75-85 (bgather), :88-111 (pgather).  Same names,
same argument meaning, same return values (xz float32 [R,2,k], indptr-or-segment-ids int64 on `device`);
`x` is an SpG (surel_plus_amd.spg.SpG) or a scipy CSR (uploaded once and cached), `encode` the Z_SF table
as a float32 CUDA tensor or None for a float payload.  The work is done by csrc/sjoin.hip (the row form),
csrc/sjoin_sizes.hip (the size pass), csrc/sjoin_f64stage.hip and csrc/sjoin_forms.hip (the fused stages, the count and pair forms),
csrc/keycols.hip and csrc/sjoin_keys.hip (the columns of an on-demand step's key rows and the joins over them).
"""
import ctypes
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import JOIN_COUNTS, JOIN_F64, JOIN_KEY32, JOIN_KEY64, JOIN_PAIRS, JOIN_ROWS, JOIN_SFPTR, check, join_fill, lib, ptr, stream_ptr

NO_ROOT = -2 ** 31      # include/subgacc.h: SUBGACC_NO_ROOT
from .sampler import _timed
from .spg import KEY_ROWS_ENCODE, HeadedSpG, SpG, StridedSpG

_scipy_cache = weakref.WeakKeyDictionary()


def _as_spg(x):
    if isinstance(x, (SpG, StridedSpG, HeadedSpG)):
        return x
    try:
        hit = _scipy_cache.get(x)
    except TypeError:
        hit = None
    if hit is None:
        with _CACHE_LOCK:       # uploaded once, complete before another thread / stream can pick it up
            try:
                hit = _scipy_cache.get(x)
            except TypeError:
                hit = None
            if hit is None:
                hit = SpG.from_scipy(x)
                torch.cuda.current_stream(hit.device).synchronize()
                try:
                    _scipy_cache[x] = hit
                except TypeError:
                    pass
    return hit


def _as_rows(edge, device):
    """[r, B] endpoints as an int64 device tensor (the reference takes torch or numpy integer arrays)."""
    if torch.is_tensor(edge):
        return edge.to(device=device, dtype=torch.int64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(edge)).astype(np.int64)).to(device)


def join_payload(z, encode, return_index=False):
    """What the members of store `z` carry, as the join needs it: (payload kind, k, the descriptor's payload fields -- table /
    table_rows / k, num_walks / num_steps for keys, uniq_table / uniq_capacity for the slots of a StridedSpG).  Every payload check
    of the join is made here.  A StridedSpG's slots become SFptr+1 through its batch's numbered table on their way in, unless
    `encode` is the batch's own slot_table(): that one is indexed by slot and needs no bound check."""
    if encode is None and z.payload_is_slot and not return_index:
        raise NotImplementedError("a sampled batch is joined with an encode table (z.slot_table())")
    if z.keyrows:           # LP keys (SpG.keyed(), key-rows batches): the join unpacks the feature rows itself, no table
        if encode is not KEY_ROWS_ENCODE or return_index:
            raise ValueError("a keyed store is joined by gather / hgather(…, encode=z.slot_table()); other tables and index pairs "
                             "need the SFptr store (z.to_csr() of a key-rows batch)")
        return (JOIN_KEY64 if z.key64 else JOIN_KEY32), z.key_m + 1, dict(num_walks=z.key_M, num_steps=z.key_m)
    if not z.payload_is_slot and z.data.dtype == torch.float64:
        if encode is not None:
            raise TypeError("a float-payload SpG is joined without an encode table (train.py:39-43)")
        return JOIN_F64, 1, {}
    by_slot = z.payload_is_slot and not return_index and encode is not None and encode is z._slot_table
    fields = dict(uniq_table=z.table, uniq_capacity=z.capacity) if z.payload_is_slot and not by_slot else {}
    if return_index:
        if z.payload_is_slot:
            z.sets.number()         # the pairs are SFptr+1: a transient batch is numbered only now
        return JOIN_SFPTR, 0, fields
    if encode is None:
        raise NotImplementedError("an integer SpG needs the encode table")
    table = encode if by_slot else encode.to(device=z.device, dtype=torch.float32).contiguous()
    if not by_slot and table.shape[0] <= z.max_data:       # host-side bound check: no device round trip on the hot path
        raise IndexError(f"index {z.max_data} is out of bounds for the encode table with {table.shape[0]} rows")
    fields.update(table=table, table_rows=table.shape[0], k=table.shape[1])
    return JOIN_SFPTR, int(table.shape[1]), fields


def _out_view(out, dev, k, R=None, worst=None, dtype=torch.float32):
    """The join's output [rows, 2, k] (float32; dtype=: the rows of the 16-bit form): a new tensor of R rows, or a view of the caller's
    buffer `out` -- its first R rows, or, for a lazy join (R stays on the device), all of it, which must hold the worst case of
    `worst` rows."""
    if out is None:
        return torch.empty((R, 2, k), dtype=dtype, device=dev)
    need = R if worst is None else worst
    if out.dtype != dtype or not out.is_contiguous() or out.device != dev or out.numel() < need * 2 * k:
        raise ValueError(f"out= must be a contiguous {str(dtype)[6:]} buffer on the store's device with room for {need} rows of 2 x {k} "
                         "(R rows; lazy=True: the worst case, S * max_len)")
    rows = R if worst is None else out.numel() // (2 * k)
    return out.view(-1)[: rows * 2 * k].view(rows, 2, k)


def _half_code(dtype, who, refused):
    """0 for dtype None / torch.float32 (the f32 rows); SUBGACC_HALF_F16 / SUBGACC_HALF_BF16 (include/subgacc_half.h) for torch.float16 /
    torch.bfloat16 -- after a ValueError for the first entry of `refused()` {what the call was given: bool} that holds: the 16-bit rows
    are those of subgacc_sjoin_fill_half's scope, and what lies outside it is refused here, before any device work.  (`refused` is
    called for a 16-bit dtype only: the f32 step pays one comparison.)"""
    if dtype is None or dtype == torch.float32:
        return 0
    code = {torch.float16: _lib.HALF_F16, torch.bfloat16: _lib.HALF_BF16}.get(dtype)
    if code is None:
        raise ValueError(f"{who}: dtype is None, torch.float32, torch.float16 or torch.bfloat16, not {dtype!r}")
    for what, given in refused().items():
        if given:
            raise ValueError(f"{who}: dtype={dtype} (16-bit rows: pairs with segment pointers over 32-bit LP keys or a packed SFptr "
                             f"store) does not go with {what}")
    return code


def _half_store_refusals(x, wide_keys=False):
    """what _half_code refuses about the store `x` (anything that is not one of the library's stores is uploaded as a packed SFptr
    or float store: its payload type says which).  wide_keys: the strided 64-bit key rows of a step are served
    (subgacc_sjoin_fill_half64, include/subgacc_half64.h)."""
    data = None if getattr(x, "payload_is_slot", False) else getattr(x, "data", None)
    return {"a HeadedSpG (headed rows)": isinstance(x, HeadedSpG),
            "a float64 store (the PPR payload)": data is not None and str(data.dtype).endswith("float64"),
            "64-bit keys": bool(getattr(x, "key64", False)) and not (wide_keys and bool(getattr(x, "payload_is_slot", False))),
            "key_rows=False (strided rows of table slots)": bool(getattr(x, "payload_is_slot", False)) and not getattr(x, "keyrows", False)}


def _half_shape_refused(num_walks, num_steps, wide_keys, small_rows=False):
    """a step's 16-bit rows exist over its key rows: the 32-bit ones (subgacc_sjoin_fill_half), -- wide_keys=True -- the 64-bit ones of
    sampler.key_rows_form == 64 (subgacc_sjoin_fill_half64) and -- small_rows=True -- the 32-bit ones of a small shape
    (sampler.small_rows_form); not at a shape without key rows"""
    from .sampler import key_rows_form, small_rows_form
    if small_rows and small_rows_form(int(num_walks), int(num_steps)):
        return False
    form = key_rows_form(int(num_walks), int(num_steps))
    return form != 32 and not (wide_keys and form == 64)


def _small_rows_wanted(who, small_rows, num_walks, num_steps, stage, refused):
    """small_rows=True at a shape where it means something -- a small shape (sampler.small_rows_form) and the row form (stage=None:
    the stages take the one-wave kernel by themselves) -- after a ValueError that names the keyword for the first entry of
    `refused()` {what the call was given: bool} that holds, before any device work.  Anywhere else the keyword changes nothing."""
    from .sampler import small_rows_form
    if not small_rows or stage is not None or not small_rows_form(int(num_walks), int(num_steps)):
        return False
    for what, given in refused().items():
        if given:
            raise ValueError(f"{who}: small_rows=True (the row form over the 32-bit key rows of the one-wave kernel, num_walks = "
                             f"{num_walks}, num_steps = {num_steps}) does not go with {what}")
    return True


def _fill_half(L, kind):
    """the library's 16-bit row fill for a payload kind: 64-bit keys have an entry point of their own"""
    return L.subgacc_sjoin_fill_half64 if kind == JOIN_KEY64 else L.subgacc_sjoin_fill_half


def sjoin(spg, own, partner, encode=None, ptr_mode=True, return_index=False, pair_block=0, out=None, lazy=False, star=False, dtype=None,
          wide_keys=False):
    """Generic segment join (include/subgacc.h: the layout's size pass + subgacc_sjoin_fill_v2) over any store: its rows are described
    by spg.join_rows(), its payload by join_payload().

    own/partner: int64 device tensors of SpG row numbers, one segment each.  pair_block = P > 0 promises that
    the list is made of blocks of P segments with block 2t+1 the mirror of block 2t (see include/subgacc.h); strided and headed
    rows and keyed stores join such lists only.
    out: optional preallocated float32 buffer with room for the R output rows (a steady-state caller re-uses one
    buffer instead of asking the allocator for a fresh GB-sized block per batch); the result is a view of it.
    lazy=True (needs out=, segment pointers, an integer SpG with its encode table or a float one): no host round trip at all -- the
    number of rows R stays on the device as ind[-1] and xz is the whole buffer viewed as [capacity, 2, k], of which the first R rows
    are valid.  Headed rows: the size pass is the library's one-launch form (SUBGACC_JOIN_OPT_SIZES) -- lazily it and the fill are
    ONE call; eagerly it runs alone first (no output), the host reads [R, status] from pinned memory, and the fill follows.
    star=True: a star list (SUBGACC_JOIN_OPT_STAR, gather_star): own = P source rows, partner = P*K target rows, pair_block = K;
    the S = 2*P*K segments are those of the expanded list [own.repeat_interleave(K) | partner] and its mirror.
    dtype=torch.float16 / torch.bfloat16: xz in that type, bit for bit xz.to(dtype) of the float32 rows, written by
    subgacc_sjoin_fill_half (include/subgacc_half.h) behind the same size pass -- half the bytes of the join's largest output, for
    callers that train under autocast.  Mirrored lists (pair_block > 0) with segment pointers over a keyed store, the key rows of a
    step or a packed SFptr store with its table, k = 2 .. 5; ValueError for ptr_mode=False, return_index, lazy, star, a HeadedSpG, a
    float64 store, 64-bit keys and rows of table slots.  out=: a buffer of that dtype.  None / torch.float32: the rows as ever.
    wide_keys=True (with a 16-bit dtype): the strided 64-bit key rows of a step (sampler.key_rows_form == 64: 4 hops, M = 128 .. 204)
    are joined too, by subgacc_sjoin_fill_half64 (include/subgacc_half64.h) -- the same bits as xz.to(dtype) of their float32 rows;
    every other refusal stands, and over any other store the keyword changes nothing.
    Returns (xz, ind, flags): xz float32 [R,2,k] (or int32 [R,2] index pairs when return_index), ind = int64 [S+1]
    segment pointers (ptr_mode) or int64 [R] segment ids, flags the join's int32[4] status words.
    """
    half = _half_code(dtype, "sjoin", lambda: {"ptr=False (segment ids)": not ptr_mode, "return_index": return_index, "lazy=True": lazy,
                                               "star=True": star, "a list that is not mirrored (pair_block <= 0)": pair_block <= 0,
                                               **_half_store_refusals(spg, wide_keys)})
    L, dev = lib(), spg.device
    S = 2 * partner.numel() if star else own.numel()
    own = own.contiguous()
    if partner is not None:
        partner = partner.contiguous()
    elif pair_block <= 0 and S > 0:
        raise ValueError("partner=None needs a mirrored segment list (pair_block > 0)")
    size_pass, rows = spg.join_rows()
    if lazy and (out is None or not ptr_mode or return_index or
                 (encode is None and "row_off" in rows and rows["payload"].dtype != torch.float64)):
        raise ValueError("lazy=True needs out=, ptr=True and feature rows (a packed integer store: with its encode table)")
    if return_index and size_pass is None:
        raise ValueError("index pairs come from the packed store (gather_index)")
    kind, k, payload = join_payload(spg, encode, return_index)
    # only a packed SFptr / float store joins a list that is not mirrored (a strided one not even an empty list)
    if pair_block <= 0 and (kind in (JOIN_KEY32, JOIN_KEY64) or "row_off" not in rows) and (S > 0 or "row_len" in rows):
        raise ValueError("this store is joined by gather / hgather (mirrored segment lists); use the packed store (to_csr() / "
                         "to_spg()) for the other forms")
    seg, flags = _seg_and_flags(S, dev)
    st, R = stream_ptr(), None              # (R stays on the device in a lazy join)
    star_bit = _lib.JOIN_OPT_STAR if star else 0
    desc = dict(rows, **payload, own=own, partner=partner, S=S, pair_block=pair_block, flags=flags, seg=seg, options=star_bit)
    if size_pass is None:
        state = torch.zeros(L.subgacc_sjoin_workspace_bytes(S), dtype=torch.uint8, device=dev)
        host = torch.empty(2, dtype=torch.int64, pin_memory=True)
        onepass = dict(options=_lib.JOIN_OPT_SIZES | star_bit, seg=None, out_seg=seg, size_state=state, size_state_bytes=state.numel(), host_tail=host)
        if lazy:
            desc.update(onepass)
        else:
            join_fill(JOIN_ROWS, kind, st, **{**desc, **onepass})     # no output: the size pass alone
            torch.cuda.current_stream(dev).synchronize()
            R, status = (int(v) for v in host.tolist())
            if status & 64:
                raise _lib.SubgAccError("the join's size state was not clean")
            if status & 16:
                raise IndexError(f"row index out of range for an SpG with {spg.n_rows} rows")
    else:
        fn, lens = size_pass
        ws = torch.empty(L.subgacc_sjoin_workspace_bytes(S), dtype=torch.uint8, device=dev)
        if star:        # (a packed store: the star list's own size pass)
            check(L.subgacc_sjoin_star_sizes(ptr(lens), spg.n_rows, ptr(own), ptr(partner), own.numel(), pair_block, ptr(seg), ptr(flags),
                                             ptr(ws), ws.numel(), st))
        else:
            check(getattr(L, fn)(ptr(lens), spg.n_rows, ptr(own), ptr(partner), S, ptr(seg), ptr(flags), ptr(ws), ws.numel(), st))
        if not lazy:
            R = _size_and_row_check(seg, S, flags, spg.n_rows)     # the one host round trip
    if half:        # the rows in 16 bits: the same descriptor, no out_* field, the library's 16-bit fill for the payload kind
        res = _out_view(out, dev, k, R, dtype=dtype)
        with _timed("sjoin_fill_half"):
            if R:
                check(_fill_half(L, kind)(ctypes.byref(_lib.join_desc(JOIN_ROWS, kind, **desc)), half, ptr(res), st))
        return res, seg, flags
    if return_index and kind == JOIN_SFPTR:          # (a float store answers with its xz, as bgather() wants it)
        res = desc["out_idx"] = torch.empty((R, 2), dtype=torch.int32, device=dev)
    else:
        res = desc["out_xz"] = _out_view(out, dev, k, R, S * spg.max_len if lazy else None)
    segid = desc["out_segid"] = None if ptr_mode else torch.empty(R, dtype=torch.int64, device=dev)
    with _timed("sjoin_fill"):
        join_fill(JOIN_ROWS, kind, st, **desc)
    if lazy and size_pass is None:
        ev = torch.cuda.Event()
        ev.record()
        _lib.keep_until(ev, (host, state))          # the kernels write both after this function has returned
    return res, (seg if ptr_mode else _with_pointers(segid, seg)), flags


def _with_pointers(segid, seg):
    """segment ids as the join's second result; the pointers they were made from ride along (gather_many / hgather_many cut by them)"""
    segid.seg_pointers = seg
    return segid


def _seg_and_flags(S, dev):
    """Segment pointers int64[S+1] and the join's int32[4] status words as ONE allocation: what the host reads of a join --
    the output size seg[S] and the status word flags[3] -- is then one contiguous 24-byte copy (`seg.join_tail`), with no
    cast / concatenate kernels in front of it (they were two of the seven nodes of a captured join)."""
    buf = torch.empty(S + 3, dtype=torch.int64, device=dev)
    flags = buf[S + 1:].view(torch.int32)
    flags.zero_()
    seg = buf[:S + 1]
    seg.join_tail = buf[S:]         # [R | flags[0], flags[1] | flags[2], flags[3]]
    return seg, flags


def tail_words(tail):
    """(R, status word) of a join_tail read back as three int64"""
    R, _, w = tail
    return int(R), (int(w) >> 32) & 0xFFFFFFFF


def _size_and_row_check(seg, S, flags, n_rows):
    """The join's one host read: the output size R = seg[S] and, in the same copy, the status word of the size pass --
    a row number outside the store is an IndexError here as it is in the reference (scipy's x[edge[0]], train.py:15);
    the kernels never dereference such a row (it reads as empty), so nothing out of bounds has happened by now."""
    R, status = tail_words(seg.join_tail.tolist())
    if status & 16:
        raise IndexError(f"row index out of range for an SpG with {n_rows} rows")
    return int(R)


# SpG.max_len / SpG.max_data make the kernel's other guards (flags[3] & 1, & 2) unreachable; SUBGACC_DEBUG=1 reads them
# back after every join anyway (one extra host sync per call).  Row numbers out of range: raised by the eager forms
# above; a lazy join (no host read at all) returns empty segments for them and leaves flags[3] & 16 set.
_DEBUG_FLAGS = os.environ.get("SUBGACC_DEBUG", "0") == "1"


def lazy_join_status(ind):
    """A lazy join reads nothing back, so a row number outside the store -- an IndexError of scipy's x[edge[0]] in the reference,
    train.py:15 -- cannot be raised when the join is queued: such a row reads as empty and the join's status word keeps the
    fact.  This reads that word for the `ind` a lazy gather() returned (one small host read, whenever the caller resolves the
    batch) and raises like the eager form; sample_and_gather(lazy=True) carries the word in its sets' status: resolve() raises."""
    flags = getattr(ind, "join_flags", None)
    if flags is not None and int(flags[3].item()) & 16:
        raise IndexError("row index out of range for the SpG (lazy join: the row was joined as an empty row)")
    return ind


def _checked(out, ind, flags, lazy=False):
    if lazy:
        ind.join_flags = flags       # see lazy_join_status()
    if _DEBUG_FLAGS and not torch.cuda.is_current_stream_capturing():      # (a capture cannot read back: the replay's finish() does)
        f = int(flags[3].item())
        if f & 16:
            raise IndexError("row index out of range for the SpG")
        if f & 1:
            raise _lib.SubgAccError("SpG row longer than SpG.max_len")
        if f & 2:
            raise IndexError("SFptr outside the encode table")
    return out, ind


def gather(edge, x, device=None, ptr=True, encode=None, out=None, lazy=False, dtype=None, wide_keys=False):
    """train.py:13-45.  Left blocks (S_u with S_v looked up) then right blocks, per pair in batch order.
    out= / lazy=: see sjoin (a serving loop's forms: caller-owned output buffer, no host round trip).
    dtype=torch.float16 / torch.bfloat16: xz in that type (sjoin: what autocast would make of the float32 rows, bit for bit);
    wide_keys=True: also over the 64-bit key rows of a step (sjoin(wide_keys=))."""
    _half_code(dtype, "gather", lambda: {"ptr=False (segment ids)": not ptr, "lazy=True": lazy, **_half_store_refusals(x, wide_keys)})
    spg = _as_spg(x)
    e = _as_rows(edge, spg.device)
    # own = [u.. | v..] is the contiguous [2, B] tensor itself; the mirrored partner list [v.. | u..] is derived by the kernels
    own = e.contiguous().view(-1)
    return _checked(*sjoin(spg, own, None, encode, ptr_mode=ptr, pair_block=e.shape[1], out=out, lazy=lazy, dtype=dtype, wide_keys=wide_keys),
                    lazy=lazy)


def _star_rows(source, targets):
    """gather_star's arguments checked on the host -- before any device work -- as (source int64 [P], targets int64 [P, K]), each a
    torch tensor where it is still (a NumPy array stays on the host until the store's device is known)"""
    def as_int(v, what, ndim):
        if not torch.is_tensor(v):
            try:
                v = np.asarray(v)
            except ValueError as e:           # (NumPy >= 1.24 refuses a ragged nested list itself)
                raise ValueError(f"gather_star: {what} must be a rectangular integer array ({e})") from None
            if v.dtype == object:
                raise ValueError(f"gather_star: {what} must be a rectangular integer array, not a ragged one")
            kind_ok = np.issubdtype(v.dtype, np.integer)
        else:
            kind_ok = not v.dtype.is_floating_point and not v.dtype.is_complex and v.dtype != torch.bool
        if not kind_ok:
            raise TypeError(f"gather_star: {what} must hold integer row numbers, not {v.dtype}")
        if v.ndim != ndim:
            raise ValueError(f"gather_star: {what} must be {ndim}-D ({'[P]' if ndim == 1 else '[P, K]'}), got shape {tuple(v.shape)}")
        return v
    source, targets = as_int(source, "source", 1), as_int(targets, "targets", 2)
    if targets.shape[0] != source.shape[0]:
        raise ValueError(f"gather_star: targets has {targets.shape[0]} rows for {source.shape[0]} sources ([P, K] for source [P])")
    return source, targets


def gather_star(source, targets, x, device=None, ptr=True, encode=None, out=None, lazy=False, kernel="pairs"):
    """One source against K targets: the MRR evaluation queries of the reference (train.py:246-280: gather over
    neg_edge = stack([source.repeat_interleave(K), target_neg.view(-1)]), utils.py:93-95) without the expanded edge tensor.

    source int [P], targets int [P, K] (NumPy or torch, as gather() takes edges).  Returns bit for bit what
    gather(stack([source.repeat_interleave(K), targets.reshape(-1)]), x, device, ptr, encode) returns -- xz, ind, dtypes and devices --
    from the library's star form (SUBGACC_JOIN_OPT_STAR): a workgroup stages a source row once and joins it with a run of its
    targets.  x: an SpG with its encode table, SpG.keyed(...) with its slot_table(), a float SpG, or a HeadedSpG.  out= / lazy= as
    for sjoin(); the worst case is P*K*(2 * max_len) rows.
    kernel: "pairs" (default) joins the expanded list with gather's pair kernels, which were faster than the star kernel on every
    store measured (profiles/star_bench.log); "star" takes the library's star form -- ind.join_flags then holds the
    join's status words: flags[1] & 1 says the star kernel ran, & 2 that a source too long for it was joined by the
    one-segment-per-wave kernel."""
    if kernel not in ("pairs", "star"):
        raise ValueError(f"gather_star: kernel must be 'pairs' or 'star', not {kernel!r}")
    if isinstance(x, StridedSpG):
        raise ValueError("gather_star joins a resident store -- an SpG (with its encode table, or keyed), a float SpG or a HeadedSpG "
                         "-- not a StridedSpG (use gather on the expanded pairs, or z.to_csr())")
    source, targets = _star_rows(source, targets)
    spg = _as_spg(x)
    P, K = int(targets.shape[0]), int(targets.shape[1])
    if P * K == 0:      # nothing to join: the expanded edge tensor is [2, 0]
        return gather(torch.empty((2, 0), dtype=torch.int64, device=spg.device), spg, device, ptr, encode, out, lazy)
    src, tgt = _as_rows(source, spg.device).contiguous(), _as_rows(targets, spg.device).reshape(-1).contiguous()
    if kernel == "pairs":
        return gather(torch.stack([src.repeat_interleave(K), tgt]), spg, device, ptr, encode, out, lazy)
    xz, ind, flags = sjoin(spg, src, tgt, encode, ptr_mode=ptr, pair_block=K, out=out, lazy=lazy, star=True)
    ind.join_flags = flags
    return _checked(xz, ind, flags, lazy=lazy)


class BatchViews:
    """The nb reference-shaped results of a join over nb batches laid out [u_0 | v_0 | u_1 | v_1 | ...]: a sequence of
    (xz_b, indptr_b) -- xz_b float32 [R_b, 2, k] the rows of batch b (a view of the one output buffer), indptr_b int64 [2B+1]
    starting at 0 (train.py:21-22; a row of ONE [nb, 2B+1] tensor), or segment ids 0..P-1 where the caller asked for ids.
    The nb+1 batch boundaries (and the join's status word) are read from the device when the first batch is TAKEN, in one small
    copy, and the views are made batch by batch as they are taken: a loop that queues the next group of batches before it
    consumes this one never waits for the GPU in between.  A row number outside the store raises IndexError at that point."""

    def __init__(self, xz, seg, seg_per_batch, ids=None, flags=None, n_rows=None, prefetch=False):
        P = int(seg_per_batch)
        S = seg.numel() - 1
        if P <= 0 or S % P:
            raise ValueError(f"{S} segments are not a whole number of batches of {P} segments")
        self.xz, self.seg, self.P, self.nb, self.ids = xz, seg, P, S // P, ids
        self._flags, self._n_rows, self._bounds, self._ptrs, self._pending = flags, n_rows, None, None, None
        if prefetch and seg.is_cuda:
            # the boundaries start their way to pinned host memory NOW, behind this join's kernels: taking the first batch later waits
            # for exactly this copy, not for whatever the stream holds by then (the next group of batches, queued in between)
            src = self._words()
            host = torch.empty(src.numel(), dtype=torch.int64, pin_memory=True)
            _lib.publish(src, host)
            ev = torch.cuda.Event()
            ev.record()
            _lib.keep_until(ev, host)
            self._pending = (host, ev, src)

    def _words(self):
        src = self.seg[::self.P]                               # [nb+1]: first row of every batch, and the total
        if self._flags is not None:
            src = torch.cat([src, self._flags[3:4].to(torch.int64)])
        return src

    def _resolve(self):
        if self._bounds is None:
            if self._pending is not None:
                host, ev, _ = self._pending
                ev.synchronize()
                words = host.tolist()
                self._pending = None
            else:
                words = self._words().tolist()
            if self._flags is not None:
                if words.pop() & 16:
                    raise IndexError(f"row index out of range for an SpG with {self._n_rows} rows")
            self._bounds = words
            if self.ids is None:
                self._ptrs = self.seg.as_strided((self.nb, self.P + 1), (self.P, 1)) - self.seg[:-1:self.P][:, None]
        return self._bounds

    def __len__(self):
        return self.nb

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self.nb))]
        if i < 0:
            i += self.nb
        if not 0 <= i < self.nb:
            raise IndexError(i)
        b = self._resolve()
        if self.ids is not None:
            return self.xz[b[i]:b[i + 1]], self.ids[b[i]:b[i + 1]]
        return self.xz[b[i]:b[i + 1]], self._ptrs[i]

    def __iter__(self):
        return (self[i] for i in range(self.nb))

    def __eq__(self, other):                    # (an empty result compares equal to []: gather_many(edges[:0]) == [])
        return list(self) == other if isinstance(other, list) else NotImplemented


def split_batches(xz, seg, batch_pairs):
    """The result of a join over nb batches of `batch_pairs` pairs (gather_many, sample_and_gather_many, a StepBuffers made with
    batch=) as its nb reference-shaped pieces: see BatchViews."""
    return BatchViews(xz, seg, 2 * int(batch_pairs))


def gather_many(edges, x, device=None, ptr=True, encode=None, out=None, lazy=False):
    """gather() for MANY reference-sized batches at once: `edges` [nb, 2, B] (the batches of an epoch are known when it starts:
    train.py:120 draws the DataLoader permutation up front) joined in ONE launch sequence -- one size pass, one scan, one fill
    over nb*B pairs -- instead of nb times three launches of 1,024 pairs that cannot fill the chip (main.py:32).  Returns
    [(xz_b, ind_b)] * nb, bit for bit what `gather(edges[b], x, device, ptr, encode)` returns for every b: xz_b float32
    [R_b, 2, k] (views of one buffer, `out` if given), ind_b int64 [2B+1] segment pointers from 0 (ptr=True) or int64 [R_b]
    segment ids 0..2B-1 (ptr=False).  One small host read when the call is made (the total number of rows, to size xz) and one when
    the first batch is taken (BatchViews); lazy=True (needs out= for the worst case -- nb*2B * SpG.max_len * 2k float32 -- and
    ptr=True) makes the call itself free of host reads: the next group can be queued before this one is consumed.
    `edges` may also be a list of [2, B_i] arrays: runs of equal B are fused, the rest (an epoch's short last batch) joined singly
    -- eagerly: out= / lazy=True with a list raise ValueError."""
    spg = _as_spg(x)
    if isinstance(edges, (list, tuple)):
        if out is not None or lazy:
            # (a list is cut into runs of equal batch size, each its own join with its own row count: one caller's buffer cannot
            #  be handed out before those counts are read, which is exactly the host read lazy=True promises not to make)
            raise ValueError("gather_many: out= / lazy=True need the batches as one [nb, 2, B] array (a list of batches is joined "
                             "run by run, eagerly); stack equal-sized batches, join a short last batch with gather()")
        res, i = [], 0
        while i < len(edges):
            j = i
            while j + 1 < len(edges) and tuple(edges[j + 1].shape) == tuple(edges[i].shape):
                j += 1
            if j == i:
                res.append(gather(edges[i], spg, device, ptr=ptr, encode=encode))
            else:
                stack = torch.stack([_as_rows(e, spg.device) for e in edges[i:j + 1]])
                res.extend(gather_many(stack, spg, device, ptr=ptr, encode=encode))
            i = j + 1
        return res
    e = _as_rows(edges, spg.device)
    if e.dim() != 3 or e.shape[1] != 2:
        raise ValueError("gather_many: edges must be [nb, 2, B]")
    nb, _, B = e.shape
    if nb == 0 or B == 0:
        return [gather(e[b], spg, device, ptr=ptr, encode=encode) for b in range(nb)]
    own = e.contiguous().view(-1)                              # [u_0 | v_0 | u_1 | v_1 | ...]: mirrored blocks of B segments
    if lazy and not ptr:
        raise ValueError("gather_many(lazy=True) needs ptr=True (segment ids are sized by the row count)")
    xz, ind, flags = sjoin(spg, own, None, encode, ptr_mode=ptr, pair_block=B, out=out, lazy=lazy)
    _checked(xz, ind, flags)
    if ptr:
        return BatchViews(xz, ind, 2 * B, flags=flags if lazy else None, n_rows=spg.n_rows, prefetch=lazy)
    # segment ids (train.py:25-30, the LSTM aggregator): the kernel wrote the ids over ALL segments; inside a batch they are 0..2B-1
    ind.remainder_(2 * B)
    return BatchViews(xz, ind.seg_pointers, 2 * B, ids=ind)


def hgather(hedge, x, device=None, encode=None):
    """train.py:48-72.  Blocks [U|w ; W|u ; V|w ; W|v], always segment ids; encode is mandatory."""
    if encode is None:
        raise NotImplementedError
    spg = _as_spg(x)
    h = _as_rows(hedge, spg.device)
    u, v, w = h[0], h[1], h[2]
    own = torch.cat([u, w, v, w])          # the mirrored partner list [w, u, w, v] is derived by the kernels
    xz, ind = _checked(*sjoin(spg, own, None, encode, ptr_mode=False, pair_block=h.shape[1]))
    assert xz.size(0) == ind.size(0)
    return xz, ind


def hgather_many(hedges, x, device=None, encode=None):
    """hgather() for MANY batches of triplets at once (main_horder.py:33: 2,048 triplets per batch, ~8k one-pair workgroups that
    cannot fill the chip): `hedges` [nb, 3, B] joined in one launch sequence; returns [(xz_b, ids_b)] * nb, bit for bit what
    hgather(hedges[b], x, device, encode) returns (segment ids 0..4B-1 per batch, train.py:57-68)."""
    if encode is None:
        raise NotImplementedError
    spg = _as_spg(x)
    h = _as_rows(hedges, spg.device)
    if h.dim() != 3 or h.shape[1] != 3:
        raise ValueError("hgather_many: hedges must be [nb, 3, B]")
    nb, _, B = h.shape
    if nb == 0 or B == 0:
        return [hgather(h[b], spg, device, encode) for b in range(nb)]
    own = torch.stack([h[:, 0], h[:, 2], h[:, 1], h[:, 2]], dim=1).contiguous().view(-1)      # per batch [u | w | v | w]: two mirrored pairs of blocks
    xz, ids, flags = sjoin(spg, own, None, encode, ptr_mode=False, pair_block=B)
    _checked(xz, ids, flags)
    ids.remainder_(4 * B)                                      # the kernel numbered the segments of all batches: 0..4B-1 inside a batch
    return BatchViews(xz, ids.seg_pointers, 4 * B, ids=ids)


def bgather(edge, x, out):
    """train.py:75-85: the per-thread block worker of pgather.  Kept for signature compatibility: fills
    out[0..3] with (left pairs, right pairs, left sizes, right sizes) as NumPy arrays."""
    spg = _as_spg(x)
    e = _as_rows(edge, spg.device)
    B = e.shape[1]
    own = torch.cat([e[0], e[1]])
    partner = torch.cat([e[1], e[0]])
    if spg.data.dtype == torch.float64:
        pairs, seg = _checked(*sjoin(spg, own, partner, None, ptr_mode=True))
        pairs = pairs.view(-1, 2)
    else:
        pairs, seg = _checked(*sjoin(spg, own, partner, None, ptr_mode=True, return_index=True))
    sizes = (seg[1:] - seg[:-1]).cpu().numpy()
    mid = int(seg[B].item())
    pairs = pairs.cpu().numpy()
    out[0], out[1] = pairs[:mid], pairs[mid:]
    out[2], out[3] = sizes[:B], sizes[B:]


def pgather(edge, M, device=None, encode=None, gather_func=None, ptr=True, njobs=4):
    """train.py:88-111.  The reference splits the batch over `njobs` Python threads; one kernel launch
    covers the whole batch here, so `gather_func` / `njobs` only keep the call signature.  The result is
    identical to gather() (as it is in the reference)."""
    return gather(edge, M, device, ptr=ptr, encode=encode)


class StepBuffers:
    """Everything one on-demand step (sample_and_gather) touches, allocated once for a fixed (B, M, m): the int32 roots, the
    strided rows and their sizes, the table of distinct LP rows and the feature table indexed by its slots, the segment
    pointers with the step's status words right behind them (one small read-back carries sizes, flags and the join's row
    count) and the output buffer.  With it a step is SIX launches -- prologue (table reset + status + root narrowing),
    walk, segment reduce, segment scan, LP unpack, join -- and no allocation; without it torch's allocator and a dozen
    few-microsecond helper kernels sit between them (1,024 pairs: ~100 us of which the walk and the join are 55).
    Reuse is the caller's business: a buffer set is busy until its step has been resolved (bench.py alternates two).
    dedup_roots=True: every DISTINCT endpoint of the batch is sampled once (subgacc_step_prologue_dedup: a generation-stamped
    hash of the endpoints names every node's first occurrence, one more small launch; the walk kernel runs over the list of
    first occurrences) -- Philox keys a walk by its root's id, so (xz, indptr) do not change; the sets of the batch sit in the
    rows of the first occurrences (sets.n_distinct of them; bufs.roots == NO_ROOT elsewhere), the other rows are empty.
    The hash is stamped with a per-step generation kept on the device: a captured step replays correctly.
    order=LocalityOrder (sampler.locality_order) or an int32 rank [num_nodes]: every step the fused-row kernel serves walks its
    rows (or, with dedup_roots, its first occurrences) in ascending rank of their root, whatever the batch size -- the rows are
    the same; `walk_order` records after each step which order ran ("rank", "id" or "batch").
    ptr=False: the step also writes the segment id of every output row (train.py:25-30, what the reference's --aggrs lstm runs
    with, main.py:217) into a buffer of its own, `segid` int64 [worst case rows]; one batch per step (batch=None).
    triplets=True: the step of sample_and_hgather -- `pairs` triplets (u, v, w), 3B roots walked once each, 4B segments
    [U|w ; W|u ; V|w ; W|v] (train.py:57-68), always with segment ids; dedup_roots=True takes the prologue that knows the roles
    (subgacc_step_prologue_dedup_roles); Philox only (the reference never samples triplets in a stream), one batch per step.
    stage="counts": the step of sample_and_counts / sample_and_hcounts (and of sample_and_mean_stage / sample_and_hmean_stage) --
    prologue, work list, walk, then the columns of the step's LP keys (subgacc_keyrows_columns) and the count form of the join over the
    key rows (subgacc_sjoin_key_counts): no size pass, no scan, no row form.  Instead of `out` and `segid` the buffers hold `counts`
    float32 [S, table_rows], `sizes` int32 [S], `ukeys` int32 [table_rows - 1] and `feat` float32 [table_rows, m+1]; table_rows - 1 is
    the number of distinct LP rows a step may show (more: sets.resolve() raises and names table_rows).  Needs 32-bit key rows and one
    batch per step (ValueError otherwise, before any device work).  A small shape (sampler.small_rows_form: 1 to 4 hops, M*m+1 <= 204)
    has such rows for the stages alone: subgacc_walk_keyrows_small writes them (self.small), with root dedup, order= and triplets as
    at the larger shapes; stage=None of such a shape stays the table form on the general kernel.
    stage="counts_attn": the step of sample_and_attn_counts / sample_and_attn_stage -- the same launches up to the columns, then the
    caller's gate g = gate(table) in torch and the attentional count form over the key rows (subgacc_sjoin_key_counts_attn).  The buffers
    are those of "counts", where `counts` holds the softmax-weighted count rows W, plus `smax` and `sden` float32 [S] (m_j and den_j, kept
    for the backward, which rejoins the step's rows: it must run before the buffers take their next step).  Same refusals.
    stage="index": the step of sample_and_index / sample_and_lstm_stage -- the same launches up to the columns, then the size pass
    (subgacc_sjoin_sizes_rows) and the index form over the key rows (subgacc_sjoin_key_index): neither xz, nor an output buffer of the row
    form, nor segment ids.  The buffers are those of "counts" without `counts`, plus `pairs` int32 [S * (M*m+1), 2] (the worst case; the
    first seg[-1] rows are a step's result) and the size pass's workspace.  Same refusals, and triplets=True (HONet has no LSTM
    aggregation, model_horder.py:56-57).
    stage="mean" (with width=H): the step of sample_and_fused_mean_stage / sample_and_fused_hmean_stage and their *_star twins -- the
    same launches up to the columns, then the caller's E = embed(table) float32 [table_rows, H] in torch and the mean first stage fused
    into the count join (subgacc_sjoin_key_mean, include/subgacc_mean.h): the count matrix is never written.  The buffers are those of
    "counts" WITHOUT `counts` -- the largest buffer of that set -- plus `mean` float32 [S, H], the stage's result.  width is required
    here and a ValueError with any other stage; every refusal of "counts" applies, and small shapes, wide_keys=True, triplets,
    dedup_roots, order= and star=K come under the rules of "counts".  Nothing is allocated or read back by the step (capturable), so
    -- as `counts` -- `mean` is valid only once `sets.resolve()` has passed: a pair whose join raised a flag is left unwritten and
    holds what an earlier step left there.  The backward joins the step's rows again, into a C of its own: it must run before the
    buffers take their next step.
    stage="attn" (with width=H): the step of sample_and_fused_attn_stage and its *_star twin -- the same launches up to the columns,
    then the caller's E = embed(table) float32 [table_rows, H] and gate g in torch and the attentional first stage fused into the
    attentional count join (subgacc_sjoin_key_attn, include/subgacc_attn.h): the softmax-weighted count matrix W is never written.
    The buffers are those of "counts_attn" WITHOUT `counts` -- the largest buffer of that set -- plus `attn` float32 [S, H], the
    aggregation W @ E; `smax` and `sden` stay.  width is required as for "mean"; every refusal of "counts_attn" applies, and small
    shapes, wide_keys=True, dedup_roots, order= and star=K come under its rules.  Capturable; `attn` is valid only once
    `sets.resolve()` has passed.  The backward joins the step's rows again, into a W of its own: it must run before the buffers
    take their next step.
    dtype=torch.float16 / torch.bfloat16: `out` -- the largest buffer of the set -- is allocated in that type, half the bytes, and the
    step's join writes it through subgacc_sjoin_fill_half (sjoin(dtype=)); sample_and_gather(buffers=) must ask for the same dtype.
    The row form over 32-bit key rows with segment pointers: ValueError for ptr=False, triplets=True, a stage, key_rows=False, a shape
    with 64-bit keys or none, and batch=.
    packed_rows=None|True|False: the hand-over of the step's rows from the walk to the join as ONE word per member and a short escape
    list per row (include/subgacc_packed.h) instead of two planes -- `self.packed`.  None: the library's choice, which
    is packed wherever the form exists: the row form (stage=None) with f32 rows, segment pointers, pairs and one batch per step, over
    32-bit key rows of a two-wave form on a graph whose ids leave three bits a count (sampler.packed_rows_form).  True: the same, and
    ValueError where it does not exist.  False: the two planes.  `ids` and `slot` show today's rows either way: of a packed step
    they are unpacked when first looked at (subgacc_unpack_packed_rows, into planes allocated then), never in the step.
    packed_half=True (with dtype=torch.float16 / torch.bfloat16): both at once -- the packed hand-over under the 16-bit rows,
    `self.packed` and `self.half` -- where sampler.packed_rows_form has a form; the walk writes the packed rows as in the f32 step
    and the step ends in subgacc_sjoin_fill_packed_half (include/subgacc_packed_half.h): six launches, nothing allocated or read
    back, (xz, indptr) bit for bit those of StepBuffers(dtype=).  Opt-in: without it a 16-bit step keeps the two planes
    (profiles/packed_half_bench.log has both).  ValueError naming the keyword without a 16-bit dtype, for packed_rows=False,
    ptr=False, triplets=True, a stage, key_rows=False, batch= and a shape or graph without a packed form (64-bit keys included).
    wide_keys=True: a stage ("counts", "counts_attn", "index") over the 64-bit key rows of a 4-hop shape with M = 128 .. 204
    (sampler.key_rows_form == 64: the paper's citation2 setting M = 200, m = 4), which the stages refuse otherwise -- `self.wide`.
    The columns pass is subgacc_keyrows_columns64 (include/subgacc_wide.h: one launch more than the 32-bit step), which also writes
    every member's column as a 32-bit surrogate key into `cols` int32 [rows * stride]; the joins read `cols` and the identity list
    `ukeys` = 1 .. c instead of `slot`, and answer exactly what they answer at a 32-bit shape.  The buffers hold `ukeys64` int64
    [table_rows - 1] (the sorted distinct keys), `cols` -- 4 bytes per member slot beside the 8 of `slot` -- and a larger `col_ws`;
    `slot` keeps the 64-bit keys.  table_rows <= 8,192 at such a shape (ValueError before any device work); at a shape with 32-bit or
    small key rows the keyword changes nothing.
    wide_keys=True with dtype=torch.float16 / torch.bfloat16 and stage=None at such a shape: the row form in 16 bits over the 64-bit key
    rows -- `self.half64`; `out` is allocated in that type, `slot` stays int64, and the step runs its usual launches and ends in
    subgacc_sjoin_fill_half64 (include/subgacc_half64.h) instead of the f32 fill: nothing more is allocated or read back, root dedup,
    order=, rng="rand_r" and out= work as in the f32 step, and `self.wide` stays False (no stage, no columns pass).  Without the keyword
    the shape is refused as ever, and so are ptr=False, triplets=True, a stage, key_rows=False, batch= and a shape without key rows
    with it.
    small_rows=True: the row form (stage=None) of a small shape (sampler.small_rows_form: the reference's mag, DBLP-coauthor and vessel
    settings) over the 32-bit key rows of the one-wave kernel, as the stages of such a shape run already -- `self.small`, `keyrows`,
    neither `table` nor `feat`: prologue (or a dedup prologue), work list, subgacc_walk_keyrows_small, size pass, the KEY32 join; no
    LP unpack, nothing allocated or read back, (xz, indptr, segment ids) bit for bit those of the table form.  Pairs with pointers
    and ptr=False, triplets=True, dedup_roots=True, order= / sort_roots, rng="rand_r", out=, and batch= for f32 rows with pointers.
    dtype=torch.float16 / torch.bfloat16 goes with ptr=False and triplets=True here -- and only here: subgacc_sjoin_fill_half_ids
    (include/subgacc_half_ids.h) writes the int64 ids beside the 16-bit rows.  Opt-in (profiles/small_step_bench.log has both routes).
    ValueError naming the keyword for key_rows=False, packed_rows=True, packed_half=True and a 16-bit dtype with batch=; at any other
    shape, and with a stage, the keyword changes nothing.
    star=K: the step of one source against K targets, the shape the reference evaluates with (utils.py:93-95; triplets: (u, v) kept,
    w replaced, dataloader.py:265-275) -- sample_and_gather_star / sample_and_hgather_star and the stage calls of that name.  `pairs`
    stays the number of joined pairs P*K (a multiple of K); the step walks every source ONCE: n = P + P*K rows (source j is row j,
    target i row P + i) under S = 2*P*K segments, own = [j // K | P + i] and its mirror; triplets: n = 2P + P*K rows in the order u, v,
    w under S = 4*P*K segments, own = [j // K | 2P + i | P + j // K | 2P + i] -- `own` / `partner`, constants of (P, K) built here
    (_star_segments).  The step takes (heads, tails) = (source [P], targets [P*K]) or ([u.. | v..], w [P*K]) and begins with
    subgacc_step_prologue_star (include/subgacc_star.h): the launch count of the plain step, nothing allocated.  Everything else is
    the one-batch pair or triplet step: both row forms, dtype=, packed_rows=, packed_half=, wide_keys=, small_rows=, order= /
    sort_roots, out=, stage="counts" / "counts_attn", each under its own rules; (xz, indptr or ids, flags) and (C, sizes, table) are
    bit for bit those of the step over the expanded list (Philox keys a walk by its root's id).  ValueError naming `star` for K < 1,
    pairs % K != 0, batch=, dedup_roots=True (the structural repeats are gone; a hash on top is not built), rng="rand_r" (a rand_r
    set depends on its place in the stream: there is nothing to be identical to) and stage="index"."""

    def __init__(self, csr, pairs, num_walks=200, num_steps=3, uniq_capacity=1 << 17, out=None, dedup_roots=False, rng="philox",
                 key_rows=True, sort_roots=True, batch=None, align_rows=True, order=None, ptr=True, triplets=False, stage=None,
                 table_rows=2048, small_rows=False, dtype=None, packed_rows=None, wide_keys=False, star=None, width=None,
                 packed_half=False):
        from .sampler import FUSED_MAX_Q, as_rank, key_rows_form, packed_rows_form, small_rows_form
        self.star = 0
        if star is not None:    # one source against K targets: refused before anything touches the device
            K = int(star)
            why = {f"K = {K} (one target a source at least)": K < 1,
                   f"pairs = {int(pairs)} (the joined pairs P*K: a multiple of K = {K})": K >= 1 and (int(pairs) < 0 or int(pairs) % K != 0),
                   "batch= (one batch per step)": batch is not None,
                   "dedup_roots=True (the repeated sources are walked once already; a hash on top is not built)": bool(dedup_roots),
                   "rng='rand_r' (a rand_r set depends on its place in the stream: there is no expanded step to be identical to)":
                       rng == "rand_r",
                   "stage='index' (no index form for stars)": stage == "index"}
            if any(why.values()):
                raise ValueError(f"StepBuffers(star={star!r}) does not go with " + "; ".join(k for k, v in why.items() if v))
            self.star = K
        self.packed, self._unpacked, self._unpacked_step = False, None, -1
        # opt-in: the row form of a small shape over the key rows of the one-wave kernel, refused before anything touches the device
        small_rows = _small_rows_wanted("StepBuffers", small_rows, num_walks, num_steps, stage, lambda: {
            "key_rows=False (the one-wave kernel writes key rows)": not key_rows,
            "packed_rows=True (no packed form at a small shape)": packed_rows is True,
            "packed_half=True (no packed form at a small shape)": bool(packed_half),
            f"dtype={dtype} with batch= (many batches per step)": batch is not None and dtype in (torch.float16, torch.bfloat16)})
        if packed_half:    # opt-in: the packed hand-over under the 16-bit rows, refused before anything touches the device
            why = {f"dtype={dtype} (the packed rows are joined in 16 bits with dtype=torch.float16 / torch.bfloat16; the f32 step is packed "
                   "by itself)": dtype not in (torch.float16, torch.bfloat16),
                   "packed_rows=False": packed_rows is False, "ptr=False": not ptr, "triplets=True": bool(triplets),
                   f"stage={stage!r}": stage is not None, "key_rows=False": not key_rows, "batch= (many batches per step)": batch is not None,
                   f"no packed form for {int(csr.num_nodes)} nodes, num_walks = {num_walks}, num_steps = {num_steps} "
                   "(sampler.packed_rows_form: 32-bit key rows of a two-wave form, three bits a count beside the id)":
                       packed_rows_form(csr.num_nodes, num_walks, num_steps, csr.indptr.dtype == torch.int64) is None}
            if any(why.values()):
                raise ValueError("StepBuffers(packed_half=True): " + "; ".join(k for k, v in why.items() if v))
        # a stage over 64-bit key rows (wide_keys=True at such a shape, nothing anywhere else): the columns pass of csrc/keycols64.hip
        self.wide = bool(wide_keys) and stage in _KEY_STAGES and bool(key_rows) and key_rows_form(int(num_walks), int(num_steps)) == 64
        self.half = _half_code(dtype, "StepBuffers", lambda: {
            # (small_rows: segment ids too -- subgacc_sjoin_fill_half_ids writes them beside the 16-bit rows)
            "ptr=False (segment ids)": not ptr and not small_rows, "triplets=True": triplets and not small_rows,
            f"stage={stage!r}": stage is not None, "key_rows=False (strided rows of table slots)": not key_rows,
            f"num_walks = {num_walks}, num_steps = {num_steps} (64-bit keys, or no key rows)":
                _half_shape_refused(num_walks, num_steps, wide_keys, small_rows),
            "batch= (many batches per step)": batch is not None})
        self.dtype = dtype if self.half else torch.float32
        # 16-bit rows over 64-bit key rows (wide_keys=True with a 16-bit dtype at such a shape): the step ends in subgacc_sjoin_fill_half64
        self.half64 = bool(self.half) and key_rows_form(int(num_walks), int(num_steps)) == 64
        self.stage, self.T = stage, int(table_rows)
        if stage not in (None,) + _KEY_STAGES:
            raise ValueError(f"StepBuffers: stage is None (the row form), 'counts', 'counts_attn', 'index', 'mean' or 'attn', not {stage!r}")
        self.width = _mean_width(stage, width)     # (refused before anything touches the device)
        if stage in _KEY_STAGES:  # refused before anything touches the device
            who = f"StepBuffers(stage='{stage}')"
            if stage == "index" and triplets:
                raise ValueError(f"{who} joins pairs: triplets=True has no index form (HONet has no LSTM aggregation)")
            _counts_stage_shape(who, num_walks, num_steps, key_rows, self.T, wide_keys)
            if batch is not None and int(batch) != int(pairs):
                raise ValueError(f"{who}: the columns are those of one batch (batch=None)")
            if out is not None or not ptr:
                raise ValueError(f"{who} writes no rows: it takes neither out= nor ptr=False")
        L, dev = lib(), csr.device
        # order=LocalityOrder / int32 rank: the walk kernel takes the rows in ascending rank of their root (subgacc_worklist_by_rank),
        # the deduplicated step its first occurrences too; self.walk_order says which order the last step ran
        self.order = as_rank(csr, order)
        self.walk_order = None
        self.B, self.M, self.m = int(pairs), int(num_walks), int(num_steps)
        # batch=b: the `pairs` of a step are pairs/b reference-sized batches of b pairs each, handed over as [nb, 2, b] (rows
        # [u_0 | v_0 | u_1 | v_1 | ...]); the join pairs row j with its mirror inside ITS batch, and split_batches() cuts the
        # result into the nb reference-shaped (xz, indptr).  None: one batch, [2, pairs].
        self.batch = self.B if batch is None else int(batch)
        if self.batch <= 0 or self.B % self.batch:
            raise ValueError(f"StepBuffers: pairs = {self.B} is not a whole number of batches of {batch}")
        if self.batch != self.B and dedup_roots:
            raise ValueError("StepBuffers: root dedup works on one batch (batch=None)")
        self.triplets = bool(triplets)
        self.ptr = bool(ptr) and not self.triplets          # hgather always answers with segment ids (train.py:57-59)
        if self.batch != self.B and not self.ptr:
            raise ValueError("StepBuffers: segment ids (ptr=False, triplets=True) are those of one batch (batch=None)")
        if self.triplets and rng != "philox":
            raise ValueError("StepBuffers(triplets=True) samples with rng='philox' (the reference never samples triplets in a rand_r "
                             "stream: there is nothing to reproduce)")
        # n roots = rows of the step, S segments of the join: pairs [u | v] -> 2B and 2B, triplets [u | v | w] -> 3B and 4B
        n, S = (3 * self.B, 4 * self.B) if self.triplets else (2 * self.B, 2 * self.B)
        if self.star:       # every source stands once: P (triplets: 2P, u and v) + P*K rows under the same S segments
            self.P = self.B // self.star
            n = (2 if self.triplets else 1) * self.P + self.B
        self.n, self.S, self.Q, self.k = n, S, self.M * self.m + 1, self.m + 1
        if self.Q > FUSED_MAX_Q or self.m < 1:
            raise ValueError(f"StepBuffers: num_walks*num_steps+1 = {self.Q} exceeds what the fused-row walk kernel holds")
        # the rows of two roots lie `stride` words apart: M*m+1 rounded up to whole 128-byte lines (subgacc_walk_cfg::row_pitch) --
        # the join reads, and the walk kernel writes, whole lines (the join alone: 3-5 % on every workload, profiles/r28_join_pitch.log)
        # (align_rows=False: rows M*m+1 words apart, the layout of rounds 1-4)
        self.stride = (self.Q + 31) // 32 * 32 if align_rows else self.Q
        self.capacity = int(uniq_capacity)
        self.roots = torch.empty(n, dtype=torch.int32, device=dev)
        self.nsize = torch.empty(n, dtype=torch.int32, device=dev)
        self.ids = torch.empty(n * self.stride, dtype=torch.int32, device=dev)
        form = key_rows_form(self.M, self.m) if key_rows else 0
        # a stage over a small shape (sampler.small_rows_form): its 32-bit key rows come from subgacc_walk_keyrows_small, which reads a
        # selecting work list; the row form (stage=None) of such a shape stays the table form on the general kernel unless
        # small_rows=True asks for the same rows under the row-form join
        self.small = (stage in _KEY_STAGES and bool(key_rows) and small_rows_form(self.M, self.m)) or small_rows
        if self.small:
            form = 32
        self.keyrows = bool(form)                 # rows of LP keys: no table, no feature table
        self.key64 = form == 64                   # ... 64-bit keys (4-hop walks with M >= 128): `slot` is int64
        self.slot = torch.empty(n * self.stride, dtype=torch.int64 if self.key64 else torch.int32, device=dev)
        self.sort_roots = bool(sort_roots)     # the walk kernel takes the rows in ascending order of root id (csrc/worklist.hip)
        self.table = None if self.keyrows else torch.empty(L.subgacc_uniq_table_bytes(self.capacity), dtype=torch.uint8, device=dev)
        self.tail = torch.zeros(S + 1 + 4 + 1, dtype=torch.int64, device=dev)  # seg [S+1] | status [4] | distinct roots [1]
        self.seg, self.status, self.n_distinct = self.tail[: S + 1], self.tail[S + 1: S + 5], self.tail[S + 5:]
        self.dedup = bool(dedup_roots)
        self.rng = rng
        if rng not in ("philox", "rand_r") or (rng == "rand_r" and self.dedup):
            raise ValueError("StepBuffers: rng is 'philox' or 'rand_r'; root dedup needs 'philox' (a rand_r set depends on its place in the stream)")
        if rng == "rand_r" and getattr(csr, "_rand_r_dead_ends", False):
            raise ValueError("StepBuffers(rng='rand_r'): this graph has dead ends (a walk reached a node without out-edges), its "
                             "rand_r stream has to be replayed per batch -- sample_and_gather(..., rng='rand_r') without buffers= "
                             "does that; the buffered step cannot")
        # packed rows: `_ids` takes the words, `_slot` the escape lists, `nesc` their lengths; nothing else of the buffers changes
        self.num_nodes = int(csr.num_nodes)
        fmt = packed_rows_form(self.num_nodes, self.M, self.m, csr.indptr.dtype == torch.int64)
        why = {"key_rows=False": not key_rows, f"stage={stage!r}": stage is not None,
               "a 16-bit dtype (without packed_half=True)": bool(self.half) and not packed_half,
               "ptr=False": not self.ptr, "triplets=True": self.triplets, "batch= (many batches per step)": self.batch != self.B,
               f"no packed form for {self.num_nodes} nodes, num_walks = {self.M}, num_steps = {self.m} (sampler.packed_rows_form)": fmt is None}
        if packed_rows and any(why.values()):
            raise ValueError("StepBuffers(packed_rows=True): " + "; ".join(k for k, v in why.items() if v))
        self.packed = packed_rows is not False and not any(why.values())
        if self.packed:
            self.nesc = torch.empty(n, dtype=torch.int32, device=dev)
            self._unpack_flags = torch.zeros(4, dtype=torch.int32, device=dev)
        if rng == "rand_r":      # the rows' places in the reference's sequential stream (subgacc_rng_positions), per step
            self.rng_pos = torch.empty(n, dtype=torch.int32, device=dev)
            self.rng_seed = torch.empty(n, dtype=torch.int32, device=dev)
            self.rng_ws = torch.empty(L.subgacc_rng_positions_workspace_bytes(n), dtype=torch.uint8, device=dev)
        if self.dedup:
            from .sampler import walk_kernel_name
            if walk_kernel_name(csr, self.M, self.m, True) != "walk_rows_kernel" and not self.small:
                raise ValueError("StepBuffers(dedup_roots=True) needs a shape the fused-row walk kernel serves (2..4 hops, M <= 256)")
            self.own = torch.empty(S, dtype=torch.int64, device=dev)
            # (triplets: no partner list -- the roles prologue leaves it to the kernels, the list is mirrored)
            self.partner = None if self.triplets else torch.empty(n, dtype=torch.int64, device=dev)
            self.worklist = torch.empty(n, dtype=torch.int32, device=dev)
            self.dedup_ws = torch.zeros(L.subgacc_step_dedup_workspace_bytes(n), dtype=torch.uint8, device=dev)
            self.dedup_steps = 0
        if self.star:       # the segment lists of the star: constants of (P, K)
            self.own, self.partner = _star_segments(self.P, self.star, self.triplets, dev)
        if stage in _KEY_STAGES:  # counts, sizes, the sorted keys and their feature rows; no output rows, no segment ids (a size pass for "index" alone)
            T = self.T
            self.counts = self._counts_buffer(S, T, dev) if stage in _COUNT_STAGES else None
            if stage == "mean":             # the stage's result; no C
                self.mean = torch.empty((S, self.width), dtype=torch.float32, device=dev) if self.width else None
            if stage == "counts_attn":      # m_j and den_j of the softmax, for the backward
                self.smax, self.sden = (None, None) if self.counts is None else \
                    (torch.empty(S, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev))
            if stage == "attn":             # the aggregation W @ E, m_j and den_j; no W
                self.attn = torch.empty((S, self.width), dtype=torch.float32, device=dev) if self.width else None
                self.smax, self.sden = torch.empty(S, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev)
            self.sizes = torch.empty(S, dtype=torch.int32, device=dev)
            self.ukeys = torch.empty(T - 1, dtype=torch.int32, device=dev)
            self.feat = torch.empty((T, self.k), dtype=torch.float32, device=dev)
            if self.wide:   # the sorted 64-bit keys, the rows as surrogate keys (what the joins read instead of `slot`), the wider set
                self.ukeys64 = torch.empty(T - 1, dtype=torch.int64, device=dev)
                self.cols = torch.empty(n * self.stride, dtype=torch.int32, device=dev)
                self.col_ws = torch.zeros(L.subgacc_keyrows_columns64_workspace_bytes(T), dtype=torch.uint8, device=dev)   # zeroed once
            else:
                self.col_ws = torch.zeros(L.subgacc_keyrows_columns_workspace_bytes(T), dtype=torch.uint8, device=dev)   # zeroed once
            self.ws = self.out = self.segid = None
            if stage == "index":    # the index pairs of the worst case, and the size pass in front of them
                self.pairs = torch.empty((S * self.Q, 2), dtype=torch.int32, device=dev)
                self.ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device=dev)
            return
        self.ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device=dev)
        self.feat = None if self.keyrows else torch.empty((self.capacity + 1, self.k), dtype=torch.float32, device=dev)
        if out is not None:         # room for the worst case: S segments (2B; triplets: 4B) of M*m+1 members
            _out_view(out, dev, self.k, worst=S * self.Q, dtype=self.dtype)
        self.out = out if out is not None else torch.empty(S * self.Q * 2 * self.k, dtype=self.dtype, device=dev)
        self.segid = None if self.ptr else torch.empty(S * self.Q, dtype=torch.int64, device=dev)

    def _counts_buffer(self, S, T, dev):
        """stage="counts": the step's C [S, table_rows]"""
        return torch.empty((S, T), dtype=torch.float32, device=dev)

    # the rows of the step: the buffers themselves, or -- packed -- the planes they are unpacked into when somebody looks
    @property
    def ids(self):
        return self._rows()[0] if self.packed else self._ids

    @ids.setter
    def ids(self, t):
        self._ids = t

    @property
    def slot(self):
        return self._rows()[1] if self.packed else self._slot

    @slot.setter
    def slot(self, t):
        self._slot = t

    def _rows(self):
        """(ids, keys) of a packed step as subgacc_walk_spg(uniq_table=NULL) writes them: unpacked once per step, on the current stream"""
        if self._unpacked is None:
            self._unpacked = (torch.empty_like(self._ids), torch.empty_like(self._slot))
        sid = getattr(self, "step_id", 0)
        if sid and self._unpacked_step != sid:
            ids, keys = self._unpacked
            check(lib().subgacc_unpack_packed_rows(ptr(self._ids), ptr(self._slot), ptr(self.nsize), ptr(self.nesc), self.n, self.stride,
                                                   self.num_nodes, self.M, self.m, ptr(ids), ptr(keys), ptr(self._unpack_flags),
                                                   stream_ptr()))
            self._unpacked_step = sid
            # an escape without a key in its row's list (flags[3] & 2) cannot come from the packed walk, which writes list and length
            # together: like the join's guards that sound rows cannot reach (_checked above), the unpack's word is read under
            # SUBGACC_DEBUG=1 only (one host sync) and never in a capture
            if _DEBUG_FLAGS and not torch.cuda.is_current_stream_capturing() and int(self._unpack_flags[3].item()) & 2:
                raise _lib.SubgAccError("packed rows: an escape at or beyond its row's nesc (the escape list does not match the row)")
        return self._unpacked


class _FitStepBuffers(StepBuffers):
    """The buffers sample_and_counts makes for ONE call without table_rows: columns for as many distinct LP rows as the columns pass
    holds (keys, feature rows and workspace: 0.5 MB) and no C -- the count kernel writes a tensor of exactly c + 1 columns, allocated
    once c has been read back (_counts_tail(fit=True)).  Never handed out."""

    def _counts_buffer(self, S, T, dev):
        return None


MEAN_MAX_WIDTH = 1024              # subgacc_sjoin_key_mean and subgacc_sjoin_key_attn: the features of a row of E
# width= of the buffers a sample_and_fused_*mean_stage* / sample_and_fused_attn_stage* call makes for itself (_step_counts): the width
# of embed(table) is known only once the step has run, so they hold no `mean` / `attn` (width 0) and the join writes a tensor of that
# call (_StepMeanJoin.forward, _StepFusedAttnJoin.fused)
_WIDTH_OF_CALL = object()
_WIDTH_STAGES = {"mean": "mean", "attn": "attn"}        # the stages that take width=H, and the buffer of that width


def _mean_width(stage, width):
    """StepBuffers(stage="mean" / "attn", width=H): H, the features of a row of the caller's E = embed(table) -- required there, refused
    with any other stage (0: no `mean` / `attn`)"""
    if stage not in _WIDTH_STAGES:
        if width is not None:
            raise ValueError(f"StepBuffers(width={width!r}) goes with stage='mean' or 'attn' alone (the width of `mean` / `attn`), "
                             f"not stage={stage!r}")
        return 0
    if width is _WIDTH_OF_CALL:
        return 0
    if width is None or not 1 <= int(width) <= MEAN_MAX_WIDTH:
        raise ValueError(f"StepBuffers(stage='{stage}') needs width=H, the features of a row of embed(table) (1 .. {MEAN_MAX_WIDTH}), "
                         f"not width={width!r}: `{_WIDTH_STAGES[stage]}` is float32 [S, H]")
    return int(width)


COUNTS_MAX_TABLE_ROWS = 16384      # subgacc_keyrows_columns sorts the distinct keys of a step in LDS
COUNTS_MAX_TABLE_ROWS_WIDE = 8192  # ... subgacc_keyrows_columns64 sorts 64-bit keys in the same 128 KiB
_COUNT_STAGES = ("counts", "counts_attn")       # the stages of a step that run over the columns of its LP keys: the count forms
# ... the index form, and the mean / attentional first stage fused into the count join
_KEY_STAGES = _COUNT_STAGES + ("index", "mean", "attn")


def _counts_stage_shape(who, num_walks, num_steps, key_rows, table_rows, wide_keys=False):
    """what the count stage of a step refuses before any device work: a shape without 32-bit key rows, key_rows=False, a table_rows
    the columns pass does not hold.  wide_keys: a shape with 64-bit key rows is served too (subgacc_keyrows_columns64), with at most
    COUNTS_MAX_TABLE_ROWS_WIDE columns; nothing changes at any other shape"""
    from .sampler import key_rows_form, small_rows_form
    if not key_rows:
        raise ValueError(f"{who} runs over the key rows of the step: key_rows=False has none")
    form = key_rows_form(int(num_walks), int(num_steps))
    if form == 64 and wide_keys:
        if not 2 <= int(table_rows) <= COUNTS_MAX_TABLE_ROWS_WIDE:
            raise ValueError(f"{who}: table_rows = {table_rows} (2 .. {COUNTS_MAX_TABLE_ROWS_WIDE} with 64-bit LP keys, wide_keys=True: "
                             "column 0 and one column per distinct LP row)")
        return
    if form != 32 and not small_rows_form(int(num_walks), int(num_steps)):
        raise ValueError(f"{who} needs 32-bit LP keys: num_walks = {num_walks}, num_steps = {num_steps} " +
                         ("has 64-bit keys (key_rows_form == 64)" if form == 64 else "has no key-rows form"))
    if not 2 <= int(table_rows) <= COUNTS_MAX_TABLE_ROWS:
        raise ValueError(f"{who}: table_rows = {table_rows} (2 .. {COUNTS_MAX_TABLE_ROWS}: column 0 and one column per distinct LP row)")


def _dedup_tick(bufs):
    """the hash's 32-bit generation must never wrap (a stale stamp would outrank a fresh one): long before it could, the
    workspace is zeroed again -- host side, once in 2^31 steps (every queued step of these buffers is behind it on the stream)"""
    bufs.dedup_steps += 1
    if bufs.dedup_steps >= (1 << 31):
        bufs.dedup_ws.zero_()
        bufs.dedup_steps = 0


def _step_sets(csr, bufs, cfg, rr, step_id):
    """the SampledSets of a buffered step: views of the step's buffers, lazily resolved"""
    from .sampler import PackedStepSets, SampledSets
    kr = bufs.keyrows
    if bufs.packed:     # the rows are unpacked when somebody looks at them (sets.ids / sets.slot), not here
        sets = PackedStepSets(bufs.nsize, None, None, None, None, None, bufs.M, bufs.m, bufs.stride, None)
        sets._bufs = bufs
    else:
        sets = SampledSets(bufs.nsize, None, bufs.ids, None, None, None, bufs.M, bufs.m, bufs.stride, None)
        sets.slot = bufs.slot
    sets.table, sets.capacity, sets.strided = bufs.table, (0 if kr else bufs.capacity), True
    if kr:
        sets.keyrows, sets.key64, sets.small_rows = True, bufs.key64, bool(getattr(bufs, "small", False))
        # number() registers the keys of the rows as they stand in the buffers (root dedup: the rows of repeated endpoints are
        # empty, and a repeated endpoint never is the first to show an LP row, so the numbering is the one of the whole batch);
        # once the buffers have taken a later batch -- or a captured step has been replayed -- the answer would describe that
        # batch, so it is refused (stamp of the step that made these sets against the buffers' current one)
        sets._keyctx = {"csr": csr, "roots": bufs.roots, "cfg": cfg, "rng_pos": bufs.rng_pos if rr else None,
                        "rng_seed": bufs.rng_seed if rr else None, "capacity": bufs.capacity,
                        "fresh": lambda: getattr(bufs, "step_id", 0) == step_id}
    # every set of a buffered step -- key rows or table form -- is a view of buffers that the NEXT step overwrites: what is computed
    # from them on demand (the member count of a deduplicated step, X / nnz) is refused once they hold a later batch
    sets._fresh = lambda: getattr(bufs, "step_id", 0) == step_id
    sets.status, sets._tail = bufs.status, bufs.tail[bufs.S: bufs.S + (6 if bufs.dedup else 5)]
    # (the rows of w are joined twice, the row of a star's source K times: the join's rows are not the members)
    sets._rows_are_members = not bufs.triplets and not getattr(bufs, "star", 0)
    sets.walk_order = bufs.walk_order
    if bufs.stage in _KEY_STAGES:   # no row form ran (the index form's row count is its caller's to read): the members are counted on demand
        sets._rows_are_members, sets._table_rows = False, bufs.T
    return sets


def _step_columns(bufs, flags, st, fit):
    """the columns of the step's LP keys (subgacc_keyrows_columns: two launches) -> (the count word on the device, T); fit: the
    number of distinct LP rows c is read back once and T = c + 1"""
    n, T = bufs.n, bufs.T
    count = bufs.status[2:3]        # the status word `distinct rows`: resolve() reads it with the flags
    if bufs.wide:   # 64-bit key rows: three launches, and the rows as surrogate keys in bufs.cols (_step_key_desc hands them to the joins)
        with _timed("keyrows_columns64"):
            check(lib().subgacc_keyrows_columns64(ptr(bufs.slot), ptr(bufs.nsize), n, bufs.stride, bufs.M, bufs.m, T, ptr(bufs.ukeys64),
                                                  ptr(bufs.ukeys), ptr(count), ptr(bufs.feat), ptr(bufs.cols), ptr(flags),
                                                  ptr(bufs.col_ws), bufs.col_ws.numel(), st))
    else:
        with _timed("keyrows_columns"):
            check(lib().subgacc_keyrows_columns(ptr(bufs.slot), ptr(bufs.nsize), n, bufs.stride, bufs.M, bufs.m, T, ptr(bufs.ukeys),
                                                ptr(count), ptr(bufs.feat), ptr(flags), ptr(bufs.col_ws), bufs.col_ws.numel(), st))
    if fit:
        words = bufs.status.tolist()
        if (words[1] & 0xFFFFFFFF) & 1:
            raise _lib.SubgAccError(f"this batch has more than {T - 1} distinct LP rows: the count form has no column for them "
                                    f"(table_rows = {T} is the most the columns pass holds; use the row form, sample_and_gather)")
        T = max(int(words[2]) + 1, 2)
    return count, T


def _step_key_desc(bufs, form, own, partner, T, flags):
    """the descriptor of a join over the key rows of a step of `bufs`: its strided rows of 32-bit LP keys, the mirrored list
    (own, partner) and T columns.  A wide step (64-bit keys): the same descriptor over bufs.cols, the rows as 32-bit surrogate keys
    whose list bufs.ukeys is 1 .. c (subgacc_keyrows_columns64)"""
    return _lib.join_desc(form, JOIN_KEY32, row_len=bufs.nsize, n_rows=bufs.n, row_stride=bufs.stride, ids=bufs.ids,
                          payload=bufs.cols if bufs.wide else bufs.slot,
                          own=own, partner=partner, S=bufs.S, pair_block=bufs.batch, table_rows=T, num_walks=bufs.M, num_steps=bufs.m,
                          flags=flags)


def _counts_tail(bufs, own, partner, flags, st, fit):
    """the end of a step with stage="counts": the columns of the step's LP keys, then the count form over the key rows -- three
    launches, nothing allocated, nothing read back -> (C, table), views of the buffers.  fit (sample_and_counts without buffers and
    without table_rows): the number of distinct LP rows c is read back once and the count kernel runs with T = c + 1 columns into a
    tensor of that width, so that the GEMM behind it has no dead column."""
    L = lib()
    count, T = _step_columns(bufs, flags, st, fit)
    C = bufs.counts
    if fit:
        C = torch.empty((bufs.S, T), dtype=torch.float32, device=bufs.sizes.device)
    d = _step_key_desc(bufs, JOIN_COUNTS, own, partner, T, flags)
    with _timed("sjoin_key_counts"):
        check(L.subgacc_sjoin_key_counts(ctypes.byref(d), ptr(bufs.ukeys), ptr(count), ptr(C), ptr(bufs.sizes), st))
    return C, bufs.feat[:T]


def _index_tail(bufs, own, partner, flags, st, fit):
    """the end of a step with stage="index": the columns of the step's LP keys, the size pass, then the index form over the key rows --
    four launches, nothing allocated, nothing read back -> (pairs, table), views of the buffers (fit: as _counts_tail, T = c + 1)"""
    L = lib()
    n, S = bufs.n, bufs.S
    count, T = _step_columns(bufs, flags, st, fit)
    check(L.subgacc_sjoin_sizes_rows(ptr(bufs.nsize), n, ptr(own), ptr(partner), S, ptr(bufs.seg), ptr(flags), ptr(bufs.ws),
                                     bufs.ws.numel(), st))
    d = _step_key_desc(bufs, JOIN_ROWS, own, partner, T, flags)
    with _timed("sjoin_key_index"):
        check(L.subgacc_sjoin_key_index(ctypes.byref(d), ptr(bufs.ukeys), ptr(count), ptr(bufs.seg), ptr(bufs.pairs), ptr(bufs.sizes), st))
    return bufs.pairs, bufs.feat[:T]


def _buffered_step(csr, e, bufs, seed, out, fit=False):
    """sample_and_gather / sample_and_hgather through a StepBuffers: six launches, nothing allocated, nothing read back
    (StepBuffers(stage="counts"): the step of sample_and_counts / sample_and_hcounts -> (C, sizes, table, sets); fit: _counts_tail;
    stage="counts_attn": the same with the step's _StepAttnJoin in the place of C; stage="index": the step of sample_and_index ->
    (pairs, indptr, table, sets))"""
    from .sampler import _timed, _walk, make_cfg, sorted_worklist, walk_kernel_name, worklist_buffers
    L, st, dev = lib(), stream_ptr(), csr.device
    B, M, m, k, n, S = bufs.B, bufs.M, bufs.m, bufs.k, bufs.n, bufs.S      # n roots (rows), S segments
    PB = bufs.batch              # pairs per mirrored block of the segment list
    star = getattr(bufs, "star", 0)
    if star:        # e = (heads, tails): the sources (triplets: [u.. | v..]) and the P*K targets of StepBuffers(star=K)
        heads, tails = e if isinstance(e, tuple) and len(e) == 2 else (None, None)
        if heads is None or heads.numel() != n - B or tails.numel() != B or heads.dtype != torch.int64 or tails.dtype != torch.int64:
            raise ValueError(f"these StepBuffers were made for {bufs.P} " + ("pairs (u, v)" if bufs.triplets else "sources") +
                             f" against [{bufs.P}, {star}] targets (star={star})")
        heads, tails = heads.contiguous(), tails.contiguous()
    elif bufs.triplets:
        if tuple(e.shape) != (3, B):
            raise ValueError(f"these StepBuffers were made for [3, {B}] triplets")
    elif tuple(e.shape) != ((2, B) if PB == B else (B // PB, 2, PB)):
        raise ValueError(f"these StepBuffers were made for [2, {B}] pairs" if PB == B else
                         f"these StepBuffers were made for [{B // PB}, 2, {PB}] pairs")
    e = None if star else e.contiguous()
    flags = bufs.status.view(torch.int32)[:4]
    small = bool(getattr(bufs, "small", False))      # a small shape (a stage, or small_rows=True): subgacc_walk_keyrows_small writes the key rows
    cfg = make_cfg(csr, M, m, -1, seed, bufs.rng, records=(2 <= m <= 4) and not small,     # (only the fused-row kernel of 2..4 hops reads hop records)
                   row_pitch=bufs.stride if bufs.stride != bufs.Q else 0)
    rr = bufs.rng == "rand_r"
    check(L.subgacc_key_shift(cfg.num_walks, cfg.num_steps))
    kr = bufs.keyrows
    bufs.step_id = step_id = getattr(bufs, "step_id", 0) + 1
    tab = (ptr(bufs.table), 0 if kr else bufs.capacity)
    if bufs.dedup:      # first occurrences only: the other rows stay empty, the segment lists point at the first occurrence
        if not torch.cuda.is_current_stream_capturing():
            _dedup_tick(bufs)
        if bufs.triplets:       # roots [u | v | w], segment blocks u, w, v, w: first occurrences over all three roles
            check(L.subgacc_step_prologue_dedup_roles(*tab, ptr(bufs.status), 4, ptr(e), ptr(bufs.roots), ptr(bufs.own),
                                                      ptr(bufs.worklist), ptr(bufs.nsize), n, B, 3, 4, ptr(bufs.dedup_ws),
                                                      bufs.dedup_ws.numel(), ptr(bufs.n_distinct), st))
        else:
            check(L.subgacc_step_prologue_dedup(*tab, ptr(bufs.status), 4, ptr(e), ptr(bufs.roots), ptr(bufs.own), ptr(bufs.partner),
                                                ptr(bufs.worklist), ptr(bufs.nsize), n, ptr(bufs.dedup_ws), bufs.dedup_ws.numel(),
                                                ptr(bufs.n_distinct), st))
    elif star:          # the sources once, then the targets: one launch over the two arrays
        check(L.subgacc_step_prologue_star(*tab, ptr(bufs.status), 4, ptr(heads), n - B, ptr(tails), B, ptr(bufs.roots), st))
    else:
        check(L.subgacc_step_prologue(*tab, ptr(bufs.status), 4, ptr(e), ptr(bufs.roots), n, st))
    # the work list the walk kernel runs over.  Root dedup: its first occurrences (no sort by id there: what that order buys is mostly
    # repeated endpoints standing next to each other, and those are gone -- measured, cit2 walk kernel 0.647 ms either way, and the
    # sort costs its 25 us; a locality order groups distinct roots of one community: with order= they are walked in ascending rank).
    # Otherwise the rows stay where the batch has them and the fused-row kernel takes them in ascending order of their root's id
    # (or rank): roots that are neighbours in id space -- the same community of a graph with id locality -- are walked at the same
    # time on the same XCD and share its L2
    if bufs.dedup and bufs.order is None:
        work, bufs.walk_order = (bufs.worklist, bufs.n_distinct), "batch"
    elif bufs.dedup or (((bufs.order is not None) or (bufs.sort_roots and n >= SORT_ROOTS_MIN))
                        and (small or walk_kernel_name(csr, M, m, True) == "walk_rows_kernel")):
        if not hasattr(bufs, "sort_bufs"):        # (made on first use)
            bufs.sort_bufs = worklist_buffers(n, dev)
        work = sorted_worklist(csr, bufs.roots, n, bufs.order.rank if bufs.order is not None else None, bufs.sort_bufs, st)
        bufs.walk_order = "rank" if bufs.order is not None else "id"
    else:
        work, bufs.walk_order = None, "batch"
    if rr:
        check(L.subgacc_rng_positions(cfg, ptr(csr.indptr), csr.num_nodes, ptr(bufs.roots), n, 1, 0, ptr(bufs.rng_pos),
                                      ptr(bufs.rng_seed), ptr(bufs.rng_ws), bufs.rng_ws.numel(), st))
    with _timed("walk_sets"):         # (root dedup: the list selects the first occurrences, the other rows are passed over)
        _walk(cfg, csr, bufs.roots, n, flags, st,
              "keys_packed" if bufs.packed else "keys_small" if small else "keys64" if bufs.key64 else "fused", ids=bufs._ids, payload=bufs._slot,
              nsize=bufs.nsize, rng=(bufs.rng_pos, bufs.rng_seed) if rr else (None, None), table=bufs.table,
              capacity=0 if kr else bufs.capacity, work=work, select=bufs.dedup, nesc=bufs.nesc if bufs.packed else None)
    if bufs.dedup or star:      # (a star: the constant lists of its StepBuffers)
        own, partner = bufs.own, bufs.partner
    elif bufs.triplets:
        own, partner = _triplet_segments(B, dev), None
    else:
        own, partner = _arange_segments(B, dev, PB)
    if bufs.stage == "counts_attn":     # (C: the step's _StepAttnJoin -- the gate is the caller's, the kernel runs once it is there)
        T = _step_columns(bufs, flags, st, fit)[1]
        C, table = _StepAttnJoin(bufs, own, partner, T, step_id, flags), bufs.feat[:T]
    elif bufs.stage == "mean":          # (C: the step's _StepMeanJoin -- E = embed(table) is the caller's, the kernel runs once it is there)
        T = _step_columns(bufs, flags, st, fit)[1]
        C, table = _StepMeanJoin(bufs, own, partner, T, step_id, flags), bufs.feat[:T]
    elif bufs.stage == "attn":          # (C: the step's _StepFusedAttnJoin -- g and E = embed(table) are the caller's)
        T = _step_columns(bufs, flags, st, fit)[1]
        C, table = _StepFusedAttnJoin(bufs, own, partner, T, step_id, flags), bufs.feat[:T]
    elif bufs.stage == "counts":
        C, table = _counts_tail(bufs, own, partner, flags, st, fit)
    elif bufs.stage == "index":
        C, table = _index_tail(bufs, own, partner, flags, st, fit)
    if bufs.stage in _KEY_STAGES:
        bufs.sets = _step_sets(csr, bufs, cfg, rr, step_id)      # the step's status: what a caller of the stage functions resolves
        return C, (bufs.seg if bufs.stage == "index" else bufs.sizes), table, bufs.sets
    check(L.subgacc_sjoin_sizes_rows(ptr(bufs.nsize), n, ptr(own), ptr(partner), S, ptr(bufs.seg), ptr(flags), ptr(bufs.ws),
                                     bufs.ws.numel(), st))
    if kr:
        kind, payload = (JOIN_KEY64 if bufs.key64 else JOIN_KEY32), dict(num_walks=M, num_steps=m)
    else:
        keys = bufs.table[: bufs.capacity * 8].view(torch.int64)
        check(L.subgacc_unpack_lp(ptr(keys), bufs.capacity, None, M, m, None, None, ptr(bufs.feat), 1, st))
        kind, payload = JOIN_SFPTR, dict(table=bufs.feat, table_rows=bufs.capacity + 1, k=k)
    xz = _out_view(out if out is not None else bufs.out, dev, k, worst=S * bufs.Q, dtype=bufs.dtype)
    rows = dict(row_len=bufs.nsize, n_rows=n, row_stride=bufs.stride, ids=bufs._ids, payload=bufs._slot, own=own, partner=partner, S=S,
                seg=bufs.seg, pair_block=PB, flags=flags)
    if bufs.packed and bufs.half:     # one word per member and the escape lists, 16-bit rows (StepBuffers(dtype=, packed_half=True))
        with _timed("sjoin_fill_packed_half"):
            check(L.subgacc_sjoin_fill_packed_half(ctypes.byref(_lib.join_desc(JOIN_ROWS, kind, **rows, **payload)), ptr(bufs.nesc),
                                                   bufs.num_nodes, bufs.half, ptr(xz), st))
    elif bufs.packed:     # one word per member and the escape lists: the same rows of xz
        with _timed("sjoin_fill"):
            check(L.subgacc_sjoin_fill_packed(ctypes.byref(_lib.join_desc(JOIN_ROWS, kind, out_xz=xz, **rows, **payload)), ptr(bufs.nesc),
                                              bufs.num_nodes, st))
    elif bufs.half and bufs.segid is not None:      # 16-bit rows and their segment ids (a small shape: ptr=False, triplets)
        with _timed("sjoin_fill_half_ids"):
            check(L.subgacc_sjoin_fill_half_ids(ctypes.byref(_lib.join_desc(JOIN_ROWS, kind, **rows, **payload)), bufs.half, ptr(xz),
                                                ptr(bufs.segid), st))
    elif bufs.half:       # 16-bit rows (StepBuffers(dtype=): key rows of 32 bits, or -- wide_keys=True -- of 64; segment pointers)
        with _timed("sjoin_fill_half"):
            check(_fill_half(L, kind)(ctypes.byref(_lib.join_desc(JOIN_ROWS, kind, **rows, **payload)), bufs.half, ptr(xz), st))
    else:
        with _timed("sjoin_fill"):
            join_fill(JOIN_ROWS, kind, st, out_xz=xz, out_segid=bufs.segid, **rows, **payload)
    sets = _step_sets(csr, bufs, cfg, rr, step_id)
    # ptr=False / triplets: the ids of the first seg[-1] rows (as xz: a view of the whole buffer, the row count stays on the device)
    return xz, (bufs.seg if bufs.ptr else _with_pointers(bufs.segid[: xz.shape[0]], bufs.seg)), sets


def _small_call_refusals(kw, strided, dtype, lazy):
    """what sample_and_gather / sample_and_hgather refuse of small_rows=True at a small shape (_small_rows_wanted), by what they were given"""
    return {"key_rows=False (the one-wave kernel writes key rows)": not kw.get("key_rows", True),
            "packed_rows=True (no packed form at a small shape)": kw.get("packed_rows") is True,
            "packed_half=True (no packed form at a small shape)": bool(kw.get("packed_half")),
            "strided=False (a packed copy of the step's rows)": strided is False,
            "fused=False or a truncating bucket (the general kernel's)": kw.get("fused") is False or kw.get("bucket", -1) > 0,
            f"dtype={dtype} with lazy=True": bool(lazy) and dtype in (torch.float16, torch.bfloat16)}


def _small_rows_match(who, small_rows, buffers):
    """buffers= of the row form run the route they were made for: the keyword of the call must say the same"""
    if buffers is not None and getattr(buffers, "stage", None) is None and bool(small_rows) != bool(getattr(buffers, "small", False)):
        raise ValueError(f"{who}: small_rows={bool(small_rows)} but buffers= were made with small_rows={bool(getattr(buffers, 'small', False))}: "
                         "StepBuffers(..., small_rows=True) holds the key rows of the one-wave kernel, without it the table of the general one")


def _small_step(csr, e, seed, out, lazy, **how):
    """sample_and_gather / sample_and_hgather with small_rows=True and without buffers=: StepBuffers for this one call (as _step_counts
    makes them for the stages), the buffered step, and -- unless lazy -- the sets resolved and (xz, ids) cut to the step's rows.
    out=: as for StepBuffers, room for the worst case."""
    bufs = StepBuffers(csr, e.shape[1], small_rows=True, **how)
    xz, ind, sets = _buffered_step(csr, e, bufs, seed, out)
    if lazy:
        return xz, ind, sets
    sets.resolve()
    R = int(sets.extra[0])
    return xz[:R], (ind if bufs.ptr else _with_pointers(ind[:R], bufs.seg)), sets


def sample_and_gather(csr, edge, num_walks=200, num_steps=3, seed=111413, rng="philox", dedup_roots=False, out=None,
                      lazy=False, strided=None, buffers=None, order=None, ptr=True, small_rows=False, dtype=None, wide_keys=False, **kw):
    """The on-demand form of the path in one call: sample the endpoints of `edge` [2, B] (node ids), build their SpG
    rows, join -> (xz, indptr, sets), the same (xz, indptr) as `gather(edge, subg_matrix(G, arange(N)))` would give for sets
    drawn with the same RNG (Philox keys every walk by (seed, root id, walk, step), so a root's set does not depend on
    where or how often it appears).  `num_steps` = walk hops.

    dedup_roots=True samples every distinct endpoint once (needs rng="philox"): evaluation batches repeat a source
    against a thousand candidates (utils.py:92-95), so half of the endpoints of such a batch are duplicates.
    strided=None picks the joined-in-place form where the fused walk kernel is the faster one (spg.prefers_fused).
    buffers=StepBuffers(...): the same step without a single allocation or helper kernel (six launches; the result is
    lazy: sets.prefetch() / sets.resolve() as with lazy=True, xz is a view of out= or of the buffers' own output).
    order=LocalityOrder (sampler.locality_order) or an int32 rank [num_nodes]: the walk kernel takes the endpoints in that order
    (with buffers=, the StepBuffers' own order= is the one used); (xz, indptr) do not change, sets.walk_order says which ran.
    ptr=False: the second result is the segment id (0 .. 2B-1) of every row of xz, int64 [R], with the pointers as its
    .seg_pointers -- gather(ptr=False) of train.py:25-30, what the reference's --aggrs lstm runs with (main.py:217); the join
    writes the ids next to the rows.  With buffers=StepBuffers(..., ptr=False): a view of the buffers' id buffer, as xz is of
    the output buffer.
    dtype=torch.float16 / torch.bfloat16: xz in that type (sjoin(dtype=): bit for bit the float32 rows under .to(dtype), half the
    bytes written); the step's rows of 32-bit LP keys with segment pointers -- ValueError for ptr=False, lazy=True, key_rows=False,
    strided=False and a shape with 64-bit keys or without key rows.  buffers= must have been made with the same dtype.
    wide_keys=True (with a 16-bit dtype): a shape with 64-bit key rows (sampler.key_rows_form == 64: 4 hops, M = 128 .. 204 -- the
    paper's citation2 setting M = 200) is served too, by subgacc_sjoin_fill_half64 (include/subgacc_half64.h), buffered
    (StepBuffers(..., dtype=, wide_keys=True)) or not, with or without dedup_roots; the other refusals stand, and at a 32-bit shape
    the keyword changes nothing.
    small_rows=True: at a small shape (sampler.small_rows_form) the step of StepBuffers(..., small_rows=True) -- the one-wave kernel's
    key rows under the row-form join, the same (xz, indptr); dtype= goes with ptr=False there.  With buffers=, those must have been made
    with the keyword (and without it when the call has none); without buffers= a set is made for this one call, the sets are resolved
    and (xz, ids) are the step's rows (lazy=True: the unresolved views of the buffered step; out=: room for the worst case, 2B * (M*m+1)
    rows).  ValueError naming the keyword for key_rows=False, packed_rows=True, packed_half=True, strided=False, fused=False, a
    truncating bucket and a 16-bit dtype with lazy=True; at any other shape the keyword changes nothing."""
    from .sampler import as_rank, key_rows_form
    from .spg import sample_spg
    small_rows = _small_rows_wanted("sample_and_gather", small_rows, num_walks, num_steps, None, lambda: _small_call_refusals(kw, strided, dtype, lazy))
    half = _half_code(dtype, "sample_and_gather", lambda: {
        "ptr=False (segment ids)": not ptr and not small_rows, "lazy=True": lazy,
        "key_rows=False (strided rows of table slots)": not kw.get("key_rows", True),
        "strided=False (a packed copy of the step's rows)": strided is False,
        f"num_walks = {num_walks}, num_steps = {num_steps} (64-bit keys, or no key rows)":
            _half_shape_refused(num_walks, num_steps, wide_keys, small_rows)})
    half64 = bool(half) and key_rows_form(int(num_walks), int(num_steps)) == 64
    if buffers is not None and (half != getattr(buffers, "half", 0) or half64 != bool(getattr(buffers, "half64", False))):
        raise ValueError(f"sample_and_gather: dtype={dtype}{', wide_keys=True' if half64 else ''} but buffers= were made with "
                         f"dtype={getattr(buffers, 'dtype', None)}{', wide_keys=True' if getattr(buffers, 'half64', False) else ''}: "
                         "StepBuffers(..., dtype=) allocates `out` in the type the step writes")
    _small_rows_match("sample_and_gather", small_rows, buffers)
    order = as_rank(csr, order)
    e = _as_rows(edge, csr.device)
    if buffers is None and e.dim() != 2:
        raise ValueError("sample_and_gather: edge must be [2, B] (many batches at once: sample_and_gather_many)")
    B = e.shape[-1]
    if buffers is not None:     # the allocation-free form of a serving loop: same rows, same (xz, indptr), lazily resolved
        if buffers.triplets or bool(ptr) != buffers.ptr or buffers.stage is not None:
            raise ValueError("buffers= were made for another result: StepBuffers(..., ptr=False) serves ptr=False, "
                             "StepBuffers(..., triplets=True) serves sample_and_hgather, StepBuffers(..., stage='counts') "
                             "sample_and_counts")
        if (dedup_roots and not buffers.dedup) or rng != buffers.rng or strided is False or kw.get("fused") is False or \
                kw.get("bucket", -1) > 0 or (num_walks, num_steps) != (buffers.M, buffers.m) or \
                kw.get("uniq_capacity", buffers.capacity) != buffers.capacity:
            raise ValueError("buffers= serves the on-demand step (the StepBuffers' rng, fused strided rows; root dedup if the StepBuffers "
                             "were made with dedup_roots=True) of the shape the StepBuffers were made for")
        if order is not None and (buffers.order is None or order.rank is not buffers.order.rank):
            raise ValueError("buffers= walks in the order its StepBuffers were made with: pass order= to StepBuffers(...)")
        return _buffered_step(csr, e, buffers, seed, out)
    if small_rows:      # the same step through buffers made for this one call
        return _small_step(csr, e, seed, out, lazy, num_walks=num_walks, num_steps=num_steps, dedup_roots=dedup_roots, rng=rng, order=order,
                           ptr=bool(ptr), dtype=dtype, sort_roots=kw.get("sort_roots", True))
    if dedup_roots:
        if rng != "philox":
            raise ValueError("dedup_roots=True needs rng='philox' (rand_r sets depend on the position in the stream)")
        roots, inv = torch.unique(e.reshape(-1), return_inverse=True)
        rows = inv.view(2, B)
    else:
        roots = e.reshape(-1)
        rows = None                   # row i of the batch's SpG = endpoint i: the segment lists are constants of B
    if strided is None:
        strided = True        # a transient batch: joined in place, whichever walk kernel made the rows
    if strided:       # joined by table slot below: the distinct LP rows need no numbering (SampledSets.number() does it on demand)
        kw.setdefault("number_rows", False)
    z, sets = sample_spg(csr, roots.to(torch.int32), num_walks=num_walks, num_steps=num_steps, seed=seed, rng=rng, lazy=lazy,
                         strided=strided, order=order, **kw)
    table = z.slot_table() if sets.strided else sets.feature_table()
    if rows is not None:
        xz, ind = gather(rows, z, e.device, ptr=bool(ptr), encode=table, out=out, lazy=lazy, dtype=dtype, wide_keys=wide_keys)
    else:
        own, partner = _arange_segments(B, e.device)
        xz, ind = _checked(*sjoin(_as_spg(z), own, partner, table, ptr_mode=bool(ptr), pair_block=B, out=out, lazy=lazy, dtype=dtype,
                                  wide_keys=wide_keys), lazy=lazy)
    if lazy:      # the join's status word travels with the sets' own: resolve() raises IndexError for a row outside the store
        sets._join_flags = getattr(ind, "join_flags", None)
    return xz, ind, sets


def _as_triplets(hedge, device, who):
    """[3, B] triplets (u, v, w) as an int64 device tensor, or ValueError"""
    h = _as_rows(hedge, device)
    if h.dim() != 2 or h.shape[0] != 3:
        raise ValueError(f"{who}: hedge must be [3, B] triplets (u, v, w), not {list(h.shape)}")
    return h


def sample_and_hgather(csr, hedge, num_walks=200, num_steps=3, seed=111413, rng="philox", dedup_roots=False, out=None, buffers=None,
                       order=None, small_rows=False, dtype=None, **kw):
    """The on-demand form of hgather (train.py:48-72, the batches of main_horder.py / train.py:142-172) in one call: the three
    roles of `hedge` [3, B] (node ids u, v, w) are walked ONCE each -- 3B roots, not the 4B that two pair steps (u, w) and (v, w)
    would walk -- and joined as [U|w ; W|u ; V|w ; W|v] -> (xz, ids, sets): bit for bit the (xz, ids) of
    `hgather(hedge, z, encode=table)` over a store z sampled for all nodes with the same seed (Philox keys every walk by (seed,
    root id, walk, step)), ids int64 [R] = segment ids 0 .. 4B-1 with their pointers as .seg_pointers.  `num_steps` = walk hops.
    dedup_roots=True samples every distinct node of the batch once, whatever its roles: the model's negatives keep (u, v) of their
    positive and replace w (dataloader.py:265-268, 275), so two of the three roots of every negative are repeats.
    buffers=StepBuffers(csr, B, ..., triplets=True): the allocation-free six-launch step (xz and ids are views of the buffers,
    their first ids.seg_pointers[-1] rows are the result; sets.prefetch() / sets.resolve() as for sample_and_gather).
    rng: "philox" only -- the reference never samples triplets in a rand_r stream, there is nothing to reproduce.
    order=: as for sample_and_gather.
    small_rows=True: at a small shape (sampler.small_rows_form: DBLP-coauthor's M = 100, 2 hops) the step of
    StepBuffers(..., triplets=True, small_rows=True), with buffers= made so or with a set made for this one call (resolved, (xz, ids)
    cut to the step's rows); the same (xz, ids).  dtype=torch.float16 / torch.bfloat16: xz in that type, bit for bit xz.to(dtype) --
    with small_rows=True at such a shape only (ValueError elsewhere: no other triplet step writes 16-bit rows), buffers= made with the
    same dtype.  ValueError naming the keyword as for sample_and_gather; at any other shape it changes nothing."""
    from .sampler import as_rank
    from .spg import sample_spg
    if rng != "philox":
        raise ValueError("sample_and_hgather samples with rng='philox' (a rand_r set depends on its root's place in a stream the "
                         "reference never draws for triplets)")
    small_rows = _small_rows_wanted("sample_and_hgather", small_rows, num_walks, num_steps, None, lambda: _small_call_refusals(kw, None, dtype, False))
    half = _half_code(dtype, "sample_and_hgather", lambda: {
        "triplets (16-bit rows with segment ids are those of small_rows=True at a small shape, sampler.small_rows_form)": not small_rows})
    if buffers is not None and half != getattr(buffers, "half", 0):
        raise ValueError(f"sample_and_hgather: dtype={dtype} but buffers= were made with dtype={getattr(buffers, 'dtype', None)}: "
                         "StepBuffers(..., dtype=) allocates `out` in the type the step writes")
    _small_rows_match("sample_and_hgather", small_rows, buffers)
    order = as_rank(csr, order)
    h = _as_triplets(hedge, csr.device, "sample_and_hgather")
    B = h.shape[1]
    if small_rows and buffers is None:      # the same step through buffers made for this one call
        return _small_step(csr, h, seed, out, False, num_walks=num_walks, num_steps=num_steps, dedup_roots=dedup_roots, order=order,
                           triplets=True, dtype=dtype, sort_roots=kw.get("sort_roots", True))
    if buffers is not None:
        if not buffers.triplets or buffers.stage is not None or (dedup_roots and not buffers.dedup) or \
                (num_walks, num_steps) != (buffers.M, buffers.m) or kw.get("uniq_capacity", buffers.capacity) != buffers.capacity or kw.get("fused") is False or kw.get("bucket", -1) > 0:
            raise ValueError("buffers= serves the triplet step of the shape its StepBuffers(..., triplets=True) were made for (root "
                             "dedup if they were made with dedup_roots=True)")
        if order is not None and (buffers.order is None or order.rank is not buffers.order.rank):
            raise ValueError("buffers= walks in the order its StepBuffers were made with: pass order= to StepBuffers(...)")
        return _buffered_step(csr, h, buffers, seed, out)
    kw.setdefault("number_rows", False)     # joined by table slot: the distinct LP rows need no numbering
    if dedup_roots:
        roots, inv = torch.unique(h.reshape(-1), return_inverse=True)
        u, v, w = inv.view(3, B)
        own = torch.cat([u, w, v, w])
    else:
        roots = h.reshape(-1)
        own = _triplet_segments(B, h.device)      # row i of the batch's SpG = root i of [u | v | w]
    z, sets = sample_spg(csr, roots.to(torch.int32), num_walks=num_walks, num_steps=num_steps, seed=seed, rng=rng, strided=True,
                         order=order, **kw)
    table = z.slot_table() if sets.strided else sets.feature_table()
    xz, ids = _checked(*sjoin(_as_spg(z), own, None, table, ptr_mode=False, pair_block=B, out=out))
    return xz, ids, sets


def _step_counts(who, csr, e, triplets, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, stage="counts",
                 wide_keys=False, star=0):
    """sample_and_counts / sample_and_hcounts: the step with stage="counts" through the caller's StepBuffers, or through a set made for
    this one call (stage="counts_attn": sample_and_attn_counts, which checks the step itself once its kernel has run).  star=K: e =
    (heads, tails) of the step of one source against K targets (StepBuffers(star=K))"""
    from .sampler import as_rank, key_rows_form
    order = as_rank(csr, order)
    wide = bool(wide_keys) and key_rows_form(int(num_walks), int(num_steps)) == 64     # (the keyword means nothing at any other shape)
    pairs = e[1].numel() if star else e.shape[1]
    if buffers is not None:
        if buffers.stage != stage or buffers.triplets != triplets or getattr(buffers, "star", 0) != star or (star and buffers.B != pairs):
            raise ValueError(f"{who}: buffers= must be StepBuffers(..., stage='{stage}'" + (", triplets=True" if triplets else "") +
                             (f", star={star}) for {pairs} pairs" if star else ")"))
        if (dedup_roots and not buffers.dedup) or (num_walks, num_steps) != (buffers.M, buffers.m) or \
                (table_rows is not None and int(table_rows) != buffers.T) or wide != bool(getattr(buffers, "wide", False)):
            raise ValueError(f"{who}: buffers= serves the step its StepBuffers were made for (num_walks, num_steps, table_rows; root "
                             "dedup if they were made with dedup_roots=True)")
        if order is not None and (buffers.order is None or order.rank is not buffers.order.rank):
            raise ValueError("buffers= walks in the order its StepBuffers were made with: pass order= to StepBuffers(...)")
        return _buffered_step(csr, e, buffers, seed, None)
    fit = table_rows is None
    T = (COUNTS_MAX_TABLE_ROWS_WIDE if wide else COUNTS_MAX_TABLE_ROWS) if fit else int(table_rows)
    _counts_stage_shape(who, num_walks, num_steps, True, T, wide_keys)
    bufs = (_FitStepBuffers if fit else StepBuffers)(csr, pairs, num_walks=num_walks, num_steps=num_steps, dedup_roots=dedup_roots,
                                                     order=order, triplets=triplets, stage=stage, table_rows=T, wide_keys=wide_keys,
                                                     star=star or None, width=_WIDTH_OF_CALL if stage in _WIDTH_STAGES else None)
    C, sizes, table, sets = _buffered_step(csr, e, bufs, seed, None, fit=fit)
    if stage not in ("counts_attn", "mean", "attn"):        # (those check the step themselves once their kernel has run)
        sets.resolve()
    return C, sizes, table, sets


def sample_and_counts(csr, edge, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None, buffers=None,
                      wide_keys=False):
    """The count form of the on-demand step: sample the endpoints of `edge` [2, B] and join their key rows as COUNTS ->
    (C float32 [2B, T], sizes int32 [2B], table float32 [T, m+1], sets).  C[j, p] = how often row p of `table` occurs in either feature
    slot of segment j (gather()'s segments: left blocks, then right blocks), p = 0 the zero row of a member without a partner; sizes =
    the segments' row counts; table = [0-row ; the batch's distinct LP rows / M] in ascending order of their packed keys.  The rows
    gather_counts(edge, z, ...) counts over the all-nodes store z of the same seed are these rows, under the store's own numbering:
    segment_sum_j(f(xz).sum(-2)) == C[j] @ f(table) for the (xz, indptr) of sample_and_gather.  A column is its key's RANK among the
    batch's distinct keys, so (C, sizes, table) are the same bits whatever the schedule, the walk order (order=), root dedup
    (dedup_roots=True: Philox as ever) and whether buffers are used.  Neither xz nor an output buffer of the row form exists.
    table_rows=None (no buffers): the number of distinct LP rows is read back once and T is exactly that + 1.  table_rows=T: T columns,
    the columns past the batch's distinct rows zero; more distinct rows than T - 1 raise SubgAccError.
    buffers=StepBuffers(csr, B, ..., stage="counts", table_rows=T): nothing is allocated and nothing read back (capturable); C, sizes
    and table are views of the buffers, and sets.resolve() raises SubgAccError naming table_rows when the step had more distinct LP
    rows than columns (C is then not to be used).  Shapes: 32-bit key rows -- 2 to 4 hops with num_steps*SHIFT+1 <= 31 over a 512- or
    1,024-slot table (sampler.key_rows_form == 32), and the small shapes, 1 to 4 hops with M*m+1 <= 204 (sampler.small_rows_form:
    csrc/walk_small.hip writes their rows); rng Philox.
    wide_keys=True (here and on the seven other stage calls -- sample_and_hcounts, sample_and_mean_stage, sample_and_hmean_stage,
    sample_and_attn_counts, sample_and_attn_stage, sample_and_index, sample_and_lstm_stage -- and on StepBuffers): the shapes with 64-bit
    keys too (sampler.key_rows_form == 64: 4 hops, M = 128 .. 204, the paper's citation2 setting M = 200), with the same results under
    the same rules; the columns pass is subgacc_keyrows_columns64 and table_rows is at most 8,192 there (ValueError before any device
    work; without table_rows a batch of more than 8,191 distinct LP rows raises SubgAccError).  It changes nothing at a shape with 32-bit
    or small key rows.  With buffers= the buffers' own setting holds: they must have been made with the same wide_keys."""
    e = _as_rows(edge, csr.device)
    if e.dim() != 2 or e.shape[0] != 2:
        raise ValueError(f"sample_and_counts: edge must be [2, B], not {list(e.shape)}")
    return _step_counts("sample_and_counts", csr, e, False, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                        wide_keys=wide_keys)


def sample_and_hcounts(csr, hedge, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None,
                       buffers=None, wide_keys=False):
    """sample_and_counts for the triplets `hedge` [3, B] (u, v, w) of the higher-order model: 3B roots walked once each, hgather's 4B
    segments [U|w ; W|u ; V|w ; W|v] -> (C float32 [4B, T], sizes int32 [4B], table, sets); the rows hgather_counts(hedge, z, ...)
    counts.  buffers=StepBuffers(csr, B, ..., triplets=True, stage="counts", table_rows=T)."""
    h = _as_triplets(hedge, csr.device, "sample_and_hcounts")
    return _step_counts("sample_and_hcounts", csr, h, True, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                        wide_keys=wide_keys)


def _step_mean(C, sizes, table, sets, embed, blocks):
    """(C @ embed(table)) / sizes as [blocks, B, H]; a segment of size 0 (a zero row of C) gives a zero row"""
    out = (C @ embed(table)) / sizes.clamp(min=1).to(torch.float32)[:, None]
    return out.view(blocks, -1, out.shape[-1])


def sample_and_mean_stage(csr, edge, embed, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None,
                          buffers=None, wide_keys=False):
    """The reference's first model stage for mean aggregation (model.py:78-83: x = pe_embedding(xz).sum(dim=-2); xl, xr =
    MeanAggregation(x, ptr).view(2, -1, H)) on the on-demand step: (C @ embed(table)) / sizes with (C, sizes, table) =
    sample_and_counts(csr, edge, ...) -- mean_stage's algebra without a resident store, and without xz [R,2,k] or the [R,2,H]
    activations.  `embed` is any row-wise module; autograd reaches its parameters through the small [T, H] activation (C is a constant
    of the batch).  Returns float32 [2, B, H] (left endpoints, right endpoints), empty segments as zero rows.  Without buffers the step
    is checked before the result is returned.  With buffers= nothing is read back, as for every buffered step: the step's SampledSets
    are `buffers.sets`, and `buffers.sets.resolve()` (after `.prefetch()`, if the loop queues ahead) raises SubgAccError when the step
    had more distinct LP rows than table_rows - 1 -- its result is then not to be used."""
    return _step_mean(*sample_and_counts(csr, edge, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys),
                      embed, 2)


def sample_and_hmean_stage(csr, hedge, embed, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None,
                           buffers=None, wide_keys=False):
    """HONet's first stage (model_horder.py:56-57: scatter_mean(pe_embedding(xz).sum(-2), ind).view(4, -1, H)) on the on-demand triplet
    step: hmean_stage's algebra over sample_and_hcounts.  Returns float32 [4, B, H] in the order (xu, xwu, xv, xwv); with buffers= the
    step is checked through `buffers.sets.resolve()`, as for sample_and_mean_stage."""
    return _step_mean(*sample_and_hcounts(csr, hedge, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys),
                      embed, 4)


class _StepAttnJoin:
    """the two library calls of sample_and_attn_counts (subgacc_sjoin_key_counts_attn / _backward) over the key rows of ONE step of
    `bufs`: the descriptor of _counts_tail, the step's stamp.  The backward joins the step's rows again, and with buffers= those rows
    live until the buffers take their next step: a backward that comes later is refused, never answered from another batch.
    bufs = None: an empty batch, nothing is launched."""
    who = "sample_and_attn_counts"

    def __init__(self, bufs, own, partner, T, step_id, flags, dev=None):
        self.bufs, self.own, self.partner, self.T, self.step_id, self.flags = bufs, own, partner, int(T), step_id, flags
        self.S = bufs.S if bufs is not None else 0
        self.dev = bufs.sizes.device if bufs is not None else dev

    def desc(self):
        return _step_key_desc(self.bufs, JOIN_COUNTS, self.own, self.partner, self.T, self.flags)

    def _require_fresh(self, what):
        now = getattr(self.bufs, "step_id", 0)
        if now != self.step_id:
            raise RuntimeError(f"{self.who}: the {what} of step {self.step_id} of these StepBuffers ran after they took "
                               f"step {now}: the rows it joins are gone (run a step's backward before the buffers' next step)")

    def forward(self, g, keep):
        S, T, dev, b = self.S, self.T, self.dev, self.bufs
        own = b is None or b.counts is None         # no buffers of the caller's: tensors of this call
        W = torch.empty((S, T), dtype=torch.float32, device=dev) if own else b.counts.detach()
        mx = den = None
        if keep:
            mx, den = (torch.empty(S, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev)) if own \
                else (b.smax.detach(), b.sden.detach())
        if b is None:
            return W, mx, den
        self._require_fresh("kernel")
        with _timed("sjoin_key_counts_attn"):
            d = self.desc()
            check(lib().subgacc_sjoin_key_counts_attn(ctypes.byref(d), ptr(b.ukeys), ptr(b.status[2:3]), ptr(g), ptr(W), ptr(mx), ptr(den),
                                                      ptr(b.sizes), stream_ptr()))
        return W, mx, den

    def backward(self, g, dW, W, mx, den):
        # zeros, not empty: the kernel writes every row of every pair it joins, but a pair that raises a flag is left unwritten, Dg is
        # summed over the segments at once and a buffered step reads no flag back before that sum
        Dg = torch.zeros_like(W)
        b = self.bufs
        if b is None:
            return Dg
        self._require_fresh("backward")
        with _timed("sjoin_key_counts_attn_backward"):
            d = self.desc()
            check(lib().subgacc_sjoin_key_counts_attn_backward(ctypes.byref(d), ptr(b.ukeys), ptr(b.status[2:3]), ptr(g), ptr(dW), ptr(W),
                                                               ptr(mx), ptr(den), ptr(Dg), stream_ptr()))
        return Dg


def _step_attn(who, csr, edge, gate, bias, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys=False, star=0):
    """sample_and_attn_counts with gate(table, count) -- count: the number of distinct LP rows c, int64 [1] on the device -- and the
    gate's bias (None: none) as an input of the autograd function -> (W, sizes, table, sets, count).  star=K: edge = (heads, tails)
    of _star_step_rows, the step of one source against K targets"""
    if star:
        e = edge
    else:
        e = _as_rows(edge, csr.device)
        if e.dim() != 2 or e.shape[0] != 2:
            raise ValueError(f"{who}: edge must be [2, B], not {list(e.shape)}")
    if not star and e.shape[1] == 0 and buffers is None:     # an empty batch: no step, the zero row alone
        T = 2 if table_rows is None else int(table_rows)
        _counts_stage_shape(who, num_walks, num_steps, True, T, wide_keys)
        dev = csr.device
        join = _StepAttnJoin(None, None, None, T, 0, None, dev)
        sizes, table = torch.empty(0, dtype=torch.int32, device=dev), torch.zeros((T, int(num_steps) + 1), dtype=torch.float32, device=dev)
        sets, count = None, torch.zeros(1, dtype=torch.int64, device=dev)
    else:
        join, sizes, table, sets = _step_counts(who, csr, e, False, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                                                stage="counts_attn", wide_keys=wide_keys, star=star)
        count = join.bufs.status[2:3]
    g = gate(table, count)
    if not (torch.is_tensor(g) and g.shape == (join.T,) and g.dtype == torch.float32 and g.device == table.device):
        raise ValueError(f"{who}: gate(table) must be a float32 [{join.T}] tensor on {table.device}, one logit per row of table")
    if torch.is_grad_enabled() and (g.requires_grad or (bias is not None and bias.requires_grad)):
        W = _CountsAttn.apply(g, bias, join)
    else:
        W = join.forward(g.detach().contiguous(), False)[0]
    if buffers is None and sets is not None:
        sets.resolve()
    return W, sizes, table, sets, count


def sample_and_attn_counts(csr, edge, gate, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None,
                           buffers=None, wide_keys=False):
    """The attentional count form of the on-demand step: sample the endpoints of `edge` [2, B], number the batch's distinct LP rows as
    sample_and_counts does, and join the key rows as SOFTMAX-WEIGHTED counts -> (W float32 [2B, T], sizes int32 [2B], table float32
    [T, m+1], sets).  gate: a callable table -> g float32 [T], the gate's logit of every row of `table` (row 0 = partner absent; the rows
    past the batch's distinct LP rows are zero rows, whose logits no segment reads).  Member t of segment j is the index pair (p_t,
    q_t) of its own and its partner's row of `table`, its logit g[p_t] + g[q_t], and
        W[j, r] = sum_t softmax_j(l)_t ([p_t = r] + [q_t = r])
    -- what counts_attn_stage's kernel writes over the all-nodes store of the same seed, under the store's own numbering, bit for bit
    (subgacc_sjoin_key_counts_attn: documented summation chains, no float atomics), so W[j] @ f(table) is the attentional aggregation
    of f(xz).sum(-2) over segment j.  W is differentiable with respect to g (subgacc_sjoin_key_counts_attn_backward, summed over the
    segments).  A column is its key's rank: one result whatever the schedule, the walk order, root dedup and buffers.
    table_rows, buffers=StepBuffers(csr, B, ..., stage="counts_attn", table_rows=T), sets: as for sample_and_counts; without buffers the
    step is checked (sets.resolve()) before the result is returned.  With buffers nothing is allocated by the sampling part and nothing
    read back (capturable); W, sizes and table are views of the buffers, and the backward, which joins the step's rows again, must run
    before the buffers take their next step: later it raises RuntimeError naming the step, it never answers from another batch."""
    return _step_attn("sample_and_attn_counts", csr, edge, lambda table, count: gate(table), None, num_walks, num_steps, seed, dedup_roots, order, table_rows,
                      buffers, wide_keys)[:4]


def sample_and_attn_stage(csr, edge, embed, gate_nn, value_nn=None, num_walks=200, num_steps=3, seed=111413, dedup_roots=False,
                          order=None, table_rows=None, buffers=None, wide_keys=False):
    """The reference's first model stage of the LP encoder for --aggr attn (model.py:59-62,78-81: x = pe_embedding(xz).sum(dim=-2);
    xl, xr = AttentionalAggregation(gate_nn, nn)(x, ptr=ptr).view(2, -1, H'')) on the on-demand step -- counts_attn_stage's algebra
    without a resident store, and without xz [R,2,k], the [R,2,H] activations or the pair rows:
        E = embed(table),  g = (E - centre) wg,  out_j = nn(W[j] @ E) [n_j > 0]     with (W, sizes, table) = sample_and_attn_counts(...)
    centre is the detached mean of E over the LIVE rows 0 .. c of the table (c = the batch's distinct LP rows, taken on the device from
    the step's count word as a mask: nothing is read back): softmax drops the constant, so the result does not depend analytically on
    table_rows, and the dead rows past c -- embed of a zero row is not zero -- do not move the centre.  embed: any row-wise module;
    gate_nn: nn.Linear(H, 1) or a one-Linear Sequential; value_nn: None or nn.Linear(H, H'') (PyG 2.2's MLP([H, 1]) / MLP([H, H]) is that
    Linear, .lins[0]).  Every parameter of embed, gate_nn and value_nn receives a gradient; the gate bias's is exactly zero, as the
    reference's is analytically.  Returns float32 [2, B, H''] (H without value_nn), empty segments as zero rows.  Keywords as
    sample_and_attn_counts; with buffers= the step's SampledSets are `buffers.sets` (`.resolve()` raises when the step had more distinct
    LP rows than table_rows - 1), and the backward must run before the buffers take their next step (RuntimeError otherwise)."""
    return _attn_stage("sample_and_attn_stage", csr, edge, embed, gate_nn, value_nn, num_walks, num_steps, seed, dedup_roots, order,
                       table_rows, buffers, wide_keys)


def _attn_stage(name, csr, edge, embed, gate_nn, value_nn, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                wide_keys=False, star=0):
    """sample_and_attn_stage; star=K: sample_and_attn_stage_star with edge = (heads, tails) of _star_step_rows"""
    other = "sample_and_gather(csr, edge, ...) and the modules on xz"
    gate = _one_linear(gate_nn, "gate_nn", None, 1, name, other)
    H = gate.in_features
    val = _one_linear(value_nn, "value_nn", H, None, name, other) if value_nn is not None else None
    dev = csr.device
    for mod in (gate, val, embed):
        for prm in (mod.parameters() if mod is not None else ()):
            if prm.device != dev or prm.dtype != torch.float32:
                raise ValueError(f"{name}: embed, gate_nn and value_nn must hold float32 parameters on the graph's device ({dev})")
    box = {}

    def logits(table, count):
        E = box["E"] = embed(table)
        if E.ndim != 2 or E.shape[0] != table.shape[0] or E.shape[1] != H:
            raise ValueError(f"{name}: embed(table) is {tuple(E.shape)}, gate_nn takes rows of {H}")
        live = (torch.arange(table.shape[0], device=dev) <= count).to(torch.float32)        # rows 0 .. c, from the step's count word
        centre = (E.detach() * live[:, None]).sum(0) / (count + 1).to(torch.float32)
        return (E - centre) @ gate.weight.view(-1)

    W, sizes, table, sets, _ = _step_attn(name, csr, edge, logits, gate.bias, num_walks, num_steps, seed, dedup_roots, order, table_rows,
                                          buffers, wide_keys, star)
    h = W @ box["E"]
    if val is not None:
        h = torch.nn.functional.linear(h, val.weight, val.bias)
    out = h * (sizes > 0).to(h.dtype)[:, None]
    return out.view(2, -1, out.shape[-1])


# ------------------------------------------------------------------------------ the on-demand step for one source against K targets
def _star_step_rows(who, csr, heads, targets, triplets):
    """the arguments of a *_star call as the step takes them: (heads int64 [P] -- triplets: [2, P] --, tails int64 [P*K], P, K) on the
    graph's device, checked on the host by _star_rows first"""
    dev = csr.device
    if triplets:
        uv = _as_rows(heads, dev)
        if uv.dim() != 2 or uv.shape[0] != 2:
            raise ValueError(f"{who}: uv must be [2, P] pairs (u, v), not {list(uv.shape)}")
        _, targets = _star_rows(uv[0], targets)
        heads = uv.contiguous()
    else:
        source, targets = _star_rows(heads, targets)
        heads = _as_rows(source, dev).contiguous()
    P, K = int(targets.shape[0]), int(targets.shape[1])
    return heads, _as_rows(targets, dev).reshape(-1).contiguous(), P, K


def _star_buffers_match(who, buffers, P, K, triplets, num_walks, num_steps, order, ptr=None, dtype=None, wide_keys=False, small_rows=False):
    """buffers= of a row-form *_star call: StepBuffers(csr, P*K, ..., star=K) of this call's geometry, shape and result"""
    from .sampler import key_rows_form
    if getattr(buffers, "star", 0) != K or buffers.B != P * K or buffers.triplets != triplets or buffers.stage is not None or \
            (ptr is not None and bool(ptr) != buffers.ptr) or (num_walks, num_steps) != (buffers.M, buffers.m):
        raise ValueError(f"{who}: buffers= were made for another geometry or result: this call takes StepBuffers(csr, {P * K}, num_walks="
                         f"{num_walks}, num_steps={num_steps}, star={K}" + (", triplets=True)" if triplets else f", ptr={bool(ptr)})"))
    half = _half_code(dtype, who, dict)
    half64 = bool(half) and key_rows_form(int(num_walks), int(num_steps)) == 64 and bool(wide_keys)
    if half != getattr(buffers, "half", 0) or (half and half64 != bool(getattr(buffers, "half64", False))):
        raise ValueError(f"{who}: dtype={dtype} but buffers= were made with dtype={getattr(buffers, 'dtype', None)}: "
                         "StepBuffers(..., dtype=) allocates `out` in the type the step writes")
    _small_rows_match(who, _small_rows_wanted(who, small_rows, num_walks, num_steps, None, dict), buffers)
    if order is not None and (buffers.order is None or order.rank is not buffers.order.rank):
        raise ValueError("buffers= walks in the order its StepBuffers were made with: pass order= to StepBuffers(...)")


def _star_step(csr, e, pairs, seed, out, lazy, **how):
    """a row-form *_star call without buffers=: StepBuffers(star=K) for this one call, the buffered step, and -- unless lazy -- the sets
    resolved and (xz, ids) cut to the step's rows (as _small_step)"""
    bufs = StepBuffers(csr, pairs, out=out, **how)
    xz, ind, sets = _buffered_step(csr, e, bufs, seed, None)
    if lazy:
        return xz, ind, sets
    sets.resolve()
    R = int(sets.extra[0])
    return xz[:R], (ind if bufs.ptr else _with_pointers(ind[:R], bufs.seg)), sets


def sample_and_gather_star(csr, source, targets, num_walks=200, num_steps=3, seed=111413, out=None, lazy=False, buffers=None, order=None,
                           ptr=True, small_rows=False, dtype=None, wide_keys=False, packed_rows=None, packed_half=False, sort_roots=True):
    """The on-demand step for the shape the reference evaluates with -- one source against K candidates (utils.py:93-95, joined batch
    by batch in train.py:246-280) -- without the expanded edge tensor: source int [P], targets int [P, K] (NumPy or torch, checked as
    gather_star checks them).  Returns bit for bit what
        sample_and_gather(csr, stack([source.repeat_interleave(K), targets.reshape(-1)]), ...)
    returns with the same seed -- xz, indptr (ptr=False: the segment ids), the status flags -- while the step walks P + P*K roots
    instead of 2*P*K: every source is sampled ONCE and K segments point at its row (StepBuffers(star=K)).  No hash, no extra launch:
    the shape itself says which roots are repeats, and Philox keys a walk by (seed, root id, walk, hop), so a set does not depend on
    where or how often its root stands.  A node that is a target twice, or a source of two stars, is walked as often as it stands.
    buffers=StepBuffers(csr, P*K, ..., star=K): the allocation-free step (six launches for the row form; lazy, views of the
    buffers, sets.prefetch() / sets.resolve() as for sample_and_gather).  Without buffers= a set is made for this one call, the sets
    are resolved and (xz, ids) are the step's rows (lazy=True: the unresolved views; out=: room for the worst case, 2*P*K * (M*m+1)
    rows).  ptr=, dtype=, wide_keys=, small_rows=, packed_rows=, packed_half=, order= and sort_roots are StepBuffers' keywords under
    StepBuffers' rules.  Philox only, and no root dedup on top.  P*K = 0: what the expanded call returns for [2, 0]."""
    from .sampler import as_rank
    who = "sample_and_gather_star"
    heads, tails, P, K = _star_step_rows(who, csr, source, targets, False)
    order = as_rank(csr, order)
    if buffers is not None:
        _star_buffers_match(who, buffers, P, K, False, num_walks, num_steps, order, ptr, dtype, wide_keys, small_rows)
        return _buffered_step(csr, (heads, tails), buffers, seed, out)
    if P * K == 0:
        return sample_and_gather(csr, _no_pairs(csr), num_walks, num_steps, seed, out=out,
                                 lazy=lazy, order=order, ptr=ptr, small_rows=small_rows, dtype=dtype, wide_keys=wide_keys)
    return _star_step(csr, (heads, tails), P * K, seed, out, lazy, num_walks=num_walks, num_steps=num_steps, star=K, order=order,
                      ptr=bool(ptr), small_rows=small_rows, dtype=dtype, wide_keys=wide_keys, packed_rows=packed_rows,
                      packed_half=packed_half, sort_roots=sort_roots)


def sample_and_hgather_star(csr, uv, w, num_walks=200, num_steps=3, seed=111413, out=None, buffers=None, order=None, small_rows=False,
                            dtype=None, sort_roots=True):
    """sample_and_gather_star for the higher-order model's evaluation: a triplet whose (u, v) is kept and whose w is replaced by K
    candidates (dataloader.py:265-275, eval_model_horder, train.py:283-317).  uv int [2, P], w int [P, K].  Returns bit for bit what
        sample_and_hgather(csr, stack([u.repeat_interleave(K), v.repeat_interleave(K), w.reshape(-1)]), ...)
    returns -- (xz, ids with .seg_pointers, sets) -- while the step walks 2*P + P*K roots instead of 3*P*K.
    buffers=StepBuffers(csr, P*K, ..., triplets=True, star=K); small_rows= / dtype= as for sample_and_hgather.  P*K = 0: what the
    expanded call returns for [3, 0]."""
    from .sampler import as_rank
    who = "sample_and_hgather_star"
    heads, tails, P, K = _star_step_rows(who, csr, uv, w, True)
    order = as_rank(csr, order)
    if buffers is not None:
        _star_buffers_match(who, buffers, P, K, True, num_walks, num_steps, order, None, dtype, False, small_rows)
        return _buffered_step(csr, (heads, tails), buffers, seed, out)
    if P * K == 0:
        return sample_and_hgather(csr, _no_pairs(csr, 3), num_walks, num_steps, seed, out=out,
                                  order=order, small_rows=small_rows, dtype=dtype)
    return _star_step(csr, (heads, tails), P * K, seed, out, False, num_walks=num_walks, num_steps=num_steps, star=K, order=order,
                      triplets=True, small_rows=small_rows, dtype=dtype, sort_roots=sort_roots)


def _star_counts(who, csr, heads, targets, triplets, num_walks, num_steps, seed, order, table_rows, buffers, wide_keys):
    """sample_and_counts_star / sample_and_hcounts_star: _step_counts over (heads, tails); an empty star is the expanded call's"""
    heads, tails, P, K = _star_step_rows(who, csr, heads, targets, triplets)
    if P * K == 0 and buffers is None:
        return (sample_and_hcounts if triplets else sample_and_counts)(csr, _no_pairs(csr, 3 if triplets else 2), num_walks, num_steps, seed, False, order, table_rows,
                                                                      None, wide_keys)
    return _step_counts(who, csr, (heads, tails), triplets, num_walks, num_steps, seed, False, order, table_rows, buffers,
                        wide_keys=wide_keys, star=K)


def sample_and_counts_star(csr, source, targets, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None, buffers=None,
                           wide_keys=False):
    """sample_and_counts for one source against K targets: source [P], targets [P, K] -> (C float32 [2*P*K, T], sizes int32 [2*P*K],
    table, sets), bit for bit those of sample_and_counts over the expanded pairs (the step's distinct keys are the same set, so ranks
    and columns are too), with P + P*K roots walked.  buffers=StepBuffers(csr, P*K, ..., stage="counts", table_rows=T, star=K)."""
    return _star_counts("sample_and_counts_star", csr, source, targets, False, num_walks, num_steps, seed, order, table_rows, buffers,
                        wide_keys)


def sample_and_hcounts_star(csr, uv, w, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None, buffers=None,
                            wide_keys=False):
    """sample_and_hcounts for (u, v) kept and w replaced by K candidates: uv [2, P], w [P, K] -> (C float32 [4*P*K, T], sizes, table,
    sets), bit for bit those of the expanded triplets, with 2*P + P*K roots walked.
    buffers=StepBuffers(csr, P*K, ..., triplets=True, stage="counts", table_rows=T, star=K)."""
    return _star_counts("sample_and_hcounts_star", csr, uv, w, True, num_walks, num_steps, seed, order, table_rows, buffers, wide_keys)


def sample_and_mean_stage_star(csr, source, targets, embed, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None,
                               buffers=None, wide_keys=False):
    """sample_and_mean_stage over sample_and_counts_star: (C @ embed(table)) / sizes as float32 [2, P*K, H]"""
    return _step_mean(*sample_and_counts_star(csr, source, targets, num_walks, num_steps, seed, order, table_rows, buffers, wide_keys),
                      embed, 2)


def sample_and_hmean_stage_star(csr, uv, w, embed, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None, buffers=None,
                                wide_keys=False):
    """sample_and_hmean_stage over sample_and_hcounts_star: float32 [4, P*K, H] in the order (xu, xwu, xv, xwv)"""
    return _step_mean(*sample_and_hcounts_star(csr, uv, w, num_walks, num_steps, seed, order, table_rows, buffers, wide_keys), embed, 4)


# ------------------------------------------------------------------------------ the mean first stage fused into the count join
class _StepMeanJoin:
    """the library calls of sample_and_fused_mean_stage over the key rows of ONE step of `bufs`: the descriptor of _counts_tail and the
    step's stamp, as _StepAttnJoin.  forward: subgacc_sjoin_key_mean, no C.  backward: the step's rows are joined again by
    subgacc_sjoin_key_counts into a C allocated for the backward alone, dE = C.t() @ (dOut / sizes) -- the gradient of the unfused
    stage, deterministic, no new kernel.  With buffers= the rows live until the buffers take their next step: a kernel or backward
    that comes later is refused, never answered from another batch."""

    def __init__(self, bufs, own, partner, T, step_id, flags):
        self.bufs, self.own, self.partner, self.T, self.step_id, self.flags = bufs, own, partner, int(T), step_id, flags
        self.S, self.dev = bufs.S, bufs.sizes.device

    def desc(self):
        return _step_key_desc(self.bufs, JOIN_COUNTS, self.own, self.partner, self.T, self.flags)

    def _require_fresh(self, what):
        now = getattr(self.bufs, "step_id", 0)
        if now != self.step_id:
            raise RuntimeError(f"sample_and_fused_mean_stage: the {what} of step {self.step_id} of these StepBuffers ran after they took "
                               f"step {now}: the rows it joins are gone (run a step's backward before the buffers' next step)")

    def forward(self, E):
        """E float32 [T, H], contiguous, detached -> out float32 [S, H]: `mean` of the caller's buffers, or a tensor of this call"""
        b, H = self.bufs, int(E.shape[1])
        out = b.mean.detach() if b.mean is not None else torch.empty((self.S, H), dtype=torch.float32, device=self.dev)
        self._require_fresh("kernel")
        with _timed("sjoin_key_mean"):
            d = self.desc()
            check(lib().subgacc_sjoin_key_mean(ctypes.byref(d), ptr(b.ukeys), ptr(b.status[2:3]), ptr(E), H, ptr(out), ptr(b.sizes),
                                               stream_ptr()))
        return out

    def backward(self, dOut):
        b = self.bufs
        self._require_fresh("backward")
        # zeros, not empty: a pair that raises a flag is left unwritten, and a buffered step reads no flag back before the product
        C = torch.zeros((self.S, self.T), dtype=torch.float32, device=self.dev)
        with _timed("sjoin_key_counts"):
            d = self.desc()
            check(lib().subgacc_sjoin_key_counts(ctypes.byref(d), ptr(b.ukeys), ptr(b.status[2:3]), ptr(C), None, stream_ptr()))
        return C.t() @ (dOut / b.sizes.clamp(min=1).to(torch.float32)[:, None])


class _FusedMean(torch.autograd.Function):
    """out [S, H] of subgacc_sjoin_key_mean as a function of E = embed(table); backward: _StepMeanJoin.backward"""

    @staticmethod
    def forward(ctx, E, join):
        ctx.join = join
        return join.forward(E.detach().contiguous())

    @staticmethod
    def backward(ctx, dOut):
        return ctx.join.backward(dOut.contiguous()), None


def _fused_mean(who, csr, e, triplets, embed, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys, star=0):
    """the four sample_and_fused_*mean_stage* calls: the step with stage="mean" (_step_counts), E = embed(table), the fused join.
    star=K: e = (heads, tails) of _star_step_rows"""
    join, sizes, table, sets = _step_counts(who, csr, e, triplets, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                                            stage="mean", wide_keys=wide_keys, star=star)
    E, dev = embed(table), table.device
    if not (torch.is_tensor(E) and E.ndim == 2 and E.shape[0] == join.T and E.dtype == torch.float32 and E.device == dev):
        raise ValueError(f"{who}: embed(table) must be a float32 [{join.T}, H] tensor on {dev}, one row per row of table" +
                         (f", not {E.dtype} {list(E.shape)} on {E.device}" if torch.is_tensor(E) else f", not {type(E).__name__}"))
    H = int(E.shape[1])
    want = join.bufs.width
    if (want and H != want) or not 1 <= H <= MEAN_MAX_WIDTH:
        raise ValueError(f"{who}: embed(table) has rows of {H} features, " +
                         (f"buffers= were made with width={want}" if want else f"the fused join takes 1 .. {MEAN_MAX_WIDTH}"))
    if torch.is_grad_enabled() and E.requires_grad:
        out = _FusedMean.apply(E, join)
    else:
        out = join.forward(E.detach().contiguous())
    if buffers is None:
        sets.resolve()
    return out.view(4 if triplets else 2, -1, H)


def sample_and_fused_mean_stage(csr, edge, embed, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None,
                                buffers=None, wide_keys=False):
    """sample_and_mean_stage without the count matrix: the reference's first model stage for mean aggregation (model.py:78-83) on the
    on-demand step, (C @ E) / sizes with E = embed(table), where the join multiplies a pair's two count rows by E while they stand in
    LDS (subgacc_sjoin_key_mean, include/subgacc_mean.h) -- neither C float32 [2B, T] nor the GEMM behind it exists in the forward.
    The result is defined by one float32 chain per (segment, feature): acc = acc + float(c) * E[x, h] over the columns x with a count
    c != 0 in ascending order, a separate multiply and add, then one division by max(size, 1) -- the same bits whatever the schedule, the
    walk order (order=), root dedup, buffers and the star form; against sample_and_mean_stage (whose GEMM sums in another order) it
    agrees to rounding, and bit for bit where every sum is exact.  `embed` is any row-wise module with float32 [T, H] output on the
    graph's device, 1 <= H <= 1,024 (ValueError naming this call otherwise); every parameter receives a gradient: the backward joins
    the step's rows again into a C of its own (subgacc_sjoin_key_counts) and returns dE = C.t() @ (dOut / sizes) -- under
    torch.no_grad(), or when E needs no gradient, no C ever exists.  Returns float32 [2, B, H], empty segments as zero rows.
    Keywords as sample_and_mean_stage; buffers=StepBuffers(csr, B, ..., stage="mean", table_rows=T, width=H): nothing is allocated or
    read back (capturable), the result is a view of `buffers.mean`, the step is checked through `buffers.sets.resolve()`, and the
    backward must run before the buffers take their next step (RuntimeError naming the step otherwise).  Without buffers the step is
    checked before the result is returned; table_rows=None reads the number of distinct LP rows back once."""
    who = "sample_and_fused_mean_stage"
    e = _as_rows(edge, csr.device)
    if e.dim() != 2 or e.shape[0] != 2:
        raise ValueError(f"{who}: edge must be [2, B], not {list(e.shape)}")
    return _fused_mean(who, csr, e, False, embed, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys)


def sample_and_fused_hmean_stage(csr, hedge, embed, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None,
                                 table_rows=None, buffers=None, wide_keys=False):
    """sample_and_hmean_stage without the count matrix (HONet's first stage, model_horder.py:56-57): sample_and_fused_mean_stage for the
    triplets `hedge` [3, B].  Returns float32 [4, B, H] in the order (xu, xwu, xv, xwv).
    buffers=StepBuffers(csr, B, ..., triplets=True, stage="mean", table_rows=T, width=H)."""
    who = "sample_and_fused_hmean_stage"
    h = _as_triplets(hedge, csr.device, who)
    return _fused_mean(who, csr, h, True, embed, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys)


def _fused_mean_star(who, csr, heads, targets, triplets, embed, num_walks, num_steps, seed, order, table_rows, buffers, wide_keys):
    """the two *_star calls: _fused_mean over (heads, tails); an empty star is the expanded call's"""
    heads, tails, P, K = _star_step_rows(who, csr, heads, targets, triplets)
    if P * K == 0 and buffers is None:
        return _fused_mean(who, csr, _no_pairs(csr, 3 if triplets else 2), triplets, embed, num_walks, num_steps, seed, False, order,
                           table_rows, None, wide_keys)
    return _fused_mean(who, csr, (heads, tails), triplets, embed, num_walks, num_steps, seed, False, order, table_rows, buffers, wide_keys,
                       star=K)


def sample_and_fused_mean_stage_star(csr, source, targets, embed, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None,
                                     buffers=None, wide_keys=False):
    """sample_and_fused_mean_stage for one source against K targets (source [P], targets [P, K]): float32 [2, P*K, H], bit for bit the
    call over the expanded pairs, with P + P*K roots walked -- the shape the reference evaluates with, where C would be written only to
    be multiplied away.  buffers=StepBuffers(csr, P*K, ..., stage="mean", table_rows=T, width=H, star=K)."""
    return _fused_mean_star("sample_and_fused_mean_stage_star", csr, source, targets, False, embed, num_walks, num_steps, seed, order,
                            table_rows, buffers, wide_keys)


def sample_and_fused_hmean_stage_star(csr, uv, w, embed, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None,
                                      buffers=None, wide_keys=False):
    """sample_and_fused_hmean_stage for (u, v) kept and w replaced by K candidates (uv [2, P], w [P, K]): float32 [4, P*K, H] in the
    order (xu, xwu, xv, xwv), bit for bit the call over the expanded triplets.
    buffers=StepBuffers(csr, P*K, ..., triplets=True, stage="mean", table_rows=T, width=H, star=K)."""
    return _fused_mean_star("sample_and_fused_hmean_stage_star", csr, uv, w, True, embed, num_walks, num_steps, seed, order, table_rows,
                            buffers, wide_keys)


# --------------------------------------------------------------------- the attentional first stage fused into the attentional count join
class _StepFusedAttnJoin(_StepAttnJoin):
    """the library calls of sample_and_fused_attn_stage over the key rows of ONE step of `bufs` (stage="attn": no `counts`).  fused:
    subgacc_sjoin_key_attn, A = W @ E without W.  The backward uses no new kernel: the step's rows are joined again by
    subgacc_sjoin_key_counts_attn into a W allocated for the backward alone (rejoin), then _StepAttnJoin.backward.  The stale-step
    rule is _StepAttnJoin's."""
    who = "sample_and_fused_attn_stage"

    def fused(self, g, E, keep):
        """g float32 [T], E float32 [T, H], contiguous, detached -> (A float32 [S, H], m, den): `attn`, `smax`, `sden` of the caller's
        buffers, or tensors of this call"""
        b, H = self.bufs, int(E.shape[1])
        A = b.attn.detach() if b.attn is not None else torch.empty((self.S, H), dtype=torch.float32, device=self.dev)
        mx, den = (b.smax.detach(), b.sden.detach()) if keep else (None, None)
        self._require_fresh("kernel")
        with _timed("sjoin_key_attn"):
            d = self.desc()
            check(lib().subgacc_sjoin_key_attn(ctypes.byref(d), ptr(b.ukeys), ptr(b.status[2:3]), ptr(g), ptr(E), H, ptr(A), ptr(mx),
                                               ptr(den), ptr(b.sizes), stream_ptr()))
        return A, mx, den

    def rejoin(self, g):
        """W float32 [S, T] of the step, for the backward alone"""
        b = self.bufs
        self._require_fresh("backward")
        # zeros, not empty: a pair that raises a flag is left unwritten, and a buffered step reads no flag back before the products
        # (_StepAttnJoin.backward's reason)
        W = torch.zeros((self.S, self.T), dtype=torch.float32, device=self.dev)
        with _timed("sjoin_key_counts_attn"):
            d = self.desc()
            check(lib().subgacc_sjoin_key_counts_attn(ctypes.byref(d), ptr(b.ukeys), ptr(b.status[2:3]), ptr(g), ptr(W), None, None, None,
                                                      stream_ptr()))
        return W


class _FusedAttn(torch.autograd.Function):
    """A [S, H] of subgacc_sjoin_key_attn as a function of g, the gate bias (whose gradient is exactly zero: softmax drops a constant)
    and E = embed(table); backward: W rejoined, dE = W.t() @ dA, dg = the rows of subgacc_sjoin_key_counts_attn_backward for
    dW = dA @ E.t(), summed over the segments"""

    @staticmethod
    def forward(ctx, g, bg, E, join):
        ctx.join = join
        ctx.has_bg = bg is not None
        g, E = g.detach().contiguous(), E.detach().contiguous()
        A, mx, den = join.fused(g, E, True)
        ctx.save_for_backward(g, E, mx, den)
        return A

    @staticmethod
    def backward(ctx, dA):
        g, E, mx, den = ctx.saved_tensors
        dA = dA.contiguous()
        W = ctx.join.rejoin(g)
        dE = W.t() @ dA
        Dg = ctx.join.backward(g, (dA @ E.t()).contiguous(), W, mx, den)
        bg = torch.zeros((1,), dtype=dA.dtype, device=dA.device) if ctx.has_bg else None
        return Dg.sum(0), bg, dE, None


def _fused_attn_stage(name, csr, edge, embed, gate_nn, value_nn, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                      wide_keys=False, star=0):
    """sample_and_fused_attn_stage; star=K: sample_and_fused_attn_stage_star with edge = (heads, tails) of _star_step_rows.
    _attn_stage with the step of stage="attn" and subgacc_sjoin_key_attn in the place of W @ E"""
    other = "sample_and_gather(csr, edge, ...) and the modules on xz"
    gate = _one_linear(gate_nn, "gate_nn", None, 1, name, other)
    H = gate.in_features
    val = _one_linear(value_nn, "value_nn", H, None, name, other) if value_nn is not None else None
    dev = csr.device
    for mod in (gate, val, embed):
        for prm in (mod.parameters() if mod is not None else ()):
            if prm.device != dev or prm.dtype != torch.float32:
                raise ValueError(f"{name}: embed, gate_nn and value_nn must hold float32 parameters on the graph's device ({dev})")
    if star:
        e = edge
    else:
        e = _as_rows(edge, dev)
        if e.dim() != 2 or e.shape[0] != 2:
            raise ValueError(f"{name}: edge must be [2, B], not {list(e.shape)}")
        if e.shape[1] == 0 and buffers is None:      # an empty batch: no step and no W either way
            return _attn_stage(name, csr, e, embed, gate_nn, value_nn, num_walks, num_steps, seed, dedup_roots, order, table_rows, None,
                               wide_keys)
    join, sizes, table, sets = _step_counts(name, csr, e, False, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                                            stage="attn", wide_keys=wide_keys, star=star)
    count = join.bufs.status[2:3]
    E = embed(table)
    if not (torch.is_tensor(E) and E.ndim == 2 and E.shape[0] == join.T and E.shape[1] == H and E.dtype == torch.float32
            and E.device == table.device):
        raise ValueError(f"{name}: embed(table) must be a float32 [{join.T}, {H}] tensor on {table.device} (gate_nn takes rows of {H})" +
                         (f", not {E.dtype} {list(E.shape)} on {E.device}" if torch.is_tensor(E) else f", not {type(E).__name__}"))
    want = join.bufs.width
    if (want and H != want) or not 1 <= H <= MEAN_MAX_WIDTH:
        raise ValueError(f"{name}: embed(table) has rows of {H} features, " +
                         (f"buffers= were made with width={want}" if want else f"the fused join takes 1 .. {MEAN_MAX_WIDTH}"))
    live = (torch.arange(table.shape[0], device=dev) <= count).to(torch.float32)        # rows 0 .. c, from the step's count word
    centre = (E.detach() * live[:, None]).sum(0) / (count + 1).to(torch.float32)
    g = (E - centre) @ gate.weight.view(-1)
    if torch.is_grad_enabled() and (g.requires_grad or E.requires_grad or (gate.bias is not None and gate.bias.requires_grad)):
        h = _FusedAttn.apply(g, gate.bias, E, join)
    else:
        h = join.fused(g.detach().contiguous(), E.detach().contiguous(), False)[0]
    if buffers is None:
        sets.resolve()
    if val is not None:
        h = torch.nn.functional.linear(h, val.weight, val.bias)
    out = h * (sizes > 0).to(h.dtype)[:, None]
    return out.view(2, -1, out.shape[-1])


def sample_and_fused_attn_stage(csr, edge, embed, gate_nn, value_nn=None, num_walks=200, num_steps=3, seed=111413, dedup_roots=False,
                                order=None, table_rows=None, buffers=None, wide_keys=False):
    """sample_and_attn_stage without the softmax-weighted count matrix: the reference's first model stage of the LP encoder for
    --aggr attn (model.py:59-62,78-81) on the on-demand step,
        E = embed(table),  g = (E - centre) wg,  out_j = nn(W[j] @ E) [n_j > 0]
    with the same live-row centre, where the join multiplies a pair's two rows of W by E while they stand in LDS
    (subgacc_sjoin_key_attn, include/subgacc_attn.h) -- neither W float32 [2B, T] nor the GEMM behind it exists in the forward.  The
    aggregation is defined by one float32 chain per (segment, feature): acc = acc + W[j, r] * E[r, h] over the columns r whose W is not
    zero, in ascending order, a separate multiply and add -- the same bits whatever the schedule, the walk order (order=), root dedup,
    buffers and the star form; against sample_and_attn_stage (whose GEMM sums in another order) it agrees to rounding.  Modules as
    for sample_and_attn_stage, embed's width H <= 1,024 (ValueError naming this call otherwise).  Every parameter of embed, gate_nn
    and value_nn receives a gradient, the gate bias's exactly zero: the backward joins the step's rows again into a W of its own
    (subgacc_sjoin_key_counts_attn) and returns dE = W.t() @ dA and dg from subgacc_sjoin_key_counts_attn_backward over
    dW = dA @ E.t() -- under torch.no_grad(), or when nothing needs a gradient, no [2B, T] tensor ever exists.  Returns float32
    [2, B, H''] (H without value_nn), empty segments as zero rows.  Keywords as sample_and_attn_stage;
    buffers=StepBuffers(csr, B, ..., stage="attn", table_rows=T, width=H): nothing is allocated or read back by the forward under
    no_grad (capturable), the aggregation is `buffers.attn`, the step is checked through `buffers.sets.resolve()`, and the backward
    must run before the buffers take their next step (RuntimeError naming both steps otherwise).  Without buffers the step is
    checked before the result is returned."""
    return _fused_attn_stage("sample_and_fused_attn_stage", csr, edge, embed, gate_nn, value_nn, num_walks, num_steps, seed, dedup_roots,
                             order, table_rows, buffers, wide_keys)


def sample_and_fused_attn_stage_star(csr, source, targets, embed, gate_nn, value_nn=None, num_walks=200, num_steps=3, seed=111413,
                                     order=None, table_rows=None, buffers=None, wide_keys=False):
    """sample_and_fused_attn_stage for one source against K targets (source [P], targets [P, K]): float32 [2, P*K, H''], bit for bit the
    call over the expanded pairs, with P + P*K roots walked -- the shape the reference evaluates with (forward only), where W would
    be written only to be multiplied away.  buffers=StepBuffers(csr, P*K, ..., stage="attn", table_rows=T, width=H, star=K)."""
    who = "sample_and_fused_attn_stage_star"
    heads, tails, P, K = _star_step_rows(who, csr, source, targets, False)
    if P * K == 0 and buffers is None:
        return sample_and_fused_attn_stage(csr, _no_pairs(csr), embed, gate_nn, value_nn, num_walks, num_steps, seed, False, order,
                                           table_rows, None, wide_keys)
    return _fused_attn_stage(who, csr, (heads, tails), embed, gate_nn, value_nn, num_walks, num_steps, seed, False, order, table_rows,
                             buffers, wide_keys, star=K)


def _no_pairs(csr, rows=2):
    """the expanded edge tensor of an EMPTY star (P*K = 0): the *_star calls answer it as the expanded call does"""
    return torch.empty((rows, 0), dtype=torch.int64, device=csr.device)


def sample_and_attn_counts_star(csr, source, targets, gate, num_walks=200, num_steps=3, seed=111413, order=None, table_rows=None,
                                buffers=None, wide_keys=False):
    """sample_and_attn_counts for one source against K targets -> (W float32 [2*P*K, T], sizes, table, sets), bit for bit those of the
    expanded pairs; W is differentiable with respect to the gate's logits as there.
    buffers=StepBuffers(csr, P*K, ..., stage="counts_attn", table_rows=T, star=K)."""
    who = "sample_and_attn_counts_star"
    heads, tails, P, K = _star_step_rows(who, csr, source, targets, False)
    if P * K == 0 and buffers is None:
        return sample_and_attn_counts(csr, _no_pairs(csr), gate, num_walks, num_steps, seed, False, order,
                                      table_rows, None, wide_keys)
    return _step_attn(who, csr, (heads, tails), lambda table, count: gate(table), None, num_walks, num_steps, seed, False, order,
                      table_rows, buffers, wide_keys, star=K)[:4]


def sample_and_attn_stage_star(csr, source, targets, embed, gate_nn, value_nn=None, num_walks=200, num_steps=3, seed=111413, order=None,
                               table_rows=None, buffers=None, wide_keys=False):
    """sample_and_attn_stage for one source against K targets: float32 [2, P*K, H''], the documented expression over
    sample_and_attn_counts_star's (W, sizes, table), every parameter of embed, gate_nn and value_nn with its gradient."""
    who = "sample_and_attn_stage_star"
    heads, tails, P, K = _star_step_rows(who, csr, source, targets, False)
    if P * K == 0 and buffers is None:
        return sample_and_attn_stage(csr, _no_pairs(csr), embed, gate_nn, value_nn, num_walks, num_steps, seed,
                                     False, order, table_rows, None, wide_keys)
    return _attn_stage(who, csr, (heads, tails), embed, gate_nn, value_nn, num_walks, num_steps, seed, False, order, table_rows,
                       buffers, wide_keys, star=K)


def sample_and_gather_many(csr, edges, num_walks=200, num_steps=3, seed=111413, rng="philox", out=None, buffers=None, order=None,
                           **kw):
    """sample_and_gather() for MANY reference-sized batches at once (main.py:32: 1,024 pairs -- 2,048 roots cannot fill the
    chip): `edges` [nb, 2, B]; all nb*2B endpoints are sampled by ONE walk launch and joined by ONE join launch, and the result
    is cut into nb reference-shaped pieces -- [(xz_b, indptr_b)] * nb, bit for bit what sample_and_gather(csr, edges[b], ...)
    returns for every b with rng="philox" (a root's set is a function of (seed, root id)), plus the sets of the whole call.
    buffers=StepBuffers(csr, nb*B, ..., batch=B): the allocation-free six-launch form; the sets are resolved here (one read).
    order=: as for sample_and_gather -- the walk order of all nb*2B endpoints, nothing else."""
    from .sampler import as_rank
    order = as_rank(csr, order)
    e = _as_rows(edges, csr.device)
    if e.dim() != 3 or e.shape[1] != 2:
        raise ValueError("sample_and_gather_many: edges must be [nb, 2, B]")
    nb, _, B = e.shape
    if rng != "philox":
        raise ValueError("sample_and_gather_many needs rng='philox' (a rand_r set depends on its root's place in the stream, i.e. on "
                         "which other batches are sampled with it)")
    if buffers is not None:
        if buffers.batch != B or buffers.B != nb * B or buffers.dedup:
            raise ValueError(f"buffers= must be StepBuffers(csr, {nb * B}, ..., batch={B})")
        xz, seg, sets = sample_and_gather(csr, e, num_walks=num_walks, num_steps=num_steps, seed=seed, rng=rng, out=out, buffers=buffers,
                                          order=order, **kw)
        sets.resolve()
        views = split_batches(xz, seg, B)
        views._resolve()      # (the pointers live in the step buffers: read now, before the buffers take another step)
        return views, sets
    from .spg import sample_spg
    kw.setdefault("number_rows", False)
    z, sets = sample_spg(csr, e.reshape(-1).to(torch.int32), num_walks=num_walks, num_steps=num_steps, seed=seed, rng=rng,
                         strided=True, order=order, **kw)
    table = z.slot_table() if sets.strided else sets.feature_table()
    own = torch.arange(nb * 2 * B, device=e.device, dtype=torch.int64)
    xz, seg = _checked(*sjoin(_as_spg(z), own, None, table, ptr_mode=True, pair_block=B, out=out))
    return split_batches(xz, seg, B), sets


# the buffered step walks its rows in ascending order of root id (csrc/worklist.hip: one radix pass, two small launches): cit2-like
# step +5.7 % pairs/s, twitter-like +5.6 %, collab +1.8 %, ppa +2.1 %; StepBuffers(sort_roots=False): batch order.  Nothing observable changes.
SORT_ROOTS_MIN = 16384      # rows from which the two extra launches pay (a 1,024-pair step is 2,048 roots: one workgroup per resident slot)
_ARANGE_SEGMENTS = {}
_CACHE_LOCK = threading.Lock()     # the reference's pgather calls the join from 4 Python threads (train.py:88-99)


def _arange_segments(B, device, block=None):
    """gather()'s segment lists for edge = [[0..B), [B..2B)] -- the rows of a batch sampled endpoint by endpoint -- kept per
    (B, device): a serving loop does not rebuild them (three small kernels) for every batch.  Shared between threads and
    streams: built under a lock and COMPLETE (the building stream is synchronised, once) before anybody else can see them.
    block = b < B: the B pairs are B/b batches laid out [u_0 | v_0 | u_1 | v_1 | ...], every row mirrored inside its batch."""
    block = int(B) if block is None else int(block)
    key = (int(B), str(device), block)
    hit = _ARANGE_SEGMENTS.get(key)
    if hit is None:
        with _CACHE_LOCK:
            hit = _ARANGE_SEGMENTS.get(key)
            if hit is None:
                own = torch.arange(2 * B, device=device, dtype=torch.int64)
                hit = (own, own.view(-1, 2, block).flip(1).contiguous().view(-1))
                if not torch.cuda.is_current_stream_capturing():
                    torch.cuda.current_stream(own.device).synchronize()
                _ARANGE_SEGMENTS[key] = hit
    return hit


def _triplet_segments(B, device):
    """hgather()'s own list [u | w | v | w] for hedge = [[0..B), [B..2B), [2B..3B)] -- the rows of a triplet batch sampled root by
    root -- kept per (B, device) like _arange_segments (the mirrored partner list [w | u | w | v] is derived by the kernels)"""
    key = (int(B), str(device), "triplets")
    hit = _ARANGE_SEGMENTS.get(key)
    if hit is None:
        with _CACHE_LOCK:
            hit = _ARANGE_SEGMENTS.get(key)
            if hit is None:
                r = torch.arange(3 * B, device=device, dtype=torch.int64).view(3, B)
                hit = torch.cat([r[0], r[2], r[1], r[2]])
                if not torch.cuda.is_current_stream_capturing():
                    torch.cuda.current_stream(hit.device).synchronize()
                _ARANGE_SEGMENTS[key] = hit
    return hit


def _star_segments(P, K, triplets=False, device=None):
    """The segment lists (own, partner) of a step of P sources against K targets each (StepBuffers(star=K)): the lists of the expanded
    batch [source.repeat_interleave(K) | targets.view(-1)] with every endpoint mapped to the row of its first occurrence -- source j
    is row j, target i row P + i: own = [j // K | P + i] over 2*P*K segments, partner its mirror.  triplets: the rows are u, v, w --
    P, P and P*K of them -- and the list is hgather's [U|w ; W|u ; V|w ; W|v] over 4*P*K segments, own = [j // K | 2P + i | P + j // K |
    2P + i], partner None (mirrored: the kernels derive it).  Constants of (P, K)."""
    i = torch.arange(int(P) * int(K), dtype=torch.int64, device=device)
    src = torch.div(i, int(K), rounding_mode="floor")
    if triplets:
        w = 2 * int(P) + i
        return torch.cat([src, w, int(P) + src, w]), None
    tgt = int(P) + i
    return torch.cat([src, tgt]), torch.cat([tgt, src])


def _packed_rows(spg, form):
    """The row fields of the store the count / pair / index forms join: these forms have no headed one (ValueError, before any
    device work)."""
    size_pass, rows = spg.join_rows()
    if size_pass is None:
        raise ValueError(f"{form} joins the packed store: keep it, or join z.to_spg() (the headed layout is for gather / hgather)")
    return rows


def gather_counts(edge, x, table_rows, device=None):
    """Count form of gather() for mean aggregation (reference consumer model.py:78-83).

    Returns (C float32 [2B, table_rows], sizes int64 [2B]) with C[j, p] = occurrences of LP row p (0 = partner
    absent) in either feature slot of segment j -- left blocks then right blocks, as gather().  For any row-wise
    embedding f:  segment_sum_j(f(xz).sum(-2)) == C[j] @ f(Z_SF), so `x = f(xz).sum(-2); aggr(x, ptr)` of the
    reference's Net.forward becomes `(C @ f(Z_SF)) / sizes[:, None]` and the [R,2,k] tensor never exists."""
    spg = _as_spg(x)
    rows = _count_rows(spg, table_rows, "gather_counts")
    e = _as_rows(edge, spg.device)
    return _counts(spg, rows, e, (e[0], e[1]), (e[1], e[0]), table_rows)


def _count_rows(spg, table_rows, form):
    """the row fields of the store the count form joins, or the refusals of gather_counts / hgather_counts (before any device work)"""
    rows = _packed_rows(spg, form)
    if "row_off" not in rows or rows["payload"].dtype != torch.int32 or spg.keyrows:
        raise TypeError(f"{form} needs a packed SFptr (integer) SpG (not a keyed() one)")
    if table_rows <= spg.max_data:
        raise IndexError(f"index {spg.max_data} is out of bounds for a table with {table_rows} rows")
    return rows


def _counts(spg, rows, e, own_blocks, partner_blocks, table_rows):
    """ONE launch of the count kernel over the mirrored blocks `own_blocks` (each [B]; block 2t+1 mirrors block 2t) of the rows `e`"""
    B = e.shape[1]
    if B and bool(((e < 0) | (e >= spg.n_rows)).any()):          # this form has no size pass to carry the check
        raise IndexError(f"row index out of range for an SpG with {spg.n_rows} rows")
    own = torch.cat(own_blocks).contiguous()
    partner = torch.cat(partner_blocks).contiguous()
    dev = spg.device
    out = torch.empty((own.numel(), int(table_rows)), dtype=torch.float32, device=dev)
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    with _timed("sjoin_counts"):
        join_fill(JOIN_COUNTS, JOIN_SFPTR, **rows, own=own, partner=partner, S=own.numel(), pair_block=B, table_rows=int(table_rows),
                  out_counts=out, flags=flags)
    sizes = rows["row_off"][own + 1] - rows["row_off"][own]
    _checked(out, sizes, flags)
    return out, sizes


def hgather_counts(hedge, x, table_rows, device=None):
    """Count form of hgather() (train.py:48-72) for HONet's mean aggregation (model_horder.py:56-57).

    Returns (C float32 [4B, table_rows], sizes int64 [4B]) with C[j, p] = occurrences of LP row p (0 = partner absent) in either
    feature slot of segment j -- hgather's blocks [U|w ; W|u ; V|w ; W|v] --, so that for any row-wise embedding f
    segment_sum_j(f(xz).sum(-2)) == C[j] @ f(Z_SF) and the [R,2,k] tensor of 4B segments never exists.  The count kernel takes any
    number of mirrored blocks (segment j = (p / pb) * 2 * pb + p % pb of pair p): own = [u | w | v | w], S = 4B, pair_block = B is
    ONE launch of the kernel gather_counts() runs; there is no second count kernel."""
    spg = _as_spg(x)
    rows = _count_rows(spg, table_rows, "hgather_counts")
    h = _as_triplets(hedge, spg.device, "hgather_counts")
    u, v, w = h[0], h[1], h[2]
    return _counts(spg, rows, h, (u, w, v, w), (w, u, w, v), table_rows)


def hmean_stage(hedge, x, encode, embed):
    """HONet's first model stage, fused:  model_horder.py:56-57
        x = pe_embedding(xz).sum(dim=-2);  xu, xwu, xv, xwv = scatter_mean(x, ind, dim=0).view(4, -1, H)
    as  (C @ embed(encode)) / sizes  with C = hgather_counts(hedge, x): mean_stage's algebra over hgather's four blocks instead of
    gather's two.  `x` is a packed SFptr SpG as for mean_stage, `embed` any row-wise module; autograd reaches its parameters
    through the small [T, H] activation -- C is a constant of the batch -- while xz [R,2,k] and the [R,2,H] activations never exist.
    Returns float32 [4, B, H] in the order (xu, xwu, xv, xwv); empty segments give zero rows."""
    table = encode if torch.is_tensor(encode) else torch.as_tensor(encode)
    spg = _as_spg(x)
    table = table.to(device=spg.device, dtype=torch.float32)
    C, sizes = hgather_counts(hedge, spg, table.shape[0])
    out = (C @ embed(table)) / sizes.clamp(min=1).to(torch.float32)[:, None]
    return out.view(4, -1, out.shape[-1])


def mean_stage(edge, x, encode, embed):
    """The reference's first model stage for mean aggregation, fused:  model.py:78-83
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = aggr.MeanAggregation()(x, ptr=ptr).view(2, -1, H)
    as  (C @ embed(encode)) / sizes  with C = gather_counts(edge, x).  `embed` is any row-wise module (the reference's
    pe_embedding MLP); autograd reaches its parameters through the small [c+1, H] activation -- C is a constant of
    the batch -- so the stage trains like the original while xz [R,2,k] and the [R,2,H] activations never exist.
    Returns float32 [2, B, H] (left endpoints, right endpoints); empty segments give zero rows."""
    table = encode if torch.is_tensor(encode) else torch.as_tensor(encode)
    spg = _as_spg(x)
    table = table.to(device=spg.device, dtype=torch.float32)
    C, sizes = gather_counts(edge, spg, table.shape[0])
    out = (C @ embed(table)) / sizes.clamp(min=1).to(torch.float32)[:, None]
    return out.view(2, -1, out.shape[-1])


def gather_pairs(edge, x, device=None):
    """Pair form of gather() (include/subgacc.h: subgacc_sjoin_pairs): every segment as its DISTINCT index pairs with
    multiplicities -- (pairs int32 [R', 2], mult int32 [R'], indptr int64 [2B+1]), segments in gather()'s order (left
    blocks, then right blocks).  pairs[r] = (SFptr+1 of a member in its own row, in the partner row or 0): the row
    gather() would have emitted is encode[pairs[r]] and it occurs mult[r] times in its segment, so for a first model
    stage of the form f(xz).sum(-2) = f(encode)[pa] + f(encode)[pb] (model.py:78) any aggregation that is a weighted
    function of the rows -- mean, the attention gate of model.py:59-62 -- is exact over these rows with `mult` as
    weights, at ~1/10 of the rows (a set of ~400 members carries a few dozen distinct LP rows)."""
    spg = _as_spg(x)
    if isinstance(spg, StridedSpG):
        spg = spg.to_csr()
    rows = _packed_rows(spg, "gather_pairs")
    if rows["payload"].dtype != torch.int32 or spg.keyrows:
        raise TypeError("gather_pairs needs an SFptr (integer) SpG (not a keyed() one)")
    L, dev, st = lib(), spg.device, stream_ptr()
    e = _as_rows(edge, dev)
    B = e.shape[1]
    own = torch.cat([e[0], e[1]]).contiguous()
    partner = torch.cat([e[1], e[0]]).contiguous()
    S = 2 * B
    seg, flags = _seg_and_flags(S, dev)
    ws = torch.empty(L.subgacc_sjoin_workspace_bytes(S), dtype=torch.uint8, device=dev)
    check(L.subgacc_sjoin_sizes(ptr(rows["row_off"]), spg.n_rows, ptr(own), ptr(partner), S, ptr(seg), ptr(flags), ptr(ws),
                                ws.numel(), st))
    R = _size_and_row_check(seg, S, flags, spg.n_rows)
    pairs = torch.empty((R, 2), dtype=torch.int32, device=dev)
    mult = torch.empty(R, dtype=torch.int32, device=dev)
    cnt = torch.zeros(S, dtype=torch.int32, device=dev)
    with _timed("sjoin_pairs"):
        join_fill(JOIN_PAIRS, JOIN_SFPTR, st, **rows, own=own, partner=partner, S=S, seg=seg, pair_block=B, out_pairs=pairs, out_mult=mult,
                  out_cnt=cnt, flags=flags)
    # rows of segment j sit at [seg[j], seg[j] + cnt[j]): close the gaps (R' ~ R/10 elements from here on)
    indptr = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=indptr[1:])
    Rc = int(indptr[-1].item())
    segid = torch.repeat_interleave(torch.arange(S, device=dev), cnt.long(), output_size=Rc)
    src = seg[:-1][segid] + (torch.arange(Rc, device=dev) - indptr[:-1][segid])
    _checked(pairs, indptr, flags)
    return pairs[src], mult[src], indptr


def attn_stage(edge, x, encode, embed, gate_nn, value_nn=None):
    """The reference's first model stage for --aggr attn, fused over the pair form of the join:  model.py:59-62,78-81
        x = pe_embedding(xz).sum(dim=-2)
        xl, xr = AttentionalAggregation(gate_nn, nn)(x, ptr=ptr).view(2, -1, H)
              = segment_sum(softmax_segment(gate_nn(x)) * nn(x))
    A row's x is e[pa] + e[pb] with e = embed(encode) ([c+1, H], tiny): gate and value are evaluated once per DISTINCT
    pair of a segment and the softmax / weighted sum carry the multiplicities -- exact (up to fp32 summation order),
    ~10x fewer rows than xz, and autograd reaches embed / gate_nn / value_nn through ordinary torch ops.
    Returns float32 [2, B, H'] (left endpoints, right endpoints); empty segments give zero rows (as PyG's do)."""
    table = encode if torch.is_tensor(encode) else torch.as_tensor(encode)
    spg = _as_spg(x)
    table = table.to(device=spg.device, dtype=torch.float32)
    pairs, mult, indptr = gather_pairs(edge, spg)
    if pairs.numel() and int(pairs.max().item()) >= table.shape[0]:
        raise IndexError(f"index {int(pairs.max().item())} is out of bounds for the encode table with {table.shape[0]} rows")
    S = indptr.numel() - 1
    e = embed(table)
    xr = e[pairs[:, 0].long()] + e[pairs[:, 1].long()]
    g = gate_nn(xr).reshape(-1)
    v = value_nn(xr) if value_nn is not None else xr
    seg = torch.repeat_interleave(torch.arange(S, device=spg.device), indptr[1:] - indptr[:-1], output_size=pairs.shape[0])
    gmax = torch.full((S,), float("-inf"), device=g.device, dtype=g.dtype).scatter_reduce(0, seg, g.detach(), "amax")
    w = mult.to(g.dtype) * torch.exp(g - gmax[seg])                 # softmax numerators, with multiplicity
    den = torch.zeros(S, device=g.device, dtype=g.dtype).index_add_(0, seg, w)
    num = torch.zeros((S, v.shape[-1]), device=g.device, dtype=v.dtype).index_add_(0, seg, w[:, None] * v)
    out = num / (den + 1e-16)[:, None]                              # torch_geometric.utils.softmax adds the same 1e-16
    return out.view(2, -1, out.shape[-1])


def gather_index(edge, x, device=None):
    """Index form of gather() (the variant that writes 8 instead of 8k bytes per row): (pairs int32 [R, 2],
    indptr int64 [2B+1]) with pairs[r] = (SFptr+1 of the member in its own row, in the partner row or 0) -- the row gather()
    would have emitted is encode[pairs[r]], in gather()'s row order (members sorted by node id inside a segment)."""
    spg = _as_spg(x)
    _packed_rows(spg, "gather_index")
    if isinstance(spg, StridedSpG):     # index pairs need the numbering of the distinct LP rows (transient batches skip it)
        if spg.keyrows:
            spg = spg.to_csr()
        else:
            spg.sets.number()
    e = _as_rows(edge, spg.device)
    own = torch.cat([e[0], e[1]])
    partner = torch.cat([e[1], e[0]])
    return _checked(*sjoin(spg, own, partner, None, ptr_mode=True, return_index=True, pair_block=e.shape[1]))


def lstm_stage(edge, x, encode, embed, lstm):
    """The reference's first model stage for --aggr lstm, over the index form of the join:  model.py:63-65,78-83
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = LSTMAggregation(H, H)(x, index=ptr).view(2, -1, H)
    LSTMAggregation packs the rows of every segment, in row order, into a dense [S, L, H] batch padded with zero rows
    (L = the longest segment), runs `lstm` (batch_first) over it and returns the output at the LAST position L-1 -- the
    padding is part of its arithmetic, so it is reproduced.  A row's x is e[pa] + e[pb] with e = embed(encode) ([c+1, H]):
    the stage reads 8 bytes per row instead of xz's 8k and never evaluates the MLP on [R, 2, k].
    Returns float32 [2, B, H'] (left endpoints, right endpoints)."""
    table = encode if torch.is_tensor(encode) else torch.as_tensor(encode)
    spg = _as_spg(x)
    table = table.to(device=spg.device, dtype=torch.float32)
    pairs, indptr = gather_index(edge, spg)
    if pairs.numel() and int(pairs.max().item()) >= table.shape[0]:
        raise IndexError(f"index {int(pairs.max().item())} is out of bounds for the encode table with {table.shape[0]} rows")
    S = indptr.numel() - 1
    lens = indptr[1:] - indptr[:-1]
    L = int(lens.max().item()) if S else 0
    e = embed(table)
    rows = e[pairs[:, 0].long()] + e[pairs[:, 1].long()]
    seg = torch.repeat_interleave(torch.arange(S, device=spg.device), lens, output_size=pairs.shape[0])
    posn = torch.arange(pairs.shape[0], device=spg.device) - indptr[:-1][seg]
    dense = rows.new_zeros((S, max(L, 1), rows.shape[-1]))
    dense[seg, posn] = rows
    out = lstm(dense)[0][:, -1]
    return out.view(2, -1, out.shape[-1])


def _relu_mlp(embed, name="float_mean_stage"):
    """(Linear(1, H), Linear(H, H')) of embed = Sequential(Linear(1, H), ReLU(), Linear(H, H')) -- the reference's pe_embedding for the
    float encoders (model.py:54-55, input_dim = 1) -- or TypeError"""
    nn = torch.nn
    if not (isinstance(embed, nn.Sequential) and len(embed) == 3 and isinstance(embed[0], nn.Linear) and isinstance(embed[1], nn.ReLU)
            and isinstance(embed[2], nn.Linear) and embed[0].in_features == 1 and embed[2].in_features == embed[0].out_features):
        raise TypeError(f"{name} fuses embed = Sequential(Linear(1, H), ReLU(), Linear(H, H')) only; for any other module "
                        "use xz, ind = gather(edge, x) and the module on xz")
    return embed[0], embed[2]


def _edge_rows(edge, name="float_mean_stage"):
    """a fused float stage's `edge` checked on the host: a [2, B] integer array (torch or NumPy), before any device work"""
    if not torch.is_tensor(edge):
        try:
            edge = np.asarray(edge)
        except ValueError as e:             # (NumPy >= 1.24 refuses a ragged nested list itself)
            raise ValueError(f"{name}: edge must be a [2, B] integer array ({e})") from None
        ok = edge.dtype != object and np.issubdtype(edge.dtype, np.integer)
    else:
        ok = not edge.dtype.is_floating_point and not edge.dtype.is_complex and edge.dtype != torch.bool
    if not ok or edge.ndim != 2 or edge.shape[0] != 2:
        raise ValueError(f"{name}: edge must be a [2, B] integer array, got {getattr(edge, 'dtype', type(edge))} "
                         f"of shape {tuple(getattr(edge, 'shape', ()))}")
    return edge


class _FloatStage:
    """What the fused float stages (float_mean_stage, float_attn_stage) share: the checks of the store, embed and edge -- every one before
    any device work --, the mirrored F64 descriptor of the join and the status words it leaves.  `unfused` names the module call a caller
    with an integer (LP) store has instead."""

    def __init__(self, name, unfused, edge, x, embed):
        self.name = name
        self.lin1, self.lin2 = _relu_mlp(embed, name)
        H = self.H = self.lin1.out_features
        if not 1 <= H <= 1024:
            raise ValueError(f"{name}: Linear(1, H) with H = {H}; the fused stage takes 1 <= H <= 1024")
        if isinstance(x, StridedSpG):
            raise TypeError(f"{name} joins a resident float store (SpG or HeadedSpG), not a StridedSpG")
        if not isinstance(x, (SpG, HeadedSpG)):
            raise TypeError(f"{name} joins a float64 SpG or HeadedSpG, not {type(x).__name__}")
        if x.keyrows or x.data.dtype != torch.float64:
            raise TypeError(f"{name} joins a float (PPR / SPD / DEG) store; an integer (LP) store has {unfused}")
        self.edge = _edge_rows(edge, name)
        self.x, self.dev = x, x.device
        dev = self.dev
        if self.lin1.weight.device != dev or self.lin2.weight.device != dev or self.lin1.weight.dtype != torch.float32:
            raise ValueError(f"{name}: embed must hold float32 parameters on the store's device ({dev})")

    def join_on(self):
        """the device side: the endpoints, the store's rows, the status words, w1 and b1"""
        dev = self.dev
        e = _as_rows(self.edge, dev)
        self.B = int(e.shape[1])
        self.own = e.contiguous().view(-1)
        _, self.rows = self.x.join_rows()
        self.flags = torch.zeros(4, dtype=torch.int32, device=dev)
        self.w1 = self.lin1.weight.view(-1)
        self.b1 = self.lin1.bias if self.lin1.bias is not None else torch.zeros(self.H, dtype=torch.float32, device=dev)

    def desc(self):
        return _lib.join_desc(JOIN_ROWS, JOIN_F64, **self.rows, own=self.own, S=2 * self.B, pair_block=self.B, flags=self.flags)

    def checked(self):
        status = int(self.flags[3].item())
        if status & 16:
            raise IndexError(f"row index out of range for an SpG with {self.x.n_rows} rows")
        if status & 1:
            raise _lib.SubgAccError("SpG row longer than SpG.max_len")

    def nonempty(self):
        """[2B] 1.0 where the endpoint's own row has members (an empty segment gives a zero row)"""
        rows, own = self.rows, self.own
        sizes = rows["row_off"][own + 1] - rows["row_off"][own] if "row_off" in rows else rows["ids"][own * rows["row_stride"]]
        return sizes > 0

    def tail(self, M):
        """W2 M + 2 b2 ([2B, H'])"""
        h = torch.nn.functional.linear(M, self.lin2.weight)
        if self.lin2.bias is not None:
            h = h + 2 * self.lin2.bias
        return h


class _ReluMean(torch.autograd.Function):
    """M [S, H] of subgacc_sjoin_relu_mean as a function of (w1, b1); backward: dL/dw1 = sum_j G_j * P_j, dL/db1 = sum_j G_j * Q_j with
    the P / Q sums the forward asked the kernel for"""

    @staticmethod
    def forward(ctx, w1, b1, join):
        M, P, Q = join(w1.detach().contiguous(), b1.detach().contiguous())
        ctx.save_for_backward(P, Q)
        return M

    @staticmethod
    def backward(ctx, G):
        P, Q = ctx.saved_tensors
        return (G * P).sum(0), (G * Q).sum(0), None


def float_mean_stage(edge, x, embed):
    """The reference's first model stage for the float encoders (PPR, SPD, DEG: utils.py:20-38, main.py:170-196), fused:  model.py:78-83
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = aggr.MeanAggregation()(x, ptr=ptr).view(2, -1, H)
    with pe_embedding = embed = Sequential(Linear(1, H), ReLU(), Linear(H, H')) over the float join's xz [R,2,1].  Mean aggregation is
    linear, so the stage is  W2 M_j + 2 b2  per segment, M_j = mean over the segment's rows of relu(w1 a + b1) + relu(w1 b + b1): the
    library's fused kernel (subgacc_sjoin_relu_mean) joins the pairs and writes M [2B, H] -- neither xz nor the [R,2,H] activations
    exist.  Autograd reaches all four parameters: w1 / b1 through the per-segment sums the kernel writes for the backward (only when
    grad is enabled and one of them requires it), W2 / b2 through ordinary torch ops.
    edge: [2, B] integer (torch or NumPy); x: a float64 SpG or HeadedSpG (topk_ppr_matrix / ppr.encoding).
    Returns float32 [2, B, H'] (left endpoints, right endpoints) as mean_stage does; empty segments give zero rows.  The result
    carries the join's status words as .join_flags (flags[1] & 2: a pair with a row too long to stage streamed).
    For --aggr attn, float_attn_stage(edge, x, embed, gate_nn, value_nn)."""
    st = _FloatStage("float_mean_stage", "mean_stage(edge, x, encode, embed)", edge, x, embed)
    st.join_on()
    B, H, dev = st.B, st.H, st.dev
    grads = torch.is_grad_enabled() and (st.w1.requires_grad or st.b1.requires_grad)

    def join(w, b):
        M = torch.empty((2 * B, H), dtype=torch.float32, device=dev)
        P, Q = (torch.empty_like(M), torch.empty_like(M)) if grads else (None, None)
        if B == 0:          # (an empty list has no pair_block the library would accept)
            return M, P, Q
        with _timed("sjoin_relu_mean"):
            d = st.desc()
            check(lib().subgacc_sjoin_relu_mean(ctypes.byref(d), ptr(w), ptr(b), H, ptr(M), ptr(P), ptr(Q), stream_ptr()))
        st.checked()
        return M, P, Q

    M = _ReluMean.apply(st.w1, st.b1, join) if grads else join(st.w1.detach(), st.b1.detach())[0]
    h = st.tail(M)
    out = (h * st.nonempty().to(h.dtype)[:, None]).view(2, B, h.shape[-1])
    out.join_flags = st.flags
    return out


def _one_linear(mod, what, d_in, d_out=None, stage="float_attn_stage", other="xz, ind = gather(edge, x) and the modules on xz"):
    """the nn.Linear of `mod` = Linear(d_in, d_out) or Sequential(Linear(d_in, d_out)) (d_out None: any; d_in None: any), or TypeError
    naming `stage` and, for any other module, `other`"""
    nn = torch.nn
    lin = mod[0] if isinstance(mod, nn.Sequential) and len(mod) == 1 else mod
    if not (isinstance(lin, nn.Linear) and (d_in is None or lin.in_features == d_in) and (d_out is None or lin.out_features == d_out)):
        shape = f"({d_in if d_in is not None else 'H'}, {d_out if d_out is not None else 'H2'})"
        raise TypeError(f"{stage} fuses {what} = Linear{shape} (or a Sequential of that one Linear; PyG's MLP([...]) as its "
                        f".lins[0]) only; for any other module use {other}")
    return lin


class _ReluAttn(torch.autograd.Function):
    """A [S, H] of subgacc_sjoin_relu_attn as a function of (w1, b1, u) -- and of the gate bias, whose gradient is exactly zero (softmax
    drops a constant); backward: subgacc_sjoin_relu_attn_backward's per-segment sums, summed over the segments"""

    @staticmethod
    def forward(ctx, w1, b1, u, bg, join):
        ctx.join = join
        ctx.has_bg = bg is not None
        A, mx, den = join.forward(w1.detach().contiguous(), b1.detach().contiguous(), u.detach().contiguous(), True)
        ctx.save_for_backward(w1.detach(), b1.detach(), u.detach(), A, mx, den)
        return A

    @staticmethod
    def backward(ctx, G):
        w1, b1, u, A, mx, den = ctx.saved_tensors
        Dw, Db, Du = ctx.join.backward(w1.contiguous(), b1.contiguous(), u.contiguous(), G.contiguous(), A, mx, den)
        bg = torch.zeros((1,), dtype=G.dtype, device=G.device) if ctx.has_bg else None
        return Dw.sum(0), Db.sum(0), Du.sum(0), bg, None


class _AttnJoin:
    """the two library calls of float_attn_stage over one _FloatStage"""

    def __init__(self, st):
        self.st = st

    def forward(self, w, b, u, keep):
        st = self.st
        S, H = 2 * st.B, st.H
        A = torch.empty((S, H), dtype=torch.float32, device=st.dev)
        mx, den = (torch.empty(S, dtype=torch.float32, device=st.dev), torch.empty(S, dtype=torch.float32, device=st.dev)) if keep \
            else (None, None)
        if st.B == 0:       # (an empty list has no pair_block the library would accept)
            return A, mx, den
        with _timed("sjoin_relu_attn"):
            d = st.desc()
            check(lib().subgacc_sjoin_relu_attn(ctypes.byref(d), ptr(w), ptr(b), ptr(u), H, ptr(A), ptr(mx), ptr(den), stream_ptr()))
        st.checked()
        return A, mx, den

    def backward(self, w, b, u, G, A, mx, den):
        st = self.st
        Dw, Db, Du = (torch.zeros_like(A) for _ in range(3))
        if st.B == 0:
            return Dw, Db, Du
        with _timed("sjoin_relu_attn_backward"):
            d = st.desc()
            check(lib().subgacc_sjoin_relu_attn_backward(ctypes.byref(d), ptr(w), ptr(b), ptr(u), st.H, ptr(G), ptr(A), ptr(mx),
                                                         ptr(den), ptr(Dw), ptr(Db), ptr(Du), stream_ptr()))
        return Dw, Db, Du


def float_attn_stage(edge, x, embed, gate_nn, value_nn=None):
    """The reference's first model stage for the float encoders with --aggr attn, fused:  model.py:59-62,78-81
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = AttentionalAggregation(gate_nn, nn)(x, ptr=ptr).view(2, -1, H'')
    with pe_embedding = embed = Sequential(Linear(1, H), ReLU(), Linear(H, H')) over the float join's xz [R,2,1] and one-Linear
    gate_nn (H' -> 1) and nn (value_nn: H' -> H'', or None).  Row t of segment j is x_t = W2 r_t + 2 b2 with r_t = relu(w1 a_t + b1) +
    relu(w1 b_t + b1), so the gate is u . r_t plus a constant the softmax drops (u = W2^T wg), and, the weights summing to 1,
        out_j = nn(W2 A_j + 2 b2) [n_j > 0],   A_j = sum_t softmax_j(u . r)_t r_t
    The library's kernels (subgacc_sjoin_relu_attn / _backward) join the pairs and write A [2B, H] -- neither xz nor the [R,2,H]
    activations exist -- and, when autograd asks, the per-segment sums for w1, b1 and u; the rest are ordinary torch ops.  Every
    parameter of embed, gate_nn and value_nn receives a gradient; the gate bias's is exactly zero, as the reference's is analytically.
    gate_nn: nn.Linear(H', 1) or nn.Sequential of that one Linear; value_nn: None, nn.Linear(H', H'') or a one-Linear Sequential.
    The reference builds them as torch_geometric MLP([H', 1]) / MLP([H', H']): with a two-entry channel list, PyG 2.2's MLP is one plain
    Linear (no norm, no activation after the last layer), held in .lins[0] -- pass that Linear.  (This rests on PyG 2.2's MLP as
    released; PyG is not a dependency here.)
    edge: [2, B] integer (torch or NumPy); x: a float64 SpG or HeadedSpG.  Returns float32 [2, B, H''] (H' without value_nn), empty
    segments giving zero rows, with the join's status words as .join_flags (flags[1] & 2: a pair with a row too long to stage streamed)."""
    st = _FloatStage("float_attn_stage", "attn_stage(edge, x, encode, embed, gate_nn, value_nn)", edge, x, embed)
    H2 = st.lin2.out_features
    gate = _one_linear(gate_nn, "gate_nn", H2, 1)
    val = _one_linear(value_nn, "value_nn", H2) if value_nn is not None else None
    for lin in (gate, val):
        if lin is not None and (lin.weight.device != st.dev or lin.weight.dtype != torch.float32):
            raise ValueError(f"float_attn_stage: gate_nn / value_nn must hold float32 parameters on the store's device ({st.dev})")
    st.join_on()
    B = st.B
    u = (gate.weight @ st.lin2.weight).view(-1)         # W2^T wg
    join = _AttnJoin(st)
    params = [st.w1, st.b1, u] + ([gate.bias] if gate.bias is not None else [])
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        A = _ReluAttn.apply(st.w1, st.b1, u, gate.bias, join)
    else:
        A = join.forward(st.w1.detach(), st.b1.detach(), u.detach(), False)[0]
    h = st.tail(A)
    if val is not None:
        h = torch.nn.functional.linear(h, val.weight, val.bias)
    out = (h * st.nonempty().to(h.dtype)[:, None]).view(2, B, h.shape[-1])
    out.join_flags = st.flags
    return out


class _CountsAttn(torch.autograd.Function):
    """W [S, T] of subgacc_sjoin_counts_attn as a function of g = embed(encode) wg -- and of the gate bias, whose gradient is exactly
    zero (softmax drops a constant); backward: subgacc_sjoin_counts_attn_backward's per-segment rows Dg, summed over the segments"""

    @staticmethod
    def forward(ctx, g, bg, join):
        ctx.join = join
        ctx.has_bg = bg is not None
        g = g.detach().contiguous()
        W, mx, den = join.forward(g, True)
        ctx.save_for_backward(g, W, mx, den)
        return W

    @staticmethod
    def backward(ctx, dW):
        g, W, mx, den = ctx.saved_tensors
        Dg = ctx.join.backward(g, dW.contiguous(), W, mx, den)
        bg = torch.zeros((1,), dtype=dW.dtype, device=dW.device) if ctx.has_bg else None
        return Dg.sum(0), bg, None


class _CountsAttnJoin:
    """the two library calls of counts_attn_stage: the mirrored count-form descriptor over a packed SFptr store, its status words"""

    def __init__(self, x, rows, own, B, T):
        self.x, self.rows, self.own, self.B, self.T = x, rows, own, B, T
        self.dev = x.device
        self.flags = torch.zeros(4, dtype=torch.int32, device=self.dev)

    def desc(self):
        return _lib.join_desc(JOIN_COUNTS, JOIN_SFPTR, **self.rows, own=self.own, S=2 * self.B, pair_block=self.B, table_rows=self.T,
                              flags=self.flags)

    def checked(self):
        status = int(self.flags[3].item())
        if status & 16:
            raise IndexError(f"row index out of range for an SpG with {self.x.n_rows} rows")
        if status & 2:
            raise IndexError(f"index {self.x.max_data} is out of bounds for the encode table with {self.T} rows")
        if status & 1:
            raise _lib.SubgAccError("SpG row longer than SpG.max_len")

    def forward(self, g, keep):
        S, dev = 2 * self.B, self.dev
        W = torch.empty((S, self.T), dtype=torch.float32, device=dev)
        mx, den = (torch.empty(S, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev)) if keep \
            else (None, None)
        if self.B == 0:     # (an empty list has no pair_block the library would accept)
            return W, mx, den
        with _timed("sjoin_counts_attn"):
            d = self.desc()
            check(lib().subgacc_sjoin_counts_attn(ctypes.byref(d), ptr(g), ptr(W), ptr(mx), ptr(den), stream_ptr()))
        self.checked()
        return W, mx, den

    def backward(self, g, dW, W, mx, den):
        Dg = torch.zeros_like(W)
        if self.B == 0:
            return Dg
        with _timed("sjoin_counts_attn_backward"):
            d = self.desc()
            check(lib().subgacc_sjoin_counts_attn_backward(ctypes.byref(d), ptr(g), ptr(dW), ptr(W), ptr(mx), ptr(den), ptr(Dg),
                                                           stream_ptr()))
        return Dg


def counts_attn_stage(edge, x, encode, embed, gate_nn, value_nn=None):
    """The reference's first model stage of the LP encoder for --aggr attn, fused with the count form of the join:  model.py:59-62,78-81
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = AttentionalAggregation(gate_nn, nn)(x, ptr=ptr).view(2, -1, H'')
    Row t of segment j is E[p_t] + E[q_t] with E = embed(encode) [T, H] (T = c+1 LP rows, row 0 = partner absent) and (p_t, q_t) its
    index pair, so with one-Linear gate_nn (wg, bg) and nn the gate is g[p_t] + g[q_t] plus a constant the softmax drops (g = (E - mean
    of E's rows) wg),
    and, the weights summing to 1,
        out_j = nn(W[j] @ E) [n_j > 0],   W[j, r] = sum_t softmax_j(l)_t ([p_t = r] + [q_t = r])
    The library's kernels (subgacc_sjoin_counts_attn / _backward) join the pairs and write the softmax-weighted count rows W [2B, T] --
    neither xz, nor the [R,2,H] activations, nor the pair rows of attn_stage exist -- and the per-segment rows of dL/dg; the GEMM, nn
    and the gradients into embed and gate_nn are ordinary torch ops.  Every parameter receives a gradient; the gate bias's is exactly
    zero, as the reference's is analytically.  Results do not depend on the order of the pairs or on run-to-run timing.
    embed: any row-wise module (the reference's pe_embedding MLP), applied to the [T, k] table as in mean_stage; gate_nn: nn.Linear(H, 1)
    or a one-Linear Sequential; value_nn: None or nn.Linear(H, H'') (PyG 2.2's MLP([H, 1]) / MLP([H, H]) is that Linear, .lins[0]).
    edge: [2, B] integer (torch or NumPy); x: a packed SFptr SpG.  Returns float32 [2, B, H''] (H without value_nn), empty segments
    giving zero rows, with the join's status words as .join_flags.  W, dW and Dg are 4 T bytes per segment each: a store with many LP
    rows, or any other gate / value module, takes attn_stage."""
    name = "counts_attn_stage"
    if isinstance(x, StridedSpG):
        raise TypeError(f"{name} needs a packed SFptr (integer) SpG, not a StridedSpG (join its to_csr())")
    if isinstance(x, HeadedSpG):
        raise ValueError(f"{name} joins the packed store: keep it, or join z.to_spg() (the headed layout is for gather / hgather)")
    if not isinstance(x, SpG):
        raise TypeError(f"{name} joins a packed SFptr (integer) SpG, not {type(x).__name__}")
    if x.keyrows or x.data.dtype != torch.int32:
        raise TypeError(f"{name} needs a packed SFptr (integer) SpG (not a keyed() one); a float (PPR / SPD / DEG) store has "
                        "float_attn_stage(edge, x, embed, gate_nn, value_nn)")
    other = "attn_stage(edge, x, encode, embed, gate_nn, value_nn)"
    gate = _one_linear(gate_nn, "gate_nn", None, 1, name, other)
    H = gate.in_features
    val = _one_linear(value_nn, "value_nn", H, None, name, other) if value_nn is not None else None
    dev = x.device
    for mod in (gate, val, embed):
        for prm in (mod.parameters() if mod is not None else ()):
            if prm.device != dev or prm.dtype != torch.float32:
                raise ValueError(f"{name}: embed, gate_nn and value_nn must hold float32 parameters on the store's device ({dev})")
    table = encode if torch.is_tensor(encode) else torch.as_tensor(np.asarray(encode))
    if table.ndim != 2 or table.shape[0] < 1 or table.dtype.is_complex or table.dtype == torch.bool:
        raise ValueError(f"{name}: encode must be the [T, k] real LP table, got {table.dtype} of shape {tuple(table.shape)}")
    if table.is_cuda and table.device != dev:
        raise ValueError(f"{name}: encode lies on {table.device}, the store on {dev}")
    e = _edge_rows(edge, name)
    if e.shape[1] and (int(e.min()) < 0 or int(e.max()) >= x.n_rows):
        raise IndexError(f"row index out of range for an SpG with {x.n_rows} rows")
    T = int(table.shape[0])
    e = _as_rows(e, dev)
    B = int(e.shape[1])
    join = _CountsAttnJoin(x, x.join_rows()[1], e.contiguous().view(-1), B, T)
    E = embed(table.to(device=dev, dtype=torch.float32))
    if E.ndim != 2 or E.shape[0] != T or E.shape[1] != H:
        raise ValueError(f"{name}: embed(encode) is {tuple(E.shape)}, gate_nn takes rows of {H}")
    # the gate's logit of every LP row, its bias left out and E centred first: softmax drops the constant 2 mean(E) . wg, and with it the
    # cancellation of E's common offset in dL/dwg = (E - mean)^T dg (the centre is a constant of autograd: sum_r dg[r] = 0)
    g = (E - E.detach().mean(0)) @ gate.weight.view(-1)
    if torch.is_grad_enabled() and (g.requires_grad or (gate.bias is not None and gate.bias.requires_grad)):
        W = _CountsAttn.apply(g, gate.bias, join)
    else:
        W = join.forward(g.detach().contiguous(), False)[0]
    h = W @ E
    if val is not None:
        h = torch.nn.functional.linear(h, val.weight, val.bias)
    own = join.own
    nonempty = (x.indptr[own + 1] - x.indptr[own]) > 0
    out = (h * nonempty.to(h.dtype)[:, None]).view(2, B, h.shape[-1])
    out.join_flags = join.flags
    return out


LSTM_WIDTHS = tuple(range(16, 129, 16))     # H' the recurrent kernel takes (include/subgacc.h: subgacc_lstm_aggr)
_LSTM_PIECE = 1024                           # entries of one piece of dG's ordered sum (a table row's run is cut into such pieces)


def _lstm_layer(lstm, dev, name="index_lstm_stage", other="lstm_stage(edge, x, encode, embed, lstm)"):
    """(W_ih, W_hh, b_ih, b_hh) of a one-layer, unidirectional, batch_first, proj_size = 0, float32 nn.LSTM on `dev`, or TypeError /
    ValueError naming `other` (lstm_stage) as the general path"""
    if not isinstance(lstm, torch.nn.LSTM):
        raise TypeError(f"{name} fuses a torch.nn.LSTM only, not {type(lstm).__name__}; for any other module use {other}")
    if lstm.num_layers != 1 or lstm.bidirectional or not lstm.batch_first or getattr(lstm, "proj_size", 0) != 0:
        raise ValueError(f"{name} fuses a one-layer, unidirectional, batch_first nn.LSTM without projection (num_layers "
                         f"{lstm.num_layers}, bidirectional {lstm.bidirectional}, batch_first {lstm.batch_first}, proj_size "
                         f"{getattr(lstm, 'proj_size', 0)}); for any other use {other}")
    H2 = lstm.hidden_size
    if H2 not in LSTM_WIDTHS:
        raise ValueError(f"{name}: hidden_size {H2} is not a multiple of 16 in [16, 128]; for any other width use {other}")
    for p in lstm.parameters():
        if p.device != dev or p.dtype != torch.float32:
            raise ValueError(f"{name}: the LSTM must hold float32 parameters on the store's device ({dev}); otherwise use {other}")
    return lstm.weight_ih_l0, lstm.weight_hh_l0, getattr(lstm, "bias_ih_l0", None), getattr(lstm, "bias_hh_l0", None)


def _nonnull(t):
    """t, or one element of its dtype when t is empty (the library takes no NULL for an array it is told holds nothing)"""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def _sorted_pieces(pairs, T):
    """The ordered sums of the LSTM backwards (dG; dP / dQ): (perm, piece_off, P, run_piece) -- perm int64 [2R], the entries 2 row + side
    of `pairs` (int32 [R, 2], values in [0, T)) in a stable sort by value; piece_off int64 [P + 1] cuts perm into P pieces of at most
    _LSTM_PIECE entries, each inside one value's run; run_piece int64 [T + 1]: the pieces of value r are [run_piece[r], run_piece[r+1])"""
    dev = pairs.device
    idx = pairs.view(-1).long()
    srt, perm = torch.sort(idx, stable=True)
    cnt = torch.bincount(idx, minlength=T)
    start = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=start[1:])
    npc = (cnt + _LSTM_PIECE - 1) // _LSTM_PIECE
    run_piece = torch.zeros(T + 1, dtype=torch.int64, device=dev)
    torch.cumsum(npc, 0, out=run_piece[1:])
    P = int(run_piece[-1].item())
    owner = torch.repeat_interleave(torch.arange(T, device=dev), npc, output_size=P)
    k = torch.arange(P, device=dev) - run_piece[:-1][owner]
    piece_off = torch.empty(P + 1, dtype=torch.int64, device=dev)
    piece_off[:-1] = start[:-1][owner] + k * _LSTM_PIECE
    piece_off[-1] = idx.numel()
    return perm, piece_off.contiguous(), P, run_piece


class _LstmJoin:
    """the two library calls of index_lstm_stage over one batch's index form (pairs, indptr) padded to L steps"""

    def __init__(self, pairs, indptr, L, T, H2):
        self.pairs, self.indptr, self.L, self.T, self.H2 = pairs, indptr, L, T, H2
        self.S = indptr.numel() - 1
        self.dev = pairs.device
        self.flags = torch.zeros(4, dtype=torch.int32, device=self.dev)

    def checked(self):
        if int(self.flags[3].item()) & 2:
            raise IndexError(f"an index of the join is out of bounds for the encode table with {self.T} rows")

    def forward(self, G, b, w_hh, keep):
        S, L, H2, dev = self.S, self.L, self.H2, self.dev
        h = torch.empty((S, H2), dtype=torch.float32, device=dev)
        hs, cs = (torch.empty((S, L, H2), dtype=torch.float32, device=dev), torch.empty((S, L, H2), dtype=torch.float32, device=dev)) \
            if keep else (None, None)
        with _timed("lstm_aggr"):
            check(lib().subgacc_lstm_aggr(ptr(_nonnull(self.pairs)), ptr(self.indptr), S, L, self.T, H2, ptr(G), ptr(b), ptr(w_hh), ptr(h), ptr(hs),
                                          ptr(cs), ptr(self.flags), stream_ptr()))
        return h, hs, cs

    def grouping(self):
        """dG's ordered sum: the row of every index entry in a stable sort of the 2R indices, cut into pieces of at most _LSTM_PIECE
        entries inside one index's run, and the pieces of every index"""
        perm, piece_off, P, run_piece = _sorted_pieces(self.pairs, self.T)
        return (perm // 2).to(torch.int32), piece_off, P, run_piece

    def backward(self, G, b, w_hh, hs, cs, dh):
        S, H2, dev = self.S, self.H2, self.dev
        tiles = (S + 15) // 16
        R = self.pairs.shape[0]
        order, piece_off, P, run_piece = self.grouping()
        rows = torch.empty((R, 4 * H2), dtype=torch.float32, device=dev)
        pieces = torch.empty((P, 4 * H2), dtype=torch.float32, device=dev) if P else None
        dG = torch.empty((self.T, 4 * H2), dtype=torch.float32, device=dev)
        dw = torch.empty((tiles, 4 * H2, H2), dtype=torch.float32, device=dev)
        db = torch.empty((tiles, 4 * H2), dtype=torch.float32, device=dev)
        with _timed("lstm_aggr_backward"):
            check(lib().subgacc_lstm_aggr_backward(ptr(_nonnull(self.pairs)), ptr(self.indptr), S, self.L, self.T, H2, ptr(G), ptr(b),
                                                   ptr(w_hh), ptr(hs), ptr(cs), ptr(dh), ptr(_nonnull(order)), ptr(piece_off), P, ptr(run_piece),
                                                   ptr(_nonnull(rows)),
                                                   ptr(pieces), ptr(dG), ptr(dw), ptr(db), ptr(self.flags), stream_ptr()))
        return dG, db.sum(0), dw.sum(0)


class _LstmAggr(torch.autograd.Function):
    """h_{L-1} [S, H'] of subgacc_lstm_aggr as a function of (G, b, W_hh); backward: subgacc_lstm_aggr_backward's dG, and the sums over
    tiles of its dW_hh / db partials"""

    @staticmethod
    def forward(ctx, G, b, w_hh, join):
        ctx.join = join
        ctx.has_b = b is not None
        G, w_hh = G.detach().contiguous(), w_hh.detach().contiguous()
        b = b.detach().contiguous() if b is not None else None
        h, hs, cs = join.forward(G, b, w_hh, True)
        ctx.save_for_backward(G, b, w_hh, hs, cs)
        return h

    @staticmethod
    def backward(ctx, dh):
        G, b, w_hh, hs, cs = ctx.saved_tensors
        dG, db, dw = ctx.join.backward(G, b if ctx.has_b else None, w_hh, hs, cs, dh.contiguous())
        return dG, (db if ctx.has_b else None), dw, None


def index_lstm_stage(edge, x, encode, embed, lstm):
    """The reference's first model stage of the LP encoder for --aggr lstm, folded into one recurrent kernel:  model.py:63-65,78-83
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = LSTMAggregation(H, H')(x, index=ptr).view(2, -1, H')
    Same arguments and result as lstm_stage.  Row t of segment j is E[p_t] + E[q_t] with E = embed(encode) [T, H] and (p_t, q_t) the index
    pair gather_index returns, so the LSTM's input projection is a lookup into G = E W_ih^T [T, 4H'] plus b = b_ih + b_hh; the library's
    kernel (subgacc_lstm_aggr) runs the recurrence gates = G[p_t] + G[q_t] + b + W_hh h_{t-1} over every segment for the batch's L steps
    (zero input past a segment's rows, as the reference's padding) on the MFMA -- neither xz, nor the dense [S, L, H] batch, nor the LSTM's
    [S, L, H'] output exist.  Under autograd the forward keeps h_t, c_t ([S, L, H'] each) and the backward (subgacc_lstm_aggr_backward)
    returns dG, db and dW_hh; torch carries dG into embed and W_ih, so every parameter receives a gradient.  A segment's result does not
    depend on the other segments of the batch, the order of its pairs' neighbours or the store layout.
    lstm: a one-layer, unidirectional, batch_first, proj_size = 0, float32 nn.LSTM on the store's device with hidden_size in 16, 32, ..,
    128; x: an integer (LP) SpG or StridedSpG (packed, on-demand or key-row batches).  Returns float32 [2, B, H'] (left endpoints, right
    endpoints) with the status words as .join_flags.  Any other LSTM, width or store takes lstm_stage."""
    name = "index_lstm_stage"
    if isinstance(x, HeadedSpG):
        raise ValueError(f"{name} joins the packed store: keep it, or join z.to_spg() (the headed layout is for gather / hgather); "
                         "lstm_stage(edge, x, encode, embed, lstm) takes the same")
    if not isinstance(x, (SpG, StridedSpG)):
        raise TypeError(f"{name} joins an integer (LP) SpG or StridedSpG, not {type(x).__name__}")
    if isinstance(x, SpG) and not x.keyrows and x.data.dtype != torch.int32:
        raise TypeError(f"{name} joins an integer (LP) store; a float (PPR / SPD / DEG) store has "
                        "float_lstm_stage(edge, x, embed, lstm)")
    dev = x.device
    w_ih, w_hh, b_ih, b_hh = _lstm_layer(lstm, dev, name)
    H2 = lstm.hidden_size
    table = encode if torch.is_tensor(encode) else torch.as_tensor(np.asarray(encode))
    if table.ndim != 2 or table.shape[0] < 1 or table.dtype.is_complex or table.dtype == torch.bool:
        raise ValueError(f"{name}: encode must be the [T, k] real LP table, got {table.dtype} of shape {tuple(table.shape)}")
    if table.is_cuda and table.device != dev:
        raise ValueError(f"{name}: encode lies on {table.device}, the store on {dev}")
    e = _edge_rows(edge, name)
    T = int(table.shape[0])
    er = _as_rows(e, dev)
    own = er.reshape(-1)
    if own.numel() and bool(((own < 0) | (own >= x.n_rows)).any()):
        raise IndexError(f"row index out of range for an SpG with {x.n_rows} rows")
    sizes = x.nsize[own] if isinstance(x, StridedSpG) else x.indptr[own + 1] - x.indptr[own]
    if own.numel() and int(sizes.sum().item()) == 0:     # no rows at all (the join asks for none): L = 1 padded step per segment
        pairs, indptr = torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(own.numel() + 1, dtype=torch.int64, device=dev)
    else:
        pairs, indptr = gather_index(er, x)
    if pairs.numel() and int(pairs.max().item()) >= T:
        raise IndexError(f"index {int(pairs.max().item())} is out of bounds for the encode table with {T} rows")
    S = indptr.numel() - 1
    L = max(int((indptr[1:] - indptr[:-1]).max().item()), 1) if S else 1
    E = embed(table.to(device=dev, dtype=torch.float32))
    if E.ndim != 2 or E.shape[0] != T or E.shape[1] != lstm.input_size:
        raise ValueError(f"{name}: embed(encode) is {tuple(E.shape)}, the LSTM takes rows of {lstm.input_size}")
    G = E @ w_ih.t()
    b = (b_ih + b_hh) if b_ih is not None else None
    join = _LstmJoin(pairs.contiguous(), indptr.contiguous(), L, T, H2)
    if S == 0:
        h = G.new_zeros((0, H2))
    elif torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (G, b, w_hh)):
        h = _LstmAggr.apply(G, b, w_hh, join)
    else:
        h = join.forward(G.detach().contiguous(), b.detach().contiguous() if b is not None else None, w_hh.detach().contiguous(), False)[0]
    if S:
        join.checked()
    out = h.view(2, -1, H2)
    out.join_flags = join.flags
    return out


def sample_and_index(csr, edge, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None, table_rows=None, buffers=None,
                     wide_keys=False):
    """The index form of the on-demand step: sample the endpoints of `edge` [2, B], number the batch's distinct LP rows as
    sample_and_counts does, and join the key rows as INDEX PAIRS -> (pairs int32 [R, 2], indptr int64 [2B+1], table float32 [T, m+1],
    sets).  Row indptr[j] + t of `pairs` is (p_t, q_t) for member t of segment j (gather()'s segments and row order: members in ascending
    node id): p_t the row of `table` of the member's own LP row, q_t that of the member of the partner's set with the same id, 0 -- the
    zero row -- without one.  table[pairs.long()] is, bit for bit, the xz of sample_and_gather over the same seed, and indptr is its
    indptr; what gather_index(edge, z) returns over the all-nodes store z of the same seed are these pairs under the store's own
    numbering.  A column is its key's RANK among the batch's distinct keys, so (pairs, indptr, table) are the same bits whatever the
    schedule, the walk order (order=), root dedup and whether buffers are used.  Neither xz nor an output buffer of the row form exists:
    the step writes 8 bytes per row instead of 8 (m+1).
    table_rows=None (no buffers): the number of distinct LP rows is read back once and T is exactly that + 1.  table_rows=T: T rows, the
    rows past the batch's distinct LP rows zero; more distinct rows than T - 1 raise SubgAccError.  Without buffers the step is resolved
    before it returns.
    buffers=StepBuffers(csr, B, ..., stage="index", table_rows=T): nothing is allocated and nothing read back (capturable); the results
    are views of the buffers -- `pairs` of the whole buffer, of which the first indptr[-1] rows are the result -- and
    buffers.sets.resolve() raises SubgAccError naming table_rows when the step had more than T - 1 distinct LP rows (the pairs of the
    others read row 0; nothing is written out of bounds).  Shapes: 32-bit key rows (2 to 4 hops, num_steps*SHIFT+1 <= 31), rng Philox."""
    who = "sample_and_index"
    e = _as_rows(edge, csr.device)
    if e.dim() != 2 or e.shape[0] != 2:
        raise ValueError(f"{who}: edge must be [2, B], not {list(e.shape)}")
    if e.shape[1] == 0 and buffers is None:      # an empty batch: no step, the zero row alone
        T = 2 if table_rows is None else int(table_rows)
        _counts_stage_shape(who, num_walks, num_steps, True, T, wide_keys)
        dev = csr.device
        return (torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                torch.zeros((T, int(num_steps) + 1), dtype=torch.float32, device=dev), None)
    pairs, indptr, table, sets = _step_counts(who, csr, e, False, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers,
                                              stage="index", wide_keys=wide_keys)
    if buffers is None:
        pairs = pairs[: int(indptr[-1].item())]
    return pairs, indptr, table, sets


class _StepLstmJoin(_LstmJoin):
    """_LstmJoin over the index pairs of ONE step of `bufs` (sample_and_lstm_stage with buffers=): pairs and indptr are views of the
    buffers and live until the buffers take their next step: a kernel or a backward that comes later is refused, never answered from
    another batch (_StepAttnJoin._require_fresh's rule)."""

    def __init__(self, pairs, indptr, L, T, H2, bufs, step_id):
        super().__init__(pairs, indptr, L, T, H2)
        self.bufs, self.step_id = bufs, step_id

    def _require_fresh(self, what):
        now = getattr(self.bufs, "step_id", 0)
        if now != self.step_id:
            raise RuntimeError(f"sample_and_lstm_stage: the {what} of step {self.step_id} of these StepBuffers ran after they took "
                               f"step {now}: the pairs it reads are gone (run a step's backward before the buffers' next step)")

    def forward(self, G, b, w_hh, keep):
        self._require_fresh("kernel")
        return super().forward(G, b, w_hh, keep)

    def backward(self, G, b, w_hh, hs, cs, dh):
        self._require_fresh("backward")
        return super().backward(G, b, w_hh, hs, cs, dh)


def sample_and_lstm_stage(csr, edge, embed, lstm, num_walks=200, num_steps=3, seed=111413, dedup_roots=False, order=None,
                          table_rows=None, buffers=None, wide_keys=False):
    """The reference's first model stage of the LP encoder for --aggr lstm (model.py:63-65,78-83: x = pe_embedding(xz).sum(dim=-2);
    xl, xr = LSTMAggregation(H, H')(x, index=ptr).view(2, -1, H'); main.py:217) on the on-demand step -- index_lstm_stage's algebra
    without a resident store, and without xz [R,2,k], the packed copy of the step's rows or their registration:
        E = embed(table),  G = E W_ih^T,  h_j = the recurrence gates = G[p_t] + G[q_t] + b + W_hh h_{t-1} over segment j, padded to L steps
    with (pairs, indptr, table) = sample_and_index(...) and L = max(the longest segment, 1): the reference pads every segment to the
    longest of its batch and takes the output at the last position, so L is part of its arithmetic.  The recurrence is subgacc_lstm_aggr
    (under autograd subgacc_lstm_aggr_backward: dG, db, dW_hh; torch carries dG into embed and W_ih), so every parameter of embed and
    lstm receives a gradient.  Because a row of `table` is its key's rank, output and gradients are the same bits whatever the
    schedule, the walk order, root dedup and buffers.
    embed: any row-wise module [T, m+1] -> [T, H]; lstm: a one-layer, unidirectional, batch_first, proj_size = 0, float32 nn.LSTM(H, H')
    on the graph's device with hidden_size in 16, 32, .., 128 -- any other takes sample_and_gather(csr, edge, ...) and the modules on xz.
    Returns float32 [2, B, H'] (left endpoints, right endpoints).  Keywords as sample_and_index.
    The stage reads two words back, the row count R and L (L sizes the kept states h_t, c_t [2B, L, H']): it is NOT capturable, with or
    without buffers.  With buffers= the sampling part allocates nothing, the step's SampledSets are `buffers.sets` (`.resolve()` raises
    when the step had more distinct LP rows than table_rows - 1), and the backward reads the pairs from the buffers: it must run before
    the buffers take their next step (RuntimeError naming the step otherwise).  The recurrent kernel's status words travel with the
    result as .join_flags, as index_lstm_stage's do; the stage does not read them."""
    name = "sample_and_lstm_stage"
    dev = csr.device
    w_ih, w_hh, b_ih, b_hh = _lstm_layer(lstm, dev, name, "sample_and_gather(csr, edge, ...) and the modules on xz")
    H2 = lstm.hidden_size
    for prm in embed.parameters():
        if prm.device != dev or prm.dtype != torch.float32:
            raise ValueError(f"{name}: embed must hold float32 parameters on the graph's device ({dev})")
    pairs, indptr, table, _ = sample_and_index(csr, edge, num_walks, num_steps, seed, dedup_roots, order, table_rows, buffers, wide_keys)
    S, T = indptr.numel() - 1, int(table.shape[0])
    E = embed(table)
    if E.ndim != 2 or E.shape[0] != T or E.shape[1] != lstm.input_size:
        raise ValueError(f"{name}: embed(table) is {tuple(E.shape)}, the LSTM takes rows of {lstm.input_size}")
    if S == 0:
        return E.new_zeros((2, 0, H2))
    R, L = torch.stack([indptr[-1], (indptr[1:] - indptr[:-1]).max()]).tolist()      # the stage's read-back: two words
    G = E @ w_ih.t()
    b = (b_ih + b_hh) if b_ih is not None else None
    L = max(int(L), 1)
    join = _LstmJoin(pairs[:R], indptr, L, T, H2) if buffers is None else _StepLstmJoin(pairs[:R], indptr, L, T, H2, buffers, buffers.step_id)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (G, b, w_hh)):
        h = _LstmAggr.apply(G, b, w_hh, join)
    else:
        h = join.forward(G.detach().contiguous(), b.detach().contiguous() if b is not None else None, w_hh.detach().contiguous(), False)[0]
    out = h.view(2, -1, H2)
    out.join_flags = join.flags     # the recurrent kernel's status words, not read here: every pair is 1 + a rank < T by construction
    return out


def hinge_tables(lin1, lin2, w_ih, b_ih=None, b_hh=None):
    """The LSTM's input projection over a float store as a table of one scalar.  With pe_embedding = (lin1 = Linear(1, H), ReLU, lin2 =
    Linear(H, H1)) and V = W_ih W2 ([4H', H]):  W_ih x_t + b_ih + b_hh = F(a_t) + F(b_t) + c_real,  F(s) = V relu(w1 s + b1), and F is
    piecewise linear with the knots -b1[c] / w1[c].  Returns (knots, P, Q, c_real, c_pad):
        knots [H] sorted ascending (+inf for a channel with w1 = 0); k(s) = hinge_intervals(s, knots) in [0, 2H]: 2r in the open
            interval behind r knots, 2r - 1 ON a knot (r = the number of knots <= s);
        P = (A * w1) V^T, Q = (A * b1) V^T  ([2H+1, 4H']): F(s) = P[k(s)] s + Q[k(s)], A [2H+1, H] the 0/1 activity of every channel in
            every interval (w1 > 0: active above its knot; w1 < 0: active below its knot; w1 = 0: everywhere iff b1 > 0; on its own
            knot a channel is off, so the gradients take relu'(0) = 0 as torch does -- F itself is continuous there);
        c_pad = b_ih + b_hh (a padded step: zero input), c_real = c_pad + 2 W_ih b2; None where every term is absent.
    knots and A are constants of autograd; P, Q, c_real, c_pad are torch products of the parameters, so their gradients reach w1, b1, W2,
    b2, W_ih, b_ih and b_hh.  Pure torch, any dtype and device."""
    w1 = lin1.weight.view(-1)
    b1 = lin1.bias if lin1.bias is not None else torch.zeros_like(w1)
    V = w_ih @ lin2.weight
    with torch.no_grad():
        inf = torch.full_like(w1, float("inf"))
        knot = torch.where(w1 != 0, -b1 / torch.where(w1 != 0, w1, torch.ones_like(w1)), inf)
        knots, _ = torch.sort(knot)
        lo = torch.cat([-inf[:1], knots])                   # [H+1] the ends of the open interval behind r knots: lo[r] < s < hi[r]
        hi = torch.cat([knots, inf[:1]])
        up, down, const = (w1 > 0)[None, :], (w1 < 0)[None, :], ((w1 == 0) & (b1 > 0))[None, :]
        A = torch.empty((2 * w1.numel() + 1, w1.numel()), dtype=w1.dtype, device=w1.device)
        A[0::2] = ((up & (knot[None, :] <= lo[:, None])) | (down & (knot[None, :] >= hi[:, None])) | const).to(w1.dtype)
        # on a knot the channels of that knot are off, as relu'(0) = 0 has it
        A[1::2] = ((up & (knot[None, :] < knots[:, None])) | (down & (knot[None, :] > knots[:, None])) | const).to(w1.dtype)
    P = (A * w1) @ V.t()
    Q = (A * b1) @ V.t()
    c_pad = (b_ih + b_hh) if b_ih is not None else None
    c_real = c_pad
    if lin2.bias is not None:
        c2 = w_ih @ (2 * lin2.bias)
        c_real = c2 if c_pad is None else c_pad + c2
    return knots, P, Q, c_real, c_pad


def hinge_intervals(s, knots):
    """k(s) of hinge_tables: 2r in the open interval behind r knots, 2r - 1 on a knot, r = the number of knots <= s (int64, in [0, 2H])"""
    s = s.contiguous()
    r = torch.bucketize(s, knots, right=True)
    return 2 * r - (r > torch.bucketize(s, knots, right=False)).to(r.dtype)


class _HingeJoin:
    """the two library calls of float_lstm_stage over one batch's float join (vals [R, 2], their intervals idx, indptr) padded to L steps"""

    def __init__(self, vals, idx, indptr, L, K, H2, flags):
        self.vals, self.idx, self.indptr, self.L, self.K, self.H2, self.flags = vals, idx, indptr, L, K, H2, flags
        self.S = indptr.numel() - 1
        self.dev = indptr.device

    def checked(self):
        if int(self.flags[3].item()) & 2:
            raise IndexError(f"an interval of the join is out of bounds for the table with {self.K} rows")

    def forward(self, tab, c_real, c_pad, w_hh, keep):
        S, L, H2, dev = self.S, self.L, self.H2, self.dev
        h = torch.empty((S, H2), dtype=torch.float32, device=dev)
        hs, cs = (torch.empty((S, L, H2), dtype=torch.float32, device=dev), torch.empty((S, L, H2), dtype=torch.float32, device=dev)) \
            if keep else (None, None)
        with _timed("lstm_aggr_hinge"):
            check(lib().subgacc_lstm_aggr_hinge(ptr(_nonnull(self.vals)), ptr(_nonnull(self.idx)), ptr(self.indptr), S, L, self.K, H2,
                                                ptr(tab), ptr(c_real), ptr(c_pad), ptr(w_hh), ptr(h), ptr(hs), ptr(cs), ptr(self.flags),
                                                stream_ptr()))
        return h, hs, cs

    def backward(self, tab, c_real, c_pad, w_hh, hs, cs, dh):
        S, H2, K, dev = self.S, self.H2, self.K, self.dev
        tiles = (S + 15) // 16
        R = self.idx.shape[0]
        perm, piece_off, P, run_piece = _sorted_pieces(self.idx, K)
        order = perm.to(torch.int32)
        rows = torch.empty((R, 4 * H2), dtype=torch.float32, device=dev)
        pieces = torch.empty((2, P, 4 * H2), dtype=torch.float32, device=dev) if P else None
        dP, dQ = (torch.empty((K, 4 * H2), dtype=torch.float32, device=dev) for _ in range(2))
        dw = torch.empty((tiles, 4 * H2, H2), dtype=torch.float32, device=dev)
        dcr, dcp = (torch.empty((tiles, 4 * H2), dtype=torch.float32, device=dev) for _ in range(2))
        with _timed("lstm_aggr_hinge_backward"):
            check(lib().subgacc_lstm_aggr_hinge_backward(
                ptr(_nonnull(self.vals)), ptr(_nonnull(self.idx)), ptr(self.indptr), S, self.L, K, H2, ptr(tab), ptr(c_real), ptr(c_pad),
                ptr(w_hh), ptr(hs), ptr(cs), ptr(dh), ptr(_nonnull(order)), ptr(piece_off), P, ptr(run_piece), ptr(_nonnull(rows)),
                ptr(pieces), ptr(dP), ptr(dQ), ptr(dw), ptr(dcr), ptr(dcp), ptr(self.flags), stream_ptr()))
        return torch.stack([dP, dQ], dim=-1), dcr.sum(0), dcp.sum(0), dw.sum(0)


class _HingeLstm(torch.autograd.Function):
    """h_{L-1} [S, H'] of subgacc_lstm_aggr_hinge as a function of (tab, c_real, c_pad, W_hh); backward: subgacc_lstm_aggr_hinge_backward's
    dP / dQ (interleaved as tab is) and the sums over tiles of its dW_hh, dc_real and dc_pad partials"""

    @staticmethod
    def forward(ctx, tab, c_real, c_pad, w_hh, join):
        ctx.join = join
        ctx.has = (c_real is not None, c_pad is not None)
        tab, w_hh = tab.detach().contiguous(), w_hh.detach().contiguous()
        c_real = c_real.detach().contiguous() if c_real is not None else None
        c_pad = c_pad.detach().contiguous() if c_pad is not None else None
        h, hs, cs = join.forward(tab, c_real, c_pad, w_hh, True)
        ctx.save_for_backward(tab, c_real, c_pad, w_hh, hs, cs)
        return h

    @staticmethod
    def backward(ctx, dh):
        tab, c_real, c_pad, w_hh, hs, cs = ctx.saved_tensors
        dtab, dcr, dcp, dw = ctx.join.backward(tab, c_real if ctx.has[0] else None, c_pad if ctx.has[1] else None, w_hh, hs, cs,
                                               dh.contiguous())
        return dtab, (dcr if ctx.has[0] else None), (dcp if ctx.has[1] else None), dw, None


def float_lstm_stage(edge, x, embed, lstm):
    """The reference's first model stage for the float encoders (PPR, SPD, DEG) with --aggr lstm, in the recurrent kernel of
    index_lstm_stage:  model.py:63-65,78-83
        x = pe_embedding(xz).sum(dim=-2);  xl, xr = LSTMAggregation(H1, H')(x, index=ptr).view(2, -1, H')
    with pe_embedding = embed = Sequential(Linear(1, H), ReLU(), Linear(H, H1)) over the float join's xz [R,2,1], every segment padded
    with zero rows to the batch's longest (L = max(longest, 1)) and the output taken at position L-1.  A row is a pair of scalars (a, b),
    and W_ih x_t = F(a) + F(b) + const with F(s) = W_ih W2 relu(w1 s + b1) piecewise linear in one scalar: hinge_tables() turns the
    parameters into P, Q [2H+1, 4H'] with F(s) = P[k(s)] s + Q[k(s)], and the library's kernel (subgacc_lstm_aggr_hinge) runs
        gates_t = ((P[ka] a + Q[ka]) + (P[kb] b + Q[kb])) + c_real + W_hh h_{t-1}   (c_pad + W_hh h_{t-1} on a padded step)
    on the MFMA -- neither the [R,2,H] activations, nor the dense [S, L, H1] batch, nor the LSTM's [S, L, H'] output exist.  The rows
    come from the float join (gather: xz float32 [R,2,1] and indptr, 8 bytes per row).  Under autograd the forward keeps h_t, c_t
    (8 S L H' bytes) and the backward (subgacc_lstm_aggr_hinge_backward) takes a [R, 4H'] workspace (16 R H' bytes) and returns dP, dQ,
    dc_real, dc_pad and dW_hh; torch carries them into every parameter of embed and lstm.  At B = 65,536 over a top-100 store with
    H' = 96 that is about 10 GB + 18 GB (derived, not measured).  With grad disabled (or nothing requiring it) no state is kept and the
    forward's bits are the same.  No float is added atomically: repeated runs give the same bits, and a segment's result does not
    depend on the other segments, the order of the pairs or the store layout.
    edge: [2, B] integer (torch or NumPy); x: a float64 SpG or HeadedSpG; lstm: a one-layer, unidirectional, batch_first, proj_size = 0,
    float32 nn.LSTM on the store's device with input_size = H1 and hidden_size in 16, 32, .., 128.  Returns float32 [2, B, H'] (left
    endpoints, right endpoints) with the join's status words as .join_flags.  There is no general float path behind this one: anything
    else is written by hand as xz, ind = gather(edge, x) and the modules on xz."""
    name = "float_lstm_stage"
    other = "xz, ind = gather(edge, x) and the modules on xz"
    st = _FloatStage(name, "index_lstm_stage(edge, x, encode, embed, lstm)", edge, x, embed)
    w_ih, w_hh, b_ih, b_hh = _lstm_layer(lstm, st.dev, name, other)
    H1, H2 = st.lin2.out_features, lstm.hidden_size
    if lstm.input_size != H1:
        raise ValueError(f"{name}: embed gives rows of {H1}, the LSTM takes rows of {lstm.input_size}; otherwise use {other}")
    dev = st.dev
    e = _as_rows(st.edge, dev)
    B = int(e.shape[1])
    own = e.contiguous().view(-1)
    if B and bool(((own < 0) | (own >= x.n_rows)).any()):
        raise IndexError(f"row index out of range for an SpG with {x.n_rows} rows")
    st.join_on()
    if B == 0 or not bool(st.nonempty().any()):     # no rows at all (the join asks for none): L = 1 padded step per segment
        xz, indptr = torch.zeros((0, 2, 1), dtype=torch.float32, device=dev), torch.zeros(2 * B + 1, dtype=torch.int64, device=dev)
        flags = st.flags
    else:
        xz, indptr, flags = sjoin(x, own, None, None, ptr_mode=True, pair_block=B)
    S = 2 * B
    if xz.shape[0] >= 1 << 30:
        raise ValueError(f"{name}: {xz.shape[0]} rows in one batch; the ordered sums index 2R entries with 32 bits")
    L = max(int((indptr[1:] - indptr[:-1]).max().item()), 1) if S else 1
    knots, P, Q, c_real, c_pad = hinge_tables(st.lin1, st.lin2, w_ih, b_ih, b_hh)
    vals = xz.reshape(-1, 2).contiguous()
    idx = hinge_intervals(vals, knots).to(torch.int32)
    tab = torch.stack([P, Q], dim=-1)
    join = _HingeJoin(vals, idx, indptr.contiguous(), L, 2 * st.H + 1, H2, flags)
    if S == 0:
        h = tab.new_zeros((0, H2))
    elif torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (tab, c_real, c_pad, w_hh)):
        h = _HingeLstm.apply(tab, c_real, c_pad, w_hh, join)
    else:
        h = join.forward(tab.detach().contiguous(), c_real.detach().contiguous() if c_real is not None else None,
                         c_pad.detach().contiguous() if c_pad is not None else None, w_hh.detach().contiguous(), False)[0]
    if S:
        join.checked()
    out = h.view(2, -1, H2)
    out.join_flags = flags
    return out

"""ctypes binding of libsubgacc_hip.so, derived from the declarations of include/subgacc.h (the C ABI), of include/subgacc_half.h
(the join's rows in a 16-bit type), of include/subgacc_small.h (key rows for the small walk shapes), of include/subgacc_packed.h
(the step's key rows as one word per member), of include/subgacc_wide.h (the columns of 64-bit key rows), of include/subgacc_half64.h
(the 16-bit rows over 64-bit key rows), of include/subgacc_packed_half.h (the packed rows joined in 16 bits), of
include/subgacc_half_ids.h (the 16-bit rows with their segment ids), of include/subgacc_star.h (the prologue of a step of one
source against K targets), of include/subgacc_mean.h (the mean first stage fused into the count join) and of include/subgacc_attn.h
(the attentional first stage fused into the attentional count join) when this module is imported: an entry point is declared there and defined under csrc/, and
nothing here names it.

There is no CPU fallback: if the library is missing, or no gfx950 device is visible when a compute entry
point is called, this module raises.  Error codes map onto the exceptions the reference raises for the
same condition (subg_acc/subg_acc.c:658, :688-721, :905-915).
"""
import ctypes as C
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# SUBGACC_LIB (dev-only): load an experiment build from elsewhere (tools/ab_*.sh) -- the shipped library is never overwritten
LIB_PATH = os.environ.get("SUBGACC_LIB") or os.path.join(_HERE, "libsubgacc_hip.so")
CSRC = os.path.join(_HERE, "csrc")

OK, ERR_BADARG, ERR_WORKSPACE, ERR_KEYWIDTH, ERR_CAPACITY, ERR_HIP, ERR_LDS, ERR_NODEVICE = 0, -1, -2, -3, -4, -5, -6, -7
RNG_RAND_R, RNG_PHILOX = 0, 1
ORDER_WALK_MAJOR, ORDER_STEP_MAJOR = 0, 1


class WalkCfg(C.Structure):
    """struct subgacc_walk_cfg"""
    _fields_ = [("num_walks", C.c_int32), ("num_steps", C.c_int32), ("bucket", C.c_int32), ("rng_mode", C.c_int32),
                ("seed", C.c_uint32), ("first_hop_wo", C.c_int32), ("order", C.c_int32),
                ("cap_root_degree", C.c_int32), ("indptr64", C.c_int32), ("emit_walks", C.c_int32),
                ("hop_records", C.c_void_p), ("rec_id_bits", C.c_int32), ("rec_beg_bits", C.c_int32),
                ("walk_pos", C.c_void_p), ("row_pitch", C.c_int32)]


class JoinDesc(C.Structure):
    """struct subgacc_join_desc (include/subgacc.h, ABI 7): what one call of subgacc_sjoin_fill_v2 joins"""
    _fields_ = [("struct_bytes", C.c_int32), ("form", C.c_int32), ("payload_kind", C.c_int32), ("max_len", C.c_int32),
                ("row_off", C.c_void_p), ("row_len", C.c_void_p), ("row_stride", C.c_int64), ("n_rows", C.c_int64),
                ("ids", C.c_void_p), ("payload", C.c_void_p), ("uniq_table", C.c_void_p), ("uniq_capacity", C.c_int64),
                ("own", C.c_void_p), ("partner", C.c_void_p), ("S", C.c_int64), ("seg", C.c_void_p), ("pair_block", C.c_int64),
                ("table", C.c_void_p), ("table_rows", C.c_int64), ("k", C.c_int32), ("num_walks", C.c_int32),
                ("num_steps", C.c_int32), ("options", C.c_int32), ("out_xz", C.c_void_p), ("out_idx", C.c_void_p),
                ("out_segid", C.c_void_p), ("out_counts", C.c_void_p), ("out_pairs", C.c_void_p), ("out_mult", C.c_void_p),
                ("out_cnt", C.c_void_p), ("flags", C.c_void_p), ("out_seg", C.c_void_p), ("size_state", C.c_void_p),
                ("size_state_bytes", C.c_int64), ("host_tail", C.c_void_p)]


JOIN_SFPTR, JOIN_F64, JOIN_KEY32, JOIN_KEY64 = 0, 1, 2, 3      # payload_kind
JOIN_ROWS, JOIN_COUNTS, JOIN_PAIRS = 0, 1, 2                   # form
JOIN_OPT_SIZES = 1                                             # options: size pass + fill in one call
JOIN_OPT_STAR = 2                                              # options: one source against K targets (gather_star)


class SubgAccError(RuntimeError):
    pass


HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "subgacc.h"))
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_STRUCTS = {"const subgacc_walk_cfg *": WalkCfg, "const subgacc_join_desc *": JoinDesc}


def parse_header(text):
    """{name: (return type, [(argument name, C type)])} of every `ret subgacc_name(args);` of a header's text, in declaration
    order.  Comments go first (the header's hold parentheses and semicolons), then the preprocessor lines."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def ctype(t):          # "const  float*" -> "const float *"
        return " ".join(t.replace("*", " * ").split())

    decls = {}
    for ret, name, args in re.findall(r"([\w\s*]+?)\b(subgacc_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for arg in ([] if args.strip() == "void" else args.split(",")):
            m = re.fullmatch(r"(.*[\s*])(\w+)", arg.strip())
            if not m:
                raise SubgAccError(f"{name}: cannot read the parameter `{arg.strip()}`")
            params.append((m.group(2), ctype(m.group(1))))
        if name in decls:
            raise SubgAccError(f"{name} is declared twice")
        decls[name] = (ctype(ret), params)
    return decls


def bind_types(decls):
    """{name: (restype, argtypes)} for the declarations of parse_header()"""
    return {name: (_ctype(ret, name, ret=True), [_ctype(t, name) for _, t in args]) for name, (ret, args) in decls.items()}


def _ctype(ctype, decl, ret=False):
    """the ctypes type of one C type -- a type the ABI does not use is an error that names the declaration, never a guess"""
    if ctype in _SCALARS:
        return _SCALARS[ctype]
    if ret and ctype == "const char *":
        return C.c_char_p
    if not ret and ctype.endswith("*"):
        return C.POINTER(_STRUCTS[ctype]) if ctype in _STRUCTS else C.c_void_p
    raise SubgAccError(f"{decl}: no ctypes type for the {'return' if ret else 'parameter'} type `{ctype}`")


def _header_text(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise SubgAccError(f"{path} is missing or unreadable: the binding is derived from it") from e


_TEXT = _header_text(HEADER)
DECLS = parse_header(_TEXT)
_TYPES = bind_types(DECLS)
SYMBOLS = tuple(DECLS)            # every entry point the header declares, in its order
ABI_VERSION = int(re.search(r"^#define\s+SUBGACC_ABI_VERSION\s+(\d+)", _TEXT, re.M).group(1))
# the second header (read after the first: a tree without include/ fails on subgacc.h): the same library, the same descriptor
HALF_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_half.h")
_HALF_TEXT = _header_text(HALF_HEADER)
HALF_DECLS = parse_header(_HALF_TEXT)
_TYPES.update(bind_types(HALF_DECLS))
HALF_SYMBOLS = tuple(HALF_DECLS)
# the third header: key rows for the small walk shapes (csrc/walk_small.hip), the same library
SMALL_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_small.h")
SMALL_DECLS = parse_header(_header_text(SMALL_HEADER))
_TYPES.update(bind_types(SMALL_DECLS))
SMALL_SYMBOLS = tuple(SMALL_DECLS)
# the fourth header: the step's key rows as one word per member (csrc/walk_rows.hip's packed store, csrc/sjoin_packed.hip), the same library
PACKED_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_packed.h")
PACKED_DECLS = parse_header(_header_text(PACKED_HEADER))
_TYPES.update(bind_types(PACKED_DECLS))
PACKED_SYMBOLS = tuple(PACKED_DECLS)
# the fifth header: the columns of a step's 64-bit key rows and their 32-bit surrogate keys (csrc/keycols64.hip), the same library
WIDE_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_wide.h")
WIDE_DECLS = parse_header(_header_text(WIDE_HEADER))
_TYPES.update(bind_types(WIDE_DECLS))
WIDE_SYMBOLS = tuple(WIDE_DECLS)
# the sixth header: the join's rows in a 16-bit type over 64-bit key rows (csrc/sjoin_half64.hip), the same library, the same descriptor
HALF64_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_half64.h")
HALF64_DECLS = parse_header(_header_text(HALF64_HEADER))
_TYPES.update(bind_types(HALF64_DECLS))
HALF64_SYMBOLS = tuple(HALF64_DECLS)
# the seventh header: the join over the step's packed rows written in a 16-bit type (csrc/sjoin_packed_half.hip), the same library
PACKED_HALF_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_packed_half.h")
PACKED_HALF_DECLS = parse_header(_header_text(PACKED_HALF_HEADER))
_TYPES.update(bind_types(PACKED_HALF_DECLS))
PACKED_HALF_SYMBOLS = tuple(PACKED_HALF_DECLS)
# the eighth header: the 16-bit rows with the segment id of every row (csrc/sjoin_half.hip), the same library, the same descriptor
HALF_IDS_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_half_ids.h")
HALF_IDS_DECLS = parse_header(_header_text(HALF_IDS_HEADER))
_TYPES.update(bind_types(HALF_IDS_DECLS))
HALF_IDS_SYMBOLS = tuple(HALF_IDS_DECLS)
# the ninth header: the prologue of a step of one source against K targets (csrc/walk_prep.hip), the same library
STAR_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_star.h")
STAR_DECLS = parse_header(_header_text(STAR_HEADER))
_TYPES.update(bind_types(STAR_DECLS))
STAR_SYMBOLS = tuple(STAR_DECLS)
# the tenth header: the LP encoder's mean first stage fused into the count join of a step (csrc/sjoin_mean.hip), the same library
MEAN_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_mean.h")
MEAN_DECLS = parse_header(_header_text(MEAN_HEADER))
_TYPES.update(bind_types(MEAN_DECLS))
MEAN_SYMBOLS = tuple(MEAN_DECLS)
# the eleventh header: the LP encoder's attentional first stage fused into the attentional count join of a step
# (csrc/sjoin_key_attn.hip), the same library
ATTN_HEADER = os.path.join(os.path.dirname(HEADER), "subgacc_attn.h")
ATTN_DECLS = parse_header(_header_text(ATTN_HEADER))
_TYPES.update(bind_types(ATTN_DECLS))
ATTN_SYMBOLS = tuple(ATTN_DECLS)
HALF_F16, HALF_BF16 = (int(re.search(rf"^#define\s+SUBGACC_HALF_{n}\s+(\d+)", _HALF_TEXT, re.M).group(1)) for n in ("F16", "BF16"))


_lib = None
# the reference prints "#SubGAcc: ..." statistics to stdout (subg_acc.c:878,1009); SUBGACC_QUIET=1 silences ours
VERBOSE = os.environ.get("SUBGACC_QUIET", "0") != "1"


def build(force=False):
    """hipcc-compile csrc/*.hip for gfx950 into surel_plus_amd/libsubgacc_hip.so (in-tree)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))]
    srcs += [HEADER, HALF_HEADER, SMALL_HEADER, PACKED_HEADER, WIDE_HEADER, HALF64_HEADER, PACKED_HALF_HEADER, HALF_IDS_HEADER, STAR_HEADER,
             MEAN_HEADER, ATTN_HEADER]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-s", "-C", CSRC, "-j4", "all"])
    return LIB_PATH


def lib():
    """Load the library (after torch, so that both bind the same libamdhip64 runtime instance)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  -- torch's bundled libamdhip64.so.7 must be the one already in the process
    if not os.path.exists(LIB_PATH):
        raise SubgAccError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           f"(or `make -C surel_plus_amd/csrc`). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in _TYPES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.subgacc_abi_version() != ABI_VERSION:
        raise SubgAccError(f"libsubgacc_hip.so ABI version mismatch: the library is {L.subgacc_abi_version()}, "
                           f"include/subgacc.h is {ABI_VERSION}")
    _lib = L
    return L


def check(rc):
    """Turn a negative subgacc_status into the exception the reference raises for that condition."""
    if rc >= 0:
        return rc
    msg = lib().subgacc_last_error().decode("utf-8", "replace")
    if rc == ERR_BADARG:
        raise TypeError(f"Input parsing error. ({msg})")
    if rc == ERR_WORKSPACE:
        raise MemoryError(msg)
    if rc == ERR_KEYWIDTH:
        raise AssertionError(msg)
    if rc == ERR_LDS:
        raise ValueError(msg)
    raise SubgAccError(f"subgacc status {rc}: {msg}")


def require_device():
    """Fail loudly unless a gfx950 GPU is usable from this process."""
    import torch
    if not torch.cuda.is_available():
        raise SubgAccError("no HIP device visible: the SubGAcc hot path only runs on MI355X (gfx950); "
                           "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def join_desc(form=JOIN_ROWS, payload_kind=JOIN_SFPTR, **fields):
    """A subgacc_join_desc: `fields` are its members by name -- torch tensors for the pointers (None = NULL), ints for the rest;
    what a form does not read stays zero."""
    d = JoinDesc()
    d.struct_bytes, d.form, d.payload_kind = C.sizeof(JoinDesc), int(form), int(payload_kind)
    for name, val in fields.items():
        if val is None:
            continue
        setattr(d, name, val.data_ptr() if hasattr(val, "data_ptr") else int(val))
    return d


def join_fill(form=JOIN_ROWS, payload_kind=JOIN_SFPTR, stream=None, **fields):
    """One join through subgacc_sjoin_fill_v2 on `stream` (a stream_ptr(), if the caller has it at hand), else on the current stream
    (fields: see join_desc)."""
    return check(lib().subgacc_sjoin_fill_v2(C.byref(join_desc(form, payload_kind, **fields)),
                                             stream if stream is not None else stream_ptr()))


def publish(src, host):
    """queue `host[:] = src` (a few int64 words: sizes, status) on the current stream WITHOUT a copy engine: see subgacc_publish_words.
    (`_lib._READBACK_COPY = True` takes torch's asynchronous copy instead: the A/B switch)"""
    if _READBACK_COPY or src.numel() > 4096 or not src.is_contiguous() or src.dtype != host.dtype or src.element_size() != 8:
        host.copy_(src, non_blocking=True)
    else:
        check(lib().subgacc_publish_words(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(host.data_ptr()), stream_ptr()))


_KEPT = []
_KEPT_LOCK = threading.Lock()


def keep_until(event, obj):
    """`obj` (the pinned buffer a publish() kernel writes) stays alive until `event` -- recorded behind that kernel -- has passed,
    even if its owner is dropped first: torch's host allocator knows nothing of a kernel that writes pinned memory and would hand
    the block to somebody else.  (Finished entries leave when the next one arrives.)
    Called from every thread that queues steps (the reference's loader runs four, train.py:88-111): look-then-pop on the shared list
    is one critical section -- without the lock a second thread could pop the entry BEHIND the finished one the first had seen,
    i.e. drop a block a kernel is still going to write.  Entries are queued by different streams, so a finished one may stand behind
    an unfinished one: every finished entry leaves, wherever it stands."""
    with _KEPT_LOCK:
        _KEPT[:] = [(ev, o) for ev, o in _KEPT if not ev.query()]
        _KEPT.append((event, obj))


_READBACK_COPY = False      # True: torch's asynchronous copy instead (how the A/B of profiles/r25_readback_ab.log was run)


def ptr(t):
    """device pointer of a torch tensor (None -> NULL)"""
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor expected"
    return C.c_void_p(t.data_ptr())

"""CPU: the ctypes binding is derived from include/subgacc.h -- the parser on header text built to trip it, the derived binding
against the real header and the built library (counted with this file's own regex, and spot-checked by hand so that the test does
not mirror the parser), the constants that stay literal in Python against the header's enumerators, and two calls."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from surel_plus_amd import _lib

SYNTHETIC = """
#ifndef X_H
#define X_H
/* a comment with a prototype: int subgacc_in_block_comment(int32_t a); and parentheses ( ; ) */
// int subgacc_in_line_comment(int64_t n);
#define SUBGACC_MACRO(x) ((x) + 1)
typedef struct subgacc_join_desc { int32_t struct_bytes, form; const void *payload; } subgacc_join_desc;
int subgacc_three_lines(const void *indptr,
                        uint64_t *recs, /* ends here ); really */
                        double *out);
int subgacc_none(void);
const char *subgacc_text(void);
size_t
subgacc_bytes(int64_t n);   // size_t subgacc_after(int64_t n);
int subgacc_desc(const subgacc_join_desc *d, const subgacc_walk_cfg*cfg, float  eps, void *stream);
#endif
"""


def test_parser_on_synthetic_header_text():
    d = _lib.parse_header(SYNTHETIC)
    assert list(d) == ["subgacc_three_lines", "subgacc_none", "subgacc_text", "subgacc_bytes", "subgacc_desc"]
    assert d["subgacc_three_lines"] == ("int", [("indptr", "const void *"), ("recs", "uint64_t *"), ("out", "double *")])
    assert d["subgacc_none"] == ("int", [])
    assert d["subgacc_text"] == ("const char *", [])
    assert d["subgacc_bytes"] == ("size_t", [("n", "int64_t")])
    assert d["subgacc_desc"] == ("int", [("d", "const subgacc_join_desc *"), ("cfg", "const subgacc_walk_cfg *"), ("eps", "float"),
                                         ("stream", "void *")])
    t = _lib.bind_types(d)
    vp = C.c_void_p
    assert t["subgacc_three_lines"] == (C.c_int, [vp, vp, vp])
    assert t["subgacc_none"] == (C.c_int, []) and t["subgacc_text"] == (C.c_char_p, [])
    assert t["subgacc_bytes"] == (C.c_size_t, [C.c_int64])
    assert t["subgacc_desc"] == (C.c_int, [C.POINTER(_lib.JoinDesc), C.POINTER(_lib.WalkCfg), C.c_float, vp])


@pytest.mark.parametrize("decl", ["int subgacc_bad(int32_t n, long double x);", "long subgacc_bad(int32_t n);",
                                  "void *subgacc_bad(void);", "int subgacc_bad(int32_t);"])
def test_a_type_outside_the_map_raises_and_names_the_function(decl):
    with pytest.raises(_lib.SubgAccError, match="subgacc_bad"):
        _lib.bind_types(_lib.parse_header("int subgacc_fine(int32_t n);\n" + decl))


def test_a_name_declared_twice_raises():
    with pytest.raises(_lib.SubgAccError, match="subgacc_twice"):
        _lib.parse_header("int subgacc_twice(void);\nint subgacc_twice(int32_t n);")


# ---- the real header, read with this file's own regexes ----
HDR = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "subgacc.h")).read(), flags=re.S))
PROTOS = re.findall(r"(\w+)\s*(\*?)\s*(subgacc_\w+)\s*\(([^)]*)\)\s*;", HDR)          # (return word, "*", name, argument text)
RESTYPE = {("int", ""): C.c_int, ("size_t", ""): C.c_size_t, ("int64_t", ""): C.c_int64, ("char", "*"): C.c_char_p}


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_every_declaration_is_bound_as_the_header_shows_it(L):
    assert [p[2] for p in PROTOS] == list(_lib.SYMBOLS)
    assert len(_lib.SYMBOLS) == 72 and _lib.ABI_VERSION == 7          # the count moves only together with the version
    assert len(set(_lib.SYMBOLS)) == len(_lib.SYMBOLS)
    for word, star, name, args in PROTOS:
        fn = getattr(L, name)                                         # AttributeError: the library does not define it
        n_params = 0 if args.strip() == "void" else args.count(",") + 1
        assert len(fn.argtypes) == n_params, name
        assert fn.restype is RESTYPE[(word, star)], name


def test_spot_checks_by_hand(L):
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    a = L.subgacc_lstm_aggr_hinge_backward.argtypes
    assert len(a) == 27 and tuple(a[3:7]) == (i64, i32, i64, i32) and a[16] is i64
    assert all(t is vp for i, t in enumerate(a) if i not in (3, 4, 5, 6, 16))
    assert L.subgacc_ppr_topk.argtypes.count(C.c_float) == 2 and L.subgacc_ppr_topk.argtypes[6:8] == [C.c_float, C.c_float]
    assert L.subgacc_keyrows_cand_capacity.restype is i64 and L.subgacc_keyrows_cand_capacity.argtypes == [i64]
    assert L.subgacc_sjoin_fill_v2.argtypes == [C.POINTER(_lib.JoinDesc), vp]
    assert L.subgacc_walk_sets.argtypes[0] is C.POINTER(_lib.WalkCfg)
    assert L.subgacc_last_error.restype is C.c_char_p and L.subgacc_last_error.argtypes == []
    assert L.subgacc_batch_sampler.argtypes[9] is C.c_uint32 and L.subgacc_rng_replay.argtypes[7] is C.c_uint64
    assert L.subgacc_hop_records_format.argtypes == [i64, i64, vp, vp]


def test_constants_match_the_header(L):
    from surel_plus_amd import spjoin
    enums = re.findall(r"\b(SUBGACC_[A-Z0-9_]+)\s*=\s*(-?\d+)", HDR)
    assert len(enums) == 21 and len({n for n, _ in enums}) == 21
    for name, value in enums:
        assert getattr(_lib, name[len("SUBGACC_"):]) == int(value), name
    expr = re.search(r"#define\s+SUBGACC_NO_ROOT\s+(\([-\d\s]+\))", HDR).group(1)
    assert spjoin.NO_ROOT == eval(expr) == -2 ** 31
    version = int(re.search(r"#define\s+SUBGACC_ABI_VERSION\s+(\d+)", HDR).group(1))
    assert L.subgacc_abi_version() == version == _lib.ABI_VERSION


def test_hop_records_format_through_void_pointers(L):
    """Host-only code (csrc/walk_prep.hip: two loops over the bit widths, no device call): byref(c_int32) outputs through the derived
    c_void_p parameters give what a handle typed POINTER(c_int32), as the binding used to be, gives -- and what the loops say."""
    typed = C.CDLL(_lib.LIB_PATH).subgacc_hop_records_format
    typed.restype, typed.argtypes = C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    for (nodes, nnz), want in {(10, 40): (54, 4, 6), (1 << 20, 1 << 30): (13, 20, 31), (1 << 31, 1 << 33): (_lib.ERR_BADARG, 31, 34)}.items():
        got = []
        for fn in (L.subgacc_hop_records_format, typed):
            ib, bb = C.c_int32(-1), C.c_int32(-1)
            got.append((fn(nodes, nnz, C.byref(ib), C.byref(bb)), ib.value, bb.value))
        assert got[0] == got[1] == want, (nodes, nnz, got)
    assert L.subgacc_hop_records_format(10, 40, None, None) == _lib.ERR_BADARG


def test_an_argument_too_few_is_a_type_error(L):
    with pytest.raises(TypeError):
        L.subgacc_key_shift(200)
    with pytest.raises(TypeError):
        L.subgacc_sjoin_fill_v2(C.byref(_lib.JoinDesc()))


def test_a_missing_header_is_an_error_that_names_the_path(tmp_path):
    """the module reads the header when it is imported: a copy of _lib.py in a tree without include/subgacc.h refuses to import"""
    import importlib.util
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    (pkg / "_lib.py").write_text(open(os.path.join(ROOT, "surel_plus_amd", "_lib.py")).read())
    spec = importlib.util.spec_from_file_location("_lib_without_header", str(pkg / "_lib.py"))
    with pytest.raises(RuntimeError, match=re.escape(os.path.join(str(tmp_path), "include", "subgacc.h"))) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == "SubgAccError"

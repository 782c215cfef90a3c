"""The locality order without a GPU: the NumPy restatement of the label propagation (tests/locality_ref.py) restores the locality
of a graph whose ids were scattered, and the C ABI's new entry points are declared, exported and refuse bad arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from locality_ref import locality_labels, locality_score, mix32, order_and_rank


def test_mix32_matches_the_header():
    # the constants stated in include/subgacc.h
    txt = open(os.path.join(ROOT, "include", "subgacc.h")).read()
    assert "0x7feb352d" in txt and "0x846ca68b" in txt
    x = 12345
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF; x ^= x >> 16
    assert int(mix32(12345)) == x


def test_label_propagation_restores_scattered_communities():
    from surel_plus_amd.graphs import community_graph, relabeled
    N = 131072
    g = community_graph(N, 20.7, device="cpu")
    base = locality_score(g.indptr.numpy(), g.indices.numpy(), np.arange(N))
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(0))
    h = relabeled(g, perm)
    ip, ix = h.indptr.numpy(), h.indices.numpy()
    scattered = locality_score(ip, ix, np.arange(N))
    _, rank = order_and_rank(locality_labels(ip, ix, rounds=8, cap=64))
    restored = locality_score(ip, ix, rank)
    assert scattered < 0.1 * base
    assert restored >= 0.85 * base, (base, scattered, restored)


def test_relabeled_keeps_the_graph():
    from surel_plus_amd.graphs import community_graph, degree_ordered, relabeled
    g = community_graph(3000, 8.0, device="cpu")
    perm = torch.randperm(3000, generator=torch.Generator().manual_seed(1))
    h = relabeled(g, perm)
    ip, ix, hp, hx = g.indptr.numpy(), g.indices.numpy(), h.indptr.numpy(), h.indices.numpy()
    rank = np.empty(3000, dtype=np.int64)
    rank[perm.numpy()] = np.arange(3000)
    for i in (0, 17, 2999):
        old = int(perm[i])
        assert np.array_equal(hx[hp[i]:hp[i + 1]], rank[ix[ip[old]:ip[old + 1]]])
    d, dperm = degree_ordered(g)
    assert np.array_equal(d.indices.numpy(), relabeled(g, dperm).indices.numpy())
    with pytest.raises(ValueError):
        relabeled(g, perm[:-1])


def test_new_symbols_are_declared_and_exported():
    from surel_plus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "subgacc.h")).read()
    for name in ("subgacc_locality_round", "subgacc_worklist_by_rank"):
        assert re.search(r"\b%s\(" % name, txt) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    import surel_plus_amd as sp
    assert sp.locality_order is sp.sampler.locality_order and sp.LocalityOrder is sp.sampler.LocalityOrder


def test_new_entry_points_refuse_bad_arguments():
    from surel_plus_amd import _lib
    L = _lib.lib()
    buf = (C.c_int32 * 64)()
    buf2 = (C.c_int32 * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    n64 = (C.c_int64 * 1)()
    pn = C.cast(n64, C.c_void_p)
    # locality_round(indptr, indptr64, indices, num_nodes, labels_in, labels_out, round, cap, stream)
    assert L.subgacc_locality_round(None, 0, p, 4, p, q, 0, 64, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, None, 4, p, q, 0, 64, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, None, q, 0, 64, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, p, None, 0, 64, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, p, p, 0, 64, None) == _lib.ERR_BADARG         # in place
    assert L.subgacc_locality_round(p, 0, p, -1, p, q, 0, 64, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, p, q, -1, 64, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, p, q, 0, 0, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, p, q, 0, -3, None) == _lib.ERR_BADARG
    assert L.subgacc_locality_round(p, 0, p, 4, p, q, 0, 65, None) == _lib.ERR_BADARG
    with pytest.raises(TypeError, match="Input parsing error"):
        _lib.check(L.subgacc_locality_round(p, 0, p, 4, p, q, 0, 0, None))
    # worklist_by_rank(roots, n, rank, num_nodes, worklist, n_work, workspace, bytes, stream)
    ws = L.subgacc_worklist_workspace_bytes(4)
    assert L.subgacc_worklist_by_rank(p, -1, p, 4, q, pn, p, ws, None) == _lib.ERR_BADARG
    assert L.subgacc_worklist_by_rank(p, 4, p, -1, q, pn, p, ws, None) == _lib.ERR_BADARG
    assert L.subgacc_worklist_by_rank(p, 4, None, 4, q, pn, p, ws, None) == _lib.ERR_BADARG
    assert L.subgacc_worklist_by_rank(None, 4, p, 4, q, pn, p, ws, None) == _lib.ERR_BADARG
    assert L.subgacc_worklist_by_rank(p, 4, p, 4, None, pn, p, ws, None) == _lib.ERR_BADARG
    assert L.subgacc_worklist_by_rank(p, 4, p, 4, q, None, p, ws, None) == _lib.ERR_BADARG
    assert b"worklist_by_rank" in L.subgacc_last_error()

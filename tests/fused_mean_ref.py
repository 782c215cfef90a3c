"""NumPy float32 restatement of the chain subgacc_sjoin_key_mean documents (include/subgacc_mean.h): per (segment j, feature h)
    acc = 0;  for x ascending over the columns with C[j, x] != 0:  acc = acc + float32(C[j, x]) * E[x, h];  out = acc / max(size_j, 1)
-- a float32 multiply, then a float32 add, then one float32 division.  A helper of tests/test_fused_mean_cpu.py and
tests/test_gpu_fused_mean.py; a row of E whose count is zero is never looked at."""
import numpy as np


def fused_mean(C, sizes, E, descending=False):
    """C [S, T] counts (any numeric type, whole numbers), sizes [S], E float32 [T, H] -> float32 [S, H].  descending: the same chain
    over the columns in descending order (what the kernel does NOT do: the tests show the two differ)"""
    C, E = np.asarray(C), np.asarray(E)
    assert E.dtype == np.float32 and E.ndim == 2 and C.ndim == 2 and C.shape[1] <= E.shape[0]
    out = np.zeros((C.shape[0], E.shape[1]), dtype=np.float32)
    for j in range(C.shape[0]):
        cols = np.flatnonzero(C[j])
        acc = np.zeros(E.shape[1], dtype=np.float32)
        for x in (cols[::-1] if descending else cols):
            prod = np.float32(C[j, x]) * E[x]              # float32 * float32 array: a float32 multiply, rounded
            assert prod.dtype == np.float32
            acc = acc + prod                                # a float32 add, rounded
        out[j] = acc / np.float32(max(int(sizes[j]), 1))
    assert out.dtype == np.float32
    return out


def bound(C, sizes, E):
    """the derived bound of |fused_mean - exact| per element: gamma_m * (C @ |E|) / size, gamma_m = m u / (1 - m u), u = 2^-24,
    m = the segment's non-zero columns + 2 (a sum of n terms: n - 1 adds, the product's rounding, the division's), float64"""
    C, E = np.asarray(C, dtype=np.float64), np.abs(np.asarray(E, dtype=np.float64))
    m = (C != 0).sum(1) + 2.0
    u = 2.0 ** -24
    gamma = m * u / (1.0 - m * u)
    size = np.maximum(np.asarray(sizes, dtype=np.float64), 1.0)
    return gamma[:, None] * (C @ E[: C.shape[1]]) / size[:, None]

"""NumPy float32 restatement of the chain subgacc_sjoin_key_attn documents (include/subgacc_attn.h): per (segment j, feature h)
    acc = 0;  for r ascending over the columns whose W[j, r] is not the bit pattern of +0.0f:  acc = acc + W[j, r] * E[r, h];  out = acc
-- a float32 multiply, then a float32 add, no division.  A helper of tests/test_fused_attn_cpu.py and tests/test_gpu_fused_attn.py;
a row of E whose weight is zero is never looked at."""
import numpy as np


def fused_attn(W, E, descending=False):
    """W float32 [S, T] (the rows subgacc_sjoin_key_counts_attn writes), E float32 [T', H] with T' >= T -> float32 [S, H].
    descending: the same chain over the columns in descending order (what the kernel does NOT do: the tests show the two differ)"""
    W, E = np.ascontiguousarray(W, dtype=np.float32), np.asarray(E)
    assert E.dtype == np.float32 and E.ndim == 2 and W.ndim == 2 and W.shape[1] <= E.shape[0]
    out = np.zeros((W.shape[0], E.shape[1]), dtype=np.float32)
    bits = W.view(np.uint32)
    for j in range(W.shape[0]):
        cols = np.flatnonzero(bits[j])                      # not the bits of +0.0f
        acc = np.zeros(E.shape[1], dtype=np.float32)
        for r in (cols[::-1] if descending else cols):
            prod = W[j, r] * E[r]                           # float32 * float32 array: a float32 multiply, rounded
            assert prod.dtype == np.float32
            acc = acc + prod                                # a float32 add, rounded
        out[j] = acc
    assert out.dtype == np.float32
    return out


def bound(W, E):
    """the derived bound of |fused_attn(W, E) - float64(W) @ float64(E)| per element, W taken as given: gamma_m * (W @ |E|),
    gamma_m = m u / (1 - m u), u = 2^-24, m = the segment's non-zero columns + 1 (a sum of n products: n - 1 adds and each
    product's rounding make n roundings on any term's way to the result; one to spare), float64"""
    W, E = np.abs(np.asarray(W, dtype=np.float64)), np.abs(np.asarray(E, dtype=np.float64))
    m = (W != 0).sum(1) + 1.0
    u = 2.0 ** -24
    gamma = m * u / (1.0 - m * u)
    return gamma[:, None] * (W @ E[: W.shape[1]])

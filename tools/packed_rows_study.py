"""How many members of a step's rows escape the packed row's static code (include/subgacc_packed.h), and what a packed
row weighs against today's 8 bytes per member.  CPU only: the oracle's sampler (Philox) over preset-like graphs at a reduced scale
-- with the id width of the FULL graph, which is what sets the code's field width -- and over the golden graphs.

    python tools/packed_rows_study.py [--scale 0.05] [--roots 4096] >> profiles/packed_rows_bench.log
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import oracle                                       # noqa: E402
from walk_rows_edges import key_shift, lp_keys      # noqa: E402

FULL_N = {"cit2": 2_927_963, "cit2loc": 2_927_963, "ppa": 576_289, "collab": 235_868}
HOPS = {"cit2": 3, "cit2loc": 3, "ppa": 3, "collab": 2}


def code_bits(num_nodes, m):
    id_bits = max(int(num_nodes - 1).bit_length(), 1)
    cb = 32 - id_bits
    return id_bits, cb, (cb - 1) // m


def escapes(keys, M, m, cb, fb):
    """bool per member: True where the key does not fit the static code"""
    s = key_shift(M)
    keys = np.asarray(keys).astype(np.uint64)
    big = np.zeros(len(keys), bool)
    code = (keys >> np.uint64(m * s)) & np.uint64(1)
    for j in range(1, m + 1):
        c = (keys >> np.uint64((m - j) * s)) & np.uint64((1 << s) - 1)
        big |= c >= (1 << fb)
        code = (code << np.uint64(fb)) | (c & np.uint64((1 << fb) - 1))
    return big | (code == (1 << cb) - 1)


def lines(nbytes):
    return (nbytes + 127) // 128


def study(name, indptr, indices, roots, M, m, num_nodes_full):
    id_bits, cb, fb = code_bits(num_nodes_full, m)
    nsize, remap, enc = oracle.gset_sampler(indptr, indices, roots, num_walks=M, num_steps=m, rng="philox", seed=1)
    keys = lp_keys(enc, M, m)[remap[1]]
    if fb < 1:
        print(f"{name:28s} id_bits {id_bits} cb {cb} fb {fb}: not eligible")
        return
    esc = escapes(keys, M, m, cb, fb)
    rowid = np.repeat(np.arange(len(nsize)), nsize)
    ne = np.bincount(rowid, weights=esc, minlength=len(nsize)).astype(np.int64)
    ns = nsize.astype(np.int64)
    live = ns > 0
    today = 8 * ns
    packed = 4 * ns + 4 * ne
    today_l = 2 * lines(4 * ns)
    packed_l = lines(4 * ns) + lines(4 * ne)
    print(f"{name:28s} id_bits {id_bits:2d} cb {cb:2d} fb {fb} {'eligible' if fb >= 3 else 'fb < 3  '} rows {live.sum():5d} "
          f"ns mean {ns[live].mean():6.1f}  ne mean {ne[live].mean():6.2f} p50 {np.median(ne[live]):4.0f} p99 {np.percentile(ne[live], 99):4.0f} "
          f"max {ne.max():4d}  share {esc.mean():.4f}  bytes {packed.sum() / max(today.sum(), 1):.3f}  lines {packed_l.sum() / max(today_l.sum(), 1):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--roots", type=int, default=4096)
    args = ap.parse_args()
    from surel_plus_amd.graphs import preset_graph, query_pairs
    print(f"# packed rows, CPU study: escape share and bytes of a packed row (4 ns + 4 ne) against 8 ns; M = 200, oracle sampler (philox), "
          f"graphs at scale {args.scale} with the full graph's id width, {args.roots} roots drawn as bench.py draws its pairs")
    for name in ("cit2", "cit2loc", "ppa", "collab"):
        csr = preset_graph(name, device="cpu", scale=args.scale)
        edge = query_pairs(csr, args.roots // 2, device="cpu")
        roots = edge.reshape(-1).numpy().astype(np.int32)
        study(f"{name} x{args.scale}", csr.indptr.numpy(), csr.indices.numpy(), roots, 200, HOPS[name], FULL_N[name])
    print("# goldens (their own id width; M, hops as recorded)")
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
    for path in sorted(glob.glob(os.path.join(gdir, "gset_*_s1.npz"))):
        g = np.load(path)
        if not {"indptr", "indices", "query"} <= set(g.files):
            continue
        M, m = int(g["M"]), int(g["m"])
        if m < 2 or m > 4 or m * key_shift(M) + 1 > 31:
            continue
        study(os.path.basename(path)[:-4], g["indptr"], g["indices"], g["query"].astype(np.int32), M, m, len(g["indptr"]) - 1)


if __name__ == "__main__":
    main()

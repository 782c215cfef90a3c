#!/usr/bin/env python3
"""Dev-only: the star join (gather_star, SUBGACC_JOIN_OPT_STAR) against gather over the same expanded pairs -- the MRR evaluation
shape of the reference (train.py:246-280: one source against K = 1,000 targets, utils.py:93-95).

    python tools/star_bench.py [--n=10] [--stores=table,keyed,ppr] [--P=64,1024] [--K=1000]

Stores: the cit2-like LP resident store as the reference keeps it (SFptr + the Z_SF table, subg_matrix over all nodes, M = 200,
3 hops), the same store keyed (SpG.keyed), and the cit2-PPR headed store (topk_ppr_matrix top-100, SpG.aligned()).  Both forms
run lazily into one caller-owned buffer ("star" is gather_star(kernel="star"), the library's star form).  For each it prints the
join kernel's time (HIP events around the library call that fills, bench.KernelTimer's "sjoin_fill"), the whole call's (events around gather / gather_star), pairs/s, and the fraction of the 8 TB/s
peak in algorithmic bytes: every output row written once plus the member it comes from (id + payload) read once, the same count
for both forms."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")


def main():
    import numpy as np
    import torch
    import bench
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import preset_graph
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    n = int(opts.get("n", "10"))
    stores = opts.get("stores", "table,keyed,ppr").split(",")
    Ps = [int(v) for v in opts.get("P", "64,1024").split(",")]
    K = int(opts.get("K", "1000"))
    dev = torch.device("cuda", 0)
    csr = preset_graph("cit2", device=dev)
    N = csr.num_nodes
    todo = []
    if "table" in stores or "keyed" in stores:
        M, k = 200, 4
        z, enc = sp.subg_matrix(csr, np.arange(N), num_walks=M, num_steps=k, rng="philox", seed=3)
        if "table" in stores:
            todo.append(("cit2-table", z, torch.from_numpy(enc.astype(np.float32) / np.float32(M)).to(dev), k, 4))
        if "keyed" in stores:
            zk = z.keyed(enc, M)
            todo.append(("cit2-keyed", zk, zk.slot_table(), k, 4))
    if "ppr" in stores:
        from surel_plus_amd.ppr import topk_ppr_matrix
        zp = topk_ppr_matrix(csr, 0.1, 1e-4, torch.arange(N, dtype=torch.int32, device=dev), 100, normalization="sym", encode=True)
        todo.append(("cit2ppr-headed", zp.aligned(), None, 1, 8))
    torch.cuda.synchronize()
    print(f"star_bench: cit2-like graph N={N:,}, K={K}, n={n} timed calls per form (median of them)", flush=True)
    for name, x, encode, k, pay in todo:
        for P in Ps:
            rng = np.random.default_rng(P)
            src = torch.from_numpy(rng.integers(0, N, P)).to(dev)
            tgt = torch.from_numpy(rng.integers(0, N, (P, K))).to(dev)
            edge = torch.stack([src.repeat_interleave(K), tgt.reshape(-1)])
            buf = torch.empty(2 * P * K * int(x.max_len) * 2 * k, dtype=torch.float32, device=dev)
            res = {}
            for form, call in (("pairs", lambda: sp.gather(edge, x, dev, encode=encode, out=buf, lazy=True)),
                               ("star", lambda: sp.gather_star(src, tgt, x, dev, encode=encode, out=buf, lazy=True, kernel="star"))):
                timer = bench.KernelTimer()
                sampler_mod.KERNEL_TIMER = timer
                calls = []
                for it in range(n + 2):
                    timer.enabled = it >= 2
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    xz, ind = call()
                    b.record()
                    if it >= 2:
                        calls.append((a, b))
                torch.cuda.synchronize()
                sampler_mod.KERNEL_TIMER = None
                rows = int(ind[-1].item())
                kern = sorted(a.elapsed_time(b) for a, b in timer.pairs["sjoin_fill"])[n // 2]
                whole = sorted(a.elapsed_time(b) for a, b in calls)[n // 2]
                res[form] = (rows, kern, whole, xz[:rows].clone() if P <= 64 else None, ind.clone())
            (rows, kp, wp, xp, ip), (rows_s, ks, ws, xs, is_) = res["pairs"], res["star"]
            same = rows == rows_s and torch.equal(ip, is_) and (xp is None or torch.equal(xp, xs))
            abytes = rows * (2 * k * 4 + 4 + pay)
            for form, kern, whole in (("pairs", kp, wp), ("star", ks, ws)):
                print(f"{name:15s} P={P:5d} K={K} {form:5s} rows {rows:>11,d}  kernel {kern * 1e3:10.1f} us  call {whole * 1e3:10.1f} us  "
                      f"{P * K / (kern * 1e-3) / 1e6:8.1f} M pairs/s  frac {abytes / (kern * 1e-3) / 8e12:.3f}", flush=True)
            print(f"{name:15s} P={P:5d} K={K} star / pairs kernel time {ks / kp:.3f}  call {ws / wp:.3f}  identical={same}", flush=True)
            del buf, edge


if __name__ == "__main__":
    main()

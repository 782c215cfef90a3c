#!/usr/bin/env python3
"""Dev-only: the LP encoder's first model stage with attentional aggregation fused with the count form of the join (counts_attn_stage,
subgacc_sjoin_counts_attn and _backward) against attn_stage (the pair form: gather_pairs, then torch on the distinct pairs) and the
reference form of model.py:59-62,78-81 -- gather -> pe_embedding = Sequential(Linear(k, H), ReLU, Linear(H, H)) -> sum(-2) ->
AttentionalAggregation(Linear(H, 1), Linear(H, H)) in torch -- on the all-N resident LP stores of bench.py: cit2 (M = 200, --num_steps 4)
and ppa (M = 200, --num_steps 4), H = 96, at B = 1,024 (main.py:32) and B = 65,536.  The reference form materialises [R, 2, H]
activations and runs at B <= 4,096 only.

    python tools/counts_attn_bench.py [--n=5] [--stores=cit2,ppa]   device-event timings (median of n calls), largest differences
                                                                      against the reference form, peak memory of each form
    python tools/counts_attn_bench.py --profile=B [--store=cit2]    only the fused calls of one shape, for rocprofv3 --kernel-trace
                                                                      --stats; prints the shape's algorithmic bytes
    python tools/counts_attn_bench.py --stats=CSV|DB --bytes=FWD,BWD  kernel time from rocprofv3's kernel_stats.csv or run_results.db
                                                                      and the share of the 8 TB/s HBM peak

Algorithmic bytes of one fused call: every member of both rows of a pair read once (4 B id + 4 B SFptr), the segment list (8 B per
segment), g (4 T B); forward: W [2B, T] written once, m and den (8 B per segment); backward: dW and W read at the segment's distinct
rows only (counted as 8 B per member, an upper bound), m and den read, Dg [2B, T] written once."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
H = 96
STORES = {"cit2": ("cit2", 200, 4), "ppa": ("ppa", 200, 4)}        # bench.py's WORKLOADS: preset, M, CLI --num_steps
SHAPES = (1024, 65536)
REF_MAX_B = 4096


def _timed(fn, n):
    import torch
    ts = []
    for _ in range(n + 1):          # the first call warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2]


def _store(name, dev):
    """the all-N resident store of bench.py's reference flow (main.py:172-178) and its feature table"""
    import numpy as np
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    preset, M, k = STORES[name]
    csr = preset_graph(preset, device=dev)
    z, sets = sp.sample_spg(csr, np.arange(csr.num_nodes), num_walks=M, num_steps=k - 1, seed=111413, rng="philox", fused=True)
    return csr, z, sets.feature_table()


def _nets(k, dev):
    import torch
    torch.manual_seed(0)
    return (torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev),
            torch.nn.Linear(H, 1).to(dev), torch.nn.Linear(H, H).to(dev))


def _reference(sp, edge, z, table, embed, gate, val):
    """the reference form (tests/gpu_helpers.py, _reference_style_attn): PyG's softmax exp(g - max) / (sum + 1e-16) written out"""
    import torch
    xz, ind = sp.gather(edge, z, edge.device, ptr=True, encode=table)
    h = embed(xz).sum(dim=-2)
    S = ind.numel() - 1
    seg = torch.repeat_interleave(torch.arange(S, device=h.device), ind[1:] - ind[:-1], output_size=h.shape[0])
    g = gate(h).reshape(-1)
    gmax = torch.full((S,), float("-inf"), device=g.device).scatter_reduce(0, seg, g.detach(), "amax")
    w = torch.exp(g - gmax[seg])
    den = torch.zeros(S, device=g.device).index_add_(0, seg, w)
    alpha = w / (den[seg] + 1e-16)
    out = torch.zeros((S, H), device=g.device).index_add_(0, seg, alpha[:, None] * val(h))
    return out.view(2, -1, H)


def _work(z, edge, T):
    """(forward bytes, backward bytes) of one fused call"""
    own = edge.reshape(-1)
    S = own.numel()
    members = int((z.indptr[own + 1] - z.indptr[own]).sum())
    rows = 8 * members + 8 * S + 4 * T
    dense = 4 * S * T
    return rows + dense + 8 * S, rows + 8 * members + 8 * S + dense


def _kernel_rows(path):
    """(name, calls, mean ns) of sjoin_counts_attn_kernel from rocprofv3's kernel_stats.csv or its run_results.db"""
    if path.endswith(".db"):
        import sqlite3
        q = "select name, count(*), avg(end - start) from kernels where name like '%sjoin_counts_attn_kernel%' group by name order by name"
        return list(sqlite3.connect(path).execute(q))
    import csv
    return [(r.get("Name") or r.get("KernelName") or "", int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]


def _stats(path, b):
    for name, calls, avg_ns in _kernel_rows(path):
        if "sjoin_counts_attn_kernel" not in name:
            continue
        bwd = "<true>" in name or "ILb1E" in name        # sjoin_counts_attn_kernel<BWD>
        nb = b[1] if bwd else b[0]
        print(f"  sjoin_counts_attn_kernel {'backward' if bwd else 'forward'}: {int(calls)} calls, mean {avg_ns / 1e3:.1f} us; "
              f"algorithmic {nb / 1e6:.1f} MB = {nb / avg_ns / 8000:.1%} of the 8 TB/s HBM peak")


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "stats" in opts:
        return _stats(opts["stats"], [int(x) for x in opts["bytes"].split(",")])
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import query_pairs
    dev = torch.device("cuda", 0)
    n = int(opts.get("n", "5"))
    if "profile" in opts:
        B = int(opts["profile"])
        csr, z, table = _store(opts.get("store", "cit2"), dev)
        nets = _nets(table.shape[1], dev)
        edge = query_pairs(csr, B, seed=9700, device=dev)
        fb, bb = _work(z, edge, table.shape[0])
        for _ in range(n):
            with torch.no_grad():
                sp.counts_attn_stage(edge, z, table, *nets)
            sp.counts_attn_stage(edge, z, table, *nets).sum().backward()
        torch.cuda.synchronize()
        print(f"profile {B} {opts.get('store', 'cit2')}: bytes={fb},{bb}")
        return
    for name in opts.get("stores", "cit2,ppa").split(","):
        csr, z, table = _store(name, dev)
        T, k = table.shape
        nets = _nets(k, dev)
        params = [p for m in nets for p in m.parameters()]
        torch.cuda.synchronize()
        print(f"counts_attn_bench: {name} all-N store N={z.n_rows:,}, max_len {z.max_len}, T = {T:,} LP rows (k = {k}), H = H'' = {H}, "
              f"median of {n} calls, device events (ms); peak = the call's peak allocation above what was allocated before it (MB)")
        print(f"{'B':>7} {'form':>18} | {'fwd':>8} {'f+b':>8} | {'peak fwd':>9} {'peak f+b':>9} | max |form - ref| (of max |ref|)")
        for B in SHAPES:
            edge = query_pairs(csr, B, seed=9700, device=dev)
            w = torch.randn(2, B, H, device=dev)
            forms = {"counts_attn_stage": lambda e: sp.counts_attn_stage(e, z, table, *nets),
                     "attn_stage": lambda e: sp.attn_stage(e, z, table, *nets)}
            if B <= REF_MAX_B:
                forms["reference"] = lambda e: _reference(sp, e, z, table, *nets)
            want = None
            if B <= REF_MAX_B:
                with torch.no_grad():
                    want = _reference(sp, edge, z, table, *nets)
            for label, f in forms.items():
                def zero():
                    for p in params:
                        p.grad = None

                def fwd():
                    with torch.no_grad():
                        f(edge)

                def fb():
                    zero()
                    (f(edge) * w).sum().backward()

                def peak(fn):
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    fn()
                    torch.cuda.synchronize()
                    return (torch.cuda.max_memory_allocated() - base) / 1e6
                try:
                    tf, tfb = _timed(fwd, n), _timed(fb, n)
                    pf, pfb = peak(fwd), peak(fb)
                except Exception as ex:          # (a store the fused kernel does not hold: said, not hidden)
                    print(f"{B:>7} {label:>18} | {type(ex).__name__}: {str(ex)[:150]}", flush=True)
                    torch.cuda.empty_cache()
                    continue
                diff = ""
                if want is not None:
                    with torch.no_grad():
                        d = float((f(edge) - want).abs().max())
                    diff = f"{d:.3g} ({d / float(want.abs().max()):.2g})"
                print(f"{B:>7} {label:>18} | {tf:8.3f} {tfb:8.3f} | {pf:9.1f} {pfb:9.1f} | {diff}", flush=True)
                torch.cuda.empty_cache()
            del want
        del z, table, csr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the fused first model stage of the float encoders with attentional aggregation (float_attn_stage, subgacc_sjoin_relu_attn
and _backward) against the reference form of model.py:59-62,78-81 -- gather -> pe_embedding = Sequential(Linear(1, H), ReLU,
Linear(H, H)) -> sum(-2) -> AttentionalAggregation(Linear(H, 1), Linear(H, H)) in torch -- on the cit2-PPR store, packed and headed,
H = 96, at B = 1,024, B = 65,536 and the MRR shape P = 64 x K = 1,000 (the shapes and store of tools/float_stage_bench.py).

    python tools/float_attn_bench.py [--n=5]                  device-event timings (median of n calls) and the largest difference
    python tools/float_attn_bench.py --profile=B --layout=L   only the fused calls of one shape, for rocprofv3 --kernel-trace --stats;
                                                              prints the shape's algorithmic bytes and VALU instructions
    python tools/float_attn_bench.py --stats=CSV|DB --bytes=FWD,BWD --valu=FWD,BWD   kernel time from rocprofv3's kernel_stats.csv
                                                              or run_results.db, the share of the 8 TB/s HBM peak and of the
                                                              78.6 T/s fp32 VALU issue rate

Algorithmic bytes: every member of both rows of a pair read once (4 B id + 8 B score), the segment list (8 B per segment); forward: A
[2B, H] written, m and den (8 B per segment); backward: G and A read, m and den read, Dw, Db, Du written ([2B, H] each).
VALU work, in wave64 lane-instructions, of the documented sequences per (member, channel): forward 13 (logit: 2 fma, 2 max, add, fma;
channel sum: 2 fma, 2 max, add, den add, fma), backward 19 (logit and G . r: 7; channel sum: 2 fma, 2 max, add, mul, fma x 4, 2
selects and an add for each of the two masks)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from float_stage_bench import H, N_CIT2, ROOT, SHAPES, _edge, _timed  # noqa: E402

sys.path.insert(0, ROOT)
VALU_FWD, VALU_BWD = 13, 19


def _nets(dev):
    import torch
    torch.manual_seed(0)
    return (torch.nn.Sequential(torch.nn.Linear(1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev),
            torch.nn.Linear(H, 1).to(dev), torch.nn.Linear(H, H).to(dev))


def _reference(sp, edge, x, embed, gate, val):
    """the reference form (tests/gpu_helpers.py, _reference_style_attn): PyG's softmax exp(g - max) / (sum + 1e-16) written out"""
    import torch
    xz, ind = sp.gather(edge, x, edge.device, ptr=True)
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


def _work(z, edge):
    """(forward bytes, backward bytes, forward VALU, backward VALU) of one fused call"""
    own = edge.reshape(-1)
    S = own.numel()
    members = int((z.indptr[own + 1] - z.indptr[own]).sum())
    rows = 12 * members + 8 * S
    sh = 4 * S * H
    return rows + sh + 8 * S, rows + 2 * sh + 8 * S + 3 * sh, VALU_FWD * members * H, VALU_BWD * members * H


def _kernel_rows(path):
    """(name, calls, mean ns) of sjoin_f64attn_kernel from rocprofv3's kernel_stats.csv or, in its default rocpd output, run_results.db"""
    if path.endswith(".db"):
        import sqlite3
        q = "select name, count(*), avg(end - start) from kernels where name like '%sjoin_f64attn_kernel%' group by name order by name"
        return list(sqlite3.connect(path).execute(q))
    import csv
    return [(r.get("Name") or r.get("KernelName") or "", int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]


def _stats(path, b, v):
    for name, calls, avg_ns in _kernel_rows(path):
        if "sjoin_f64attn_kernel" not in name:
            continue
        bwd = "<true>" in name or "ILb1E" in name        # sjoin_f64attn_kernel<BWD>
        nb, nv = (b[1], v[1]) if bwd else (b[0], v[0])
        what = "backward" if bwd else "forward"
        print(f"  sjoin_f64attn_kernel {what}: {int(calls)} calls, mean {avg_ns / 1e3:.1f} us; algorithmic {nb / 1e6:.1f} MB "
              f"= {nb / avg_ns / 8000:.1%} of the 8 TB/s HBM peak; {nv / 1e9:.2f} G VALU lane-instructions = "
              f"{nv / 64 * 2 / avg_ns / (256 * 4 * 2.4):.1%} of the fp32 VALU issue rate")


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "stats" in opts:
        return _stats(opts["stats"], [int(x) for x in opts["bytes"].split(",")], [int(x) for x in opts["valu"].split(",")])
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import ppr_like_spg
    dev = torch.device("cuda", 0)
    n = int(opts.get("n", "5"))
    z = ppr_like_spg(N_CIT2, topk=100, seed=3, device=dev)
    stores = {"packed": z, "headed": z.aligned()}
    nets = _nets(dev)
    params = [p for m in nets for p in m.parameters()]
    torch.cuda.synchronize()
    if "profile" in opts:
        shape, x = opts["profile"], stores[opts.get("layout", "packed")]
        edge = _edge(shape, z.n_rows, dev)
        fb, bb, fv, bv = _work(z, edge)
        for _ in range(n):
            with torch.no_grad():
                sp.float_attn_stage(edge, x, *nets)
            sp.float_attn_stage(edge, x, *nets).sum().backward()
        torch.cuda.synchronize()
        print(f"profile {shape} {opts.get('layout', 'packed')}: bytes={fb},{bb} valu={fv},{bv}")
        return
    print(f"float_attn_bench: cit2-PPR store N={z.n_rows:,} (top-100), H = H' = H'' = {H}, median of {n} calls, device events (ms)")
    print(f"{'shape':>12} {'layout':>7} | {'fused fwd':>9} {'fused f+b':>9} | {'ref fwd':>9} {'ref f+b':>9} | "
          f"{'fwd x':>6} {'f+b x':>6} | max |fused - ref|")
    for shape in SHAPES:
        edge = _edge(shape, z.n_rows, dev)
        w = torch.randn(2, edge.shape[1], H, device=dev)
        label = "P64xK1000" if shape == "mrr" else f"B={int(shape):,}"
        for layout, x in stores.items():
            def zero():
                for p in params:
                    p.grad = None

            def fused_fwd():
                with torch.no_grad():
                    sp.float_attn_stage(edge, x, *nets)

            def fused_fb():
                zero()
                (sp.float_attn_stage(edge, x, *nets) * w).sum().backward()

            def ref_fwd():
                with torch.no_grad():
                    _reference(sp, edge, x, *nets)

            def ref_fb():
                zero()
                (_reference(sp, edge, x, *nets) * w).sum().backward()
            tf, tfb, rf, rfb = (_timed(f, n) for f in (fused_fwd, fused_fb, ref_fwd, ref_fb))
            with torch.no_grad():
                got, want = sp.float_attn_stage(edge, x, *nets), _reference(sp, edge, x, *nets)
                diff = float((got - want).abs().max())
                rel = diff / float(want.abs().max())
            print(f"{label:>12} {layout:>7} | {tf:9.3f} {tfb:9.3f} | {rf:9.3f} {rfb:9.3f} | {rf / tf:6.1f} {rfb / tfb:6.1f} | "
                  f"{diff:.3g} ({rel:.2g} of max |ref|)", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

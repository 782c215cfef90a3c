#!/usr/bin/env python3
"""Dev-only: the fused first model stage of the float encoders (float_mean_stage, subgacc_sjoin_relu_mean) against the reference form
of model.py:78-83 -- gather -> pe_embedding = Sequential(Linear(1, H), ReLU, Linear(H, H)) -> sum(-2) -> segment mean -- on the
cit2-PPR store (graphs.ppr_like_spg(2,927,963): top-100 rows, float64 scores), packed and headed (SpG.aligned()), H = 96
(--hidden_channels), at B = 1,024 (main.py:32), B = 65,536 and the MRR shape P = 64 sources x K = 1,000 targets (train.py:246-280, the
expanded [2, P*K] list).

    python tools/float_stage_bench.py [--n=5]                 device-event timings (median of n calls) and the largest difference
    python tools/float_stage_bench.py --profile=B --layout=L  only the fused calls of one shape (B = 1024 / 65536 / mrr), for
                                                              rocprofv3 --kernel-trace --stats; prints the shape's algorithmic bytes
    python tools/float_stage_bench.py --stats=CSV --bytes=FWD,FWDBWD   kernel time from rocprofv3's kernel_stats.csv and the fraction
                                                              of the 8 TB/s HBM peak those algorithmic bytes are

Algorithmic bytes of one fused call: every member of both rows of a pair read once (4 B id + 8 B score), the segment list (8 B per
segment), and the [2B, H] outputs written once (M; with the backward sums P and Q as well, three of them)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
N_CIT2, H = 2_927_963, 96
SHAPES = ("1024", "65536", "mrr")


def _edge(shape, N, dev):
    import numpy as np
    import torch
    rng = np.random.default_rng(7)
    if shape == "mrr":
        P, K = 64, 1000
        return torch.from_numpy(np.stack([np.repeat(rng.integers(0, N, P), K), rng.integers(0, N, P * K)])).to(dev)
    return torch.from_numpy(rng.integers(0, N, (2, int(shape)))).to(dev)


def _mlp(dev):
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)


def _reference(sp, edge, x, mlp):
    import torch
    xz, ind = sp.gather(edge, x, edge.device, ptr=True)
    h = mlp(xz).sum(dim=-2)
    n = ind[1:] - ind[:-1]
    seg = torch.repeat_interleave(torch.arange(n.numel(), device=h.device), n, output_size=h.shape[0])
    out = torch.zeros(n.numel(), h.shape[-1], device=h.device).index_add_(0, seg, h) / n.clamp(min=1)[:, None]
    return out.view(2, -1, h.shape[-1])


def _bytes(z, edge):
    """algorithmic bytes of one fused call: (forward, forward with the backward sums)"""
    own = edge.reshape(-1)
    members = int((z.indptr[own + 1] - z.indptr[own]).sum())
    rows = 12 * members + 8 * own.numel()
    out = 4 * own.numel() * H
    return rows + out, rows + 3 * out


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


def _stats(path, fwd_bytes, bwd_bytes):
    import csv
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "sjoin_f64mean_kernel" not in name:
            continue
        avg_ns = float(row["AverageNs"])
        pq = "<true>" in name or "ILb1E" in name        # sjoin_f64mean_kernel<PQ>
        b = bwd_bytes if pq else fwd_bytes
        what = "forward + backward sums (P, Q)" if pq else "forward (M only)"
        print(f"  sjoin_f64mean_kernel {what}: {int(row['Calls'])} calls, mean {avg_ns / 1e3:.1f} us; algorithmic {b / 1e6:.1f} MB "
              f"= {b / avg_ns:.0f} GB/s = {b / avg_ns / 8000:.1%} of the 8 TB/s HBM peak")


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    if "stats" in opts:
        fb, bb = (int(v) for v in opts["bytes"].split(","))
        return _stats(opts["stats"], fb, bb)
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import ppr_like_spg
    dev = torch.device("cuda", 0)
    n = int(opts.get("n", "5"))
    z = ppr_like_spg(N_CIT2, topk=100, seed=3, device=dev)
    stores = {"packed": z, "headed": z.aligned()}
    mlp = _mlp(dev)
    torch.cuda.synchronize()
    if "profile" in opts:
        shape, x = opts["profile"], stores[opts.get("layout", "packed")]
        edge = _edge(shape, z.n_rows, dev)
        fb, bb = _bytes(z, edge)
        for _ in range(n):
            with torch.no_grad():
                sp.float_mean_stage(edge, x, mlp)
            out = sp.float_mean_stage(edge, x, mlp)
            out.sum().backward()
        torch.cuda.synchronize()
        print(f"profile {shape} {opts.get('layout', 'packed')}: bytes={fb},{bb}")
        return
    print(f"float_stage_bench: cit2-PPR store N={z.n_rows:,} (top-100), H = H' = {H}, median of {n} calls, device events (ms)")
    print(f"{'shape':>12} {'layout':>7} | {'fused fwd':>9} {'fused f+b':>9} | {'ref fwd':>9} {'ref f+b':>9} | "
          f"{'fwd x':>6} {'f+b x':>6} | max |fused - ref|")
    for shape in SHAPES:
        edge = _edge(shape, z.n_rows, dev)
        w = torch.randn(2, edge.shape[1], H, device=dev)
        label = "P64xK1000" if shape == "mrr" else f"B={int(shape):,}"
        for layout, x in stores.items():
            def fused_fwd():
                with torch.no_grad():
                    sp.float_mean_stage(edge, x, mlp)

            def fused_fb():
                mlp.zero_grad()
                (sp.float_mean_stage(edge, x, mlp) * w).sum().backward()

            def ref_fwd():
                with torch.no_grad():
                    _reference(sp, edge, x, mlp)

            def ref_fb():
                mlp.zero_grad()
                (_reference(sp, edge, x, mlp) * w).sum().backward()
            tf, tfb, rf, rfb = (_timed(f, n) for f in (fused_fwd, fused_fb, ref_fwd, ref_fb))
            with torch.no_grad():
                got, want = sp.float_mean_stage(edge, x, mlp), _reference(sp, edge, x, mlp)
                diff = float((got - want).abs().max())
                rel = diff / float(want.abs().max())
            print(f"{label:>12} {layout:>7} | {tf:9.3f} {tfb:9.3f} | {rf:9.3f} {rfb:9.3f} | {rf / tf:6.1f} {rfb / tfb:6.1f} | "
                  f"{diff:.3g} ({rel:.2g} of max |ref|)", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

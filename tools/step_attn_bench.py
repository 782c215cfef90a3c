#!/usr/bin/env python3
"""Dev-only: the LP encoder's attentional first stage on the on-demand step (sample_and_attn_stage through
StepBuffers(stage="counts_attn")) on the cit2-like graph of bench.py, M = 200, 3 hops, H = H'' = 96.

    python tools/step_attn_bench.py [--B=1024,4096,65536] [--steps=20] [--warmup=5] [--parts=a,b,c,d,k] [--table_rows=2048,1024]
        a   the stage step: forward and forward + backward, peak memory above its buffers
        b   the buffered row-form step followed by the reference form on its xz (embed(xz).sum(-2), gate, segment softmax, weighted
            sum of nn(x)), where its [R,2,H] activations fit: the route the stage replaces
        c   sample_and_mean_stage on the same batch: what attention costs over mean
        d   counts_attn_stage over the resident all-nodes store (sampled once, not timed)
        k   the two new kernels alone, forward and backward, next to sjoin_key_counts_kernel on the same batch (device events around
            the launches), their bytes and the fraction of the HBM peak

Every step time is the median of three regions of --steps steps after --warmup steps, between device events.  The stage steps read
nothing back inside a region; the reference form reads its row count once per step, as tools/step_stage_bench.py says."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_stage_bench import H, HBM_PEAK, HOPS, M, OPTS, REF_MAX_B, _fmt, _KernelTimer, _peak, _regions  # noqa: E402


def _nets(dev):
    import torch
    torch.manual_seed(0)
    embed = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)
    return embed, torch.nn.Linear(H, 1).to(dev), torch.nn.Linear(H, H).to(dev)


def _runner(csr, dev, B, nets, train):
    """run(f): f on the next of four batches; train: forward + backward with fresh gradients"""
    import torch
    from surel_plus_amd.graphs import query_pairs
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    wgt = torch.randn(2, B, H, device=dev)
    it = [0]

    def run(f):
        e = es[it[0] % 4]
        it[0] += 1
        if not train:
            with torch.no_grad():
                return f(e)
        for m in nets:
            for p in m.parameters():
                p.grad = None
        (f(e) * wgt).sum().backward()
    return run


def _reference_attn(embed, gate, val, xz, seg, B, dev):
    import torch
    n = seg[1:] - seg[:-1]
    R = int(seg[-1])            # (the reference reads the row count: its xz is exactly R rows)
    x = embed(xz[:R]).sum(dim=-2)
    ids = torch.repeat_interleave(torch.arange(2 * B, device=dev), n, output_size=R)
    gl = gate(x).reshape(-1)
    gmax = torch.full((2 * B,), float("-inf"), device=dev).scatter_reduce(0, ids, gl.detach(), "amax")
    w = torch.exp(gl - gmax[ids])
    den = torch.zeros(2 * B, device=dev).index_add_(0, ids, w)
    alpha = w / (den[ids] + 1e-16)
    return torch.zeros((2 * B, H), device=dev).index_add_(0, ids, alpha[:, None] * val(x)).view(2, B, H)


def parts_abc(sp, csr, dev, B, K, W, T, parts):
    nets = _nets(dev)
    embed, gate, val = nets
    kw = dict(num_walks=M, num_steps=HOPS)
    for train in (False, True):
        what = "forward + backward" if train else "forward"
        run = _runner(csr, dev, B, nets, train)
        if "a" in parts:
            ab = sp.StepBuffers(csr, B, stage="counts_attn", table_rows=T, **kw)
            step = lambda: run(lambda e: sp.sample_and_attn_stage(csr, e, embed, gate, val, buffers=ab, **kw))      # noqa: E731
            med, ms = _regions(step, K, W)
            print(_fmt(f"(a) B={B:>6} T={T}  attn stage step, {what}", med, ms, B) + f"   peak above the buffers {_peak(step):9.1f} MB",
                  flush=True)
            try:
                ab.sets.resolve()
            except sp.SubgAccError as err:      # more distinct LP rows than columns: the times stand, the result would not
                print(f"(a) B={B:>6} T={T}  OVERFLOW: {err}", flush=True)
            print(f"(a) B={B:>6} T={T}  distinct LP rows of the last batch: {int(ab.status[2]):,}; buffers: W {ab.counts.numel() * 4 / 1e6:.0f} MB, "
                  f"rows {(ab.ids.numel() + ab.slot.numel()) * 4 / 1e6:.0f} MB", flush=True)
            del ab
        if "c" in parts:
            cb = sp.StepBuffers(csr, B, stage="counts", table_rows=T, **kw)
            step = lambda: run(lambda e: sp.sample_and_mean_stage(csr, e, embed, buffers=cb, **kw))       # noqa: E731
            med, ms = _regions(step, K, W)
            print(_fmt(f"(c) B={B:>6} T={T}  mean stage step, {what}", med, ms, B) + f"   peak above the buffers {_peak(step):9.1f} MB",
                  flush=True)
            del cb
        if "b" in parts and B <= REF_MAX_B:
            rb = sp.StepBuffers(csr, B, **kw)

            def reference(e):
                xz, seg, _ = sp.sample_and_gather(csr, e, buffers=rb, **kw)
                return _reference_attn(embed, gate, val, xz, seg, B, dev)
            step = lambda: run(reference)       # noqa: E731
            med, ms = _regions(step, K, W)
            print(_fmt(f"(b) B={B:>6}  row-form step + reference attn form on xz, {what}", med, ms, B) +
                  f"   peak above the buffers {_peak(step):9.1f} MB   (reads the row count back every step)", flush=True)
            del rb
        elif "b" in parts:
            print(f"(b) B={B:>6}  the reference form does not fit at this size ([R,2,H] activations)", flush=True)


def part_d(sp, csr, dev, shapes, K, W):
    import numpy as np
    z, sets = sp.sample_spg(csr, np.arange(csr.num_nodes), num_walks=M, num_steps=HOPS, seed=111413, rng="philox", fused=True)
    table = sets.feature_table()
    nets = _nets(dev)
    for B in shapes:
        for train in (False, True):
            what = "forward + backward" if train else "forward"
            run = _runner(csr, dev, B, nets, train)
            step = lambda: run(lambda e: sp.counts_attn_stage(e, z, table, *nets))      # noqa: E731
            try:
                med, ms = _regions(step, K, W)
            except ValueError as err:       # the store's table does not fit the kernel's LDS
                print(f"(d) B={B:>6}  counts_attn_stage over the resident store, T = {table.shape[0]:,}: refused ({str(err)[:110]} ...)", flush=True)
                break
            print(_fmt(f"(d) B={B:>6}  counts_attn_stage over the resident store, T = {table.shape[0]:,}, {what}", med, ms, B) +
                  f"   peak {_peak(step):9.1f} MB", flush=True)


def part_k(sp, sampler_mod, csr, dev, B, T, n=20):
    import torch
    from surel_plus_amd.graphs import query_pairs
    kw = dict(num_walks=M, num_steps=HOPS)
    e = query_pairs(csr, B, seed=9300, device=dev)
    ab, cb = sp.StepBuffers(csr, B, stage="counts_attn", table_rows=T, **kw), sp.StepBuffers(csr, B, stage="counts", table_rows=T, **kw)
    g = torch.randn(T, device=dev).requires_grad_()
    dW = torch.randn(2 * B, T, device=dev)
    timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
    for _ in range(n):
        Wt = sp.sample_and_attn_counts(csr, e, lambda t: g, buffers=ab, **kw)[0]
        Wt.backward(dW)
        g.grad = None
        sp.sample_and_counts(csr, e, buffers=cb, **kw)
    fwd, bwd, cnt = (timer.median_ms(k) for k in ("sjoin_key_counts_attn", "sjoin_key_counts_attn_backward", "sjoin_key_counts"))
    sampler_mod.KERNEL_TIMER = None
    try:
        ab.sets.resolve()
    except sp.SubgAccError as err:
        print(f"(k) B={B:>6} T={T}  OVERFLOW: {err}", flush=True)
    members = int(ab.sizes.to(torch.int64).sum())
    row_b, w_b = 8 * members, 4 * 2 * B * T
    line = lambda ms: f"{ms:.4f} ms: rows {row_b / 1e6:.1f} MB + [2B, T] {w_b / 1e6:.1f} MB = {(row_b + w_b) / ms / 1e9:.2f} TB/s " \
                      f"({(row_b + w_b) / ms / 1e-3 / HBM_PEAK:.1%} of the HBM peak)"       # noqa: E731
    print(f"(k) B={B:>6} T={T}  {int(ab.status[2]):,} distinct LP rows, {members:,} members", flush=True)
    print(f"(k) B={B:>6} T={T}  attn forward kernel  {line(fwd)}", flush=True)
    print(f"(k) B={B:>6} T={T}  attn backward kernel {line(bwd)}   (dW and W are read at a segment's own columns only)", flush=True)
    print(f"(k) B={B:>6} T={T}  count kernel         {line(cnt)}", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5"))
    Ts = [int(t) for t in OPTS.get("table_rows", "2048,1024").split(",")]
    shapes = [int(b) for b in OPTS.get("B", "1024,4096,65536").split(",")]
    parts = OPTS.get("parts", "a,b,c,d,k").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"step_attn_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops, H = H'' = {H}; median of three regions of {K} steps "
          f"after {W} warm-up steps, device events", flush=True)
    for B in shapes:
        for i, T in enumerate(Ts):
            parts_abc(sp, csr, dev, B, K, W, T, [p for p in parts if p in "ac" or (p == "b" and i == 0)])
            if "k" in parts:
                part_k(sp, sampler_mod, csr, dev, B, T)
            torch.cuda.empty_cache()
    if "d" in parts:
        part_d(sp, csr, dev, shapes, K, W)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the LP encoder's mean first stage on the on-demand step (sample_and_mean_stage through StepBuffers(stage="counts")) on
the cit2-like graph of bench.py, M = 200, 3 hops, H = 96.

    python tools/step_stage_bench.py [--B=1024,4096,65536] [--steps=20] [--warmup=5] [--parts=a,b,c] [--table_rows=2048]
        a   the stage step against the buffered row-form step followed by the reference form on its xz (embed(xz).sum(-2), segment
            mean): forward and forward + backward; where the reference form does not fit (B = 65,536: [R,2,H] activations) the stage
            step alone; peak memory of either
        b   the columns pass and the count kernel alone against the join kernel of the same batch (device events around the
            launches), their bytes and the fraction of the HBM peak
        c   the stage step against mean_stage over the resident all-nodes store, and what sampling that store costs

Every step time is the median of three regions of --steps steps after --warmup steps, between device events.  The stage step reads
nothing back inside a region.  The reference form does, once per step: it embeds exactly the R rows of xz, as the reference's gather
hands them over, and R is on the device (one host synchronisation per step, inside its regions and said in its log line)."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
M, HOPS, H = 200, 3, 96
HBM_PEAK = 8.0e12           # bytes / s (MI355X)
REF_MAX_B = 4096            # the reference form's [R,2,H] activations fit up to here


def _regions(step, K, W):
    import torch
    for _ in range(W):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(K):
            step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / K)
    return sorted(ms)[1], ms


def _peak(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


class _KernelTimer:
    """sampler.KERNEL_TIMER: device events around the launches spjoin brackets by name"""

    def __init__(self):
        self.pairs = {}

    def __call__(self, name):
        import contextlib
        import torch

        @contextlib.contextmanager
        def bracket():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            yield
            b.record()
            self.pairs.setdefault(name, []).append((a, b))
        return bracket()

    def median_ms(self, name):
        import torch
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in self.pairs.get(name, []))
        return ts[len(ts) // 2] if ts else float("nan")


def _fmt(label, med, ms, B):
    return f"{label:<66} {med:9.4f} ms / step  {B / med / 1e3:7.2f} M pairs/s   regions {' '.join(f'{v:.4f}' for v in ms)}"


def _embed(dev):
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(HOPS + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)


def _steps(sp, csr, dev, B, T, embed, train):
    """(stage step, row-form step + reference form) as closures over their own buffers; train: forward + backward"""
    import torch
    from surel_plus_amd.graphs import query_pairs
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    wgt = torch.randn(2, B, H, device=dev)
    kw = dict(num_walks=M, num_steps=HOPS)
    it = [0]

    def run(f):
        e = es[it[0] % 4]
        it[0] += 1
        if not train:
            with torch.no_grad():
                return f(e)
        for p in embed.parameters():
            p.grad = None
        (f(e) * wgt).sum().backward()

    cb = sp.StepBuffers(csr, B, stage="counts", table_rows=T, **kw)
    rb = sp.StepBuffers(csr, B, **kw) if B <= REF_MAX_B else None

    def stage(e):
        return sp.sample_and_mean_stage(csr, e, embed, buffers=cb, **kw)

    def reference(e):
        xz, seg, sets = sp.sample_and_gather(csr, e, buffers=rb, **kw)
        n = seg[1:] - seg[:-1]
        R = int(seg[-1])            # (the reference reads the row count: its xz is exactly R rows)
        x = embed(xz[:R]).sum(dim=-2)
        ids = torch.repeat_interleave(torch.arange(2 * B, device=dev), n, output_size=R)
        return (torch.zeros(2 * B, H, device=dev).index_add_(0, ids, x) / n.clamp(min=1)[:, None]).view(2, B, H)
    return (lambda: run(stage)), ((lambda: run(reference)) if rb is not None else None), cb


def part_a(sp, csr, dev, B, K, W, T):
    embed = _embed(dev)
    for train in (False, True):
        what = "forward + backward" if train else "forward"
        stage, ref, cb = _steps(sp, csr, dev, B, T, embed, train)
        med, ms = _regions(stage, K, W)
        pk = _peak(stage)
        print(_fmt(f"(a) B={B:>6} T={T}  stage step, {what}", med, ms, B) + f"   peak above the buffers {pk:9.1f} MB", flush=True)
        if ref is None:
            print(f"(a) B={B:>6}  the reference form does not fit at this size (38-102 GB of activations): the stage step alone; its buffers: "
                  f"counts {cb.counts.numel() * 4 / 1e6:.0f} MB, rows {(cb.ids.numel() + cb.slot.numel()) * 4 / 1e6:.0f} MB", flush=True)
            continue
        medr, msr = _regions(ref, K, W)
        pkr = _peak(ref)
        print(_fmt(f"(a) B={B:>6}  row-form step + reference form on xz, {what}", medr, msr, B) + f"   peak above the buffers {pkr:9.1f} MB"
              "   (reads the row count back every step)", flush=True)
        print(f"(a) B={B:>6}  {what}: reference / stage = {medr / med:.2f}x", flush=True)
    cb = _steps(sp, csr, dev, B, T, embed, False)[2]
    from surel_plus_amd.graphs import query_pairs
    _, _, _, sets = sp.sample_and_counts(csr, query_pairs(csr, B, seed=9300, device=dev), num_walks=M, num_steps=HOPS, buffers=cb)
    sets.resolve()
    print(f"(a) B={B:>6}  distinct LP rows of the batch: {int(cb.status[2]):,} (table_rows = {T})", flush=True)


def part_b(sp, sampler_mod, csr, dev, B, T, n=20):
    import torch
    from surel_plus_amd.graphs import query_pairs
    kw = dict(num_walks=M, num_steps=HOPS)
    e = query_pairs(csr, B, seed=9300, device=dev)
    cb, rb = sp.StepBuffers(csr, B, stage="counts", table_rows=T, **kw), sp.StepBuffers(csr, B, **kw)
    timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
    for _ in range(n):
        sp.sample_and_counts(csr, e, buffers=cb, **kw)
        _, _, sets = sp.sample_and_gather(csr, e, buffers=rb, **kw)
    col, cnt, join, walk = (timer.median_ms(k) for k in ("keyrows_columns", "sjoin_key_counts", "sjoin_fill", "walk_sets"))
    sampler_mod.KERNEL_TIMER = None
    sets.prefetch().resolve()
    rows = int(sets.extra[0])
    members = int(cb.nsize.to(torch.int64).sum())
    key_b, row_b, c_b, xz_b = 4 * members, 8 * rows, 4 * 2 * B * T, rows * 8 * (HOPS + 1)
    print(f"(b) B={B:>6} T={T}  walk {walk:.4f} ms | columns pass {col:.4f} ms: {key_b / 1e6:.1f} MB of keys = {key_b / col / 1e9:.2f} TB/s "
          f"({key_b / col / 1e-3 / HBM_PEAK:.1%} of the HBM peak)", flush=True)
    print(f"(b) B={B:>6} T={T}  count kernel {cnt:.4f} ms: rows {row_b / 1e6:.1f} MB + C {c_b / 1e6:.1f} MB = {(row_b + c_b) / cnt / 1e9:.2f} TB/s "
          f"({(row_b + c_b) / cnt / 1e-3 / HBM_PEAK:.1%}) | join kernel (row form) {join:.4f} ms: rows {row_b / 1e6:.1f} MB + xz {xz_b / 1e6:.1f} MB "
          f"= {(row_b + xz_b) / join / 1e9:.2f} TB/s ({(row_b + xz_b) / join / 1e-3 / HBM_PEAK:.1%})", flush=True)


def part_c(sp, csr, dev, B, K, W, T):
    import numpy as np
    import torch
    from surel_plus_amd.graphs import query_pairs
    embed = _embed(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    z, sets = sp.sample_spg(csr, np.arange(csr.num_nodes), num_walks=M, num_steps=HOPS, seed=111413, rng="philox", fused=True)
    table = sets.feature_table()
    b.record()
    b.synchronize()
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    it = [0]

    def store():
        e = es[it[0] % 4]
        it[0] += 1
        with torch.no_grad():
            sp.mean_stage(e, z, table, embed)
    stage = _steps(sp, csr, dev, B, T, embed, False)[0]
    med, ms = _regions(stage, K, W)
    meds, mss = _regions(store, K, W)
    print(_fmt(f"(c) B={B:>6} T={T}  stage step (samples its {2 * B:,} roots)", med, ms, B), flush=True)
    print(_fmt(f"(c) B={B:>6}  mean_stage over the resident store, T = {table.shape[0]:,}", meds, mss, B) +
          f"   sampling the store of {csr.num_nodes:,} nodes: {a.elapsed_time(b):.1f} ms once "
          f"(= {a.elapsed_time(b) / max(med - meds, 1e-9):.0f} steps of the difference)", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5"))
    T = int(OPTS.get("table_rows", "2048"))
    shapes = [int(b) for b in OPTS.get("B", "1024,4096,65536").split(",")]
    parts = OPTS.get("parts", "a,b,c").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"step_stage_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops, H = {H}; median of three regions of {K} steps after "
          f"{W} warm-up steps, device events", flush=True)
    for B in shapes:
        if "a" in parts:
            part_a(sp, csr, dev, B, K, W, T)
        if "b" in parts:
            part_b(sp, sampler_mod, csr, dev, B, T)
    if "c" in parts:
        part_c(sp, csr, dev, shapes[-1], K, W, T)


if __name__ == "__main__":
    main()

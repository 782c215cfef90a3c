#!/usr/bin/env python3
"""Dev-only: the higher-order path (main_horder.py: triplets (u, v, w), hgather, HONet's first stage) on the cit2-like graph of bench.py
with M = 100, 3 hops (the README's main_horder.py command), B = 2,048 (main_horder.py:33) and B = 65,536 triplets.

    python tools/horder_bench.py [--B=2048,65536] [--steps=50] [--warmup=10] [--parts=step,ids,stage]
        step   the triplet step (sample_and_hgather through StepBuffers(triplets=True): 3B roots, one join of 4B segments) against the
               two buffered pair steps (u, w) and (v, w) that give the same rows (4B roots, w walked twice), and against those two
               batches as one step of StepBuffers(batch=B) (4B roots, one join of 4B segments)
        ids    the pair step with ptr=False against ptr=True: the step, and the join kernel alone (device events around its launch)
        stage  hmean_stage against the reference form (hgather -> embed(xz).sum(-2) -> segment mean) at B = 2,048, H = 96: forward,
               forward + backward, peak memory; the count kernel's time and bytes, and what a kernel that stages w once could save
    python tools/horder_bench.py --only=pairs --root=DIR
        the two pair steps alone, with the package of the checkout DIR (the parent commit, built): what that commit can do for the
        same triplets, to be run on the same box in the same job

Every step time is the median of three regions of --steps steps after --warmup steps, between device events; nothing is read back
inside a region (the steps are queued as a serving loop queues them)."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.abspath(OPTS.get("root") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
M, HOPS, H = 100, 3, 96


def _regions(step, K, W):
    """(median, [three regions]) ms per step"""
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


class _KernelTimer:
    """sampler.KERNEL_TIMER: device events around the launches spjoin brackets by name"""

    def __init__(self):
        self.pairs, self.enabled = {}, False

    def __call__(self, name):
        import contextlib
        import torch

        @contextlib.contextmanager
        def bracket():
            if not self.enabled:
                yield
                return
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


def _triplets(csr, B, seed, dev):
    """(u, v) as the training mix of bench.py draws pairs, w uniform (dataloader.py:265-268 draws the negatives' w uniformly)"""
    import torch
    from surel_plus_amd.graphs import query_pairs
    e = query_pairs(csr, B, seed=seed, device=dev)
    w = torch.randint(0, csr.num_nodes, (1, B), device=dev, generator=torch.Generator(device=dev).manual_seed(seed + 77))
    return torch.cat([e, w]).contiguous()


def _fmt(label, med, ms):
    return f"{label:<62} {med:8.4f} ms / step   regions {' '.join(f'{v:.4f}' for v in ms)}"


def _kernels(sampler_mod, step, n=20):
    """' walk .. ms, join .. ms': the step's walk and join launches between device events of their own (sums over the step's launches,
    median over n steps); outside the regions -- an event pair costs a few microseconds around its kernel"""
    import torch
    walk, join = [], []
    for _ in range(n):
        timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
        timer.enabled = True
        step()
        torch.cuda.synchronize()
        walk.append(sum(a.elapsed_time(b) for a, b in timer.pairs.get("walk_sets", [])))
        join.append(sum(a.elapsed_time(b) for a, b in timer.pairs.get("sjoin_fill", [])))
    sampler_mod.KERNEL_TIMER = None
    return f"   walk {sorted(walk)[n // 2]:.4f} ms, join {sorted(join)[n // 2]:.4f} ms"


def part_pairs(sp, sampler_mod, csr, dev, B, K, W, tag, **kw):
    """two buffered pair steps (u, w) and (v, w): the rows of the triplet step, w walked twice"""
    bufs = [sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, **kw) for _ in range(2)]
    hs = [_triplets(csr, B, 9000 + s, dev) for s in range(4)]
    es = [(h[[0, 2]].contiguous(), h[[1, 2]].contiguous()) for h in hs]
    it = [0]

    def step():
        a, b = es[it[0] % 4]
        it[0] += 1
        sp.sample_and_gather(csr, a, num_walks=M, num_steps=HOPS, buffers=bufs[0], **kw)
        sp.sample_and_gather(csr, b, num_walks=M, num_steps=HOPS, buffers=bufs[1], **kw)
    med, ms = _regions(step, K, W)
    print(_fmt(f"B={B:>6}  two pair steps (u,w) + (v,w), 4B roots [{tag}]", med, ms) + _kernels(sampler_mod, step), flush=True)
    return med


def part_both(sp, sampler_mod, csr, dev, B, K, W):
    """the two pair batches (u, w) and (v, w) as ONE buffered step (StepBuffers(batch=B): 4B roots, one join of 4B segments, pointers):
    what one launch instead of two does to the join, apart from the ids and from walking w once"""
    import torch
    bufs = sp.StepBuffers(csr, 2 * B, num_walks=M, num_steps=HOPS, batch=B)
    es = [torch.stack([h[[0, 2]], h[[1, 2]]]).contiguous() for h in (_triplets(csr, B, 9000 + s, dev) for s in range(4))]
    it = [0]

    def step():
        e = es[it[0] % 4]
        it[0] += 1
        sp.sample_and_gather(csr, e, num_walks=M, num_steps=HOPS, buffers=bufs)
    med, ms = _regions(step, K, W)
    print(_fmt(f"B={B:>6}  both pair batches in one step, 4B roots, pointers", med, ms) + _kernels(sampler_mod, step), flush=True)


def part_step(sp, sampler_mod, csr, dev, B, K, W):
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, triplets=True)
    hs = [_triplets(csr, B, 9000 + s, dev) for s in range(4)]
    it = [0]

    def step():
        h = hs[it[0] % 4]
        it[0] += 1
        sp.sample_and_hgather(csr, h, num_walks=M, num_steps=HOPS, buffers=bufs)
    med, ms = _regions(step, K, W)
    print(_fmt(f"B={B:>6}  triplet step, 3B roots, ids written", med, ms) + _kernels(sampler_mod, step), flush=True)
    return med


def part_ids(sp, sampler_mod, csr, dev, B, K, W):
    from surel_plus_amd.graphs import query_pairs
    es = [query_pairs(csr, B, seed=9100 + s, device=dev) for s in range(4)]
    for ptr in (True, False):
        bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, ptr=ptr)
        it = [0]

        def step():
            e = es[it[0] % 4]
            it[0] += 1
            return sp.sample_and_gather(csr, e, num_walks=M, num_steps=HOPS, buffers=bufs, ptr=ptr)
        med, ms = _regions(step, K, W)
        timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
        timer.enabled = True
        for _ in range(20):
            _, _, sets = step()
        join_ms = timer.median_ms("sjoin_fill")
        sampler_mod.KERNEL_TIMER = None
        sets.prefetch().resolve()
        rows, k = int(sets.extra[0]), HOPS + 1
        out_bytes = rows * (8 * k + (0 if ptr else 8))
        print(_fmt(f"B={B:>6}  pair step ptr={ptr!s:<5}", med, ms) +
              f"   join kernel {join_ms:.4f} ms, {rows:,} rows, {out_bytes / 1e6:.1f} MB written = {out_bytes / join_ms / 1e9:.2f} TB/s", flush=True)


def part_stage(sp, sampler_mod, csr, dev, B, n=5):
    import numpy as np
    import torch
    z, sets = sp.sample_spg(csr, np.arange(csr.num_nodes), num_walks=M, num_steps=HOPS, seed=111413, rng="philox", fused=True)
    table = sets.feature_table()
    T, k = table.shape
    torch.manual_seed(0)
    embed = torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)
    hedge = _triplets(csr, B, 9200, dev)
    wgt = torch.randn(4, B, H, device=dev)

    def reference():
        xz, ind = sp.hgather(hedge, z, dev, encode=table)
        x = embed(xz).sum(dim=-2)
        cnt = torch.zeros(4 * B, device=dev).index_add_(0, ind, torch.ones(ind.numel(), device=dev))
        return (torch.zeros(4 * B, H, device=dev).index_add_(0, ind, x) / cnt.clamp(min=1)[:, None]).view(4, B, H)

    def timed(fn):
        ts = []
        for _ in range(n + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return sorted(ts[1:])[n // 2]

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e6
    print(f"first stage: all-N store N={z.n_rows:,} max_len {z.max_len}, T = {T:,} LP rows (k = {k}), B = {B:,} triplets, H = {H}; median of {n} "
          f"calls (ms), peak = the call's allocation above what was there (MB)", flush=True)
    with torch.no_grad():
        want = reference()
    for label, f in (("hmean_stage", lambda: sp.hmean_stage(hedge, z, table, embed)), ("reference form", reference)):
        def fwd():
            with torch.no_grad():
                f()

        def fb():
            for p in embed.parameters():
                p.grad = None
            (f() * wgt).sum().backward()
        try:
            tf, tfb, pf, pfb = timed(fwd), timed(fb), peak(fwd), peak(fb)
            with torch.no_grad():
                d = float((f() - want).abs().max())
            print(f"  {label:<15} fwd {tf:8.3f}  f+b {tfb:8.3f} | peak fwd {pf:9.1f}  f+b {pfb:9.1f} | max |form - ref| {d:.3g} "
                  f"(of max |ref| {d / float(want.abs().max()):.2g})", flush=True)
        except Exception as ex:          # (a store the count kernel does not hold: said, not hidden)
            print(f"  {label:<15} {type(ex).__name__}: {str(ex)[:200]}", flush=True)
    # one launch over [u | w | v | w]: its time and bytes, and what staging w once (three row reads per triplet) could save
    try:
        timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
        timer.enabled = True
        for _ in range(n + 2):
            sp.hgather_counts(hedge, z, T)
        ms = timer.median_ms("sjoin_counts")
        lens = (z.indptr[1:] - z.indptr[:-1])[hedge]
        rows4 = 8 * int(lens[0].sum() + lens[1].sum() + 2 * lens[2].sum())
        rows3 = 8 * int(lens.sum())
        counts = 4 * 4 * B * T
        print(f"  count kernel, one launch over [u|w|v|w]: {ms:.4f} ms; row bytes {rows4 / 1e6:.1f} MB (w read twice) + count rows "
              f"{counts / 1e6:.1f} MB = {(rows4 + counts) / ms / 1e9:.2f} TB/s; with w staged once the rows would be {rows3 / 1e6:.1f} MB: "
              f"{(rows4 - rows3) / (rows4 + counts):.1%} of the kernel's bytes", flush=True)
    except Exception as ex:
        print(f"  count kernel: {type(ex).__name__}: {str(ex)[:200]}", flush=True)
    finally:
        sampler_mod.KERNEL_TIMER = None


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W = int(OPTS.get("steps", "50")), int(OPTS.get("warmup", "10"))
    shapes = [int(b) for b in OPTS.get("B", "2048,65536").split(",")]
    parts = OPTS.get("parts", "step,ids,stage").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"horder_bench: package {os.path.dirname(sp.__file__)}; cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops; median of three "
          f"regions of {K} steps after {W} warm-up steps, device events", flush=True)
    if OPTS.get("only") == "pairs":
        for B in shapes:
            part_pairs(sp, sampler_mod, csr, dev, B, K, W, "ptr=True, this package")
        return
    for B in shapes:
        if "step" in parts:
            t3 = part_step(sp, sampler_mod, csr, dev, B, K, W)
            t4 = part_pairs(sp, sampler_mod, csr, dev, B, K, W, "ptr=True")
            t4i = part_pairs(sp, sampler_mod, csr, dev, B, K, W, "ptr=False", ptr=False)
            part_both(sp, sampler_mod, csr, dev, B, K, W)
            print(f"B={B:>6}  triplet step / two pair steps: {t3 / t4:.3f} (ptr=True), {t3 / t4i:.3f} (ptr=False: ids written, as the triplet "
                  f"step writes them)", flush=True)
        if "ids" in parts:
            part_ids(sp, sampler_mod, csr, dev, B, K, W)
    if "stage" in parts:
        part_stage(sp, sampler_mod, csr, dev, 2048)


if __name__ == "__main__":
    main()

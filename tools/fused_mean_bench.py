#!/usr/bin/env python3
"""Dev-only: the LP encoder's mean first stage fused into the count join (sample_and_fused_mean_stage and its twins, StepBuffers(stage=
"mean"), subgacc_sjoin_key_mean) against the stage it stands beside (sample_and_mean_stage and its twins, StepBuffers(stage="counts"),
subgacc_sjoin_key_counts + the GEMM) in the same library and the same run, on the cit2-like graph of bench.py, M = 200, H = 96.

    python tools/fused_mean_bench.py [--B=1024,4096,65536] [--steps=10] [--rounds=5] [--warmup=3] [--parts=a,b,c,d] [--table_rows=2048]
        a   the buffered step, 3 hops: forward under no_grad and forward + backward, with peak memory above the buffers (pairs at
            every B; the triplet twins, sample_and_fused_hmean_stage against sample_and_hmean_stage, up to B = 4,096)
        b   the join launches alone over one step's rows: sjoin_key_mean against sjoin_key_counts + (C @ E) / sizes
        c   the evaluation shape: the *_star calls with K = 1,000 at P*K = 66,000, pairs and triplets, forward under no_grad
        d   wide_keys=True at (200, 4) with table_rows = 8,192, forward under no_grad

The two sides alternate round by round; a round is --steps steps between device events; per side the median (min .. max) of the rounds.
A verdict is given only beyond the other side's spread: FASTER / SLOWER when the medians differ by more than the larger (max - min),
LEVEL otherwise.  Nothing is read back inside a round."""
import ctypes
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
M, H = 200, 96


def _ab(sides, K, R, W):
    """sides {name: closure}: W warm-up steps each, then R rounds of K steps, the sides alternating -> {name: (median, min, max)} ms / step"""
    import torch
    for f in sides.values():
        for _ in range(W):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(R):
        for name, f in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(K):
                f()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / K)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def _peak(fn):
    import gc
    import torch
    gc.collect()                # (the dead buffers of an earlier case, freed inside the call, would make the peak negative)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def _report(label, res, new="fused", old="unfused", extra=""):
    (mn, lon, hin), (mo, loo, hio) = res[new], res[old]
    spread = max(hin - lon, hio - loo)
    verdict = "LEVEL" if abs(mn - mo) <= spread else ("FASTER" if mn < mo else "SLOWER")
    print(f"{label:<58} {new} {mn:8.4f} ({lon:.4f} .. {hin:.4f})  {old} {mo:8.4f} ({loo:.4f} .. {hio:.4f}) ms   {old} / {new} = "
          f"{mo / mn:5.2f}x  {verdict}{extra}", flush=True)


def _embed(dev, k):
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)


def _runner(embed, train, wgt):
    import torch

    def run(f):
        if not train:
            with torch.no_grad():
                return f()
        for p in embed.parameters():
            p.grad = None
        (f() * wgt).sum().backward()
    return run


def part_a(sp, csr, dev, B, K, R, W, T, hops=3, wide=False, tag="(a)", modes=(False, True), triplets=False):
    import torch
    from surel_plus_amd.graphs import query_pairs
    embed = _embed(dev, hops + 1)
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    if triplets:        # (u, v) of a batch with the u of the next one as w
        es = [torch.cat([es[s], es[(s + 1) % 4][:1]]) for s in range(4)]
    new, old = (sp.sample_and_fused_hmean_stage, sp.sample_and_hmean_stage) if triplets else \
        (sp.sample_and_fused_mean_stage, sp.sample_and_mean_stage)
    kw = dict(num_walks=M, num_steps=hops, wide_keys=wide)
    mb = sp.StepBuffers(csr, B, stage="mean", table_rows=T, width=H, triplets=triplets, **kw)
    cb = sp.StepBuffers(csr, B, stage="counts", table_rows=T, triplets=triplets, **kw)
    wgt = torch.randn(4 if triplets else 2, B, H, device=dev)
    it = [0]

    def batch():
        it[0] += 1
        return es[it[0] % 4]
    for train in modes:
        run = _runner(embed, train, wgt)
        sides = {"fused": lambda: run(lambda: new(csr, batch(), embed, buffers=mb, **kw)),
                 "unfused": lambda: run(lambda: old(csr, batch(), embed, buffers=cb, **kw))}
        res = _ab(sides, K, R, W)
        pk = {k: _peak(f) for k, f in sides.items()}
        what = "forward + backward" if train else "forward, no_grad"
        _report(f"{tag} B={B:>6} T={T} {hops} hops  step, {what}", res,
                extra=f"   peak above the buffers: fused {pk['fused']:.1f} MB, unfused {pk['unfused']:.1f} MB")
    mb.sets.resolve(), cb.sets.resolve()
    own = lambda b: sum(t.numel() * t.element_size() for t in vars(b).values() if torch.is_tensor(t)) / 1e6     # noqa: E731
    print(f"{tag} B={B:>6} T={T}  buffers: stage='mean' {own(mb):.1f} MB (mean {mb.mean.numel() * 4 / 1e6:.1f} MB), stage='counts' "
          f"{own(cb):.1f} MB (counts {cb.counts.numel() * 4 / 1e6:.1f} MB); distinct LP rows of the last batch {int(mb.status[2]):,}", flush=True)


def part_b(sp, csr, dev, B, K, R, W, T):
    import torch
    from surel_plus_amd import _lib, spjoin
    from surel_plus_amd.graphs import query_pairs
    kw = dict(num_walks=M, num_steps=3)
    mb = sp.StepBuffers(csr, B, stage="mean", table_rows=T, width=H, **kw)
    join, sizes, table, sets = spjoin._buffered_step(csr, query_pairs(csr, B, seed=9300, device=dev), mb, 111413, None)
    with torch.no_grad():
        E = _embed(dev, 4)(table).contiguous()
    Cm = torch.empty((mb.S, T), dtype=torch.float32, device=dev)
    L, d = _lib.lib(), join.desc()
    args = (_lib.ptr(mb.ukeys), _lib.ptr(mb.status[2:3]))

    def counts():
        _lib.check(L.subgacc_sjoin_key_counts(ctypes.byref(d), *args, _lib.ptr(Cm), _lib.ptr(mb.sizes), _lib.stream_ptr()))

    def unfused():
        counts()
        return (Cm @ E) / sizes.clamp(min=1).to(torch.float32)[:, None]
    res = _ab({"fused": lambda: join.forward(E), "unfused": unfused, "counts alone": counts}, K, R, W)
    sets.resolve()
    _report(f"(b) B={B:>6} T={T}  sjoin_key_mean | sjoin_key_counts + GEMM", res)
    m, lo, hi = res["counts alone"]
    members = int(mb.nsize.to(torch.int64).sum())
    print(f"(b) B={B:>6} T={T}  sjoin_key_counts alone {m:.4f} ({lo:.4f} .. {hi:.4f}) ms; C {Cm.numel() * 4 / 1e6:.1f} MB, E "
          f"{E.numel() * 4 / 1e3:.0f} KB, out {mb.S * H * 4 / 1e6:.1f} MB, rows {members * 8 / 1e6:.1f} MB", flush=True)


def part_c(sp, csr, dev, K, R, W, T, P=66, Kt=1000, triplets=False):
    import torch
    embed = _embed(dev, 4)
    kw = dict(num_walks=M, num_steps=3)
    g = torch.Generator(device="cpu").manual_seed(5)
    src = [torch.randint(0, csr.num_nodes, (P,), generator=g).to(dev) for _ in range(4)]
    tgt = [torch.randint(0, csr.num_nodes, (P, Kt), generator=g).to(dev) for _ in range(4)]
    if triplets:        # uv [2, P]: the sources with the next batch's sources as v
        src = [torch.stack([src[s], src[(s + 1) % 4]]) for s in range(4)]
    new, old = (sp.sample_and_fused_hmean_stage_star, sp.sample_and_hmean_stage_star) if triplets else \
        (sp.sample_and_fused_mean_stage_star, sp.sample_and_mean_stage_star)
    mb = sp.StepBuffers(csr, P * Kt, stage="mean", table_rows=T, width=H, star=Kt, triplets=triplets, **kw)
    cb = sp.StepBuffers(csr, P * Kt, stage="counts", table_rows=T, star=Kt, triplets=triplets, **kw)
    it = [0]

    def batch():
        it[0] += 1
        return src[it[0] % 4], tgt[it[0] % 4]
    run = _runner(embed, False, None)
    sides = {"fused": lambda: run(lambda: new(csr, *batch(), embed, buffers=mb, **kw)),
             "unfused": lambda: run(lambda: old(csr, *batch(), embed, buffers=cb, **kw))}
    res = _ab(sides, K, R, W)
    pk = {k: _peak(f) for k, f in sides.items()}
    mb.sets.resolve(), cb.sets.resolve()
    _report(f"(c) star{' triplets' if triplets else ''} P={P} K={Kt:,} (P*K = {P * Kt:,}) T={T}  step, forward, no_grad", res,
            extra=f"   peak above the buffers: fused {pk['fused']:.1f} MB, unfused {pk['unfused']:.1f} MB")


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, R, W = int(OPTS.get("steps", "10")), int(OPTS.get("rounds", "5")), int(OPTS.get("warmup", "3"))
    T = int(OPTS.get("table_rows", "2048"))
    shapes = [int(b) for b in OPTS.get("B", "1024,4096,65536").split(",")]
    parts = OPTS.get("parts", "a,b,c,d").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"fused_mean_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, H = {H}; sides alternate, median (min .. max) of {R} rounds of "
          f"{K} steps after {W} warm-up steps, device events; a verdict only beyond the other side's spread", flush=True)
    for B in shapes:
        if "a" in parts:
            part_a(sp, csr, dev, B, K, R, W, T)
        if "b" in parts:
            part_b(sp, csr, dev, B, K, R, W, T)
        if "a" in parts and B <= 4096:      # the triplet twins (4B segments)
            part_a(sp, csr, dev, B, K, R, W, T, tag="(a) triplets", triplets=True)
    if "c" in parts:
        part_c(sp, csr, dev, K, R, W, T)
        part_c(sp, csr, dev, K, R, W, T, triplets=True)
    if "d" in parts:
        for B in shapes:
            part_a(sp, csr, dev, B, K, R, W, 8192, hops=4, wide=True, tag="(d) wide_keys", modes=(False,))


if __name__ == "__main__":
    main()

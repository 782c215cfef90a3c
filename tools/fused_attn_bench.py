#!/usr/bin/env python3
"""Dev-only: the LP encoder's attentional first stage fused into the attentional count join (sample_and_fused_attn_stage and its star
twin, StepBuffers(stage="attn"), subgacc_sjoin_key_attn) against the stage it stands beside (sample_and_attn_stage and its star twin,
StepBuffers(stage="counts_attn"), subgacc_sjoin_key_counts_attn + the GEMM) in the same library and the same run, on the cit2-like
graph of bench.py, M = 200, 3 hops, H = 96.

    python tools/fused_attn_bench.py [--B=1024,4096,65536] [--steps=10] [--rounds=5] [--warmup=3] [--parts=a,b,c] [--table_rows=2048,1024]
        a   the buffered step: forward under no_grad and forward + backward, with peak memory above the buffers and the buffer sets' bytes
        b   the join launches alone over one step's rows: sjoin_key_attn against sjoin_key_counts_attn + W @ E
        c   the evaluation shape: the *_star calls with K = 1,000 at P*K = 66,000, forward under no_grad

The two sides alternate round by round; a round is --steps steps between device events; per side the median (min .. max) of the rounds.
A verdict is given only beyond the other side's spread: FASTER / SLOWER when the medians differ by more than the larger (max - min),
LEVEL otherwise.  Nothing is read back inside a round."""
import ctypes
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SUBGACC_QUIET", "1")
from fused_mean_bench import _ab, _peak, _report  # noqa: E402  (the alternating A/B, the peak and the verdict: one text for both tools)

M, H, HOPS = 200, 96, 3


def _nets(dev):
    import torch
    torch.manual_seed(0)
    nn = torch.nn
    return [m.to(dev) for m in (nn.Sequential(nn.Linear(HOPS + 1, H), nn.ReLU(), nn.Linear(H, H)), nn.Linear(H, 1), nn.Linear(H, H))]


def _runner(nets, train, wgt):
    import torch

    def run(f):
        if not train:
            with torch.no_grad():
                return f()
        for m in nets:
            for p in m.parameters():
                p.grad = None
        (f() * wgt).sum().backward()
    return run


def part_a(sp, csr, dev, B, K, R, W, T):
    import torch
    from surel_plus_amd.graphs import query_pairs
    nets = _nets(dev)
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    kw = dict(num_walks=M, num_steps=HOPS)
    fb = sp.StepBuffers(csr, B, stage="attn", table_rows=T, width=H, **kw)
    ub = sp.StepBuffers(csr, B, stage="counts_attn", table_rows=T, **kw)
    wgt = torch.randn(2, B, H, device=dev)
    it = [0]

    def batch():
        it[0] += 1
        return es[it[0] % 4]
    for train in (False, True):
        run = _runner(nets, train, wgt)
        sides = {"fused": lambda: run(lambda: sp.sample_and_fused_attn_stage(csr, batch(), *nets, buffers=fb, **kw)),
                 "unfused": lambda: run(lambda: sp.sample_and_attn_stage(csr, batch(), *nets, buffers=ub, **kw))}
        res = _ab(sides, K, R, W)
        pk = {k: _peak(f) for k, f in sides.items()}
        what = "forward + backward" if train else "forward, no_grad"
        _report(f"(a) B={B:>6} T={T} {HOPS} hops  step, {what}", res,
                extra=f"   peak above the buffers: fused {pk['fused']:.1f} MB, unfused {pk['unfused']:.1f} MB")
    fb.sets.resolve(), ub.sets.resolve()
    own = lambda b: sum(t.numel() * t.element_size() for t in vars(b).values() if torch.is_tensor(t)) / 1e6     # noqa: E731
    print(f"(a) B={B:>6} T={T}  buffers: stage='attn' {own(fb):.1f} MB (attn {fb.attn.numel() * 4 / 1e6:.1f} MB), stage='counts_attn' "
          f"{own(ub):.1f} MB (counts {ub.counts.numel() * 4 / 1e6:.1f} MB); distinct LP rows of the last batch {int(fb.status[2]):,}",
          flush=True)


def part_b(sp, csr, dev, B, K, R, W, T):
    import torch
    from surel_plus_amd import _lib, spjoin
    from surel_plus_amd.graphs import query_pairs
    kw = dict(num_walks=M, num_steps=HOPS)
    fb = sp.StepBuffers(csr, B, stage="attn", table_rows=T, width=H, **kw)
    join, sizes, table, sets = spjoin._buffered_step(csr, query_pairs(csr, B, seed=9300, device=dev), fb, 111413, None)
    with torch.no_grad():
        E = _nets(dev)[0](table).contiguous()
        g = (E @ torch.randn(H, device=dev)).contiguous()
    Wm = torch.empty((fb.S, T), dtype=torch.float32, device=dev)
    L, d = _lib.lib(), join.desc()
    args = (_lib.ptr(fb.ukeys), _lib.ptr(fb.status[2:3]), _lib.ptr(g))

    def weights():
        _lib.check(L.subgacc_sjoin_key_counts_attn(ctypes.byref(d), *args, _lib.ptr(Wm), None, None, _lib.ptr(fb.sizes), _lib.stream_ptr()))

    def unfused():
        weights()
        return Wm @ E
    res = _ab({"fused": lambda: join.fused(g, E, False), "unfused": unfused, "weights alone": weights}, K, R, W)
    sets.resolve()
    _report(f"(b) B={B:>6} T={T}  sjoin_key_attn | sjoin_key_counts_attn + GEMM", res)
    m, lo, hi = res["weights alone"]
    members = int(fb.nsize.to(torch.int64).sum())
    print(f"(b) B={B:>6} T={T}  sjoin_key_counts_attn alone {m:.4f} ({lo:.4f} .. {hi:.4f}) ms; W {Wm.numel() * 4 / 1e6:.1f} MB, E "
          f"{E.numel() * 4 / 1e3:.0f} KB, out {fb.S * H * 4 / 1e6:.1f} MB, rows {members * 8 / 1e6:.1f} MB", flush=True)


def part_c(sp, csr, dev, K, R, W, T, P=66, Kt=1000):
    import torch
    nets = _nets(dev)
    kw = dict(num_walks=M, num_steps=HOPS)
    g = torch.Generator(device="cpu").manual_seed(5)
    src = [torch.randint(0, csr.num_nodes, (P,), generator=g).to(dev) for _ in range(4)]
    tgt = [torch.randint(0, csr.num_nodes, (P, Kt), generator=g).to(dev) for _ in range(4)]
    fb = sp.StepBuffers(csr, P * Kt, stage="attn", table_rows=T, width=H, star=Kt, **kw)
    ub = sp.StepBuffers(csr, P * Kt, stage="counts_attn", table_rows=T, star=Kt, **kw)
    it = [0]

    def batch():
        it[0] += 1
        return src[it[0] % 4], tgt[it[0] % 4]
    run = _runner(nets, False, None)
    sides = {"fused": lambda: run(lambda: sp.sample_and_fused_attn_stage_star(csr, *batch(), *nets, buffers=fb, **kw)),
             "unfused": lambda: run(lambda: sp.sample_and_attn_stage_star(csr, *batch(), *nets, buffers=ub, **kw))}
    res = _ab(sides, K, R, W)
    pk = {k: _peak(f) for k, f in sides.items()}
    fb.sets.resolve(), ub.sets.resolve()
    _report(f"(c) star P={P} K={Kt:,} (P*K = {P * Kt:,}) T={T}  step, forward, no_grad", res,
            extra=f"   peak above the buffers: fused {pk['fused']:.1f} MB, unfused {pk['unfused']:.1f} MB")


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, R, W = int(OPTS.get("steps", "10")), int(OPTS.get("rounds", "5")), int(OPTS.get("warmup", "3"))
    tables = [int(t) for t in OPTS.get("table_rows", "2048,1024").split(",")]
    shapes = [int(b) for b in OPTS.get("B", "1024,4096,65536").split(",")]
    parts = OPTS.get("parts", "a,b,c").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"fused_attn_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops, H = {H}; sides alternate, median (min .. max) of "
          f"{R} rounds of {K} steps after {W} warm-up steps, device events; a verdict only beyond the other side's spread", flush=True)
    for T in tables:
        for B in shapes:
            if "a" in parts:
                part_a(sp, csr, dev, B, K, R, W, T)
            if "b" in parts:
                part_b(sp, csr, dev, B, K, R, W, T)
        if "c" in parts:
            part_c(sp, csr, dev, K, R, W, T)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the on-demand step for one source against K targets (StepBuffers(star=K), sample_and_gather_star /
sample_and_hgather_star) against the routes that take the expanded list, on the cit2-like graph of bench.py.

    python tools/star_step_bench.py [--parts=pairs,triplets] [--B=1024,8192,65536] [--K=1000] [--steps=20] [--warmup=5] [--rounds=5]
        pairs     an evaluation batch (every source against K targets, utils.py:93-95) at (M, m) = (200, 3), and at (100, 2) with
                  small_rows=True: the star step (P + P*K roots) against the expanded plain step and the expanded step with
                  dedup_roots=True (2*P*K endpoints each, the second one walking the distinct ones).
        triplets  (u, v) kept, w replaced by K candidates (dataloader.py:265-275): the star step (2*P + P*K roots) against the expanded
                  triplet step (3*P*K roots), same shapes.
    P is B // K rounded up to at least one source, so P*K is about B.

The sides of every comparison alternate in one process and one library: --rounds rounds of (--steps steps of each side) after --warmup
steps of each, every region between device events; the figure is the median over the rounds with (min .. max).  A side counts as
faster only beyond the other side's own spread: the verdict column says `faster`, `slower` or `level`.  The per-launch lines (the walk
launch and the join) come from a separate pass of --steps steps per side with sampler.KERNEL_TIMER set: mean per launch."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SUBGACC_QUIET", "1")
SHAPES = ((200, 3, {}), (100, 2, dict(small_rows=True)))

from small_step_bench import _ab, _compare, _per_launch  # noqa: E402  (the alternating A/B and its report)


def _stars(csr, P, K, dev, seed, heads=1):
    """four batches (heads [heads, P], targets [P, K]) of random nodes"""
    import torch
    gen = torch.Generator(device=dev)
    return [(torch.randint(0, csr.num_nodes, (heads, P), device=dev, generator=gen.manual_seed(seed + s)),
             torch.randint(0, csr.num_nodes, (P, K), device=dev, generator=gen)) for s in range(4)]


def part_pairs(sp, csr, dev, P, Kt, K, W, rounds):
    import torch
    for M, m, how in SHAPES:
        made, kw = dict(num_walks=M, num_steps=m, **how), dict(num_walks=M, num_steps=m, **how)
        stars = [(h[0], t) for h, t in _stars(csr, P, Kt, dev, 9100)]
        edges = [torch.stack([s.repeat_interleave(Kt), t.reshape(-1)]) for s, t in stars]
        star = sp.StepBuffers(csr, P * Kt, star=Kt, **made)
        plain, dd = sp.StepBuffers(csr, P * Kt, **made), sp.StepBuffers(csr, P * Kt, dedup_roots=True, **made)
        it = [0]

        def run_star():
            it[0] += 1
            return sp.sample_and_gather_star(csr, *stars[it[0] % 4], buffers=star, **kw)

        def run(bufs, dedup):
            it[0] += 1
            return sp.sample_and_gather(csr, edges[it[0] % 4], buffers=bufs, dedup_roots=dedup, **kw)

        sides = {"star": run_star, "expanded": lambda: run(plain, False), "expanded, dedup_roots=True": lambda: run(dd, True)}
        head = f"pairs    M={M:>3} m={m} P={P:>3} K={Kt} ({star.n:>6} / {plain.n:>6} roots)"
        r = _ab(sides, K, W, rounds)
        _compare(head, list(sides), r, "expanded")
        print(f"{head}  star / expanded, dedup_roots=True = {r['star'][0] / r['expanded, dedup_roots=True'][0]:.2f}", flush=True)
        _per_launch(head, sides, K)


def part_triplets(sp, csr, dev, P, Kt, K, W, rounds):
    import torch
    for M, m, how in SHAPES:
        made, kw = dict(num_walks=M, num_steps=m, triplets=True, **how), dict(num_walks=M, num_steps=m, **how)
        stars = _stars(csr, P, Kt, dev, 9200, heads=2)
        hedges = [torch.stack([uv[0].repeat_interleave(Kt), uv[1].repeat_interleave(Kt), w.reshape(-1)]) for uv, w in stars]
        star, plain = sp.StepBuffers(csr, P * Kt, star=Kt, **made), sp.StepBuffers(csr, P * Kt, **made)
        it = [0]

        def run_star():
            it[0] += 1
            return sp.sample_and_hgather_star(csr, *stars[it[0] % 4], buffers=star, **kw)

        def run():
            it[0] += 1
            return sp.sample_and_hgather(csr, hedges[it[0] % 4], buffers=plain, **kw)

        sides = {"star": run_star, "expanded": run}
        head = f"triplets M={M:>3} m={m} P={P:>3} K={Kt} ({star.n:>6} / {plain.n:>6} roots)"
        _compare(head, list(sides), _ab(sides, K, W, rounds), "expanded")
        _per_launch(head, sides, K)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W, rounds = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5")), int(OPTS.get("rounds", "5"))
    Kt = int(OPTS.get("K", "1000"))
    parts = OPTS.get("parts", "pairs,triplets").split(",")
    csr = preset_graph("cit2", device=dev)
    props = torch.cuda.get_device_properties(0)
    print(f"star_step_bench: {props.name}, {props.multi_processor_count} CUs, torch {torch.__version__}; cit2-like graph N={csr.num_nodes:,}; "
          f"sides alternated, median (min .. max) of {rounds} rounds of {K} buffered steps after {W} warm-up steps, device events; Philox", flush=True)
    for B in (int(v) for v in OPTS.get("B", "1024,8192,65536").split(",")):
        P = max(1, (B + Kt // 2) // Kt)
        for part, fn in (("pairs", part_pairs), ("triplets", part_triplets)):
            if part in parts:
                fn(sp, csr, dev, P, Kt, K, W, rounds)
    print("not measured: kernel counters, the stage forms, 16-bit rows, 2 and 4 hops at M = 200, graphs other than cit2-like, "
          "bench.py (it does not reach this code)", flush=True)


if __name__ == "__main__":
    main()

"""Dev-only: A/B of the walk order -- order=None against order=locality_order(csr) -- alternating, median of repeats.

    python3 tools/locality_ab.py [REPS] [STEPS]            (defaults 5, 20)

Configurations: the cit2 parameters (M=200, 3 hops, 65,536 query_pairs per step, StepBuffers, Philox) on
  cit2loc_perm   cit2loc with its ids randomly permuted (graphs.relabeled): communities without id locality
  cit2loc        communities of consecutive ids
  cit2           the structureless power-law graph
Per configuration and order: walk-kernel ms (HIP events around the walk launch, median over the steps of a repeat), step pairs/s
(wall time of STEPS queued steps), the offline all-N build (subg_matrix over np.arange(N), wall ms) and, for the rank order, the
builder's own ms (locality_order, 8 rounds).  Every figure is the median of REPS repeats; the two orders alternate inside a repeat."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SUBGACC_QUIET"] = "1"
import numpy as np
import torch

import surel_plus_amd as sp
from surel_plus_amd import sampler
from surel_plus_amd.graphs import preset_graph, query_pairs, relabeled

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, M, HOPS = 65536, 200, 3


class WalkTimer:
    """sampler.KERNEL_TIMER: HIP events around the walk launch of every step"""
    def __init__(self):
        self.pairs = []

    def __call__(self, name):
        timer = self

        class _T:
            def __enter__(self):
                if name == "walk_sets":
                    self.a = torch.cuda.Event(enable_timing=True)
                    self.a.record()
                return self

            def __exit__(self, *exc):
                if name == "walk_sets":
                    b = torch.cuda.Event(enable_timing=True)
                    b.record()
                    timer.pairs.append((self.a, b))
                return False
        return _T()

    def take(self):
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.pairs]
        self.pairs = []
        return ms


def steps(csr, order, batches, timer):
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, order=order)
    for e in batches[:2]:                                       # warm-up
        sp.sample_and_gather(csr, e, num_walks=M, num_steps=HOPS, buffers=bufs)[2].resolve()
    timer.take()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for i in range(STEPS):
        last = sp.sample_and_gather(csr, batches[i % len(batches)], num_walks=M, num_steps=HOPS, buffers=bufs)[2]
    last.resolve()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    walk = timer.take()
    assert bufs.walk_order == ("rank" if order is not None else "id"), bufs.walk_order
    return statistics.median(walk), B * STEPS / dt


def offline(csr, order):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z, enc = sp.subg_matrix(csr, np.arange(csr.num_nodes), num_walks=M, num_steps=HOPS + 1, rng="philox", order=order)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert z.sets.walk_order == ("rank" if order is not None else "batch")
    del z, enc
    return dt * 1e3


def builder(csr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lo = sp.locality_order(csr)
    torch.cuda.synchronize()
    return lo, (time.perf_counter() - t0) * 1e3


def main():
    timer = WalkTimer()
    sampler.KERNEL_TIMER = timer
    dev = "cuda"
    base = preset_graph("cit2loc", device=dev)
    perm = torch.randperm(base.num_nodes, generator=torch.Generator().manual_seed(0)).to(dev)
    graphs = {"cit2loc_perm": relabeled(base, perm), "cit2loc": base, "cit2": preset_graph("cit2", device=dev)}
    del perm
    print(f"locality_ab: B={B} pairs/step, M={M}, {HOPS} hops, Philox, StepBuffers; {REPS} repeats x {STEPS} steps, "
          f"device {torch.cuda.get_device_name(0)}", flush=True)
    rows = []
    for name, csr in graphs.items():
        batches = [query_pairs(csr, B, seed=s) for s in range(4)]
        lo, _ = builder(csr)                                    # warm-up of the builder (and of the sort)
        res = {k: [] for k in ("walk_id", "walk_rank", "pps_id", "pps_rank", "off_id", "off_rank", "build")}
        for r in range(REPS):
            lo, bms = builder(csr)
            res["build"].append(bms)
            for tag, order in (("id", None), ("rank", lo)) if r % 2 == 0 else (("rank", lo), ("id", None)):
                w, pps = steps(csr, order, batches, timer)
                res["walk_" + tag].append(w)
                res["pps_" + tag].append(pps)
                res["off_" + tag].append(offline(csr, order))
            print(f"  {name} rep {r}: walk id {res['walk_id'][-1]:.3f} / rank {res['walk_rank'][-1]:.3f} ms, "
                  f"pairs/s id {res['pps_id'][-1] / 1e6:.2f} M / rank {res['pps_rank'][-1] / 1e6:.2f} M, "
                  f"offline id {res['off_id'][-1]:.1f} / rank {res['off_rank'][-1]:.1f} ms, builder {bms:.1f} ms", flush=True)
        med = {k: statistics.median(v) for k, v in res.items()}
        labels = int(torch.unique(lo.labels).numel())
        rows.append((name, med, labels))
        del lo
    print()
    print("| graph | walk ms, id order | walk ms, rank order | change | step M pairs/s, id | step M pairs/s, rank | change | "
          "offline all-N ms, id | offline ms, rank | builder ms | labels |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for name, m, labels in rows:
        print(f"| {name} | {m['walk_id']:.3f} | {m['walk_rank']:.3f} | {100 * (m['walk_rank'] / m['walk_id'] - 1):+.1f} % | "
              f"{m['pps_id'] / 1e6:.2f} | {m['pps_rank'] / 1e6:.2f} | {100 * (m['pps_rank'] / m['pps_id'] - 1):+.1f} % | "
              f"{m['off_id']:.1f} | {m['off_rank']:.1f} | {m['build']:.1f} | {labels:,} |")


if __name__ == "__main__":
    main()

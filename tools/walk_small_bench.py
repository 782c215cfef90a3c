#!/usr/bin/env python3
"""Dev-only: the one-wave key-row kernel of the small walk shapes (csrc/walk_small.hip) and the on-demand stages over its rows, on
the cit2-like graph of bench.py.

    python tools/walk_small_bench.py [--parts=walk,stage] [--roots=2048,131072] [--B=1024,65536] [--steps=20] [--warmup=5] [--rounds=5]
        walk    the walk alone, Philox: subgacc_walk_keyrows_small against subgacc_walk_spg with a table of distinct rows -- the table
                form, which the general kernel (walk_sets_kernel<SPG>) runs at these shapes -- at (M, m) = (100, 2) and (50, 1).  The
                two sides do not write the same thing: the table form also registers every set's LP keys in the table of distinct
                rows (global atomics), the key rows carry the keys themselves.  That is the choice a step has at these shapes.
        stage   sample_and_mean_stage and sample_and_hmean_stage at (100, 2), H = 96, through StepBuffers(stage="counts"), against
                the buffered row-form step (the table form on the general kernel) followed by the reference form on its xz
                (embed(xz).sum(-2), segment mean): forward, and forward + backward.

The two sides of every comparison alternate: --rounds rounds of (side A: --steps steps, side B: --steps steps) after --warmup steps of
each, every region between device events; the figure is the median over the rounds, the spread is (min .. max).  The reference form
reads the row count back once per step (its xz is exactly R rows), inside its regions."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
H = 96
WALK_SHAPES = ((100, 2), (50, 1))
STAGE_SHAPE = (100, 2)


def _ab(sides, K, W, rounds):
    """{name: (median ms per step, min, max)} of the sides, alternated round by round"""
    import torch
    for f in sides.values():
        for _ in range(W):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for name, f in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(K):
                f()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / K)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def _line(label, r, unit, per):
    med, lo, hi = r
    return f"{label:<78} {med:9.4f} ms ({lo:.4f} .. {hi:.4f})  {per / med / 1e3:8.2f} M {unit}/s"


def part_walk(sp, csr, dev, n, K, W, rounds):
    import torch
    from surel_plus_amd import _lib, sampler
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    q = torch.randint(0, csr.num_nodes, (n,), device=dev, generator=torch.Generator(device=dev).manual_seed(9400 + n)).to(torch.int32)
    for M, m in WALK_SHAPES:
        Q = M * m + 1
        P = (Q + 31) // 32 * 32                      # the step's pitch: whole 128-byte lines
        cfg = sampler.make_cfg(csr, M, m, -1, 111413, "philox", records=False, row_pitch=P)
        ids = torch.empty(n * P, dtype=torch.int32, device=dev)
        pay = torch.empty(n * P, dtype=torch.int32, device=dev)
        ids2, pay2 = torch.empty_like(ids), torch.empty_like(pay)
        ns, ns2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        flags = torch.zeros(4, dtype=torch.int32, device=dev)
        cap = 1 << 17
        table = torch.empty(L.subgacc_uniq_table_bytes(cap), dtype=torch.uint8, device=dev)
        _lib.check(L.subgacc_uniq_reset(ptr(table), cap, st))
        g = (cfg, ptr(csr.indptr), ptr(csr.indices), csr.num_nodes, ptr(q), n)

        def small():
            _lib.check(L.subgacc_walk_keyrows_small(*g, None, None, None, None, ptr(ids), ptr(pay), ptr(ns), ptr(flags), st))

        def general():
            _lib.check(L.subgacc_walk_spg(*g, 0, None, None, ptr(table), cap, ptr(ids2), ptr(pay2), ptr(ns2), ptr(flags), st))

        r = _ab({"small": small, "general": general}, K, W, rounds)
        torch.cuda.synchronize()
        assert torch.equal(ns, ns2) and not flags.any(), "the two kernels disagree"
        member = torch.arange(P, device=dev)[None, :] < ns[:, None]
        assert torch.equal(ids.view(n, P)[member], ids2.view(n, P)[member]), "the two kernels disagree"
        members = int(ns.to(torch.int64).sum())
        print(_line(f"walk  M={M:>3} m={m} roots={n:>6}  subgacc_walk_keyrows_small (one wave per root)", r["small"], "roots", n), flush=True)
        print(_line(f"walk  M={M:>3} m={m} roots={n:>6}  subgacc_walk_spg, table form (walk_sets_kernel<SPG>)", r["general"], "roots", n), flush=True)
        print(f"walk  M={M:>3} m={m} roots={n:>6}  general / small = {r['general'][0] / r['small'][0]:.2f}x   ({members / n:.1f} members a set, "
              f"equal ids and sizes)", flush=True)


def _embed(dev, k):
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)


def part_stage(sp, csr, dev, B, K, W, rounds, T, triplets):
    import torch
    from surel_plus_amd.graphs import query_pairs
    M, m = STAGE_SHAPE
    kw = dict(num_walks=M, num_steps=m)
    blocks = 4 if triplets else 2
    if triplets:
        gen = torch.Generator(device=dev)
        es = [torch.randint(0, csr.num_nodes, (3, B), device=dev, generator=gen.manual_seed(9500 + s)) for s in range(4)]
    else:
        es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    name = "sample_and_hmean_stage" if triplets else "sample_and_mean_stage"
    embed = _embed(dev, m + 1)
    wgt = torch.randn(blocks, B, H, device=dev)
    cb = sp.StepBuffers(csr, B, stage="counts", table_rows=T, triplets=triplets, **kw)
    rb = sp.StepBuffers(csr, B, triplets=triplets, **kw)
    assert cb.small and not rb.keyrows
    it = [0]

    def stage(e):
        return (sp.sample_and_hmean_stage if triplets else sp.sample_and_mean_stage)(csr, e, embed, buffers=cb, **kw)

    def reference(e):
        if triplets:
            xz, ids, _ = sp.sample_and_hgather(csr, e, buffers=rb, **kw)
            seg = ids.seg_pointers
        else:
            xz, seg, _ = sp.sample_and_gather(csr, e, buffers=rb, **kw)
        n = seg[1:] - seg[:-1]
        R = int(seg[-1])            # (the reference reads the row count: its xz is exactly R rows)
        x = embed(xz[:R]).sum(dim=-2)
        sid = torch.repeat_interleave(torch.arange(blocks * B, device=dev), n, output_size=R)
        return (torch.zeros(blocks * B, H, device=dev).index_add_(0, sid, x) / n.clamp(min=1)[:, None]).view(blocks, B, H)

    for train in (False, True):
        what = "forward + backward" if train else "forward"

        def run(f):
            e = es[it[0] % 4]
            it[0] += 1
            if not train:
                with torch.no_grad():
                    return f(e)
            for p in embed.parameters():
                p.grad = None
            (f(e) * wgt).sum().backward()

        try:
            r = _ab({"stage": lambda: run(stage), "reference": lambda: run(reference)}, K, W, rounds)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            r = _ab({"stage": lambda: run(stage)}, K, W, rounds)
            print(_line(f"stage {name} B={B:>6} T={T}  stage step, {what}", r["stage"], "items", B), flush=True)
            print(f"stage {name} B={B:>6}  {what}: the reference form's activations do not fit at this size: the stage step alone", flush=True)
            continue
        print(_line(f"stage {name} B={B:>6} T={T}  stage step, {what}", r["stage"], "items", B), flush=True)
        print(_line(f"stage {name} B={B:>6}  row-form step + reference form on xz, {what}", r["reference"], "items", B), flush=True)
        print(f"stage {name} B={B:>6}  {what}: reference / stage = {r['reference'][0] / r['stage'][0]:.2f}x", flush=True)
    with torch.no_grad():
        a, b = stage(es[0]), reference(es[0])
    cb.sets.resolve()
    print(f"stage {name} B={B:>6}  distinct LP rows of the batch: {int(cb.status[2]):,} (table_rows = {T}); largest difference between the two "
          f"forms {float((a - b).abs().max()):.2e} of {float(b.abs().max()):.2e}", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W, rounds = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5")), int(OPTS.get("rounds", "5"))
    T = int(OPTS.get("table_rows", "4096"))
    parts = OPTS.get("parts", "walk,stage").split(",")
    csr = preset_graph("cit2", device=dev)
    props = torch.cuda.get_device_properties(0)
    print(f"walk_small_bench: {props.name}, {props.multi_processor_count} CUs, torch {torch.__version__}; cit2-like graph N={csr.num_nodes:,}; "
          f"sides alternated, median (min .. max) of {rounds} rounds of {K} steps after {W} warm-up steps, device events", flush=True)
    if "walk" in parts:
        for n in (int(v) for v in OPTS.get("roots", "2048,131072").split(",")):
            part_walk(sp, csr, dev, n, K, W, rounds)
    if "stage" in parts:
        for B in (int(v) for v in OPTS.get("B", "1024,65536").split(",")):
            for triplets in (False, True):
                part_stage(sp, csr, dev, B, K, W, rounds, T, triplets)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the row-form on-demand step at the small walk shapes with and without small_rows=True, and its 16-bit rows, on the
cit2-like graph of bench.py.

    python tools/small_step_bench.py [--parts=step,dedup,triplets,half] [--B=1024,8192,65536] [--steps=20] [--warmup=5] [--rounds=5]
        step      the buffered f32 step (pairs, segment pointers) at (M, m) = (100, 2) and (50, 1): StepBuffers(small_rows=True) -- the
                  one-wave kernel's key rows under the KEY32 join -- against the same StepBuffers without the keyword -- the general
                  kernel's table form, subgacc_unpack_lp and the SFPTR join.
        dedup     an evaluation-shaped batch (every source against 1,000 targets, utils.py:92-95): small_rows=True with and without
                  dedup_roots=True, and the step without the keyword (which refuses root dedup at these shapes).
        triplets  sample_and_hgather at (100, 2), B = 2,048 (main_horder.py:33) and 65,536, with and without the keyword.
        half      all sides with the keyword: the dtype=torch.bfloat16 step against the f32 step, with segment pointers and with
                  segment ids; and the launch of subgacc_sjoin_fill_half_ids against subgacc_sjoin_fill_v2 with out_segid over the same
                  rows, beside the byte model per member (8 read + 4k + 8 written against 8 + 8k + 8: 0.70 at k = 3, 0.75 at k = 2).

The sides of every comparison alternate in one process and one library: --rounds rounds of (--steps steps of each side) after --warmup
steps of each, every region between device events; the figure is the median over the rounds with (min .. max).  A side counts as
faster only beyond the other side's own spread: the verdict column says `faster`, `slower` or `level`.  The per-launch lines come from
a separate pass of --steps steps per side with sampler.KERNEL_TIMER set (device events around the walk and the join): mean per launch."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
SHAPES = ((100, 2), (50, 1))
TRIPLET_SHAPE = (100, 2)


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


class LaunchTimer:
    """sampler.KERNEL_TIMER: device events around every timed launch -> {name: mean ms}"""

    def __init__(self):
        self.events = []

    def __call__(self, name):
        import torch
        timer = self

        class Region:
            def __enter__(self):
                self.a = torch.cuda.Event(enable_timing=True)
                self.a.record()

            def __exit__(self, *exc):
                b = torch.cuda.Event(enable_timing=True)
                b.record()
                timer.events.append((name, self.a, b))
                return False

        return Region()

    def means(self):
        import torch
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.events:
            out.setdefault(name, []).append(a.elapsed_time(b))
        return {k: sum(v) / len(v) for k, v in out.items()}


def _launches(f, K):
    from surel_plus_amd import sampler
    f()
    timer = sampler.KERNEL_TIMER = LaunchTimer()
    try:
        for _ in range(K):
            f()
        return timer.means()
    finally:
        sampler.KERNEL_TIMER = None


def _verdict(a, b):
    """side a against side b: beyond b's own spread, and b beyond a's"""
    if a[2] < b[1]:
        return "faster"
    if a[1] > b[2]:
        return "slower"
    return "level"


def _line(label, r):
    med, lo, hi = r
    return f"{label:<96} {med:9.4f} ms ({lo:.4f} .. {hi:.4f})"


def _compare(head, names, r, base):
    for n in names:
        print(_line(f"{head}  {n}", r[n]), flush=True)
    for n in names:
        if n != base:
            print(f"{head}  {n} / {base} = {r[n][0] / r[base][0]:.2f}  ->  {_verdict(r[n], r[base])}", flush=True)


def _per_launch(head, sides, K):
    for n, f in sides.items():
        m = _launches(f, K)
        print(f"{head}  per launch, {n}: " + ", ".join(f"{k} {v:.4f} ms" for k, v in m.items()), flush=True)


def _eval_batch(csr, B, dev, seed):
    """[2, B] pairs: every source against 1,000 targets"""
    import torch
    gen = torch.Generator(device=dev).manual_seed(seed)
    src = torch.randint(0, csr.num_nodes, ((B + 999) // 1000,), device=dev, generator=gen)
    return torch.stack([src.repeat_interleave(1000)[:B], torch.randint(0, csr.num_nodes, (B,), device=dev, generator=gen)])


def part_step(sp, csr, dev, B, K, W, rounds):
    from surel_plus_amd.graphs import query_pairs
    for M, m in SHAPES:
        kw = dict(num_walks=M, num_steps=m)
        es = [query_pairs(csr, B, seed=9600 + s, device=dev) for s in range(4)]
        new, old = sp.StepBuffers(csr, B, small_rows=True, **kw), sp.StepBuffers(csr, B, **kw)
        assert new.small and not old.keyrows
        it = [0]

        def run(bufs, small):
            it[0] += 1
            return sp.sample_and_gather(csr, es[it[0] % 4], buffers=bufs, small_rows=small, **kw)

        sides = {"small_rows=True": lambda: run(new, True), "table form": lambda: run(old, False)}
        head = f"step     M={M:>3} m={m} B={B:>6}"
        _compare(head, list(sides), _ab(sides, K, W, rounds), "table form")
        _per_launch(head, sides, K)


def part_dedup(sp, csr, dev, B, K, W, rounds):
    for M, m in SHAPES:
        kw = dict(num_walks=M, num_steps=m)
        es = [_eval_batch(csr, B, dev, 9700 + s) for s in range(4)]
        dd = sp.StepBuffers(csr, B, small_rows=True, dedup_roots=True, **kw)
        new, old = sp.StepBuffers(csr, B, small_rows=True, **kw), sp.StepBuffers(csr, B, **kw)
        it = [0]

        def run(bufs, small, dedup):
            it[0] += 1
            return sp.sample_and_gather(csr, es[it[0] % 4], buffers=bufs, small_rows=small, dedup_roots=dedup, **kw)

        sides = {"small_rows=True, dedup_roots=True": lambda: run(dd, True, True), "small_rows=True": lambda: run(new, True, False),
                 "table form": lambda: run(old, False, False)}
        head = f"dedup    M={M:>3} m={m} B={B:>6} (evaluation batch)"
        _compare(head, list(sides), _ab(sides, K, W, rounds), "table form")
        _per_launch(head, sides, K)


def part_triplets(sp, csr, dev, B, K, W, rounds):
    import torch
    M, m = TRIPLET_SHAPE
    kw = dict(num_walks=M, num_steps=m)
    gen = torch.Generator(device=dev)
    hs = [torch.randint(0, csr.num_nodes, (3, B), device=dev, generator=gen.manual_seed(9800 + s)) for s in range(4)]
    new, old = sp.StepBuffers(csr, B, triplets=True, small_rows=True, **kw), sp.StepBuffers(csr, B, triplets=True, **kw)
    it = [0]

    def run(bufs, small):
        it[0] += 1
        return sp.sample_and_hgather(csr, hs[it[0] % 4], buffers=bufs, small_rows=small, **kw)

    sides = {"small_rows=True": lambda: run(new, True), "table form": lambda: run(old, False)}
    head = f"triplets M={M:>3} m={m} B={B:>6}"
    _compare(head, list(sides), _ab(sides, K, W, rounds), "table form")
    _per_launch(head, sides, K)


def part_half(sp, csr, dev, B, K, W, rounds):
    import torch
    from surel_plus_amd.graphs import query_pairs
    for M, m in SHAPES:
        k = m + 1
        kw = dict(num_walks=M, num_steps=m, small_rows=True)
        es = [query_pairs(csr, B, seed=9900 + s, device=dev) for s in range(4)]
        for ptr in (True, False):
            f32 = sp.StepBuffers(csr, B, ptr=ptr, **kw)
            b16 = sp.StepBuffers(csr, B, ptr=ptr, dtype=torch.bfloat16, **kw)
            it = [0]

            def run(bufs, dtype):
                it[0] += 1
                return sp.sample_and_gather(csr, es[it[0] % 4], buffers=bufs, ptr=ptr, dtype=dtype, **kw)

            sides = {"dtype=torch.bfloat16": lambda: run(b16, torch.bfloat16), "f32": lambda: run(f32, None)}
            head = f"half     M={M:>3} m={m} B={B:>6} {'segment pointers' if ptr else 'segment ids     '}"
            _compare(head, list(sides), _ab(sides, K, W, rounds), "f32")
            if not ptr:     # the two fills over the same rows (the steps above alternate over the same four batches)
                a, b = _launches(sides["dtype=torch.bfloat16"], K), _launches(sides["f32"], K)
                model = (8 + 4 * k + 8) / (8 + 8 * k + 8)
                print(f"{head}  launch: subgacc_sjoin_fill_half_ids {a['sjoin_fill_half_ids']:.4f} ms, subgacc_sjoin_fill_v2 with out_segid "
                      f"{b['sjoin_fill']:.4f} ms: ratio {a['sjoin_fill_half_ids'] / b['sjoin_fill']:.2f} (byte model {model:.2f}); walk "
                      f"{a['walk_sets']:.4f} / {b['walk_sets']:.4f} ms", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W, rounds = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5")), int(OPTS.get("rounds", "5"))
    parts = OPTS.get("parts", "step,dedup,triplets,half").split(",")
    csr = preset_graph("cit2", device=dev)
    props = torch.cuda.get_device_properties(0)
    print(f"small_step_bench: {props.name}, {props.multi_processor_count} CUs, torch {torch.__version__}; cit2-like graph N={csr.num_nodes:,}; "
          f"sides alternated, median (min .. max) of {rounds} rounds of {K} buffered steps after {W} warm-up steps, device events; Philox", flush=True)
    Bs = [int(v) for v in OPTS.get("B", "1024,8192,65536").split(",")]
    for part, fn in (("step", part_step), ("dedup", part_dedup), ("half", part_half)):
        if part in parts:
            for B in Bs:
                fn(sp, csr, dev, B, K, W, rounds)
    if "triplets" in parts:
        for B in (int(v) for v in OPTS.get("triplets_B", "2048,65536").split(",")):
            part_triplets(sp, csr, dev, B, K, W, rounds)
    print("not measured: kernel counters, rng='rand_r', 3 and 4 hops, bench.py (it does not reach this code)", flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the on-demand stages over 64-bit key rows (wide_keys=True) on the cit2-like graph of bench.py at the paper's citation2
sampler setting, M = 200, 4 hops (the `cit2m4` workload), H = 96.  Made like tools/step_stage_bench.py: the same warm-up, the same
statistic.

    python tools/wide_stage_bench.py [--B=1024,4096,65536] [--steps=20] [--warmup=5] [--parts=a,b] [--table_rows=8192]
        a   sample_and_mean_stage(wide_keys=True) through StepBuffers(stage="counts", wide_keys=True) against the only route there was:
            the buffered 4-hop row-form step followed by the reference form on its xz (embed(xz).sum(-2), segment mean) -- forward and
            forward + backward, peak memory of either; where the reference form does not fit, the stage step alone.  Then the
            distinct LP rows of the batch: whether the 8,192-column limit binds
        b   subgacc_keyrows_columns64 alone over the step's rows (device events around the call: scan + finish + translate), the same
            call over no rows (the finish kernel alone), and subgacc_keyrows_columns over the 3-hop step of the same batch, per byte of
            keys read; the walk and the count kernel of the step beside them.  The split of the three launches is the kernel trace's
            (rocprofv3 --kernel-trace --stats over this part)

Every step time is the median of three regions of --steps steps after --warmup steps, between device events."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("SUBGACC_QUIET", "1")
from step_stage_bench import _fmt, _KernelTimer, _peak, _regions  # noqa: E402

M, HOPS, H = 200, 4, 96
HBM_PEAK = 8.0e12           # bytes / s (MI355X)
REF_MAX_B = 4096            # the reference form's [R,2,H] activations fit up to here


def _embed(dev):
    import torch
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(HOPS + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)


def _steps(sp, csr, dev, B, T, embed, train):
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

    cb = sp.StepBuffers(csr, B, stage="counts", table_rows=T, wide_keys=True, **kw)
    rb = sp.StepBuffers(csr, B, **kw) if B <= REF_MAX_B else None

    def stage(e):
        return sp.sample_and_mean_stage(csr, e, embed, buffers=cb, wide_keys=True, **kw)

    def reference(e):
        xz, seg, sets = sp.sample_and_gather(csr, e, buffers=rb, **kw)
        n = seg[1:] - seg[:-1]
        R = int(seg[-1])            # (the reference reads the row count: its xz is exactly R rows)
        x = embed(xz[:R]).sum(dim=-2)
        ids = torch.repeat_interleave(torch.arange(2 * B, device=dev), n, output_size=R)
        return (torch.zeros(2 * B, H, device=dev).index_add_(0, ids, x) / n.clamp(min=1)[:, None]).view(2, B, H)
    return (lambda: run(stage)), ((lambda: run(reference)) if rb is not None else None), cb


def part_a(sp, csr, dev, B, K, W, T):
    from surel_plus_amd.graphs import query_pairs
    embed = _embed(dev)
    for train in (False, True):
        what = "forward + backward" if train else "forward"
        stage, ref, cb = _steps(sp, csr, dev, B, T, embed, train)
        med, ms = _regions(stage, K, W)
        pk = _peak(stage)
        print(_fmt(f"(a) B={B:>6} T={T}  wide stage step, {what}", med, ms, B) + f"   peak above the buffers {pk:9.1f} MB", flush=True)
        if ref is None:
            print(f"(a) B={B:>6}  the reference form is not run at this size ([R,2,H] activations): the stage step alone; its buffers: "
                  f"counts {cb.counts.numel() * 4 / 1e6:.0f} MB, ids {cb.ids.numel() * 4 / 1e6:.0f} MB, 64-bit keys "
                  f"{cb.slot.numel() * 8 / 1e6:.0f} MB, surrogates {cb.cols.numel() * 4 / 1e6:.0f} MB", flush=True)
            continue
        medr, msr = _regions(ref, K, W)
        pkr = _peak(ref)
        print(_fmt(f"(a) B={B:>6}  row-form step + reference form on xz, {what}", medr, msr, B) + f"   peak above the buffers {pkr:9.1f} MB"
              "   (reads the row count back every step)", flush=True)
        print(f"(a) B={B:>6}  {what}: reference / stage = {medr / med:.2f}x", flush=True)
    cb = _steps(sp, csr, dev, B, T, embed, False)[2]
    for s in range(4):
        sp.sample_and_counts(csr, query_pairs(csr, B, seed=9300 + s, device=dev), num_walks=M, num_steps=HOPS, buffers=cb, wide_keys=True)
        st = cb.status.tolist()
        print(f"(a) B={B:>6}  batch {s}: distinct LP rows kept {int(st[2]):,} of at most {T - 1:,} columns; more than that (flags[2] & 1): "
              f"{bool(int(st[1]) & 1)}", flush=True)


def _call_ms(fn, n=20):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def part_b(sp, sampler_mod, csr, dev, B, T):
    import torch
    from surel_plus_amd import _lib
    from surel_plus_amd.graphs import query_pairs
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    e = query_pairs(csr, B, seed=9300, device=dev)
    wb = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS, stage="counts", table_rows=T, wide_keys=True)
    nb = sp.StepBuffers(csr, B, num_walks=M, num_steps=3, stage="counts", table_rows=T)
    timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
    for _ in range(10):
        sp.sample_and_counts(csr, e, num_walks=M, num_steps=HOPS, buffers=wb, wide_keys=True)
    walk, col, cnt = (timer.median_ms(k) for k in ("walk_sets", "keyrows_columns64", "sjoin_key_counts"))
    timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
    for _ in range(10):
        sp.sample_and_counts(csr, e, num_walks=M, num_steps=3, buffers=nb)
    walk3, col3, cnt3 = (timer.median_ms(k) for k in ("walk_sets", "keyrows_columns", "sjoin_key_counts"))
    sampler_mod.KERNEL_TIMER = None
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def wide(n):
        _lib.check(L.subgacc_keyrows_columns64(ptr(wb.slot), ptr(wb.nsize), n, wb.stride, M, HOPS, T, ptr(wb.ukeys64), ptr(wb.ukeys),
                                               ptr(count), ptr(wb.feat), ptr(wb.cols), ptr(flags), ptr(wb.col_ws), wb.col_ws.numel(), st()))

    def narrow(n):
        _lib.check(L.subgacc_keyrows_columns(ptr(nb.slot), ptr(nb.nsize), n, nb.stride, M, 3, T, ptr(nb.ukeys), ptr(count), ptr(nb.feat),
                                             ptr(flags), ptr(nb.col_ws), nb.col_ws.numel(), st()))
    w_all, w_fin = _call_ms(lambda: wide(wb.n)), _call_ms(lambda: wide(0))
    n_all, n_fin = _call_ms(lambda: narrow(nb.n)), _call_ms(lambda: narrow(0))
    mw, mn = int(wb.nsize.to(torch.int64).sum()), int(nb.nsize.to(torch.int64).sum())
    print(f"(b) B={B:>6} T={T}  inside the step, 4 hops: walk {walk:.4f} ms | columns64 {col:.4f} ms | count kernel over the surrogates "
          f"{cnt:.4f} ms || 3 hops: walk {walk3:.4f} ms | columns {col3:.4f} ms | count kernel {cnt3:.4f} ms", flush=True)
    print(f"(b) B={B:>6} T={T}  subgacc_keyrows_columns64, {mw:,} members: {w_all:.4f} ms for the three launches, {w_fin:.4f} ms for the "
          f"finish kernel alone (n = 0); keys read twice: {16 * mw / 1e6:.1f} MB + {4 * mw / 1e6:.1f} MB written = "
          f"{20 * mw / w_all / 1e9:.2f} TB/s ({20 * mw / w_all / 1e-3 / HBM_PEAK:.1%} of the HBM peak); "
          f"{w_all / (8 * mw / 1e6) * 1e3:.3f} us per MB of keys", flush=True)
    print(f"(b) B={B:>6} T={T}  subgacc_keyrows_columns (3 hops), {mn:,} members: {n_all:.4f} ms for the two launches, {n_fin:.4f} ms for the "
          f"finish kernel alone; {4 * mn / 1e6:.1f} MB of keys = {4 * mn / n_all / 1e9:.2f} TB/s; "
          f"{n_all / (4 * mn / 1e6) * 1e3:.3f} us per MB of keys", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5"))
    T = int(OPTS.get("table_rows", "8192"))
    shapes = [int(b) for b in OPTS.get("B", "1024,4096,65536").split(",")]
    parts = OPTS.get("parts", "a,b").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"wide_stage_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops (64-bit LP keys), H = {H}; median of three regions "
          f"of {K} steps after {W} warm-up steps, device events", flush=True)
    for B in shapes:
        if "a" in parts:
            part_a(sp, csr, dev, B, K, W, T)
        if "b" in parts:
            part_b(sp, sampler_mod, csr, dev, B, T)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

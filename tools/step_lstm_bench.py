#!/usr/bin/env python3
"""Dev-only: the LP encoder's LSTM first stage on the on-demand step (sample_and_lstm_stage through StepBuffers(stage="index")) on the
cit2-like graph of bench.py, M = 200, 3 hops, H = H' = 96.

    python tools/step_lstm_bench.py [--B=1024,4096] [--steps=20] [--warmup=5] [--ref_steps=3] [--parts=a,b,c,k] [--table_rows=2048]
        a   the stage step with buffers: forward and forward + backward, peak memory above its buffers
        b   the route the stage replaces: the buffered row-form step (key rows; writes xz, which nothing reads), StridedSpG(sets).to_csr()
            (registers the step's keys, copies the rows packed) and index_lstm_stage over that copy
        c   the buffered row-form step, the same packed copy and lstm_stage (the reference form: dense [S, L, H] batch, nn.LSTM), where
            it fits (the LSTM's reserve space below 2^31 words: B <= 3,101 here); --ref_steps steps per region, one warm-up step
        k   sjoin_key_index's kernel next to the row-form fill of the same batch (device events around the launches), 8 against 8 k
            bytes per row

Every step time is the median of three regions of --steps steps after --warmup steps, between device events.  Every route reads
words back inside a region: the stage its two (R, L), the others what their registration, packed copy and checks read."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_stage_bench import H, HBM_PEAK, HOPS, M, OPTS, _fmt, _KernelTimer, _peak, _regions  # noqa: E402


REF_WORDS = 6       # words per hidden unit, segment and step that the vendor LSTM keeps (four gates, cell state, hidden state)


def _nets(dev):
    import torch
    torch.manual_seed(0)
    embed = torch.nn.Sequential(torch.nn.Linear(HOPS + 1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev)
    return embed, torch.nn.LSTM(H, H, batch_first=True).to(dev)


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


def _mb(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors if t is not None) / 1e6


def parts_abc(sp, csr, dev, B, K, W, KR, T, parts):
    import torch
    nets = _nets(dev)
    embed, lstm = nets
    kw = dict(num_walks=M, num_steps=HOPS)
    rows = torch.arange(2 * B, device=dev).view(2, B)       # row i of a step's rows = endpoint i of [u | v]
    for train in (False, True):
        what = "forward + backward" if train else "forward"
        run = _runner(csr, dev, B, nets, train)
        if "a" in parts:
            ib = sp.StepBuffers(csr, B, stage="index", table_rows=T, **kw)
            step = lambda: run(lambda e: sp.sample_and_lstm_stage(csr, e, embed, lstm, buffers=ib, **kw))      # noqa: E731
            med, ms = _regions(step, K, W)
            print(_fmt(f"(a) B={B:>6} T={T}  lstm stage step, {what}", med, ms, B) + f"   peak above the buffers {_peak(step):9.1f} MB",
                  flush=True)
            try:
                ib.sets.resolve()
            except sp.SubgAccError as err:      # more distinct LP rows than table rows: the times stand, the result would not
                print(f"(a) B={B:>6} T={T}  OVERFLOW: {err}", flush=True)
            print(f"(a) B={B:>6} T={T}  distinct LP rows of the last batch: {int(ib.status[2]):,}; rows of the last batch {int(ib.seg[-1]):,}, "
                  f"longest segment {int(ib.sizes.max())}; buffers: pairs {_mb(ib.pairs):.0f} MB, rows {_mb(ib.ids, ib.slot):.0f} MB", flush=True)
            del ib
        for part, stage, k, w in (("b", sp.index_lstm_stage, K, W), ("c", sp.lstm_stage, KR, 1)):
            if part not in parts:
                continue
            if part == "c" and 2 * B * (M * HOPS + 1) * REF_WORDS * H >= 1 << 31:
                # nn.LSTM's reserve space holds REF_WORDS * H' words per (segment, step): past 2^31 words its 32-bit offsets wrap
                # (B = 4,096 faulted in it, in the forward alone) -- the reference form is not run where it does not fit
                if not train:
                    print(f"(c) B={B:>6}  the reference form does not fit: [2B, L, {REF_WORDS} H'] words of the LSTM's reserve space "
                          f"reach 2^31 from B = {((1 << 31) // ((M * HOPS + 1) * REF_WORDS * H)) // 2 + 1:,} on", flush=True)
                continue
            rb = sp.StepBuffers(csr, B, **kw)

            def detour(e):
                _, _, sets = sp.sample_and_gather(csr, e, buffers=rb, **kw)
                z = sp.StridedSpG(sets, csr.num_nodes).to_csr()
                return stage(rows, z, sets.feature_table(), embed, lstm)
            step = lambda: run(detour)       # noqa: E731
            name = "index_lstm_stage" if part == "b" else "lstm_stage (reference form)"
            try:
                med, ms = _regions(step, k, w)
                print(_fmt(f"({part}) B={B:>6}  row-form step + to_csr + {name}, {what}", med, ms, B) +
                      f"   peak above the buffers {_peak(step):9.1f} MB", flush=True)
            except torch.OutOfMemoryError:
                print(f"({part}) B={B:>6}  row-form step + to_csr + {name}, {what}: does not fit in memory", flush=True)
            if not train:
                print(f"({part}) B={B:>6}  buffers: xz {_mb(rb.out):.0f} MB, rows {_mb(rb.ids, rb.slot):.0f} MB", flush=True)
            del rb
            torch.cuda.empty_cache()


def part_k(sp, sampler_mod, csr, dev, B, T, n=20):
    from surel_plus_amd.graphs import query_pairs
    kw = dict(num_walks=M, num_steps=HOPS)
    e = query_pairs(csr, B, seed=9300, device=dev)
    ib, rb = sp.StepBuffers(csr, B, stage="index", table_rows=T, **kw), sp.StepBuffers(csr, B, **kw)
    timer = sampler_mod.KERNEL_TIMER = _KernelTimer()
    for _ in range(n):
        sp.sample_and_index(csr, e, buffers=ib, **kw)
        sp.sample_and_gather(csr, e, buffers=rb, **kw)
    idx, col, fill, walk = (timer.median_ms(k) for k in ("sjoin_key_index", "keyrows_columns", "sjoin_fill", "walk_sets"))
    sampler_mod.KERNEL_TIMER = None
    try:
        ib.sets.resolve()
    except sp.SubgAccError as err:
        print(f"(k) B={B:>6} T={T}  OVERFLOW: {err}", flush=True)
    R = int(ib.seg[-1])
    row_b, idx_b, xz_b = 8 * R, 8 * R, 8 * (HOPS + 1) * R
    line = lambda ms, out: f"{ms:.4f} ms: rows {row_b / 1e6:.1f} MB + output {out / 1e6:.1f} MB = {(row_b + out) / ms / 1e9:.2f} TB/s " \
                           f"({(row_b + out) / ms / 1e-3 / HBM_PEAK:.1%} of the HBM peak)"       # noqa: E731
    print(f"(k) B={B:>6} T={T}  {int(ib.status[2]):,} distinct LP rows, {R:,} output rows; walk {walk:.4f} ms, columns pass {col:.4f} ms",
          flush=True)
    print(f"(k) B={B:>6} T={T}  sjoin_key_index (8 B / row)      {line(idx, idx_b)}", flush=True)
    print(f"(k) B={B:>6} T={T}  row-form fill   ({8 * (HOPS + 1)} B / row)     {line(fill, xz_b)}", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    K, W, KR = int(OPTS.get("steps", "20")), int(OPTS.get("warmup", "5")), int(OPTS.get("ref_steps", "3"))
    T = int(OPTS.get("table_rows", "2048"))
    shapes = [int(b) for b in OPTS.get("B", "1024,4096").split(",")]
    parts = OPTS.get("parts", "a,b,c,k").split(",")
    csr = preset_graph("cit2", device=dev)
    print(f"step_lstm_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops, H = H' = {H}, table_rows = {T}; median of three "
          f"regions of {K} steps after {W} warm-up steps (part c: {KR} steps after 1), device events", flush=True)
    for B in shapes:
        parts_abc(sp, csr, dev, B, K, W, KR, T, parts)
        if "k" in parts:
            part_k(sp, sampler_mod, csr, dev, B, T)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the step's packed one-word rows joined in bf16 / fp16 (subgacc_sjoin_fill_packed_half) against the forms the library had
before it, on the cit2-like graph of bench.py at M = 200 and 3 hops (k = 4, 16-byte rows).  The yardstick is the TWO-PLANE half form
-- subgacc_sjoin_fill_half, StepBuffers(dtype=bf16) -- in the same library and the same run.

    python tools/packed_half_bench.py [--B=1024,8192,65536] [--rounds=40] [--warmup=10] [--steps=20] [--parts=a,b] [--M=200] [--hops=3]
        (a) the join launch alone, device events around every launch, four forms ALTERNATING inside every round over the rows of the
            same sets (two StepBuffers stepped with the same seed and batch, one packed and one not):
              2p-bf16   subgacc_sjoin_fill_half over the two planes            (the parent's 16-bit form: the yardstick)
              pk-f32    subgacc_sjoin_fill_packed over the packed rows         (the parent's packed form)
              pk-bf16   subgacc_sjoin_fill_packed_half, bf16
              pk-fp16   subgacc_sjoin_fill_packed_half, fp16
            median, quartiles, min .. max of --rounds launches each after --warmup rounds, and the bytes per member; a ratio is to be
            read against the spread of the two-plane form in the same run (its interquartile range over its median): inside it the
            two are level
        (b) the whole buffered step (sample_and_gather through StepBuffers): dtype=bf16 against dtype=bf16, packed_half=True, regions
            of --steps steps, the two alternating, three regions each after --warmup steps

Bytes per member: two planes 8 read; packed 4 (1 + e / n) read with e escapes in n members (counted from the step's nesc); 8k written
in f32, 4k in 16 bits.  A library built with -DSJ_PACKHALF_THREADS=128 / 256 (SUBGACC_LIB=...) forces the lanes of a pair's workgroup
at pitches up to 640."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
M, HOPS = int(OPTS.get("M", "200")), int(OPTS.get("hops", "3"))
K = HOPS + 1
HBM_PEAK = 8.0e12           # bytes / s (MI355X)
NAMES = ("2p-bf16", "pk-f32", "pk-bf16", "pk-fp16")
BASE = NAMES[0]


def _launch_times(launch, rounds, warmup):
    """{name: sorted ms of `rounds` launches}, the forms alternating inside every round"""
    import torch
    for _ in range(warmup):
        for name in NAMES:
            launch[name]()
    torch.cuda.synchronize()
    ev = {name: [] for name in NAMES}
    for _ in range(rounds):
        for name in NAMES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch[name]()
            b.record()
            ev[name].append((a, b))
    torch.cuda.synchronize()
    return {name: sorted(a.elapsed_time(b) for a, b in ev[name]) for name in NAMES}


def _quart(t):
    return t[len(t) // 4], t[len(t) // 2], t[(3 * len(t)) // 4]


def part_a(sp, csr, dev, B, rounds, warmup):
    import ctypes
    import torch
    from surel_plus_amd import _lib, spjoin
    from surel_plus_amd.graphs import query_pairs
    L, st = _lib.lib(), _lib.stream_ptr()
    e = query_pairs(csr, B, seed=9300, device=dev)
    kw = dict(num_walks=M, num_steps=HOPS)
    bu = sp.StepBuffers(csr, B, dtype=torch.bfloat16, **kw)
    bp = sp.StepBuffers(csr, B, dtype=torch.bfloat16, packed_half=True, **kw)
    assert bp.packed and bp.half and not bu.packed
    xz_u, seg_u, su = sp.sample_and_gather(csr, e, buffers=bu, dtype=torch.bfloat16, **kw)
    xz_p, seg_p, spk = sp.sample_and_gather(csr, e, buffers=bp, dtype=torch.bfloat16, **kw)
    su.resolve(), spk.resolve()
    R = int(seg_u[-1].item())
    assert torch.equal(seg_u, seg_p) and torch.equal(xz_u[:R].view(torch.int16), xz_p[:R].view(torch.int16)), "the packed-half step is not the half step"
    esc = int(bp.nesc[bp.nsize > 0].sum().item())
    own, partner = spjoin._arange_segments(B, dev)
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    common = dict(row_len=bu.nsize, n_rows=bu.n, row_stride=bu.stride, own=own, partner=partner, S=bu.S, pair_block=B, num_walks=M, num_steps=HOPS,
                  seg=bu.seg, flags=flags)
    out = {"2p-bf16": torch.empty((R, 2, K), dtype=torch.bfloat16, device=dev), "pk-f32": torch.empty((R, 2, K), dtype=torch.float32, device=dev),
           "pk-bf16": torch.empty((R, 2, K), dtype=torch.bfloat16, device=dev), "pk-fp16": torch.empty((R, 2, K), dtype=torch.float16, device=dev)}
    d2p = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY32, ids=bu._ids, payload=bu._slot, **common)
    dpk32 = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY32, ids=bp._ids, payload=bp._slot, out_xz=out["pk-f32"], **common)
    dpk = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY32, ids=bp._ids, payload=bp._slot, **common)
    ne, N = _lib.ptr(bp.nesc), bp.num_nodes
    launch = {"2p-bf16": lambda: _lib.check(L.subgacc_sjoin_fill_half(ctypes.byref(d2p), _lib.HALF_BF16, _lib.ptr(out["2p-bf16"]), st)),
              "pk-f32": lambda: _lib.check(L.subgacc_sjoin_fill_packed(ctypes.byref(dpk32), ne, N, st)),
              "pk-bf16": lambda: _lib.check(L.subgacc_sjoin_fill_packed_half(ctypes.byref(dpk), ne, N, _lib.HALF_BF16, _lib.ptr(out["pk-bf16"]), st)),
              "pk-fp16": lambda: _lib.check(L.subgacc_sjoin_fill_packed_half(ctypes.byref(dpk), ne, N, _lib.HALF_F16, _lib.ptr(out["pk-fp16"]), st))}
    ts = _launch_times(launch, rounds, warmup)
    f32 = out["pk-f32"]
    assert torch.equal(out["2p-bf16"].view(torch.int16), out["pk-bf16"].view(torch.int16)) and not flags.any()
    assert torch.equal(out["pk-bf16"].view(torch.int16), f32.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(out["pk-fp16"].view(torch.int16), f32.to(torch.float16).view(torch.int16))
    per = {"2p-bf16": 8 + 4 * K, "pk-f32": 4 * (1 + esc / R) + 8 * K, "pk-bf16": 4 * (1 + esc / R) + 4 * K, "pk-fp16": 4 * (1 + esc / R) + 4 * K}
    med = {n: _quart(t)[1] for n, t in ts.items()}
    q1, _, q3 = _quart(ts[BASE])
    spread = (q3 - q1) / med[BASE]
    tag = f"(a) join launch  B={B:>6} k={K} pitch={bu.stride} R={R:>10,} esc/member={esc / R:.4f}"
    for n in NAMES:
        t = ts[n]
        a, _, c = _quart(t)
        byts = R * per[n]
        print(f"{tag}  {n:<7} median {med[n] * 1e3:9.2f} us   q1 {a * 1e3:9.2f}  q3 {c * 1e3:9.2f}  min {t[0] * 1e3:9.2f}  max {t[-1] * 1e3:9.2f}   "
              f"{per[n]:6.2f} B/member = {byts / 1e6:8.1f} MB = {byts / med[n] / 1e9:5.2f} TB/s ({byts / med[n] / 1e-3 / HBM_PEAK:.1%} of the HBM peak)",
              flush=True)
    for n in NAMES[1:]:
        r = med[n] / med[BASE]
        verdict = "level" if abs(r - 1.0) <= spread else ("FASTER" if r < 1.0 else "SLOWER")
        print(f"{tag}  {n} / {BASE} = {r:.3f}   byte ratio {per[n] / per[BASE]:.3f}   ({BASE} interquartile spread {spread:.1%} of its median: {verdict})",
              flush=True)


def part_b(sp, csr, dev, B, steps, warmup):
    import torch
    from surel_plus_amd.graphs import query_pairs
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    kw = dict(num_walks=M, num_steps=HOPS)
    bufs = {"2p-bf16": sp.StepBuffers(csr, B, dtype=torch.bfloat16, **kw), "pk-bf16": sp.StepBuffers(csr, B, dtype=torch.bfloat16, packed_half=True, **kw)}
    it = [0]

    def step(name):
        e = es[it[0] % 4]
        it[0] += 1
        sp.sample_and_gather(csr, e, buffers=bufs[name], dtype=torch.bfloat16, **kw)

    for name in bufs:
        for _ in range(warmup):
            step(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in bufs}
    for _ in range(3):
        for name in bufs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                step(name)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / steps)
    med = {name: sorted(v)[1] for name, v in ms.items()}
    base = ms["2p-bf16"]
    spread = (max(base) - min(base)) / med["2p-bf16"]
    for name in bufs:
        print(f"(b) buffered step  B={B:>6} k={K}  {name:<7} {med[name]:9.4f} ms / step  {B / med[name] / 1e3:7.2f} M pairs/s   regions "
              f"{' '.join(f'{v:.4f}' for v in ms[name])}", flush=True)
    r = med["pk-bf16"] / med["2p-bf16"]
    verdict = "level" if abs(r - 1.0) <= spread else ("FASTER" if r < 1.0 else "SLOWER")
    print(f"(b) buffered step  B={B:>6} k={K}  pk-bf16 / 2p-bf16 = {r:.3f}   (2p-bf16 regions min .. max {spread:.1%} of their median: {verdict})", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    rounds, warmup, steps = int(OPTS.get("rounds", "40")), int(OPTS.get("warmup", "10")), int(OPTS.get("steps", "20"))
    shapes = [int(b) for b in OPTS.get("B", "1024,8192,65536").split(",")]
    parts = OPTS.get("parts", "a,b").split(",")
    csr = preset_graph("cit2", device=dev, scale=float(OPTS.get("scale", "1")))
    form = sp.sampler.packed_rows_form(csr.num_nodes, M, HOPS, csr.indptr.dtype == torch.int64)
    print(f"packed_half_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops, packed form (cb, fb) = {form}, library "
          f"{os.path.basename(os.environ.get('SUBGACC_LIB', '')) or 'as shipped'}; (a) {rounds} launches of each form, alternating, after {warmup} warm-up rounds, device "
          f"events around each launch; (b) three regions of {steps} steps each, alternating, after {warmup} warm-up steps", flush=True)
    if form is None:
        print("no packed form at this shape on this graph: nothing to measure", flush=True)
        return
    for B in shapes:
        if "a" in parts:
            part_a(sp, csr, dev, B, rounds, warmup)
        if "b" in parts:
            part_b(sp, csr, dev, B, steps, warmup)


if __name__ == "__main__":
    main()

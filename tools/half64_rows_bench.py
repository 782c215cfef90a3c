#!/usr/bin/env python3
"""Dev-only: the join's rows in bf16 / fp16 over 64-bit key rows (subgacc_sjoin_fill_half64) against the f32 fill (subgacc_sjoin_fill_v2,
payload KEY64) over the same rows and the same seg, on the cit2-like graph of bench.py at M = 200 and 4 hops (k = 5, 20-byte rows):
the paper's citation2 sampler setting, bench.py's cit2m4.

    python tools/half64_rows_bench.py [--B=1024,8192,65536] [--rounds=40] [--warmup=10] [--steps=20] [--parts=a,b]
        (a) the join launch alone, device events around every launch: f32, bf16 and fp16 ALTERNATE over the strided 64-bit key rows of
            one on-demand step -- median, min .. max and the quartiles of --rounds launches each after --warmup rounds; the ratio is
            median 16-bit / median f32, to be read against the spread the f32 launch shows in the same run
        (b) the whole buffered step (sample_and_gather through StepBuffers) in f32 and in bf16 (wide_keys=True): regions of --steps
            steps, the two alternating, three regions each

Bytes: per member 12 read (id + 8-byte key) and 8k = 40 written in f32, 4k = 20 in 16 bits; TB/s = those bytes over the median.
A library built with -DSJ_HALF64_THREADS=128 / 256 (SUBGACC_LIB=...) forces the lanes of a pair's workgroup."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
M, HOPS, K = 200, 4, 5
READ, W32, W16 = 12, 8 * K, 4 * K      # bytes per member
HBM_PEAK = 8.0e12           # bytes / s (MI355X)
NAMES = ("f32", "bf16", "fp16")


def _launch_times(launch, rounds, warmup):
    """{name: sorted ms of `rounds` launches}, the three forms alternating inside every round"""
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


def _report(B, R, ts):
    med = {n: t[len(t) // 2] for n, t in ts.items()}
    f = ts["f32"]
    spread = (f[(3 * len(f)) // 4] - f[len(f) // 4]) / med["f32"]
    for n in NAMES:
        t = ts[n]
        byts = R * (READ + (W32 if n == "f32" else W16))
        print(f"(a) step rows (strided, 64-bit keys) B={B:>6} k={K} R={R:>10,}  {n:<4} median {med[n] * 1e3:9.2f} us   min {t[0] * 1e3:9.2f}  "
              f"q1 {t[len(t) // 4] * 1e3:9.2f}  q3 {t[(3 * len(t)) // 4] * 1e3:9.2f}  max {t[-1] * 1e3:9.2f}   {READ} + "
              f"{W32 if n == 'f32' else W16} B/member, {byts / 1e6:8.1f} MB = {byts / med[n] / 1e9:5.2f} TB/s "
              f"({byts / med[n] / 1e-3 / HBM_PEAK:.1%} of the HBM peak)", flush=True)
    for n in NAMES[1:]:
        r = med[n] / med["f32"]
        verdict = "not slower" if r <= 1.0 + spread else "SLOWER than the f32 fill beyond its spread"
        print(f"(a) step rows (strided, 64-bit keys) B={B:>6} k={K}  {n} / f32 = {r:.3f}   (f32 interquartile spread {spread:.1%} of its "
              f"median; byte ratio {(READ + W16) / (READ + W32):.3f})   {verdict}", flush=True)


def part_a(sp, csr, dev, B, rounds, warmup):
    import ctypes
    import torch
    from surel_plus_amd import _lib, spjoin
    from surel_plus_amd.graphs import query_pairs
    L, st = _lib.lib(), _lib.stream_ptr()
    e = query_pairs(csr, B, seed=9300, device=dev)
    # the strided key rows of one on-demand step (its buffers keep them), joined again launch by launch
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=HOPS)
    assert bufs.key64 and bufs.slot.dtype == torch.int64
    _, seg, sets = sp.sample_and_gather(csr, e, num_walks=M, num_steps=HOPS, buffers=bufs)
    sets.resolve()
    R = int(seg[-1].item())
    own, partner = spjoin._arange_segments(B, dev)
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    fields = dict(row_len=bufs.nsize, n_rows=bufs.n, row_stride=bufs.stride, ids=bufs.ids, payload=bufs.slot, own=own, partner=partner,
                  S=bufs.S, pair_block=B, num_walks=M, num_steps=HOPS, seg=bufs.seg, flags=flags)
    out = {"f32": torch.empty((R, 2, K), dtype=torch.float32, device=dev), "bf16": torch.empty((R, 2, K), dtype=torch.bfloat16, device=dev),
           "fp16": torch.empty((R, 2, K), dtype=torch.float16, device=dev)}
    d32 = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY64, out_xz=out["f32"], **fields)
    d16 = _lib.join_desc(_lib.JOIN_ROWS, _lib.JOIN_KEY64, **fields)
    launch = {"f32": lambda: _lib.check(L.subgacc_sjoin_fill_v2(ctypes.byref(d32), st)),
              "bf16": lambda: _lib.check(L.subgacc_sjoin_fill_half64(ctypes.byref(d16), _lib.HALF_BF16, _lib.ptr(out["bf16"]), st)),
              "fp16": lambda: _lib.check(L.subgacc_sjoin_fill_half64(ctypes.byref(d16), _lib.HALF_F16, _lib.ptr(out["fp16"]), st))}
    ts = _launch_times(launch, rounds, warmup)
    same = all(torch.equal(out[n].view(torch.int16), out["f32"].to(out[n].dtype).view(torch.int16)) for n in NAMES[1:])
    assert same and not flags.any(), "the 16-bit rows are not the f32 rows rounded"
    _report(B, R, ts)


def part_b(sp, csr, dev, B, steps, W):
    import torch
    from surel_plus_amd.graphs import query_pairs
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    kw = dict(num_walks=M, num_steps=HOPS)
    bufs = {"f32": sp.StepBuffers(csr, B, **kw), "bf16": sp.StepBuffers(csr, B, dtype=torch.bfloat16, wide_keys=True, **kw)}
    it = [0]

    def step(name):
        e = es[it[0] % 4]
        it[0] += 1
        half = {} if name == "f32" else dict(dtype=torch.bfloat16, wide_keys=True)
        sp.sample_and_gather(csr, e, buffers=bufs[name], **half, **kw)

    for name in bufs:
        for _ in range(W):
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
    for name in bufs:
        print(f"(b) buffered step  B={B:>6} k={K}  {name:<4} {med[name]:9.4f} ms / step  {B / med[name] / 1e3:7.2f} M pairs/s   regions "
              f"{' '.join(f'{v:.4f}' for v in ms[name])}   out buffer {bufs[name].out.numel() * bufs[name].out.element_size() / 1e6:.0f} MB", flush=True)
    print(f"(b) buffered step  B={B:>6} k={K}  bf16 / f32 = {med['bf16'] / med['f32']:.3f}", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    rounds, warmup, steps = int(OPTS.get("rounds", "40")), int(OPTS.get("warmup", "10")), int(OPTS.get("steps", "20"))
    shapes = [int(b) for b in OPTS.get("B", "1024,8192,65536").split(",")]
    parts = OPTS.get("parts", "a,b").split(",")
    csr = preset_graph("cit2", device=dev, scale=float(OPTS.get("scale", "1")))
    print(f"half64_rows_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}, {HOPS} hops; library {os.environ.get('SUBGACC_LIB', 'as built')}; "
          f"(a) {rounds} launches of each form, alternating, after {warmup} warm-up rounds, device events around each launch; (b) three "
          f"regions of {steps} steps each, alternating, after {warmup} warm-up steps", flush=True)
    for B in shapes:
        if "a" in parts:
            part_a(sp, csr, dev, B, rounds, warmup)
        if "b" in parts:
            part_b(sp, csr, dev, B, steps, warmup)


if __name__ == "__main__":
    main()

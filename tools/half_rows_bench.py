#!/usr/bin/env python3
"""Dev-only: the join's rows in bf16 / fp16 (subgacc_sjoin_fill_half) against the f32 fill (subgacc_sjoin_fill_v2) over the same rows and
the same seg, on the cit2-like graph of bench.py at M = 200: 3 hops (k = 4, 16-byte rows) and 2 hops (k = 3, 12-byte rows).

    python tools/half_rows_bench.py [--B=1024,65536] [--hops=3,2] [--rounds=40] [--warmup=10] [--steps=20] [--parts=a,b]
        (a) the join launch alone, device events around every launch: f32, bf16 and fp16 ALTERNATE over the strided key rows of one
            on-demand step, then over a keyed resident store of the same sets (packed rows) -- median, min .. max and the quartiles of
            --rounds launches each after --warmup rounds; the ratio is median 16-bit / median f32, to be read against the spread
            the f32 launch shows in the same run
        (b) the whole buffered step (sample_and_gather through StepBuffers) in f32 and in bf16: regions of --steps steps, the two
            alternating, three regions each

Bytes: per member 8 read (id + key) and 8k written in f32, 4k in 16 bits; TB/s = those bytes over the median."""
import os
import sys

OPTS = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
M = 200
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


def _report(tag, B, k, R, ts):
    med = {n: t[len(t) // 2] for n, t in ts.items()}
    f = ts["f32"]
    spread = (f[(3 * len(f)) // 4] - f[len(f) // 4]) / med["f32"]
    for n in NAMES:
        t = ts[n]
        byts = R * (8 + (8 if n == "f32" else 4) * k)
        print(f"(a) {tag} B={B:>6} k={k} R={R:>10,}  {n:<4} median {med[n] * 1e3:9.2f} us   min {t[0] * 1e3:9.2f}  q1 {t[len(t) // 4] * 1e3:9.2f}  "
              f"q3 {t[(3 * len(t)) // 4] * 1e3:9.2f}  max {t[-1] * 1e3:9.2f}   {byts / 1e6:8.1f} MB = {byts / med[n] / 1e9:5.2f} TB/s "
              f"({byts / med[n] / 1e-3 / HBM_PEAK:.1%} of the HBM peak)", flush=True)
    for n in NAMES[1:]:
        r = med[n] / med["f32"]
        verdict = "not slower" if r <= 1.0 + spread else "SLOWER than the f32 fill beyond its spread"
        print(f"(a) {tag} B={B:>6} k={k}  {n} / f32 = {r:.3f}   (f32 interquartile spread {spread:.1%} of its median; byte ratio "
              f"{(8 + 4 * k) / (8 + 8 * k):.3f})   {verdict}", flush=True)


def _launchers(_lib, kind, fields, seg, flags, R, k, dev):
    """the three launches over one list: the f32 fill into out_xz, the 16-bit fills into buffers of their own"""
    import ctypes
    import torch
    L, st = _lib.lib(), _lib.stream_ptr()
    out = {"f32": torch.empty((R, 2, k), dtype=torch.float32, device=dev), "bf16": torch.empty((R, 2, k), dtype=torch.bfloat16, device=dev),
           "fp16": torch.empty((R, 2, k), dtype=torch.float16, device=dev)}
    d32 = _lib.join_desc(_lib.JOIN_ROWS, kind, seg=seg, flags=flags, out_xz=out["f32"], **fields)
    d16 = _lib.join_desc(_lib.JOIN_ROWS, kind, seg=seg, flags=flags, **fields)
    launch = {"f32": lambda: _lib.check(L.subgacc_sjoin_fill_v2(ctypes.byref(d32), st)),
              "bf16": lambda: _lib.check(L.subgacc_sjoin_fill_half(ctypes.byref(d16), _lib.HALF_BF16, _lib.ptr(out["bf16"]), st)),
              "fp16": lambda: _lib.check(L.subgacc_sjoin_fill_half(ctypes.byref(d16), _lib.HALF_F16, _lib.ptr(out["fp16"]), st))}
    return launch, out


def _same(out):
    import torch
    return all(torch.equal(out[n].view(torch.int16), out["f32"].to(out[n].dtype).view(torch.int16)) for n in NAMES[1:])


def part_a(sp, csr, dev, B, hops, rounds, warmup):
    import torch
    from surel_plus_amd import _lib, spjoin
    from surel_plus_amd.graphs import query_pairs
    L, k = _lib.lib(), hops + 1
    e = query_pairs(csr, B, seed=9300, device=dev)
    # ---- the strided key rows of one on-demand step (its buffers keep them), joined again launch by launch
    bufs = sp.StepBuffers(csr, B, num_walks=M, num_steps=hops)
    _, seg, sets = sp.sample_and_gather(csr, e, num_walks=M, num_steps=hops, buffers=bufs)
    sets.resolve()
    R = int(seg[-1].item())
    own, partner = spjoin._arange_segments(B, dev)
    flags = torch.zeros(4, dtype=torch.int32, device=dev)
    fields = dict(row_len=bufs.nsize, n_rows=bufs.n, row_stride=bufs.stride, ids=bufs.ids, payload=bufs.slot, own=own, partner=partner,
                  S=bufs.S, pair_block=B, num_walks=M, num_steps=hops)
    launch, out = _launchers(_lib, _lib.JOIN_KEY32, fields, bufs.seg, flags, R, k, dev)
    ts = _launch_times(launch, rounds, warmup)
    assert _same(out) and not flags.any(), "the 16-bit rows are not the f32 rows rounded"
    _report("step rows (strided)", B, k, R, ts)
    del launch, out
    # ---- a keyed resident store of the same sets: packed rows, row i = the set of endpoint i
    z, zsets = sp.sample_spg(csr, e.reshape(-1).to(torch.int32), num_walks=M, num_steps=hops, rng="philox")
    enc = torch.round(zsets.feature_table().double() * M).to(torch.int64)
    zk = z.keyed(enc, M)
    S = 2 * B
    pseg = torch.empty(S + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(L.subgacc_sjoin_workspace_bytes(S), 8), dtype=torch.uint8, device=dev)
    _lib.check(L.subgacc_sjoin_sizes(_lib.ptr(zk.indptr), zk.n_rows, _lib.ptr(own), _lib.ptr(partner), S, _lib.ptr(pseg), _lib.ptr(flags),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr()))
    assert torch.equal(pseg, bufs.seg), "the store's sets are not the step's"
    _, rows = zk.join_rows()
    fields = dict(rows, own=own, partner=partner, S=S, pair_block=B, num_walks=M, num_steps=hops)
    launch, out = _launchers(_lib, _lib.JOIN_KEY32, fields, pseg, flags, R, k, dev)
    ts = _launch_times(launch, rounds, warmup)
    assert _same(out) and not flags.any(), "the 16-bit rows are not the f32 rows rounded"
    _report("keyed store (packed)", B, k, R, ts)


def part_b(sp, csr, dev, B, hops, K, W):
    import torch
    from surel_plus_amd.graphs import query_pairs
    es = [query_pairs(csr, B, seed=9300 + s, device=dev) for s in range(4)]
    kw = dict(num_walks=M, num_steps=hops)
    bufs = {"f32": sp.StepBuffers(csr, B, **kw), "bf16": sp.StepBuffers(csr, B, dtype=torch.bfloat16, **kw)}
    it = [0]

    def step(name):
        e = es[it[0] % 4]
        it[0] += 1
        sp.sample_and_gather(csr, e, buffers=bufs[name], dtype=None if name == "f32" else torch.bfloat16, **kw)

    for name in bufs:
        for _ in range(W):
            step(name)
    torch.cuda.synchronize()
    ms = {name: [] for name in bufs}
    for _ in range(3):
        for name in bufs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(K):
                step(name)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / K)
    med = {name: sorted(v)[1] for name, v in ms.items()}
    for name in bufs:
        print(f"(b) buffered step  B={B:>6} k={hops + 1}  {name:<4} {med[name]:9.4f} ms / step  {B / med[name] / 1e3:7.2f} M pairs/s   regions "
              f"{' '.join(f'{v:.4f}' for v in ms[name])}   out buffer {bufs[name].out.numel() * bufs[name].out.element_size() / 1e6:.0f} MB", flush=True)
    print(f"(b) buffered step  B={B:>6} k={hops + 1}  bf16 / f32 = {med['bf16'] / med['f32']:.3f}", flush=True)


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    dev = torch.device("cuda", 0)
    rounds, warmup, K = int(OPTS.get("rounds", "40")), int(OPTS.get("warmup", "10")), int(OPTS.get("steps", "20"))
    shapes = [int(b) for b in OPTS.get("B", "1024,65536").split(",")]
    parts = OPTS.get("parts", "a,b").split(",")
    csr = preset_graph("cit2", device=dev, scale=float(OPTS.get("scale", "1")))
    print(f"half_rows_bench: cit2-like graph N={csr.num_nodes:,}, M = {M}; (a) {rounds} launches of each form, alternating, after {warmup} warm-up "
          f"rounds, device events around each launch; (b) three regions of {K} steps each, alternating, after {warmup} warm-up steps", flush=True)
    for hops in (int(h) for h in OPTS.get("hops", "3,2").split(",")):
        for B in shapes:
            if "a" in parts:
                part_a(sp, csr, dev, B, hops, rounds, warmup)
            if "b" in parts:
                part_b(sp, csr, dev, B, hops, K, warmup)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: the LP encoder's first model stage with LSTM aggregation folded into one recurrent kernel (index_lstm_stage,
subgacc_lstm_aggr and _backward) against lstm_stage (index form, then a dense [S, L, H] batch through nn.LSTM) and the reference form of
model.py:63-65,78-83 -- gather -> pe_embedding = Sequential(Linear(k, H), ReLU, Linear(H, H)) -> sum(-2) -> to_dense_batch -> nn.LSTM ->
last position -- on the all-N resident LP stores of bench.py: cit2 and ppa (M = 200, --num_steps 4), H = H' = 96, at B = 1,024
(main.py:32) and B = 65,536.  Every form runs where it fits in memory; one that does not is reported as such.

    python tools/lstm_aggr_bench.py [--n=3] [--stores=cit2,ppa] [--batches 1024 65536]   device-event timings (median of n calls), the
                                                                 batch's L and padding share, largest differences, peak memory per form
    python tools/lstm_aggr_bench.py --profile=B [--store=cit2]   only the fused forward + backward of one shape, for
                                                                 rocprofv3 --kernel-trace --stats"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SUBGACC_QUIET", "1")
H = 96
STORES = {"cit2": ("cit2", 200, 4), "ppa": ("ppa", 200, 4)}        # bench.py's WORKLOADS: preset, M, CLI --num_steps
REF_MAX_B = 4096


def _timed(fn, n):
    import torch
    ts = []
    for _ in range(n + 1):          # the first call warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2]


def _store(name, dev):
    import numpy as np
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import preset_graph
    preset, M, k = STORES[name]
    csr = preset_graph(preset, device=dev)
    z, sets = sp.sample_spg(csr, np.arange(csr.num_nodes), num_walks=M, num_steps=k - 1, seed=111413, rng="philox", fused=True)
    return csr, z, sets.feature_table()


def _nets(k, dev):
    import torch
    torch.manual_seed(0)
    return (torch.nn.Sequential(torch.nn.Linear(k, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev),
            torch.nn.LSTM(H, H, batch_first=True).to(dev))


def _reference(edge, z, table, embed, lstm):
    import torch
    import surel_plus_amd as sp
    xz, ind = sp.gather(edge, z, "cuda", ptr=True, encode=table)
    x = embed(xz).sum(dim=-2)
    S = ind.numel() - 1
    lens = ind[1:] - ind[:-1]
    seg = torch.repeat_interleave(torch.arange(S, device=x.device), lens, output_size=x.shape[0])
    pos = torch.arange(x.shape[0], device=x.device) - ind[:-1][seg]
    dense = x.new_zeros((S, max(int(lens.max()), 1), x.shape[-1]))
    dense[seg, pos] = x
    return lstm(dense)[0][:, -1].view(2, -1, x.shape[-1])


def _run(form, edge, z, table, nets, grad):
    import torch
    import surel_plus_amd as sp
    fn = {"fused": sp.index_lstm_stage, "lstm_stage": sp.lstm_stage, "reference": _reference}[form]
    if not grad:
        with torch.no_grad():
            return fn(edge, z, table, *nets)
    for m in nets:
        m.zero_grad(set_to_none=True)
    out = fn(edge, z, table, *nets)
    out.sum().backward()
    return out


def _measure(form, edge, z, table, nets, grad, n):
    """(median ms, peak bytes above the start, output) or None when it does not fit"""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        out = _run(form, edge, z, table, nets, grad).detach()
        peak = torch.cuda.max_memory_allocated() - base
        ms = _timed(lambda: _run(form, edge, z, table, nets, grad), n)
        return ms, peak, out
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def main():
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import query_pairs
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--stores", default="cit2,ppa")
    ap.add_argument("--store", default="cit2")
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.profile:
        csr, z, table = _store(a.store, dev)
        nets = _nets(table.shape[1], dev)
        edge = query_pairs(csr, a.profile, seed=1)
        for _ in range(3):
            _run("fused", edge, z, table, nets, True)
        torch.cuda.synchronize()
        print(f"profiled: {a.store} B={a.profile} fused forward + backward x3")
        return
    print(f"# {torch.cuda.get_device_name()}  H = H' = {H}, median of {a.n} calls (ms); peak = allocator bytes above the start")
    for name in a.stores.split(","):
        csr, z, table = _store(name, dev)
        nets = _nets(table.shape[1], dev)
        for B in a.batches:
            edge = query_pairs(csr, B, seed=1)
            pairs, ind = sp.gather_index(edge, z)
            lens = (ind[1:] - ind[:-1]).double()
            L = int(lens.max())
            print(f"{name} B={B}: S={2 * B} R={pairs.shape[0]} L={L} padding share {1 - float(lens.mean()) / L:.3f} "
                  f"dense [S, L, H] = {2 * B * L * H * 4 / 1e9:.2f} GB")
            res = {}
            for grad in (False, True):
                for form in ("fused", "lstm_stage", "reference"):
                    if form == "reference" and B > REF_MAX_B:
                        continue
                    r = _measure(form, edge, z, table, nets, grad, a.n)
                    what = "fwd+bwd" if grad else "fwd"
                    if r is None:
                        print(f"  {form:10s} {what:8s} did not fit")
                        continue
                    ms, peak, out = r
                    res[(form, grad)] = out
                    print(f"  {form:10s} {what:8s} {ms:10.3f} ms  peak {peak / 1e9:8.3f} GB")
            for form in ("lstm_stage", "reference"):
                if (form, False) in res and ("fused", False) in res:
                    d = float((res[("fused", False)] - res[(form, False)]).abs().max())
                    print(f"  max |fused - {form}| = {d:.3e} (largest entry {float(res[(form, False)].abs().max()):.3e})")
            del res
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

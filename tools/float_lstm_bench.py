#!/usr/bin/env python3
"""Dev-only: the float encoders' first model stage with LSTM aggregation in the recurrent kernel (float_lstm_stage,
subgacc_lstm_aggr_hinge and _backward) against the hand-written reference form of model.py:63-65,78-83 -- gather -> pe_embedding =
Sequential(Linear(1, H), ReLU, Linear(H, H)) -> sum(-2) -> to_dense_batch -> nn.LSTM -> last position -- on the cit2-PPR store of
bench.py (graphs.ppr_like_spg(2,927,963): top-100 rows), H = H1 = H' = 96, at B = 1,024, B = 65,536 and the MRR shape P = 64 x
K = 1,000.  Every form runs where it fits in memory; one that does not is reported as such.

    python tools/float_lstm_bench.py [--n=3] [--shapes=1024,65536,mrr]   device-event timings (median of n calls), the batch's L and
                                                              padding share, peak memory of each form, largest differences
    python tools/float_lstm_bench.py --profile=B              only the fused forward + backward of one shape, for
                                                              rocprofv3 --kernel-trace --stats"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from float_stage_bench import H, N_CIT2, ROOT, SHAPES, _edge, _timed  # noqa: E402

sys.path.insert(0, ROOT)
REF_MAX_B = 4096        # the reference form is not run above this: at S = 131,072 segments of L = 100 steps MIOpen's LSTM (the 5 GB dense
                        # batch, 2^32.2 gate elements) ended in a memory-access fault on the MI355X instead of an out-of-memory error


def _nets(dev):
    import torch
    torch.manual_seed(0)
    return (torch.nn.Sequential(torch.nn.Linear(1, H), torch.nn.ReLU(), torch.nn.Linear(H, H)).to(dev),
            torch.nn.LSTM(H, H, batch_first=True).to(dev))


def _reference(edge, x, embed, lstm):
    import torch
    import surel_plus_amd as sp
    xz, ind = sp.gather(edge, x, edge.device, ptr=True)
    h = embed(xz).sum(dim=-2)
    S = ind.numel() - 1
    lens = ind[1:] - ind[:-1]
    seg = torch.repeat_interleave(torch.arange(S, device=h.device), lens, output_size=h.shape[0])
    pos = torch.arange(h.shape[0], device=h.device) - ind[:-1][seg]
    dense = h.new_zeros((S, max(int(lens.max()), 1), h.shape[-1]))
    dense[seg, pos] = h
    return lstm(dense)[0][:, -1].view(2, -1, h.shape[-1])


def _run(form, edge, x, nets, grad):
    import torch
    import surel_plus_amd as sp
    fn = sp.float_lstm_stage if form == "fused" else _reference
    if not grad:
        with torch.no_grad():
            return fn(edge, x, *nets)
    for m in nets:
        m.zero_grad(set_to_none=True)
    out = fn(edge, x, *nets)
    out.sum().backward()
    return out


def _measure(form, edge, x, nets, grad, n):
    """(median ms, peak bytes above the start, output) or None when the form does not fit"""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        out = _run(form, edge, x, nets, grad).detach()
        peak = torch.cuda.max_memory_allocated() - base
        return _timed(lambda: _run(form, edge, x, nets, grad), n), peak, out
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    import torch
    import surel_plus_amd as sp
    from surel_plus_amd.graphs import ppr_like_spg
    dev = torch.device("cuda", 0)
    n = int(opts.get("n", "3"))
    z = ppr_like_spg(N_CIT2, topk=100, seed=3, device=dev)
    nets = _nets(dev)
    torch.cuda.synchronize()
    if "profile" in opts:
        edge = _edge(opts["profile"], z.n_rows, dev)
        for _ in range(n):
            _run("fused", edge, z, nets, True)
        torch.cuda.synchronize()
        print(f"profiled: shape {opts['profile']} fused forward + backward x{n}")
        return
    print(f"# {torch.cuda.get_device_name()}  cit2-PPR store N={z.n_rows:,} (top-100), H = H1 = H' = {H}, median of {n} calls (ms); "
          "peak = allocator bytes above the start")
    for shape in opts.get("shapes", ",".join(SHAPES)).split(","):
        edge = _edge(shape, z.n_rows, dev)
        _, ind = sp.gather(edge, z, dev, ptr=True)
        lens = (ind[1:] - ind[:-1]).double()
        L, S = int(lens.max()), ind.numel() - 1
        label = "P64xK1000" if shape == "mrr" else f"B={int(shape):,}"
        print(f"{label}: S={S} R={int(ind[-1])} L={L} padding share {1 - float(lens.mean()) / L:.3f} "
              f"dense [S, L, H] = {S * L * H * 4 / 1e9:.2f} GB", flush=True)
        del ind, lens
        res = {}
        for grad in (False, True):
            for form in ("fused", "reference"):
                if form == "reference" and edge.shape[1] > REF_MAX_B:
                    print(f"  {form:10s} {'fwd+bwd' if grad else 'fwd':8s} not run (B > {REF_MAX_B}: see REF_MAX_B)", flush=True)
                    continue
                r = _measure(form, edge, z, nets, grad, n)
                what = "fwd+bwd" if grad else "fwd"
                if r is None:
                    print(f"  {form:10s} {what:8s} did not fit", flush=True)
                    continue
                ms, peak, out = r
                res[(form, grad)] = out
                print(f"  {form:10s} {what:8s} {ms:10.3f} ms  peak {peak / 1e9:8.3f} GB", flush=True)
        if ("fused", False) in res and ("reference", False) in res:
            d = float((res[("fused", False)] - res[("reference", False)]).abs().max())
            print(f"  max |fused - reference| = {d:.3e} (largest entry {float(res[('reference', False)].abs().max()):.3e})", flush=True)
        del res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

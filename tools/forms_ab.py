#!/usr/bin/env python3
"""Dev-only: same-box A/B of library BUILDS for the count form, the pair form and the count form with attention (sjoin_counts_kernel,
sjoin_pairs_kernel, sjoin_counts_attn_kernel<BWD>) and for the joins over the key rows of a step (sjoin_key_counts_kernel,
sjoin_key_counts_attn_kernel<BWD>, sjoin_key_index_kernel), alternating, one fresh process per (repetition, library):

    python tools/forms_ab.py [--libs=tools/build/libsubgacc_parent.so,-] [--reps=5] [--n=20]       (`-` = the shipped library)

Each process builds the all-N cit2 LP store of tools/counts_attn_bench.py (N = 2.9 M rows, T = 1,433 LP rows) and brackets the kernels
with HIP events on the launch stream (bench.KernelTimer, as tools/bench_studies.py's first-stage study does): gather_counts and
gather_pairs at B = 65,536, counts_attn_stage forward and backward at B = 1,024 and 65,536; then the key-row kernels in a buffered
step of the batch of tools/step_attn_bench.py --parts=k (M = 200, 3 hops, T = 2,048 columns) at both sizes; median of n launches each,
in us.  The outputs of every timed call of the last round are hashed (sha256 of C, of W / max / den, of Dg, of the pairs), and the
driver FAILS when a hash differs between two libraries: the builds must give the same bits.
The verdict per kernel: the LAST library's median of its repetitions' medians against the FIRST library's plus the spread (max - min)
of the first library's own repetitions.  Boxes of the pool differ by 5-10 %: only numbers of one call compare."""
import hashlib
import json
import os
import subprocess
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("SUBGACC_QUIET", "1")


STEP_M, STEP_HOPS, STEP_T = 200, 3, 2048      # tools/step_attn_bench.py's step, its first table_rows


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().contiguous().cpu().numpy())
    return h.hexdigest()[:16]


def _hash_attn_calls(cls, tag, hashes, live):
    """the (W, max, den) and Dg that cls.forward / cls.backward return, hashed while live[0] names the round"""
    fwd, bwd = cls.forward, cls.backward

    def forward(self, g, keep):
        r = fwd(self, g, keep)
        if live[0]:
            hashes[f"{tag} W/max/den {live[0]}"] = _sha(*r)
        return r

    def backward(self, g, dW, W, mx, den):
        r = bwd(self, g, dW, W, mx, den)
        if live[0]:
            hashes[f"{tag} Dg {live[0]}"] = _sha(r)
        return r
    cls.forward, cls.backward = forward, backward


def one(n):
    import torch
    import bench
    import counts_attn_bench as cab
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod, spjoin
    from surel_plus_amd.graphs import query_pairs
    dev = torch.device("cuda", 0)
    csr, z, table = cab._store("cit2", dev)
    nets = cab._nets(table.shape[1], dev)
    T = table.shape[0]
    out, hashes, live = {}, {}, [None]
    _hash_attn_calls(spjoin._CountsAttnJoin, "sjoin_counts_attn", hashes, live)
    _hash_attn_calls(spjoin._StepAttnJoin, "sjoin_key_counts_attn", hashes, live)
    kw = dict(num_walks=STEP_M, num_steps=STEP_HOPS)
    for B in (65536, 1024):
        edge = query_pairs(csr, B, seed=9700, device=dev)
        torch.manual_seed(B)
        w = torch.randn(2, B, cab.H, device=dev)
        timer = bench.KernelTimer()
        sampler_mod.KERNEL_TIMER = timer
        for it in range(n + 1):
            timer.enabled = it > 0          # the first round warms up
            live[0] = f"B={B}" if it == n else None
            if B == 65536:
                C = sp.gather_counts(edge, z, T)        # (C, sizes)
                pairs = sp.gather_pairs(edge, z)
                if live[0]:
                    hashes[f"sjoin_counts C {live[0]}"], hashes[f"sjoin_pairs pairs {live[0]}"] = _sha(*C), _sha(*pairs)
                del C, pairs
            (sp.counts_attn_stage(edge, z, table, *nets) * w).sum().backward()
            torch.cuda.synchronize()
        # the key-row kernels: one buffered step per stage over the same batch, the launches bracketed by name
        e = query_pairs(csr, B, seed=9300, device=dev)
        ab, cb, ib = (sp.StepBuffers(csr, B, stage=s, table_rows=STEP_T, **kw) for s in ("counts_attn", "counts", "index"))
        g = torch.randn(STEP_T, device=dev).requires_grad_()
        dW = torch.randn(2 * B, STEP_T, device=dev)
        for it in range(n + 1):
            timer.enabled = it > 0
            live[0] = f"B={B}" if it == n else None
            sp.sample_and_attn_counts(csr, e, lambda t: g, buffers=ab, **kw)[0].backward(dW)
            g.grad = None
            C = sp.sample_and_counts(csr, e, buffers=cb, **kw)[0]
            pairs, indptr = sp.sample_and_index(csr, e, buffers=ib, **kw)[:2]
            torch.cuda.synchronize()
            if live[0]:
                hashes[f"sjoin_key_counts C {live[0]}"] = _sha(C)
                hashes[f"sjoin_key_index pairs {live[0]}"] = _sha(pairs[: int(indptr[-1])])
        for b in (ab, cb, ib):
            b.sets.resolve()                # a step that overflowed its columns or raised a flag is no measurement
        del ab, cb, ib, dW
        sampler_mod.KERNEL_TIMER = None
        live[0] = None
        for name, ev in timer.pairs.items():
            if name.startswith("sjoin_"):       # (the step's walk and columns pass are bracketed too: not what is compared here)
                    out[f"{name} B={B}"] = round(1e3 * median(a.elapsed_time(b) for a, b in ev), 2)
    print("FORMS_AB " + json.dumps({"us": out, "sha256": hashes}), flush=True)


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    n = int(opts.get("n", "20"))
    if "--one" in sys.argv:
        return one(n)
    libs = opts.get("libs", "tools/build/libsubgacc_parent.so,-").split(",")
    got, sha = {lib: [] for lib in libs}, None
    for rep in range(int(opts.get("reps", "5"))):
        for lib in libs:
            env = dict(os.environ)
            env.pop("SUBGACC_LIB", None)
            if lib != "-":
                env["SUBGACC_LIB"] = os.path.join(ROOT, lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"--n={n}"], env=env, capture_output=True, text=True,
                               timeout=int(opts.get("timeout", "280")))
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("FORMS_AB ")]
            if r.returncode != 0 or not line:      # nothing more is started on this GPU
                sys.exit(f"rep {rep} {lib}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            res = json.loads(line[0][9:])
            got[lib].append(res["us"])
            print(f"rep {rep} {lib}: {json.dumps(res['us'])}", flush=True)
            sha = sha or res["sha256"]
            if res["sha256"] != sha:               # the builds must give the same bits
                diff = {k: (sha.get(k), v) for k, v in res["sha256"].items() if sha.get(k) != v}
                sys.exit(f"rep {rep} {lib}: outputs differ from rep 0 {libs[0]}: {diff}")
    print("\nsha256 of every timed call's outputs, the same in all %d runs:" % sum(len(v) for v in got.values()))
    for k, v in sha.items():
        print(f"  {k:42} {v}")
    old, new = libs[0], libs[-1]
    print(f"\n{'kernel launch (us)':42} | {old + ' median':>36} {'spread':>7} | {new + ' median':>10} | verdict (new <= old + spread)")
    for k in got[old][0]:
        a, b = [r[k] for r in got[old]], [r[k] for r in got[new]]
        ma, mb, spread = median(a), median(b), max(a) - min(a)
        print(f"{k:42} | {ma:36.2f} {spread:7.2f} | {mb:10.2f} | {'within' if mb <= ma + spread else 'SLOWER'} ({(mb / ma - 1) * 100:+.1f} %)")


if __name__ == "__main__":
    main()

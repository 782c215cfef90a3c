#!/usr/bin/env python3
"""Dev-only: same-box A/B of library BUILDS for the count form, the pair form and the count form with attention (sjoin_counts_kernel,
sjoin_pairs_kernel, sjoin_counts_attn_kernel<BWD>), alternating, one fresh process per (repetition, library):

    python tools/forms_ab.py [--libs=tools/build/libsubgacc_parent.so,-] [--reps=5] [--n=20]       (`-` = the shipped library)

Each process builds the all-N cit2 LP store of tools/counts_attn_bench.py (N = 2.9 M rows, T = 1,433 LP rows) and brackets the kernels
with HIP events on the launch stream (bench.KernelTimer, as tools/bench_studies.py's first-stage study does): gather_counts and
gather_pairs at B = 65,536, counts_attn_stage forward and backward at B = 1,024 and 65,536; median of n launches each, in us.
The verdict per kernel: the LAST library's median of its repetitions' medians against the FIRST library's plus the spread (max - min)
of the first library's own repetitions.  Boxes of the pool differ by 5-10 %: only numbers of one call compare."""
import json
import os
import subprocess
import sys
from statistics import median

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("SUBGACC_QUIET", "1")


def one(n):
    import torch
    import bench
    import counts_attn_bench as cab
    import surel_plus_amd as sp
    from surel_plus_amd import sampler as sampler_mod
    from surel_plus_amd.graphs import query_pairs
    dev = torch.device("cuda", 0)
    csr, z, table = cab._store("cit2", dev)
    nets = cab._nets(table.shape[1], dev)
    T = table.shape[0]
    out = {}
    for B in (65536, 1024):
        edge = query_pairs(csr, B, seed=9700, device=dev)
        w = torch.randn(2, B, cab.H, device=dev)
        timer = bench.KernelTimer()
        sampler_mod.KERNEL_TIMER = timer
        for it in range(n + 1):
            timer.enabled = it > 0          # the first round warms up
            if B == 65536:
                sp.gather_counts(edge, z, T)
                sp.gather_pairs(edge, z)
            (sp.counts_attn_stage(edge, z, table, *nets) * w).sum().backward()
            torch.cuda.synchronize()
        sampler_mod.KERNEL_TIMER = None
        for name, ev in timer.pairs.items():
            out[f"{name} B={B}"] = round(1e3 * median(a.elapsed_time(b) for a, b in ev), 2)
    print("FORMS_AB " + json.dumps(out), flush=True)


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    n = int(opts.get("n", "20"))
    if "--one" in sys.argv:
        return one(n)
    libs = opts.get("libs", "tools/build/libsubgacc_parent.so,-").split(",")
    got = {lib: [] for lib in libs}
    for rep in range(int(opts.get("reps", "5"))):
        for lib in libs:
            env = dict(os.environ)
            env.pop("SUBGACC_LIB", None)
            if lib != "-":
                env["SUBGACC_LIB"] = os.path.join(ROOT, lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"--n={n}"], env=env, capture_output=True, text=True,
                               timeout=280)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("FORMS_AB ")]
            if r.returncode != 0 or not line:      # nothing more is started on this GPU
                sys.exit(f"rep {rep} {lib}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            got[lib].append(json.loads(line[0][9:]))
            print(f"rep {rep} {lib}: {line[0][9:]}", flush=True)
    old, new = libs[0], libs[-1]
    print(f"\n{'kernel launch (us)':42} | {old + ' median':>36} {'spread':>7} | {new + ' median':>10} | verdict (new <= old + spread)")
    for k in got[old][0]:
        a, b = [r[k] for r in got[old]], [r[k] for r in got[new]]
        ma, mb, spread = median(a), median(b), max(a) - min(a)
        print(f"{k:42} | {ma:36.2f} {spread:7.2f} | {mb:10.2f} | {'within' if mb <= ma + spread else 'SLOWER'} ({(mb / ma - 1) * 100:+.1f} %)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Dev-only: do two source trees compile to the same gfx950 kernels?  No GPU needed.

    python tools/kernel_digest.py OLD NEW [--jobs=8] [--keep=DIR]

OLD / NEW: a source tree (every surel_plus_amd/csrc/*.hip of it is compiled with its Makefile's FLAGS plus `--cuda-device-only -S`)
or a comma-separated list of .s files made that way.  One line per kernel symbol: `same` / `DIFF` / `only-old` / `only-new`, the file(s)
it sits in, a hash of its instruction text, and from its .amdhsa_kernel block next_free_vgpr, next_free_sgpr, accum_offset,
group_segment_fixed_size (LDS) and private_segment_fixed_size (scratch) -- for a DIFF both sides, old -> new.  The text compared is
everything from the kernel's label to its end with comments and the .loc / .file / .cfi / .p2align lines dropped and the compiler's
local labels (.LBB<fn>_<n>, .LJTI<fn>_<n>, .Ltmp<n>, .Lfunc_*<n>) reduced to their per-function part: the function index changes with
the file a kernel sits in, nothing else may.  A kernel that a tree instantiates in two files is reported (`doubled`).
Exit status 1 when anything is not `same`."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
DROP = re.compile(r"\s*\.(loc|file|cfi_\w+|p2align)\b")


def makefile_flags(csrc):
    out = subprocess.check_output(["make", "-s", "-C", csrc, "--eval", "print-flags: ; @echo $(FLAGS)", "print-flags"], text=True)
    return out.strip().splitlines()[-1].split()


def compile_tree(tree, keep, jobs):
    csrc = tree if os.path.exists(os.path.join(tree, "Makefile")) else os.path.join(tree, "surel_plus_amd", "csrc")
    flags = makefile_flags(csrc)
    os.makedirs(keep, exist_ok=True)
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(f):
        out = os.path.join(keep, f[:-4] + ".s")
        subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, f), "-o", out])
        return out

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, srcs))


def normalise(lines):
    tmp = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or DROP.match(ln):
            continue
        ln = re.sub(r"\.L(BB|JTI)\d+_(\d+)", r".L\1_\2", ln)
        ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
        ln = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), ln)
        out.append(ln)
    return "\n".join(out)


def kernels_of(path):
    """{symbol: (hash, figures)} of one .s file"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    res = {}
    for name in names:
        beg = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(beg, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        body = lines[beg:end + 1]
        fig = {}
        for ln in body:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
            if m and m.group(1) in FIGURES:
                fig[m.group(1)] = m.group(2)
        res[name] = (hashlib.sha256(normalise(body).encode()).hexdigest()[:16], tuple(fig.get(k, "-") for k in FIGURES))
    return res


def digest(arg, keep, jobs):
    files = compile_tree(arg, keep, jobs) if os.path.isdir(arg) else arg.split(",")
    res, doubled = {}, []
    for f in files:
        for name, v in kernels_of(f).items():
            if name in res:
                doubled.append((name, res[name][0], os.path.basename(f)))
            res[name] = (os.path.basename(f),) + v
    return res, doubled


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) for a in argv if a.startswith("--"))
    if len(args) != 2:
        sys.exit(__doc__)
    keep = opts.get("keep") or tempfile.mkdtemp(prefix="kernel_digest_")
    jobs = int(opts.get("jobs", "8"))
    (old, dbl_old), (new, dbl_new) = (digest(a, os.path.join(keep, side), jobs) for a, side in zip(args, ("old", "new")))
    fmt = lambda v: " ".join("%s=%s" % (k.replace("_fixed_size", "").replace("next_free_", ""), x) for k, x in zip(FIGURES, v))
    count = {"same": 0, "DIFF": 0, "only-old": 0, "only-new": 0}
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name), new.get(name)
        if o and n:
            where = o[0] if o[0] == n[0] else "%s -> %s" % (o[0], n[0])
            if o[1] == n[1] and o[2] == n[2]:
                verdict, what = "same", "%s  %s" % (n[1], fmt(n[2]))
            else:
                verdict, what = "DIFF", "%s -> %s  %s  ->  %s" % (o[1], n[1], fmt(o[2]), fmt(n[2]))
        else:
            verdict, (where, h, fig) = ("only-old", o) if o else ("only-new", n)
            what = "%s  %s" % (h, fmt(fig))
        count[verdict] += 1
        print("%-8s  %-36s  %s  %s" % (verdict, where, what, name))
    for side, dbl in (("old", dbl_old), ("new", dbl_new)):
        for name, f1, f2 in dbl:
            print("doubled   %s: %s and %s  %s" % (side, f1, f2, name))
    print("# %d kernels: %s, doubled %d" % (len(set(old) | set(new)), ", ".join("%s %d" % kv for kv in count.items()), len(dbl_old) + len(dbl_new)))
    return 0 if count["same"] == len(set(old) | set(new)) and not dbl_old and not dbl_new else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

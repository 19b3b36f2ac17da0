#!/usr/bin/env python3
"""Which kernels of two gfx950 builds have different instruction streams.  Reads the assembly the build keeps
(csrc/.build/*gfx950.s; no GPU needed), cuts it into kernels at `<symbol>:` ... `.end_amdhsa_kernel`, drops comments, directives
and the compiler's function ordinal in `.LBB<fn>_<n>` labels, and compares per demangled kernel name.

usage: python tools/isa_diff.py A.s B.s      (exit status 1 if anything differs)"""
import re
import subprocess
import sys


def kernels(path):
    """{mangled symbol: (normalised instruction lines, resource figures from the kernel descriptor)}"""
    lines = open(path).read().splitlines()
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur, body = {}, None, []
    for l in lines:
        m = re.match(r"^([A-Za-z_]\w*):", l)
        if cur is None and m and m.group(1) in names:
            cur, body, res = m.group(1), [], {}
        elif cur is not None:
            t = re.sub(r"\s*;.*$", "", l).strip()
            r = re.match(r"\.amdhsa_(next_free_vgpr|group_segment_fixed_size)\s+(\d+)", t)
            if r:
                res[r.group(1)] = int(r.group(2))
            if t and not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:", t):
                body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t).replace(cur, "<self>"))
            if ".end_amdhsa_kernel" in l:
                out[cur] = (body, res)
                cur = None
    return out


def demangle(syms):
    r = subprocess.run(["c++filt"], input="\n".join(syms), stdout=subprocess.PIPE, text=True, check=True)
    return {s: re.sub(r"\(.*$", "", d.replace("void ", "", 1)) for s, d in zip(syms, r.stdout.splitlines())}


def show(name, k):
    body, res = k
    n = sum(1 for l in body if not l.endswith(":"))
    return f"{name}  VGPRs {res.get('next_free_vgpr')}  LDS {res.get('group_segment_fixed_size')} B  {n} instr."


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    dn = demangle(sorted(set(a) | set(b)))
    a = {dn[s]: v for s, v in a.items()}
    b = {dn[s]: v for s, v in b.items()}
    same = [n for n in a if n in b and a[n][0] == b[n][0]]
    for n in sorted(set(a) & set(b)):
        if a[n][0] != b[n][0]:
            print("differs:  " + show(n, a[n]) + "  ->  " + show("", b[n]).strip())
    for n in sorted(set(a) - set(b)):
        print("only in A: " + show(n, a[n]))
    for n in sorted(set(b) - set(a)):
        print("only in B: " + show(n, b[n]))
    print(f"{len(same)} kernels identical, {len(a)} in A, {len(b)} in B")
    return 0 if len(same) == len(a) == len(b) else 1


if __name__ == "__main__":
    sys.exit(main())

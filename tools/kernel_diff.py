#!/usr/bin/env python3
"""Device code of two builds of the kernel units, side by side:
    tools/kernel_diff.py <csrc of build A> <csrc of build B> [unit ...]
For every kernel unit (the Makefile's KSRC, or the ones named) it compiles both trees' <unit>.hip with the library's flags and
prints the size and SHA-256 of the object's .hip_fatbin section.  Where the sections differ it compiles both to gfx950 assembly
(--cuda-device-only -S) and compares kernel by kernel: comments stripped, function-local (LDS) symbols and local labels
renumbered in order of appearance.  Per kernel: "identical", or the line counts and the number of differing lines; with
--show N the first N differing lines of each.  It compares two builds and looks for nothing in particular."""
import argparse
import concurrent.futures
import difflib
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OBJCOPY = os.environ.get("OBJCOPY", "/opt/rocm/lib/llvm/bin/llvm-objcopy")
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-slp-vectorize").split()


def units_of(csrc):
    for line in open(os.path.join(csrc, "Makefile")):
        if line.startswith("KSRC"):
            return line.split(":=")[1].split()
    raise SystemExit("no KSRC in the Makefile")


def stage(csrc, tmp):
    """Both trees are compiled at ONE path, one after the other: the device section carries an id hashed from the source's path."""
    work = os.path.join(tmp, "w")
    shutil.rmtree(work, ignore_errors=True)
    dst = os.path.join(work, "pkg", "csrc")
    shutil.copytree(csrc, dst, ignore=shutil.ignore_patterns("*.o", "*.so", "var_*"))
    shutil.copytree(os.path.join(csrc, "..", "..", "include"), os.path.join(work, "include"))
    return dst


def fatbin(csrc, unit, tmp, tag):
    obj, sec = os.path.join(csrc, unit + ".o"), os.path.join(tmp, f"{tag}_{unit}.fatbin")  # (the id hashes the command line too)
    subprocess.run([HIPCC, *FLAGS, "-c", unit + ".hip", "-o", unit + ".o"], check=True, stderr=subprocess.DEVNULL, cwd=csrc)
    subprocess.run([OBJCOPY, "--dump-section", f".hip_fatbin={sec}", obj], check=True)
    data = open(sec, "rb").read()
    return len(data), hashlib.sha256(data).hexdigest()[:16]


def kernels(csrc, unit, tmp, tag):
    """kernel name -> normalised instruction lines (read at once: the next tree is staged over this one)"""
    out = os.path.join(csrc, unit + ".s")
    subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", unit + ".hip", "-o", unit + ".s"], check=True, stderr=subprocess.DEVNULL, cwd=csrc)
    found, name, body = {}, None, []
    for raw in open(out):
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(_Z\w+):$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                found[name] = normalise(body)
                name = None
            elif not line.lstrip().startswith((".p2align", ".loc", ".file", ".cfi")):
                body.append(line.strip())
    return found


def normalise(body):
    names = {}

    def sub(m):
        return names.setdefault(m.group(0), f"{'L' if m.group(0).startswith('.L') else 'S'}{len(names)}")

    return [re.sub(r"\.LBB\d+_\d+|_ZZ\w+|__unnamed_\d+|llvm\.amdgcn\.[\w.]+", sub, line) for line in body]


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0][:90]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("units", nargs="*")
    ap.add_argument("--show", type=int, default=0)
    args = ap.parse_args()
    units = args.units or units_of(args.b)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(8) as pool:
        fat = {}
        for t, c in (("a", args.a), ("b", args.b)):
            staged = stage(c, tmp)
            fat.update({(u, t): pool.submit(fatbin, staged, u, tmp, t) for u in units})
            concurrent.futures.wait([fat[(u, t)] for u in units])
        print(f"  {'object':<17}{'bytes A':>8} {'bytes B':>8}  {'A':<16}  {'B':<16}")
        differ = []
        for u in units:
            (na, ha), (nb, hb) = fat[(u, "a")].result(), fat[(u, "b")].result()
            print(f"  {u:<17}{na:>8} {nb:>8}  {ha}  {hb}  {'identical' if (na, ha) == (nb, hb) else 'differs'}")
            if (na, ha) != (nb, hb):
                differ.append(u)
        asm = {}
        for t, c in (("a", args.a), ("b", args.b)):
            staged = stage(c, tmp)
            asm.update({(u, t): pool.submit(kernels, staged, u, tmp, t) for u in differ})
            concurrent.futures.wait([asm[(u, t)] for u in differ])
        for u in differ:
            ka, kb = asm[(u, "a")].result(), asm[(u, "b")].result()
            same = [k for k in ka if k in kb and ka[k] == kb[k]]
            print(f"\n  {u}: {len(ka)} kernels in A, {len(kb)} in B, {len(same)} identical instruction for instruction")
            for k in sorted(set(ka) | set(kb)):
                if k in same:
                    print(f"    identical  {demangle(k)}")
                elif k not in ka or k not in kb:
                    print(f"    only in {'A' if k in ka else 'B'}  {demangle(k)}")
                else:
                    d = [l for l in difflib.unified_diff(ka[k], kb[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
                    print(f"    DIFFERS    {demangle(k)}: {len(ka[k])} / {len(kb[k])} lines, {len(d)} differing")
                    for l in d[:args.show]:
                        print("        " + l)
    return 0


if __name__ == "__main__":
    sys.exit(main())

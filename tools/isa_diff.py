#!/usr/bin/env python3
"""Compare the gfx950 kernels of two assembly files, kernel by kernel.

    hipcc <Makefile flags> --cuda-device-only -S old.hip -o old.s   (and new)
    tools/isa_diff.py old.s new.s [--map 'REGEX=>REPL' ...]

Kernels are paired by demangled name with template arguments (parameter
list dropped). --map rewrites OLD names to the NEW spelling when a refactor
renamed them. Per kernel, everything from its entry label to the next
function is compared: the instruction stream, the .amdhsa_* resource block
and the compiler's "Kernel info" summary. Symbol names and the function
number in local labels are normalised; nothing else is filtered.
Exit status 1 if any paired kernel differs or any kernel has no partner.
"""
import argparse
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [normalised lines]} for every .amdhsa_kernel in path."""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out, cur, name = {}, None, ""
    for l in lines:
        # a kernel ends where a section opens that is not its own .text, its
        # .rodata descriptor or its csdata summary
        if l.startswith("\t.section") and name not in l and \
                ".rodata" not in l and ".AMDGPU.csdata" not in l:
            cur = None
        elif l.split(":")[0] in names:  # the kernel's entry label
            name = l.split(":")[0]
            cur = out.setdefault(name, [])
        if cur is not None:
            cur.append(l)
    for name, body in out.items():
        text = "\n".join(body).replace(name, "KERNEL").replace(name[2:], "KERNEL")
        text = re.sub(r"(\.LBB|\bBB|\.Lfunc_end|\.Ltmp)\d+", r"\1", text)
        out[name] = [" ".join(l.split()) for l in text.split("\n")]
    return out


def identities(mangled):
    dem = subprocess.run(["c++filt"], input="\n".join(mangled), text=True,
                         capture_output=True, check=True).stdout.split("\n")
    ids = {}
    for m, d in zip(mangled, dem):
        d = d.replace("(anonymous namespace)::", "").replace("> >", ">>")
        d = d[5:] if d.startswith("void ") else d
        depth = 0
        for i, c in enumerate(d):
            depth += (c == "<") - (c == ">")
            if c == "(" and depth == 0:
                d = d[:i]
                break
        ids[d] = m
    return ids


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=>REPL")
    args = ap.parse_args()
    old_k, new_k = kernels(args.old), kernels(args.new)
    old_ids, new_ids = identities(list(old_k)), identities(list(new_k))
    for rule in args.map:
        pat, repl = rule.split("=>")
        old_ids = {re.sub(pat, repl, k): v for k, v in old_ids.items()}
        print("map: %s" % rule)
    print("kernels: %d old, %d new" % (len(old_k), len(new_k)))
    same, differ = 0, []
    for ident in sorted(set(old_ids) & set(new_ids)):
        a, b = old_k[old_ids[ident]], new_k[new_ids[ident]]
        if a == b:
            same += 1
            continue
        differ.append(ident)
        print("DIFFERS: %s (%d / %d lines)" % (ident, len(a), len(b)))
        # the resource block and summary, side by side where they disagree
        res = lambda t: {l.split()[0] + " " + l.split()[1]: l.strip() for l in t
                         if l.strip().startswith((".amdhsa_", "; ")) and len(l.split()) > 2}
        ra, rb = res(a), res(b)
        for key in ra:
            if key in rb and ra[key] != rb[key]:
                print("    %-50s | %s" % (ra[key], rb[key]))
    print("paired: %d, identical: %d, different: %d" %
          (same + len(differ), same, len(differ)))
    for ident in sorted(set(old_ids) - set(new_ids)):
        print("only in old: %s" % ident)
    for ident in sorted(set(new_ids) - set(old_ids)):
        print("only in new: %s" % ident)
    return 1 if differ or set(old_ids) ^ set(new_ids) else 0


if __name__ == "__main__":
    sys.exit(main())

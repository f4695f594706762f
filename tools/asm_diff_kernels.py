#!/usr/bin/env python3
"""Compare the gfx950 instructions of every kernel in two assembly listings
of one unit, crc32c_kernels.hip or any other csrc/*.hip (CPU only): the check
that a change left the existing kernels' code alone.

  hipcc -x hip --offload-arch=gfx950 --offload-device-only -O3 -std=c++17 \\
      -munsafe-fp-atomics -fuse-cuid=none -Iinclude -S \\
      blazingmq_amd/csrc/crc32c_kernels.hip -o new.s        (and old.s likewise)
  tools/asm_diff_kernels.py old.s new.s [--drop-arg ', false'] [--show N]

Kernels are matched by demangled name; --drop-arg removes a trailing template
argument from the second listing's names first (a parameter added with the
old behaviour at that value), and kernels of the second listing that then
have no partner are listed as new.  Labels, comments and directives are not
instructions; symbol names inside operands are compared demangled the same
way.  Exit status 1 when a matched kernel differs."""
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: [instruction lines]} of the .amdhsa kernels in a listing."""
    lines = open(path).read().splitlines()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    out = {}
    cur = None
    for raw in lines:
        line = raw.split(";")[0].rstrip()
        if line.endswith(":") and line[:-1] in names:
            cur = out.setdefault(line[:-1], [])
            continue
        if cur is None:
            continue
        line = line.strip()
        if line.startswith(".section") or line.startswith(".Lfunc_end"):
            cur = None
        elif line and not line.startswith(".") and not line.endswith(":"):
            # local labels carry the function's ordinal in the file
            line = re.sub(r"\.L(BB|post_getpc|func_end|func_begin)\d+", r".L\1", line)
            cur.append(re.sub(r"\s+", " ", line))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    return dict(zip(names, res))


def plain(name):
    """A kernel's demangled name without the return type templates carry."""
    return name[5:] if name.startswith("void ") else name


def main():
    args = sys.argv[1:]
    drop = None
    if "--drop-arg" in args:
        i = args.index("--drop-arg")
        drop = args[i + 1]
        del args[i:i + 2]
    show = 0
    if "--show" in args:  # print the first N differing lines of each kernel
        i = args.index("--show")
        show = int(args[i + 1])
        del args[i:i + 2]
    old, new = kernels(args[0]), kernels(args[1])
    dold, dnew = demangle(list(old)), demangle(list(new))
    by_name = {}
    for mangled, name in dnew.items():
        key = name
        if drop and (drop + ">(") in name:
            key = name.replace(drop + ">(", ">(")
        elif drop and ("<" + drop.lstrip(", ") + ">(") in name:
            key = name.replace("<" + drop.lstrip(", ") + ">(", "(")
        by_name[plain(key)] = mangled
    bad = 0
    for mangled, name in sorted(dold.items(), key=lambda kv: kv[1]):
        partner = by_name.pop(plain(name), None)
        if partner is None:
            print("MISSING  %s" % name)
            bad = 1
            continue
        a, b = old[mangled], new[partner]
        # a kernel's own (mangled) name may appear in its operands
        b = [l.replace(partner, mangled) for l in b]
        if a == b:
            print("same     %6d instructions  %s" % (len(a), name))
        else:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("DIFFERS  %d vs %d instructions, first at %d  %s" % (len(a), len(b), first, name))
            bad = 1
            if show:
                for x, y in [(x, y) for x, y in zip(a, b) if x != y][:show]:
                    print("           - %s\n           + %s" % (x, y))
    for key, mangled in sorted(by_name.items()):
        print("new      %6d instructions  %s" % (len(new[mangled]), dnew[mangled]))
    return bad


if __name__ == "__main__":
    sys.exit(main())

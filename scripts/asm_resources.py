#!/usr/bin/env python3
"""Compare two `make asm` outputs kernel by kernel.

    scripts/asm_resources.py BEFORE_DIR AFTER_DIR [--map OLD_REGEX=NEW ...]

Each directory holds resource_usage.txt and bloom_kernels.s.  Kernels are keyed
by demangled name (source locations dropped); --map rewrites a BEFORE name
(re.sub) so that a kernel whose signature changed lines up with its successor.
Prints the kernels only one side has, every resource difference, and every
kernel whose ISA text differs once its own symbol and the function number in
its block labels are replaced (a few differing lines are printed).
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    short = [n.replace("void dlsm::(anonymous namespace)::", "") for n in out.split("\n")]
    return dict(zip(names, short))


def resources(path):
    table, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = table.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[key] = val
    return table


def bodies(path, wanted):
    """ISA text of each wanted symbol: from its label to its s_endpgm."""
    out, cur = {}, None
    for line in open(path):
        if cur is None:
            m = re.match(r"^(\S+):\s", line)
            if m and m.group(1) in wanted:
                cur = m.group(1)
                out[cur] = []
        else:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            if not re.match(r"\s*(;|\.)", line):  # comments and directives carry names and line numbers
                out[cur].append(re.sub(r"\.L(BB|tmp)\d+_", r".L\1_", line.replace(cur, "SELF")))
    return out


def main():
    argv, args, maps = sys.argv[1:], [], []
    while argv:
        a = argv.pop(0)
        if a == "--map":
            old, _, new = argv.pop(0).partition("=")
            maps.append((re.compile(old), new))
        else:
            args.append(a)
    before_dir, after_dir = args
    rb, ra = resources(before_dir + "/resource_usage.txt"), resources(after_dir + "/resource_usage.txt")
    db, da = demangle(list(rb)), demangle(list(ra))
    mapped = {}  # demangled-before -> (renamed, mangled)
    for mangled, name in db.items():
        new = name
        for rx, rep in maps:
            new = rx.sub(rep, new)
        mapped[new] = (name, mangled)
    after = {da[m]: m for m in ra}
    print(f"kernels: {len(rb)} before, {len(ra)} after")
    for name in sorted(set(mapped) - set(after)):
        print(f"gone: {mapped[name][0]}")
    for name in sorted(set(after) - set(mapped)):
        print(f"new:  {name}")
    same = diff = 0
    renamed = {}
    for name in sorted(set(after) & set(mapped)):
        old_name, old_m = mapped[name]
        b, a = rb[old_m], ra[after[name]]
        if b == a:
            same += 1
        else:
            diff += 1
            print(f"resources differ: {name}")
            for f in FIELDS:
                if b.get(f) != a.get(f):
                    print(f"    {f}: {b.get(f)} -> {a.get(f)}")
        renamed[old_m] = after[name]
    print(f"resources identical: {same}, different: {diff}")
    tb = bodies(before_dir + "/bloom_kernels.s", set(renamed))
    ta = bodies(after_dir + "/bloom_kernels.s", set(renamed.values()))
    isa_same = 0
    for old_m, new_m in sorted(renamed.items(), key=lambda kv: da[kv[1]]):
        x, y = tb[old_m], ta[new_m]
        pairs = [(p, q) for p, q in zip(x, y) if p != q]
        nd = len(pairs) + abs(len(x) - len(y))
        if nd == 0:
            isa_same += 1
            continue
        print(f"ISA {nd} of {len(x)} lines differ: {da[new_m]}")
        if db[old_m] != da[new_m]:
            print(f"    was {db[old_m]}")
        if len(x) == len(y) and nd <= 4:
            for p, q in pairs:
                print(f"    - {p.strip()}\n    + {q.strip()}")
    print(f"ISA identical: {isa_same} of {len(renamed)}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""devcmp.py PARENT.so NEW.so [--prefix NAME]: per-symbol comparison of the gfx950 code in two shared libraries."""
import hashlib, os, re, struct, subprocess, sys, tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path):
    data = open(path, "rb").read()
    out = []
    pos = 0
    while True:
        b = data.find(MAGIC, pos)
        if b < 0:
            break
        n = struct.unpack_from("<Q", data, b + 24)[0]
        p = b + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(data[b + off:b + off + size])
        pos = b + 24
    return out


def symbols(path):
    syms = {}
    for i, co in enumerate(code_objects(path)):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
            name = f.name
        txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", name], capture_output=True, text=True, check=True).stdout
        os.unlink(name)
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = m.group(1)
                k = 1  # a weak symbol that several translation units carry (library templates): name, name#2, ... sorted below
                while cur in syms:
                    k += 1
                    cur = m.group(1) + "#%d" % k
                syms[cur] = []
                continue
            if cur is None or not line.strip():
                continue
            syms[cur].append(line.split("//")[0].strip())
    # padding between functions and at the end of a code object belongs to no function
    for body in syms.values():
        while body and body[-1].startswith(("s_nop", "s_code_end", "...")):
            body.pop()
    # copies of one name in a canonical order, whatever the order of the translation units
    groups = {}
    for s in syms:
        groups.setdefault(s.split("#")[0], []).append(s)
    for base, names in groups.items():
        if len(names) > 1:
            bodies = sorted(syms[n] for n in names)
            for n, body in zip(sorted(names), bodies):
                syms[n] = body
    return syms


def main():
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    same = [s for s in a if s in b and a[s] == b[s]]
    differ = [s for s in a if s in b and a[s] != b[s]]
    missing = [s for s in a if s not in b]
    added = [s for s in b if s not in a]
    demangle = lambda s: subprocess.run(["c++filt", s.split("#")[0]], capture_output=True, text=True).stdout.strip()
    print(f"parent: {len(a)} device symbols, {sum(len(v) for v in a.values())} instructions")
    print(f"new:    {len(b)} device symbols, {sum(len(v) for v in b.values())} instructions")
    print(f"identical: {len(same)}   differing: {len(differ)}   missing in new: {len(missing)}   only in new: {len(added)}")
    for tag, lst in (("DIFFERS", differ), ("MISSING", missing), ("ADDED", added)):
        for s in sorted(lst):
            na = len(a.get(s, [])), len(b.get(s, []))
            print(f"{tag} {demangle(s)}  instructions parent {na[0]} new {na[1]}")
    for pref in ("extend_kernel", "seed_hit_kernel"):
        ss = [s for s in a if pref in s]
        print(f"{pref}: {len(ss)} instantiations, identical {sum(1 for s in ss if s in b and a[s] == b[s])}, "
              f"instructions parent {sum(len(a[s]) for s in ss)} new {sum(len(b.get(s, [])) for s in ss)}")


main()

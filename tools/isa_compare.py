#!/usr/bin/env python3
"""tools/isa_compare.py parent.s new.s: two gfx950 assembly files of hr_api.hip (tools/isa.sh's command with -S --offload-device-only, one per
commit) symbol by symbol.  Functions are matched by demangled name — a kernel that had C linkage in one build by its bare name — and compared as
text without the function's ordinal in its block labels (BB<n>_, .Lfunc_end<n>), which moves with the order of definition.  Prints every symbol
that differs with the count of changed lines, then the totals.  tools/kres_compare.py does the same for the resource remarks."""
import difflib
import re
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if name is None:
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name] = body
            name = None
            continue
        body.append(line)
    return out


def norm(lines, own):
    res = []
    for l in lines:
        l = re.sub(r"BB\d+_", "BB_", l)
        l = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", l)
        l = l.replace(own, "<self>")
        res.append(l)
    return res


def demangle(names):
    d = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return dict(zip(names, d))


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    da, db = demangle(list(a)), demangle(list(b))
    # a kernel that had C linkage in the parent demangles to its bare name: match on the name before the argument list when the full one is missing
    bare = lambda s: re.sub(r"^void ", "", s).split("(")[0]
    A = {}
    for n in a:
        A[da[n]] = n
        A.setdefault(bare(da[n]), n)
    same = differ = 0
    missing = []
    for n in b:
        key = db[n] if db[n] in A else bare(db[n])
        if key not in A:
            missing.append(db[n])
            continue
        pn = A[key]
        x, y = norm(a[pn], pn), norm(b[n], n)
        if x == y:
            same += 1
        else:
            differ += 1
            changed = sum(1 for l in difflib.unified_diff(x, y, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print("DIFFERS  %-90s %d of %d lines" % (db[n][:90], changed, len(y)))
    gone = [da[n] for n in a if da[n] not in set(db.values()) and bare(da[n]) not in {bare(v) for v in db.values()}]
    print("%d symbols in the new build: %d byte-identical to the parent's, %d differ, %d without a parent" % (len(b), same, differ, len(missing)))
    for m in missing:
        print("  new: " + m)
    for g in gone:
        print("  gone: " + g)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/kres_compare.py parent_remarks.txt new_remarks.txt: the kernels' resource figures (tools/kres.py's parse of `hipcc
-Rpass-analysis=kernel-resource-usage` output) of two builds side by side, by demangled name.  An instantiation whose template list only grew by
trailing `false` arguments is matched with the parent's spelling of it; what the parent does not have is listed apart.
PARENT_ARITY below is the number of template arguments each kernel family had in the PARENT build: it is a table, not derived — when a family
gains or loses a template parameter, bring it up to date for the next comparison, or its rows will all be listed as new."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402

PARENT_ARITY = {"trace_kernel": 7, "accumulate_kernel": 3, "wf_start_kernel": 2, "seed_seg_kernel": 4, "noise_kernel": 1}
PATTERN = re.compile(r"trace_kernel|seed_seg_kernel|accumulate_kernel|wf_|tonemap|bilateral|noise_kernel|governor|select_|counts_min|seed_isaac64|seed_pc|debug_render|trace_debug|guide_|atrous|denoise_|bucket_kernel|robust_kernel|restore_|spread_")
KEYS = ["vgpr", "sgpr", "vspill", "sspill", "scratch", "lds", "occ"]


def demangled(table):
    names = list(table)
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    return {re.sub(r"\(.*$", "", re.sub(r"^void ", "", d)): table[n] for n, d in zip(names, out)}


def parent_name(name):
    """The parent's spelling of the same instantiation, or None when the appended template arguments are not all `false`."""
    m = re.match(r"(\w+)<(.*)>$", name)
    if not m or m.group(1) not in PARENT_ARITY:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    base = PARENT_ARITY[m.group(1)]
    if any(a != "false" for a in args[base:]):
        return None
    return "%s<%s>" % (m.group(1), ", ".join(args[:base])) if base else m.group(1)


def main():
    old, new = demangled(kres.parse(sys.argv[1])), demangled(kres.parse(sys.argv[2]))
    cells = lambda v: "  ".join("%7s" % v.get(k) for k in KEYS)   # noqa: E731
    print("%-78s %s" % ("kernel", "  ".join("%7s" % k for k in KEYS)))
    same = diff = 0
    fresh = []
    for name, v in new.items():
        if not PATTERN.search(name):
            continue
        p = parent_name(name)
        if p is None or p not in old:
            fresh.append((name, v))
            continue
        eq = all(old[p].get(k) == v.get(k) for k in KEYS)
        same += eq
        diff += not eq
        print("%-78s %s  %s" % (name, cells(v), "same as parent" if eq else "PARENT: " + cells(old[p])))
    print("\nnew in this build:")
    for name, v in fresh:
        print("%-78s %s" % (name, cells(v)))
    print("\n%d kernels the parent also has: %d with identical figures, %d that differ" % (same + diff, same, diff))


if __name__ == "__main__":
    main()

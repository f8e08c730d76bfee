#!/usr/bin/env python3
"""Whether a change left existing kernels' machine code alone: compare the function
bodies of every kernel whose name contains SUBSTR in two device assembly listings

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S file.hip -o listing.s

of the same source file at two commits.  Kernels are matched by their leading
template arguments (a new trailing template parameter renames every instantiation;
--new-suffix picks the instantiations of the new listing that stand for the old
ones, e.g. 'Lb0E' for a new bool parameter that is false).  Symbol names are
normalised before comparing, so only instructions, labels and directives inside
the bodies count.  Also prints each kernel's VGPRs, SGPRs, scratch and kernarg
bytes.  Exit status 1 when a body differs or a kernel has no counterpart."""
import argparse
import re
import sys


def bodies(path, sub):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and sub in m.group(1):
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            if line.startswith("\t.section") or line.startswith(".Lfunc_end"):
                cur = None
            else:
                out[cur].append(re.sub(r"_Z\w*%s\w*" % re.escape(sub), "K", line))
    return out


def resources(path, sub):
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*%s\S*)(.*?)\.end_amdhsa_kernel" % re.escape(sub), open(path).read(), re.S):
        get = lambda k: re.search(r"\.amdhsa_%s (\S+)" % k, m.group(2)).group(1)  # noqa: E731
        res[m.group(1)] = "vgpr %s sgpr %s scratch %s kernarg %s" % (
            get("next_free_vgpr"), get("next_free_sgpr"), get("private_segment_fixed_size"), get("kernarg_size"))
    return res


def targs(name, sub):
    """The template-argument string that follows the kernel's name in the mangling."""
    return name.split(sub, 1)[1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("substr")
    ap.add_argument("--new-suffix", default="", help="mangled text of the new trailing template argument(s)")
    a = ap.parse_args()
    old, new = bodies(a.old, a.substr), bodies(a.new, a.substr)
    r_old, r_new = resources(a.old, a.substr), resources(a.new, a.substr)
    bad = 0
    matched = set()
    for name in old:
        lead = re.match(r"I((?:L[a-z]\d+E)+)", targs(name, a.substr)).group(1)
        cand = [n for n in new if targs(n, a.substr).startswith("I" + lead + a.new_suffix)
                and re.match(r"I((?:L[a-z]\d+E)+)", targs(n, a.substr)).group(1) == lead + a.new_suffix]
        if len(cand) != 1:
            print("%s: %d counterparts" % (lead, len(cand)))
            bad += 1
            continue
        matched.add(cand[0])
        same = old[name] == new[cand[0]]
        bad += not same
        print("%s: %s (%d lines); old %s; new %s" % (lead, "identical" if same else "DIFFERENT", len(old[name]),
                                                     r_old.get(name), r_new.get(cand[0])))
    for n in new:
        if n not in matched:
            print("new only %s: %s" % (re.match(r"I((?:L[a-z]\d+E)+)", targs(n, a.substr)).group(1), r_new.get(n)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

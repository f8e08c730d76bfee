#!/usr/bin/env python3
"""Whether a change left existing kernels' machine code alone: compare the function
bodies of every kernel whose name contains SUBSTR in two device assembly listings

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S file.hip -o listing.s

of the same source file at two commits, or of the file a kernel moved out of and the
one it moved into.  Kernels are matched by name and leading template arguments, a
kernel without template arguments on either side by its name alone (a new trailing
template parameter renames every instantiation; --new-suffix picks the instantiations
of the new listing that stand for the old ones, e.g. 'Lb0E' for a new bool parameter
that is false).  Symbol names and the file-wide numbering of local labels are
normalised before comparing, so only instructions, labels and directives inside the
bodies count.  Also prints each kernel's VGPRs, SGPRs, scratch and kernarg
bytes, and its instruction count.  Exit status 1 when a body differs or a kernel has
no counterpart."""
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
                out[cur].append(local_labels(re.sub(r"_Z\w*%s\w*" % re.escape(sub), "K", line)))
    return out


def local_labels(line):
    """Block and jump-table labels carry the function's ordinal in its file (.LBB36_3,
    'Header=BB36_92' in a comment): drop it, and the padding before a label's comment
    that its length shifts, so a kernel that moved to another file (or past other
    functions) still compares."""
    line = re.sub(r"(?<!\w)(\.L)?(BB|JTI)\d+_(\d+)", r"\1\2_\3", line)
    return re.sub(r"^(\.L\w+:)\s+;", r"\1 ;", line)


def resources(path, sub):
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S*%s\S*)(.*?)\.end_amdhsa_kernel" % re.escape(sub), open(path).read(), re.S):
        get = lambda k: re.search(r"\.amdhsa_%s (\S+)" % k, m.group(2)).group(1)  # noqa: E731
        res[m.group(1)] = "vgpr %s sgpr %s scratch %s kernarg %s" % (
            get("next_free_vgpr"), get("next_free_sgpr"), get("private_segment_fixed_size"), get("kernarg_size"))
    return res


def ninstr(body):
    return sum(1 for x in body if x.startswith("\t") and not x.startswith(("\t.", "\t;")))


def key(name, sub):
    """(the kernel's own name, its leading template arguments or '' without any) from
    the mangling: SUBSTR may match several kernels (k_rle_scan: k_rle_scan16b<..>,
    k_rle_scan_fold), with or without template arguments."""
    for m in re.finditer(r"\d+", name):
        for i in range(m.start(), m.end()):  # 'N_118k_x': the length is a suffix of the digits
            n = int(name[i:m.end()])
            ident = name[m.end():m.end() + n]
            if len(ident) == n and sub in ident and name[m.end() + n:m.end() + n + 1] in ("I", "E"):
                rest = name[m.end() + n:]
                t = re.match(r"I((?:L[a-z]\d+E)+)", rest)
                # (type arguments: the rest of the mangling tells the instantiations apart)
                return ident, t.group(1) if t else (rest if rest.startswith("I") else "")
    return name, ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("substr")
    ap.add_argument("--new-suffix", default="", help="mangled text of the new trailing template argument(s)")
    a = ap.parse_args()
    old, new = bodies(a.old, a.substr), bodies(a.new, a.substr)
    r_old, r_new = resources(a.old, a.substr), resources(a.new, a.substr)
    show = lambda k: k[0] + ("<%s>" % k[1] if k[1] else "")  # noqa: E731
    bad = 0
    matched = set()
    for name in old:
        base, lead = key(name, a.substr)
        # a kernel without template arguments on either side is matched by its name alone
        cand = [n for n in new if key(n, a.substr)[0] == base
                and (not lead or not key(n, a.substr)[1] or key(n, a.substr)[1] == lead + a.new_suffix)]
        if len(cand) != 1:
            print("%s: %d counterparts; old %s" % (show((base, lead)), len(cand), r_old.get(name)))
            bad += 1
            continue
        matched.add(cand[0])
        same = old[name] == new[cand[0]]
        bad += not same
        print("%s: %s (%d -> %d instructions); old %s; new %s" % (
            show((base, lead)), "identical" if same else "DIFFERENT", ninstr(old[name]), ninstr(new[cand[0]]),
            r_old.get(name), r_new.get(cand[0])))
    for n in new:
        if n not in matched:
            print("new only %s: %s" % (show(key(n, a.substr)), r_new.get(n)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""kernel_asm_diff.py BEFORE.s AFTER.s -- compare, kernel by kernel, the instructions of two device-only assembly listings of one
translation unit (what tools/kernel_resources.sh leaves in /tmp/isa).  A kernel's text is everything between its label and its
.Lfunc_end; comment lines, local labels' numbers and the listing's directives are dropped, so two builds whose kernels are the same
instructions compare equal even when the compiler numbered their basic blocks differently.  Prints one line per kernel present in
both listings (identical / N differing lines) and lists the kernels only one side has.  For a kernel that differs it also compares
the two instruction MULTISETS with register numbers blanked: how many instructions one side has and the other has not, and how many
of those compute on floating-point values (v_*_f32 / f16 / f64, MFMA, conversions, v_exp / v_rcp, DPP maxima) -- zero there means the
two builds perform the same arithmetic and differ in integer address arithmetic, scalar bookkeeping and register assignment only."""
import collections
import difflib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", t):
                body.append("<label>")
            continue
        body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    for k in a:
        if k not in b:
            print("only before: %s" % k)
            continue
        if a[k] == b[k]:
            print("identical (%5d instructions)  %s" % (len([x for x in a[k] if x != "<label>"]), k[:90]))
        else:
            d = [l for l in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            print("DIFFERENT (%d lines of %d)  %s" % (len(d), len(a[k]), k[:90]))
            ca, cb = (collections.Counter(re.sub(r"\b([vsa])\[?\d+(:\d+)?\]?", r"\1#", x) for x in side) for side in (a[k], b[k]))
            only_a, only_b = ca - cb, cb - ca
            fp = lambda c: sum(n for t, n in c.items() if re.match(r"v_(mfma|exp|rcp|cvt|fma|pk_)|v_\w+_(f16|f32|f64|bf16)", t))
            print("    register numbers blanked: %d instructions only before, %d only after; floating-point among them: %d / %d"
                  % (sum(only_a.values()), sum(only_b.values()), fp(only_a), fp(only_b)))
            for l in d[:int(sys.argv[3]) if len(sys.argv) > 3 else 0]:
                print("    " + l)
    for k in b:
        if k not in a:
            print("only after:  %s" % k[:100])


if __name__ == "__main__":
    main()

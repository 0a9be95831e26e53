#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assembly files (hipcc <the file's Makefile flags> --cuda-device-only -S), for a change that
moves kernels between files, where a per-file diff says nothing.  A body runs from its `_Z...:` label to `.Lfunc_end`; lines with
__hip_cuid_, the function index in .LBBn_ labels and trailing `;` comments are dropped.  Prints the kernels whose bodies differ and those on one
side only; exit status 1 if any body differs.   usage: tools/kernel_asm_diff.py parent.s change.s [parent.s change.s ...]
A kernel that changed its name is compared by listing the pair:  --pair <name in parent> <name in change>  (substrings of the mangled names)."""
import re, sys

def bodies(path):
    out, cur = {}, None
    for l in open(path):
        m = re.match(r'^(_Z\w+):', l)
        if m: cur = m.group(1); out[cur] = []
        elif l.startswith('.Lfunc_end'): cur = None
        elif cur and '__hip_cuid_' not in l:      # (a body ends with its kernel descriptor, which names the kernel and returns to its section)
            l = '\t.text' if l.startswith('\t.section\t.text.') else l.replace(cur, '@')
            out[cur].append(re.sub(r'\.LBB\d+_', '.LBB_', l.split(';')[0]).rstrip())
    return out

args, pairs = sys.argv[1:], []
while '--pair' in args: i = args.index('--pair'); pairs.append((args[i + 1], args[i + 2])); del args[i:i + 3]
a, b = {}, {}
for k in range(0, len(args), 2): a.update(bodies(args[k])); b.update(bodies(args[k + 1]))
for pa, pb in pairs:      # rename the change's kernel to the parent's name
    na, nb = [n for n in a if pa in n], [n for n in b if pb in n]
    assert len(na) == 1 and len(nb) == 1, (pa, na, pb, nb)
    b[na[0]] = b.pop(nb[0])
differ = [n for n in sorted(a) if n in b and a[n] != b[n]]
for n in differ: print("DIFFERS  %s  (%d -> %d lines)" % (n, len(a[n]), len(b[n])))
for n in sorted(set(a) - set(b)): print("parent only  " + n)
for n in sorted(set(b) - set(a)): print("change only  " + n)
print("%d kernels on both sides, %d identical" % (len(set(a) & set(b)), len(set(a) & set(b)) - len(differ)))
sys.exit(1 if differ else 0)

#!/usr/bin/env python3
"""Instruction counts along one path through a kernel in a hipcc -S listing (tools/isa_blocks.py counts whole blocks).
   tools/isa_path.py file.s <kernel-name-substring> <step> [<step> ...]
A step is a label of the kernel without its dot: "LBB8_52" counts from that label to the next label (branches on the way fall through);
"LBB8_52>LBB8_54" counts from the label up to and including the branch to the second label (the branch is taken).  The steps need
not be contiguous: the path is the reader's, read off the listing.  Prints vector-ALU (v_*), LDS (ds_*), vector memory and scalar
counts per step and in total, and the v_* opcodes of the whole path."""
import collections
import re
import sys


def main():
    s = open(sys.argv[1]).read()
    m = re.search(r'^(\S*%s\S*):.*?\n(.*?)\n\s*s_endpgm' % re.escape(sys.argv[2]), s, re.S | re.M)
    if not m:
        sys.exit("no kernel matching %r" % sys.argv[2])
    lines = m.group(2).split('\n')
    labels = {}
    for i, l in enumerate(lines):
        mm = re.match(r'^\.(LBB\d+_\d+):', l)
        if mm:
            labels[mm.group(1)] = i
    total = collections.Counter()
    ops = collections.Counter()
    for step in sys.argv[3:]:
        start, _, until = step.partition('>')
        if start not in labels or (until and until not in labels):
            sys.exit("no label for step %r" % step)
        c = collections.Counter()
        i = labels[start] + 1
        while i < len(lines):
            l = lines[i]
            if not until and re.match(r'^\.LBB\d+_\d+:', l):
                break
            t = l.strip()
            i += 1
            if not t or t[0] in ';.':
                continue
            op = t.split()[0]
            kind = ('valu' if op.startswith('v_') else 'lds' if op.startswith('ds_') else
                    'vmem' if op.startswith(('global_', 'scratch_', 'buffer_', 'flat_')) else 'scalar')
            c[kind] += 1
            if kind == 'valu':
                ops[re.sub(r'_(e32|e64|dpp|sdwa)$', '', op)] += 1
            if until and re.match(r's_c?branch\w*\s+\.%s$' % re.escape(until), t):
                break
        else:
            if until:
                sys.exit("step %r: no branch to %s behind %s" % (step, until, start))
        print("%-22s valu %4d  lds %3d  vmem %3d  scalar %4d" % (step, c['valu'], c['lds'], c['vmem'], c['scalar']))
        total.update(c)
    print("%-22s valu %4d  lds %3d  vmem %3d  scalar %4d" % ("path", total['valu'], total['lds'], total['vmem'], total['scalar']))
    print("  " + ' '.join("%s:%d" % kv for kv in ops.most_common()))


if __name__ == "__main__":
    main()

"""Loops of a kernel in a hipcc -S listing and their instruction mix:
python tools/isa_loops.py file.s name [top]
Per loop: the instruction count, its split into MFMA / AccVGPR moves / other
VALU / SALU / memory / other (waits, branches, barriers), and the `top` most
frequent opcodes."""
import re
import sys
from collections import Counter

s = open(sys.argv[1]).read()
m = re.search(r'^(_Z[\w]*%s[\w]*):[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(sys.argv[2]), s, re.S | re.M)


def code(line):
    """A listing line without its comment (`.LBB2_8: ; =>This Inner Loop ...` is a label)."""
    return line.split(';', 1)[0].strip()


lines = [code(l) for l in m.group(2).splitlines()]
labels = {t[:-1]: i for i, t in enumerate(lines) if t.startswith('.LBB') and t.endswith(':')}
OTHER = ('s_waitcnt', 's_nop', 's_branch', 's_cbranch', 's_barrier', 's_endpgm', 's_sleep', 's_setprio', 's_sethalt')
MEMORY = ('buffer_', 'global_', 'flat_', 'scratch_', 'ds_', 's_load', 's_buffer_load')


def ops(seg):
    return [t.split()[0] for t in seg if t and not t.startswith('.') and not t.endswith(':')]


def kind(op):
    if op.startswith('v_mfma') or op.startswith('v_smfmac'):
        return 'mfma'
    if op.startswith('v_accvgpr'):
        return 'accvgpr'
    if op.startswith(MEMORY):
        return 'memory'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith(OTHER):
        return 'other'
    if op.startswith('s_'):
        return 'salu'
    return 'other'


print(m.group(1), 'instructions', len(ops(lines)))
for i, t in enumerate(lines):
    if 'branch' in t:
        tgt = t.split()[-1]
        if tgt in labels and labels[tgt] < i:
            o = ops(lines[labels[tgt]:i + 1])
            c = Counter(o)
            k = Counter(kind(x) for x in o)
            print('loop', tgt, 'instructions', len(o))
            print('   split', ' '.join('%s %d' % (n, k[n]) for n in ('mfma', 'accvgpr', 'valu', 'salu', 'memory', 'other')))
            print('  ', sorted(c.items(), key=lambda x: -x[1])[:int(sys.argv[3]) if len(sys.argv) > 3 else 30])

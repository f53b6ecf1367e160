"""Compare the loops of the kernels whose demangled name contains PATTERN in two device-ISA dumps of the same source
(tools/isa/dump.sh, e.g. before and after an epilogue change):

    python tools/isa/loop_diff.py before.s after.s "k_reduce_rows"

The loops are the basic blocks LLVM's comments place in a loop (header, body, latch); kernels are matched by name without
their parameter list (an added argument does not hide them).  Label numbers are normalised; everything else (opcodes,
registers, offsets, waits) must match for 'identical'; 'renamed' = the same opcode sequence with other register numbers
(e.g. one more scalar live through the kernel); 'DIFFERS' = another instruction sequence, exit status 1."""
import re
import subprocess
import sys


def kernels(path, pat):
    out, cur = {}, None
    for line in open(path).read().split('\n'):
        m = re.match(r'^(_Z\w+):\s', line)
        if m:
            name = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip()
            name = name.split('(')[0]
            cur = out.setdefault(name, []) if pat in name else None
        elif cur is not None:
            cur.append(line)
            if 's_endpgm' in line:
                cur = None
    return out


def loops(body):
    """Instructions of every basic block LLVM places inside a loop (header, body, latch), in layout order."""
    ins, inloop = [], False
    for raw in body:
        m = re.match(r'^(\.LBB\w+|; %bb\.\d+):\s*(.*)$', raw)
        if m:
            inloop = 'Loop' in m.group(2)
            continue
        t = raw.split(';')[0].strip()
        if inloop and t and not t.startswith('.'):
            ins.append(re.sub(r'\.LBB\d+_\d+', 'L', t))
    return ins


def main():
    a, b, pat = sys.argv[1:4]
    ka, kb = kernels(a, pat), kernels(b, pat)
    bad = 0
    for name in sorted(set(ka) | set(kb)):
        la, lb = loops(ka.get(name, [])), loops(kb.get(name, []))
        ops = [t.split()[0] for t in la] == [t.split()[0] for t in lb]
        verdict = 'identical' if la == lb else 'renamed' if ops else 'DIFFERS'
        bad += verdict == 'DIFFERS'
        print('%-9s %5d / %5d loop instructions  %s' % (verdict, len(la), len(lb), name))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()

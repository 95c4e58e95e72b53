"""Kernel resource table from the remarks of `hipcc ... -Rpass-analysis=kernel-resource-usage` (stderr saved to a file).

    python tools/resource_table.py PARENT.log CHANGE.log      one markdown row per kernel, parent / change; differing rows are marked"""
import re
import subprocess
import sys

KEYS = ['VGPRs', 'AGPRs', 'TotalSGPRs', 'ScratchSize [bytes/lane]', 'Occupancy [waves/SIMD]', 'LDS Size [bytes/block]']


def parse(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r'remark: (?:\[[^\]]*\])?\s*(.*)$', line)
        if not m:
            continue
        t = m.group(1).replace('[-Rpass-analysis=kernel-resource-usage]', '').strip()
        if t.startswith('Function Name:'):
            name = t.split(':', 1)[1].strip()
            out[name] = {}
        elif name and ':' in t:
            k, v = t.rsplit(':', 1)
            if k.strip() in KEYS:
                out[name][k.strip()] = v.strip()
    return out


def demangle(names):
    try:
        res = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return {n: re.sub(r'\(.*', '', re.sub(r'^void ', '', r.replace('(anonymous namespace)::', ''))) for n, r in zip(names, res)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(parent, change):
    p, c = parse(parent), parse(change)
    names = sorted(set(p) | set(c))
    short = demangle(names)
    print('| kernel | ' + ' | '.join(k.split(' [')[0] for k in KEYS) + ' | |')
    print('|---' * (len(KEYS) + 2) + '|')
    for n in names:
        cells, diff = [], False
        for k in KEYS:
            a, b = p.get(n, {}).get(k, '-'), c.get(n, {}).get(k, '-')
            diff |= a != b
            cells.append(a if a == b else '%s / %s' % (a, b))
        print('| `%s` | ' % short[n] + ' | '.join(cells) + ' | %s |' % ('changed' if diff else ''))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])

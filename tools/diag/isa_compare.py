"""per-kernel comparison of two builds' device assembly (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S), next to regs.py:
    isa_compare.py --old gemm.s --new gemm_nt.s gemm_tn.s
For every kernel (matched by mangled name) the memory, matrix and synchronisation instructions must be the same in number AND in
order (a cluster of MFMAs that drifts across a barrier keeps every count), and the scratch size, the occupancy and the static LDS bytes
equal; register counts and every other mnemonic that moved are listed.  Exit 1 on a mismatch."""
import argparse, collections, re, subprocess, sys

# longest prefix wins: global_load_lds* is counted apart from global_load*
PINNED = ('v_mfma', 'ds_read', 'ds_write', 'global_load_lds', 'global_load', 'global_store', 'global_atomic', 's_barrier', 's_waitcnt', 's_setprio')
MUST = ('ScratchSize', 'Occupancy', 'LDSByteSize')
INFO = ('NumVgprs', 'NumAgprs')


def pin(op):
    return max((p for p in PINNED if op.startswith(p)), key=len, default=None)


def kernels(paths):
    """{mangled name: ops (mnemonic histogram), seq (pinned instructions in order), info (the figures hipcc prints after the body)}"""
    out, cur, body = {}, None, False
    for path in paths:
        for line in open(path):
            m = re.match(r'\s+\.type\s+(\S+),@function', line)
            if m:
                cur, body = {'ops': collections.Counter(), 'seq': [], 'info': {}}, True
                out[m.group(1)] = cur
            elif cur is None:
                continue
            elif line.startswith('.Lfunc_end'):
                body = False
            elif body and re.match(r'\t[a-z]\w+', line):
                op = line.split()[0]
                cur['ops'][op] += 1
                if pin(op):
                    cur['seq'].append(op)
            else:
                m = re.match(r'; (\w+): (\d+)', line)
                if m and m.group(1) in MUST + INFO:
                    cur['info'].setdefault(m.group(1), int(m.group(2)))
    return out


ap = argparse.ArgumentParser()
ap.add_argument('--old', nargs='+', required=True)
ap.add_argument('--new', nargs='+', required=True)
a = ap.parse_args()
old, new = kernels(a.old), kernels(a.new)
names = subprocess.run(['c++filt'], input='\n'.join(old), capture_output=True, text=True).stdout.split('\n')
bad = identical = 0
for k, dn in zip(old, names):
    dn = dn.replace('(anonymous namespace)::', '').replace('dgemm::', '')
    if k not in new:
        print('MISSING ', dn)
        bad += 1
        continue
    o, n = old[k], new[k]
    fail = [f'{x} {o["info"].get(x)} -> {n["info"].get(x)}' for x in MUST if o['info'].get(x) != n['info'].get(x)]
    po, pn = (collections.Counter(map(pin, x['seq'])) for x in (o, n))
    fail += [f'{p} {po[p]} -> {pn[p]}' for p in PINNED if po[p] != pn[p]]
    if not fail and o['seq'] != n['seq']:
        at = next(i for i, (x, y) in enumerate(zip(o['seq'], n['seq'])) if x != y)
        fail.append(f'order differs from pinned instruction {at} of {len(o["seq"])}: {" ".join(o["seq"][at:at + 4])} -> {" ".join(n["seq"][at:at + 4])}')
    moved = [f'{x} {o["info"].get(x)} -> {n["info"].get(x)}' for x in INFO if o['info'].get(x) != n['info'].get(x)]
    moved += [f'{op} {o["ops"][op]} -> {n["ops"][op]}' for op in sorted(set(o['ops']) | set(n['ops'])) if o['ops'][op] != n['ops'][op] and not pin(op)]
    bad += bool(fail)
    identical += not fail and not moved
    if fail or moved:
        print('MISMATCH' if fail else 'moved   ', dn, '|', '; '.join(fail + moved))
extra = sorted(set(new) - set(old))
print(f'{len(old)} kernels: {identical} identical, {len(old) - identical - bad} with allowed differences, {bad} mismatched; new only: {len(extra)}')
sys.exit(1 if bad or extra else 0)

"""Bits of the two loss entries (dclip_distill_loss / _rows, dclip_interactive_loss) over a fixed case list, for comparing two builds of the
library (profiles/loss_stripes_ab.txt).  Not a test: a permanent pin of the bits would forbid every later numeric improvement.
    python tools/diag/loss_bits.py [--lib PATH/libdistillclip_hip.so] [--host-only] > run.txt      one fresh process per run
    python tools/diag/loss_bits.py --compare parent1.txt parent2.txt new1.txt [new2.txt ...] [--parents 2]
A run prints `ws <entry> <B> <E> <bytes>` for the two workspace queries (host functions: --host-only stops there, no GPU needed), then
one line per case and output, `<case> <output> <sha256 of the tensor's bytes>`, and for the 16 scalars of dclip_distill_loss also
`<case> scalars <16 hex words>`.  The cases are the shapes the tests name (tests/test_loss_exact_gpu.py, tests/icl_cases.py):
  SWEEP with W_ALL and with every term alone; the BLOCKS and PARTITION row blocks of B = 130 at E in BLOCK_E without statistics (cos_diff,
  logits_mse and the tower terms) and with gathered ones (W_ALL: a statistics-only call per block, then the gradient calls); statistics-only
  calls that own every row; one tower; B = 1 (part of SWEEP); B = 512 at E = 512; every case of icl_cases.CASES.
--compare: every line but the distill scalars must be equal in all files (gradients, statistics and the interactive entry use no
atomics).  The distill scalars are sums of atomically accumulated copies: a slot on which the parent's two runs agree must be the same
in every new run; a slot on which they differ is listed with all values and not held (tests/test_loss_exact_gpu.py bounds it).
Exit 1 on a required equality that fails."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
WS_B, WS_E = (1, 8, 17, 130, 512, 4096), (16, 48, 272, 768, 1024)


def run(args):
    import torch
    import distillclip_amd._lib as _lib
    if args.lib:
        _lib._LIB_PATH = os.path.abspath(args.lib)
    l = _lib.lib()
    for B in WS_B:
        for E in WS_E:
            print(f'ws distill {B} {E} {l.dclip_distill_loss_workspace(B, E)}')
            print(f'ws interactive {B} {E} {l.dclip_interactive_loss_workspace(B, E)}')
    if args.host_only:
        return
    import icl_cases as ic
    import test_loss_exact_gpu as tl
    from distillclip_amd import ops
    dev = torch.device('cuda', 0)

    def show(case, **tensors):
        for name, t in tensors.items():
            if t is None:
                continue
            raw = t.detach().contiguous().cpu().numpy().tobytes()
            print(f'{case} {name} {hashlib.sha256(raw).hexdigest()}')
            if name == 'out' and case.startswith('distill'):
                print(f'{case} scalars {" ".join(f"{w & 0xffffffff:08x}" for w in t.cpu().view(torch.int32).tolist())}', flush=True)

    def distill(case, e, weights, tau, two=True, **kw):
        a = [e[k].to(dev) for k in (('si', 'ti', 'st', 'tt') if two else ('si', 'ti'))]
        r = ops.distill_loss(*a, weights=weights, temperature=tau, **kw)
        torch.cuda.synchronize()
        if kw.get('stats_only'):
            show(case, stats=r)
            return r
        show(case, out=r[0], d_img=r[1], d_txt=r[2])

    alone = [({n: 1.0}, 0.5 if n in ('out_kl', 'soft_label') else None) for n in tl.NAMES]
    for B, E in tl.SWEEP + [(512, 512)]:
        e = tl.inputs(B, E) if (B, E) in tl.SWEEP else tl._draw(B, E, 2022)
        distill(f'distill/B{B}-E{E}/all', e, tl.W_ALL, 0.5)
        for w, tau in alone:
            distill(f'distill/B{B}-E{E}/{next(iter(w))}', e, w, tau)
    for B, E in ((17, 48), (130, 768)):
        distill(f'distill/B{B}-E{E}/one-tower', tl.inputs(B, E), {n: tl.W_ALL[n] for n in tl.TOWER}, 2.0, two=False)
    for B, E in ((17, 48), (40, 768), (130, 272)):
        distill(f'distill/B{B}-E{E}/stats-only', tl.inputs(B, E), tl.W_ALL, 2.0, row0=0, rows=B, stats_only=True)
    blocks = sorted(set(tl.BLOCKS) | set(tl.PARTITION))
    no_stats = {n: tl.W_ALL[n] for n in tl.TOWER + ['cos_diff', 'logits_mse']}
    for E in tl.BLOCK_E:
        B, e = 130, tl.inputs(130, E)
        for r0, rows in blocks:
            distill(f'distill/B{B}-E{E}/rows{r0}+{rows}', e, no_stats, 0.5, row0=r0, rows=rows)
        gathered = torch.empty(6, B, device=dev)
        for r0, rows in tl.PARTITION:
            gathered[:, r0:r0 + rows] = distill(f'distill/B{B}-E{E}/rows{r0}+{rows}/stats-only', e, tl.W_ALL, 0.5, row0=r0, rows=rows,
                                                stats_only=True)
        for r0, rows in blocks:
            distill(f'distill/B{B}-E{E}/rows{r0}+{rows}/gathered', e, tl.W_ALL, 0.5, row0=r0, rows=rows, gathered_stats=gathered)
    for c in ic.CASES:
        out, di, dt = ops.interactive_loss(*(c.e[k].to(dev) for k in ic.KEYS), c.tau)
        torch.cuda.synchronize()
        show(f'icl/{c!r}', out=out, d_img=di, d_txt=dt)


def compare(paths, nparent):
    import struct
    runs = []
    for p in paths:
        d = {}
        for line in open(p):
            f = line.split()
            if len(f) >= 3 and (f[0] == 'ws' or '/' in f[0]):
                key = ' '.join(f[:4]) if f[0] == 'ws' else f'{f[0]} {f[1]}'
                d[key] = f[4:] if f[0] == 'ws' else f[2:]
        runs.append(d)
    p1, parents, news = runs[0], runs[:nparent], runs[nparent:]
    same = lambda rs, key, pick=lambda v: v: all(pick(r[key]) == pick(rs[0][key]) for r in rs)
    bad = 0
    for i, r in enumerate(runs[1:], 1):
        if set(r) != set(p1):
            print(f'{paths[i]}: {len(set(r) ^ set(p1))} lines that {paths[0]} lacks or has alone')
            bad += 1
    kinds = {}
    val = lambda h: struct.unpack('f', struct.pack('I', int(h, 16)))[0]
    for key in p1:
        if any(key not in r for r in runs):
            continue
        case, name = key.rsplit(' ', 1) if not key.startswith('ws') else (key, 'workspace bytes')
        atomic = case.startswith('distill') and name in ('out', 'scalars')
        kind = ('icl ' if case.startswith('icl') else '' if key.startswith('ws') else 'distill ') + name
        k = kinds.setdefault(kind, dict(lines=0, parent_differs=0, new_differs=0))
        k['lines'] += 1
        if name == 'out' and atomic:                        # judged slot by slot on the `scalars` line
            k['parent_differs'] += not same(parents, key)
            continue
        if name == 'scalars':
            for slot in range(16):
                pick = lambda v: v[slot]
                vals = ' '.join(f'{pick(r[key])} ({val(pick(r[key]))!r})' + (' |' if i == nparent - 1 else '') for i, r in enumerate(runs))
                if not same(parents, key, pick):
                    k['parent_differs'] += 1
                    print(f'not held (the parent differs from itself): {case} slot {slot}: {vals}')
                elif not same(runs, key, pick):
                    k['new_differs'] += 1
                    print(f'DIFFERS{"" if same(news, key, pick) else " (and the new runs from each other)"}: {case} slot {slot}: {vals}')
            continue
        if not same(parents, key):
            k['parent_differs'] += 1
            print(f'the parent differs from itself where no atomics are used: {key}')
        if any(n[key] != p1[key] for n in news):
            k['new_differs'] += 1
            print(f'DIFFERS: {key}')
    for kind, k in kinds.items():
        unit = 'slots' if kind.endswith('scalars') else 'lines'
        print(f'{kind:24s} {k["lines"]:5d} lines: parent against itself {k["parent_differs"]} {unit} differ; '
              f'new against parent {k["new_differs"]} {unit} differ' + (' (where the parent agrees with itself)' if unit == 'slots' else ''))
        bad += k['new_differs'] if kind != 'distill out' else 0
    print('EQUAL' if not bad else f'{bad} required equalities failed')
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib')
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--compare', nargs='+')
    ap.add_argument('--parents', type=int, default=2, help='--compare: how many of the files, the first ones, are runs of the parent')
    a = ap.parse_args()
    sys.exit(compare(a.compare, a.parents) if a.compare else run(a))

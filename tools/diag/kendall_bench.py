"""Kendall tau against human ratings: `dclip_kendall_tau` at the two sizes the caption-metric literature reports,
n = 16 992 (Flickr8k-Expert: 5 664 scores x 3 annotators, ratings in {1..4}) and n = 47 830 (Flickr8k-CF, ratings in {0, 1/3, 2/3, 1}),
C = 3 score vectors (CLIP-S, Ref-S, RefCLIP-S) in one call.

Per size (workspace and outputs allocated once, device events around `--reps` back-to-back calls, `--rounds` rounds, the two sizes
alternating so that both see the same clocks and neighbours): ms per call as min / median / max over the rounds and pair-column
comparisons per second (C n (n - 1) / 2 per call, from the shapes).  Then `metrics.kendall_tau` (the Python call, allocations included),
the counts against np.unique multiplicities and the taus against SciPy, and for context the only alternative a user has without this
kernel, in the same session: `scores.cpu()` plus `scipy.stats.kendalltau` per column, host clock around both.  The kernel is O(n^2) and
SciPy O(n log n); the feature is "no device wait, one launch sequence", not a speed-up.

    python tools/diag/kendall_bench.py [--reps 10] [--rounds 7] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from distillclip_amd._lib import lib                            # noqa: E402
from distillclip_amd.metrics import kendall_tau                 # noqa: E402

C = 3
SIZES = ((16992, 'expert'), (47830, 'cf'))


def make(n, kind, seed):
    """scores that follow the ratings, as a metric's do: CLIP-S-like, Ref-S-like and their harmonic mean"""
    r = np.random.RandomState(seed)
    if kind == 'expert':                                        # every score three times, three annotators in {1..4} around one level
        group = r.randint(0, 4, size=n // 3)
        level = np.clip(np.repeat(group, 3) + r.randint(-1, 2, size=n), 0, 3)
        y = level + 1.0
        a, b = np.repeat(r.randn(n // 3) + group, 3), np.repeat(1.5 * r.randn(n // 3) + group, 3)
    else:                                                       # {0, 1/3, 2/3, 1}, mostly 0 as the crowd-flower ratings are
        level = r.choice(4, size=n, p=(0.7, 0.15, 0.1, 0.05))
        y = level / 3.0
        a, b = r.randn(n) + level, 1.5 * r.randn(n) + level
    a, b = np.maximum(0.3 * a + 1.0, 0), np.maximum(0.3 * b + 1.0, 0)
    x = np.stack([a, b, 2 * a * b / np.maximum(a + b, 1e-9)])
    return x.astype(np.float32), y.astype(np.float32)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def tie_pairs(v, axis=None):
    _, mult = np.unique(v, axis=axis, return_counts=True)
    mult = mult.astype(np.int64)
    return int((mult * (mult - 1) // 2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'kendall_bench.py measures on an MI355X; there is no CPU path'
    from scipy.stats import kendalltau
    l = lib()
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for n, kind in SIZES:
        x, y = make(n, kind, 1)
        d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        tau = torch.empty(C, 2, dtype=torch.float64, device='cuda')
        cnt = torch.empty(C, 8, dtype=torch.int64, device='cuda')
        ws = torch.empty(l.dclip_kendall_tau_workspace(n, C), dtype=torch.uint8, device='cuda')

        def call(d_x=d_x, d_y=d_y, n=n, tau=tau, cnt=cnt, ws=ws):
            l.dclip_kendall_tau(d_x.data_ptr(), n, C, d_y.data_ptr(), n, tau.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), st)
        runs.append(dict(n=n, kind=kind, x=x, y=y, d_x=d_x, d_y=d_y, tau=tau, cnt=cnt, call=call, ms=[]))
    for r in runs:                                              # warm-up of both sizes
        for _ in range(3):
            r['call']()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for r in runs:
            r['ms'].append(timed(r['call'], args.reps))
    res = {'C': C, 'reps': args.reps, 'rounds': args.rounds, 'sizes': {}}
    for r in runs:
        n, ts = r['n'], r['ms']
        med = statistics.median(ts)
        pairs = C * n * (n - 1) // 2
        out = {'ms_min': min(ts), 'ms_median': med, 'ms_max': max(ts), 'spread_rel': (max(ts) - min(ts)) / med,
               'pair_column_comparisons': pairs, 'comparisons_per_s': pairs / (med * 1e-3)}
        print(f'n={n:6d} C={C}: {min(ts):8.3f} / {med:8.3f} / {max(ts):8.3f} ms per call (min / median / max of {args.rounds} rounds x '
              f'{args.reps} calls)  {out["comparisons_per_s"] / 1e12:6.3f} T pair-column comparisons / s', flush=True)
        # the Python call, allocations included
        for _ in range(2):
            kendall_tau(r['d_x'], r['d_y'])
        torch.cuda.synchronize()
        out['python_call_ms_median'] = statistics.median([timed(lambda: kendall_tau(r['d_x'], r['d_y']), args.reps) for _ in range(3)])
        # the alternative: copy the scores to the host (a device wait) and call SciPy per column
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hx, hy = r['d_x'].cpu().numpy(), r['d_y'].cpu().numpy()
            sp = [[kendalltau(hx[c], hy, variant=v).statistic for v in 'bc'] for c in range(C)]
            host.append((time.perf_counter() - t0) * 1e3)
        out['copy_plus_scipy_ms_median'] = statistics.median(host)
        print(f'           metrics.kendall_tau {out["python_call_ms_median"]:.3f} ms per call; scores.cpu() + scipy.stats.kendalltau x {C} '
              f'columns x 2 variants {out["copy_plus_scipy_ms_median"]:.1f} ms (host clock)', flush=True)
        # what was computed: ties and distinct values against np.unique, taus against SciPy
        r['call']()
        cnt, tau = r['cnt'].cpu().numpy(), r['tau'].cpu().numpy()
        n0 = n * (n - 1) // 2
        ok = True
        for c in range(C):
            want = [tie_pairs(r['x'][c]), tie_pairs(r['y']), tie_pairs(np.stack([r['x'][c], r['y']], axis=1), axis=0),
                    np.unique(r['x'][c]).size, np.unique(r['y']).size, 0]
            ok &= cnt[c, 2:].tolist() == want and int(cnt[c, 0] + cnt[c, 1] + cnt[c, 2] + cnt[c, 3] - cnt[c, 4]) == n0
        err = float(np.abs(tau - np.array(sp)).max())
        out.update(counts_agree_with_numpy=bool(ok), max_abs_tau_difference_from_scipy=err, tau_b=tau[:, 0].tolist(), tau_c=tau[:, 1].tolist())
        print(f'           counts agree with np.unique: {ok}; max |tau - scipy| {err:.2e}; tau_b {tau[:, 0].round(4).tolist()} '
              f'tau_c {tau[:, 1].round(4).tolist()}', flush=True)
        res['sizes'][str(n)] = out
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

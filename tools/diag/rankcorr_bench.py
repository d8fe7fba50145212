"""Spearman and Pearson against human ratings: `dclip_rank_correlation` at the two sizes the caption-metric
literature reports, n = 16 992 (Flickr8k-Expert: 5 664 scores x 3 annotators, ratings in {1..4}) and n = 47 830 (Flickr8k-CF, ratings in
{0, 1/3, 2/3, 1}), C = 3 score vectors (CLIP-S, Ref-S, RefCLIP-S) in one call, on the data of tools/diag/kendall_bench.py.

Per size (workspace and outputs allocated once, device events around `--reps` back-to-back calls, `--rounds` rounds after a warm-up):
ms per call as min / median / max over the rounds and comparisons per second, 2 n^2 (C + 1) per call from the shapes (a `<` and an
`==` per column, item and vector, the ratings being one of the C + 1 vectors).  In the same rounds of the same process, alternating
with it so that both see the same clocks and neighbours, `dclip_kendall_tau` at the same n and C: n (n - 1) / 2 (C + 1) pair-columns per
call.  Then `metrics.rank_correlation` (the Python call, allocations included), the results against SciPy, and for context the only
alternative a user has without this kernel: `scores.cpu()` plus `scipy.stats.spearmanr` / `pearsonr` per column, host clock around
both, the device wait included.  The kernel is O(n^2) and SciPy O(n log n); the feature is "no device wait", not a speed-up.

    python tools/diag/rankcorr_bench.py [--reps 10] [--rounds 7] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                                              # noqa: E402
import torch                                                    # noqa: E402
from distillclip_amd._lib import lib                            # noqa: E402
from distillclip_amd.metrics import rank_correlation            # noqa: E402
from kendall_bench import C, SIZES, make, timed                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'rankcorr_bench.py measures on an MI355X; there is no CPU path'
    from scipy.stats import pearsonr, spearmanr
    l = lib()
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for n, kind in SIZES:
        x, y = make(n, kind, 1)
        d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        corr = torch.empty(C, 2, dtype=torch.float64, device='cuda')
        ws = torch.empty(l.dclip_rank_correlation_workspace(n, C), dtype=torch.uint8, device='cuda')
        tau = torch.empty(C, 2, dtype=torch.float64, device='cuda')
        cnt = torch.empty(C, 8, dtype=torch.int64, device='cuda')
        kws = torch.empty(l.dclip_kendall_tau_workspace(n, C), dtype=torch.uint8, device='cuda')

        def call(d_x=d_x, d_y=d_y, n=n, corr=corr, ws=ws):
            l.dclip_rank_correlation(d_x.data_ptr(), n, C, d_y.data_ptr(), n, corr.data_ptr(), None, None, ws.data_ptr(), ws.numel(), st)

        def kendall(d_x=d_x, d_y=d_y, n=n, tau=tau, cnt=cnt, kws=kws):
            l.dclip_kendall_tau(d_x.data_ptr(), n, C, d_y.data_ptr(), n, tau.data_ptr(), cnt.data_ptr(), kws.data_ptr(), kws.numel(), st)
        runs.append(dict(n=n, kind=kind, x=x, y=y, d_x=d_x, d_y=d_y, corr=corr, call=call, kendall=kendall, ms=[], kendall_ms=[]))
    for r in runs:                                              # warm-up of both entries at both sizes
        for _ in range(3):
            r['call']()
            r['kendall']()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for r in runs:
            r['ms'].append(timed(r['call'], args.reps))
            r['kendall_ms'].append(timed(r['kendall'], args.reps))
    res = {'C': C, 'reps': args.reps, 'rounds': args.rounds, 'sizes': {}}
    for r in runs:
        n, ts, ks = r['n'], r['ms'], r['kendall_ms']
        med, kmed = statistics.median(ts), statistics.median(ks)
        comps, pairs = 2 * n * n * (C + 1), n * (n - 1) // 2 * (C + 1)
        out = {'ms_min': min(ts), 'ms_median': med, 'ms_max': max(ts), 'spread_rel': (max(ts) - min(ts)) / med,
               'comparisons': comps, 'comparisons_per_s': comps / (med * 1e-3),
               'kendall_ms_min': min(ks), 'kendall_ms_median': kmed, 'kendall_ms_max': max(ks),
               'kendall_pair_columns': pairs, 'kendall_pair_columns_per_s': pairs / (kmed * 1e-3)}
        out['rate_over_kendall_rate'] = out['comparisons_per_s'] / out['kendall_pair_columns_per_s']
        print(f'n={n:6d} C={C}: rank_correlation {min(ts):8.3f} / {med:8.3f} / {max(ts):8.3f} ms per call (min / median / max of '
              f'{args.rounds} rounds x {args.reps} calls)  {out["comparisons_per_s"] / 1e12:6.3f} T comparisons / s', flush=True)
        print(f'           kendall_tau      {min(ks):8.3f} / {kmed:8.3f} / {max(ks):8.3f} ms per call, same rounds            '
              f'{out["kendall_pair_columns_per_s"] / 1e12:6.3f} T pair-columns / s  (rate ratio {out["rate_over_kendall_rate"]:.2f})', flush=True)
        # the Python call, allocations included
        for _ in range(2):
            rank_correlation(r['d_x'], r['d_y'])
        torch.cuda.synchronize()
        out['python_call_ms_median'] = statistics.median([timed(lambda: rank_correlation(r['d_x'], r['d_y']), args.reps) for _ in range(3)])
        # the alternative: copy the scores to the host (a device wait) and call SciPy per column
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hx, hy = r['d_x'].cpu().numpy().astype(np.float64), r['d_y'].cpu().numpy().astype(np.float64)
            sp = [[spearmanr(hx[c], hy).statistic, pearsonr(hx[c], hy).statistic] for c in range(C)]
            host.append((time.perf_counter() - t0) * 1e3)
        out['copy_plus_scipy_ms_median'] = statistics.median(host)
        print(f'           metrics.rank_correlation {out["python_call_ms_median"]:.3f} ms per call; scores.cpu() + scipy.stats.spearmanr + '
              f'pearsonr x {C} columns {out["copy_plus_scipy_ms_median"]:.1f} ms (host clock)', flush=True)
        r['call']()
        corr = r['corr'].cpu().numpy()
        err = np.abs(corr - np.array(sp)).max(axis=0)
        out.update(max_abs_rho_difference_from_scipy=float(err[0]), max_abs_r_difference_from_scipy=float(err[1]),
                   spearman=corr[:, 0].tolist(), pearson=corr[:, 1].tolist())
        print(f'           max |rho - scipy| {err[0]:.2e}, max |r - scipy| {err[1]:.2e}; rho {corr[:, 0].round(4).tolist()} '
              f'r {corr[:, 1].round(4).tolist()}', flush=True)
        res['sizes'][str(n)] = out
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

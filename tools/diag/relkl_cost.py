"""Cost of the intra-modal relational KL term (`intra_kl`, dclip_relation_kl), protocol of tools/diag/icl_cost.py
(alternating rounds in one process, medians with the range):
python tools/diag/relkl_cost.py [--steps 40] [--rounds 5] [--none-only] [--kernels-only]
  1. the kernel alone at B = 512, E = 512, tau = 0.07, 7 rounds of 10 calls after a warm-up, against the yardstick of the same rounds:
       dclip_interactive_loss   four launches; two directions with ONE dot_tile per tile, one exp per element in stripe B;
       dclip_relation_kl        five launches; one direction with TWO dot_tiles per tile, four exps per element in stripe B.
     The two walk the same number of dot_tiles.  The target is 1.5 x the yardstick's time.  Both include the output and workspace
     allocations of their ops wrapper.
  2. the bench.py l_clip step (same loop as icl_cost.py), taking turns:
       none      losses out_l1 + out_cos + 0.1 * cos_diff: the launches of a tree without the feature;
       intra_kl  the same plus intra_kl at temperature 0.07 (one dclip_relation_kl call per tower).
--none-only: part 2's `none` alone, for a comparison with the parent commit's `tools/diag/icl_cost.py --none-only` (the same loop) with the
two processes taking turns in one session."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench                                                                  # noqa: E402


def kernels_alone(dev):
    from distillclip_amd import ops
    B, E, tau = 512, 512, 0.07
    g = torch.Generator().manual_seed(2022)
    si, ti, st, tt = (torch.randn(B, E, generator=g).to(dev) for _ in range(4))
    calls = {
        'dclip_interactive_loss': lambda: ops.interactive_loss(si, ti, st, tt, tau),
        'dclip_relation_kl': lambda: ops.relation_kl(si, ti, tau),
    }
    for fn in calls.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(7):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 10 * 1e3)
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(f'{name} alone, B={B} E={E}: {med[name]:.1f} us / call (min {min(ts):.1f}, max {max(ts):.1f})', flush=True)
    yard, got = med['dclip_interactive_loss'], med['dclip_relation_kl']
    print(f'target: 1.5 x {yard:.1f} us = {1.5 * yard:.1f} us; measured {got:.1f} us ({got / yard:.2f} x): '
          f'{"met" if got <= 1.5 * yard else "MISSED"}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--none-only', action='store_true')
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    import distillclip_amd
    from distillclip_amd.model import LossCalculator
    print('package:', os.path.dirname(distillclip_amd.__file__), flush=True)
    dev = torch.device('cuda', 0)
    if not args.none_only:
        kernels_alone(dev)
        if args.kernels_only:
            return
    wl = bench.WORKLOADS['lclip']
    model = bench.build_model(wl, 2022, dev)
    (opt,), _ = model.configure_optimizers()
    B = args.batch or wl['batch']
    image, text, _ = bench.make_inputs(wl, 2022, B)
    batch = [image.to(dev), text.to(dev)]
    base = ['out_l1', 'out_cos', 'cos_diff']
    assert list(model.loss_control.loss_name) == base, model.loss_control.loss_name
    losses = {'none': model.loss_control}
    if not args.none_only:
        losses['intra_kl'] = LossCalculator(base + ['intra_kl'], {'cos_diff': 0.1}, temperature=0.07)

    def step(lc):
        model.loss_control = lc
        loss = model.training_step(batch)
        opt.zero_grad()
        model.backward_and_sync(loss, defer_wait=True)
        opt.step(zero_grad=True, overlap=True, join=False)

    res = {k: [] for k in losses}
    for r in range(args.rounds):
        for name, lc in losses.items():
            for _ in range(3):
                step(lc)
            opt.join()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(lc)
            opt.join()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / args.steps)
            print(f'round {r} {name}: {res[name][-1]:.3f} ms / step', flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, v in res.items():
        print(f'{name}: {med[name]:.3f} ms (range {min(v):.3f}-{max(v):.3f})' +
              ('' if name == 'none' else f', {1e3 * (med[name] - med["none"]):+.0f} us against none'))


if __name__ == '__main__':
    main()

"""Cost of layer-wise trust ratios (FusedAdamW(trust_ratio=True), dclip_lamb_table) in the l_clip workload, protocol of
tools/diag/groups_cost.py (alternating rounds in one process, medians with the range):
python tools/diag/lamb_cost.py [--steps 40] [--rounds 5] [--none-only] [--kernels-only]
  1. the kernels alone over the two l_clip students' tables cut at every parameter tensor, one tower after the other:
       dclip_adamw_table                      one launch per tower, 28 B per element (the yardstick of the same session);
       dclip_adamw_table, zero_grad           32 B;
       dclip_lamb_table, zero_grad            three launches per tower: moments + partial norms 28 B, ratios, apply 16 B: 44 B;
       dclip_lamb_table, zero_grad, EMA       apply 24 B: 52 B.
     The target for the three launches is the yardstick's time x 44 / 28 x 1.15.
  2. the bench.py step (same loop: overlapped, un-joined optimizer, fused gradient clearing), taking turns:
       none     trust_ratio off: the launches of a tree without the feature;
       lamb     trust_ratio on.
--none-only: part 2's `none` alone, for a comparison with the parent commit's `tools/diag/groups_cost.py --none-only` (the same loop) with the
two processes taking turns in one session."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench                                                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--none-only', action='store_true')
    ap.add_argument('--kernels-only', action='store_true')
    args = ap.parse_args()
    import distillclip_amd
    from distillclip_amd import ops
    from distillclip_amd.optim import FusedLAMB
    print('package:', os.path.dirname(distillclip_amd.__file__), flush=True)
    wl = bench.WORKLOADS['lclip']
    dev = torch.device('cuda', 0)
    model = bench.build_model(wl, 2022, dev)
    (opt,), _ = model.configure_optimizers()
    B = args.batch or wl['batch']
    image, text, _ = bench.make_inputs(wl, 2022, B)
    batch = [image.to(dev), text.to(dev)]
    towers = model.towers()
    opts = {'none': opt}
    if not args.none_only:
        opts['lamb'] = FusedLAMB(towers, lr=opt.lr, weight_decay=opt.weight_decay, extra_params=list(opt.extras))

    def step(o):
        loss = model.training_step(batch)
        o.zero_grad()
        model.backward_and_sync(loss, defer_wait=True)
        o.step(zero_grad=True, overlap=True, join=False)

    for o in opts.values():
        for _ in range(3):
            step(o)
        o.join()
    torch.cuda.synchronize()

    if not args.none_only:
        # 1. the kernels alone (the moments and weights move, which the timing does not mind)
        model.backward_and_sync(model.training_step(batch))
        torch.cuda.synchronize()
        lamb = opts['lamb']
        cut = {id(tw): lamb._group_ranges(tw, units=True) for tw in towers}
        n = sum(b - a for tw in towers for a, b in opt._ranges(tw))
        tabs = {id(tw): lamb._table_of(id(tw), tw.flat, cut[id(tw)]) for tw in towers}
        bufs = {id(tw): ops.lamb_buffers(len(cut[id(tw)]), tabs[id(tw)]['tiles'], dev) for tw in towers}
        ema = {id(tw): tw.flat.clone() for tw in towers}
        print(f'{n / 1e6:.1f} M elements; units per tower: ' + ', '.join(f'{len(cut[id(tw)])} in {tabs[id(tw)]["tiles"]} tiles' for tw in towers), flush=True)

        def table(zero_grad):
            def go(tw):
                t = tabs[id(tw)]
                ops.adamw_table(tw.flat, tw.flat_grad, *opt._moments(tw), None, t['dev'], len(cut[id(tw)]), t['tiles'], 1e-6, opt.betas, opt.eps, 100, zero_grad)
            return go

        def lamb_k(e):
            def go(tw):
                t = tabs[id(tw)]
                ops.lamb_table(tw.flat, tw.flat_grad, *opt._moments(tw), ema[id(tw)] if e else None, t['dev'], len(cut[id(tw)]), t['tiles'], 1e-6, opt.betas, opt.eps,
                               100, *bufs[id(tw)], True, 1e-4 if e else 0.0)
            return go

        kernels = {'dclip_adamw_table': (table(False), 28), 'dclip_adamw_table, zero_grad': (table(True), 32), 'dclip_lamb_table, zero_grad': (lamb_k(False), 44),
                   'dclip_lamb_table, zero_grad, EMA': (lamb_k(True), 52)}
        times = {k: [] for k in kernels}
        for _ in range(9):
            for name, (fn, _) in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    for tw in towers:
                        fn(tw)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / 20 * 1e3)
        med = {}
        for name, ts in times.items():
            us = med[name] = statistics.median(ts[1:])
            mb = kernels[name][1] * n / 1e6
            print(f'{name} alone: {mb:.1f} MB, {us:.1f} us (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f}), {mb / us:.2f} TB/s', flush=True)
        target = med['dclip_adamw_table'] * 44 / 28 * 1.15
        got = med['dclip_lamb_table, zero_grad']
        print(f'target for the three launches: {med["dclip_adamw_table"]:.1f} us x 44 / 28 x 1.15 = {target:.1f} us; measured {got:.1f} us: {"met" if got <= target else "MISSED"}', flush=True)
        opt.zero_grad()
        if args.kernels_only:
            return

    # 2. the step, alternating
    res = {k: [] for k in opts}
    for r in range(args.rounds):
        for name, o in opts.items():
            for _ in range(3):
                step(o)
            o.join()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(o)
            o.join()
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

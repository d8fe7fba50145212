"""Cost of parameter groups in the fused AdamW step of the l_clip workload, protocol of tools/diag/ema_cost.py
(alternating rounds in one process, medians with the range):
python tools/diag/groups_cost.py [--steps 40] [--rounds 5] [--none-only]
  1. the kernels alone over the two l_clip students' ranges cut by no_decay_groups, one tower after the other: dclip_adamw_table (ONE launch
     per tower, per-range hyper-parameters from the device table) against dclip_adamw_multi over the same ranges and so the same bytes
     (one launch per 24 ranges with one lr and one weight_decay: what the bytes cost through the old entry, not the grouped step), and
     against dclip_adamw_multi over the towers' uncut ranges (one launch per tower: the step without groups);
  2. the bench.py step (same loop: overlapped, un-joined optimizer, fused gradient clearing) in three ways, taking turns:
       none     groups = None: the launches of a tree without groups;
       table    no_decay_groups through dclip_adamw_table;
       old24    the same groups stepped through the 24-range entries, one launch per 24 ranges of one (lr_scale, weight_decay) pair:
                what a user could have had without the table kernel.
--none-only: part 2's `none` alone, for a comparison with the parent commit's `tools/diag/ema_cost.py --off-only` (the same loop) with the two
processes taking turns in one session."""
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
    args = ap.parse_args()
    import distillclip_amd
    from distillclip_amd import ops
    from distillclip_amd.optim import FusedAdamW, no_decay_groups
    print('package:', os.path.dirname(distillclip_amd.__file__), flush=True)
    wl = bench.WORKLOADS['lclip']
    dev = torch.device('cuda', 0)
    model = bench.build_model(wl, 2022, dev)
    (opt,), _ = model.configure_optimizers()
    B = args.batch or wl['batch']
    image, text, _ = bench.make_inputs(wl, 2022, B)
    batch = [image.to(dev), text.to(dev)]

    class Old24(FusedAdamW):
        """the grouped step through the existing entries: per tower, one launch per 24 ranges of each distinct (lr_scale, weight_decay)"""

        def _adamw_table(self, tw, bufs, ranges, zero_grad, st, ema_weight, gscale, record):
            p, g, m, v, _ = bufs
            by_key = {}
            for a, b, s, wd in ranges:
                by_key.setdefault((s, wd), []).append((p[a:b], g[a:b], m[a:b], v[a:b]))
            for (s, wd), items in by_key.items():
                with self._with_hyper(s, wd):
                    for i in range(0, len(items), ops.ADAMW_MAX_RANGES):
                        ops.adamw_multi_scaled(items[i:i + ops.ADAMW_MAX_RANGES], self.lr, self.betas, self.eps, self.weight_decay, self.step_count, zero_grad, gscale, st)

    towers = model.towers()
    extras = list(opt.extras)
    mk = lambda cls, groups: cls(towers, lr=opt.lr, weight_decay=opt.weight_decay, extra_params=extras, groups=groups)
    opts = {'none': opt}
    if not args.none_only:
        opts.update(table=mk(FusedAdamW, no_decay_groups(model)), old24=mk(Old24, no_decay_groups(model)))

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
        tab = opts['table']
        cut = {id(tw): tab._group_ranges(tw) for tw in towers}
        n = sum(b - a for tw in towers for a, b in opt._ranges(tw))
        print(f'{n / 1e6:.1f} M elements; ranges per tower: ' + ', '.join(f'{len(opt._ranges(tw))} -> {len(cut[id(tw)])}' for tw in towers), flush=True)
        hyper = (1e-6, opt.betas, opt.eps, opt.weight_decay)
        views = lambda tw, rs: [(tw.flat[a:b], tw.flat_grad[a:b], opt._moments(tw)[0][a:b], opt._moments(tw)[1][a:b]) for a, b, *_ in rs]

        def multi(rs_of):
            def go(tw):
                items = views(tw, rs_of(tw))
                for i in range(0, len(items), ops.ADAMW_MAX_RANGES):
                    ops.adamw_multi_scaled(items[i:i + ops.ADAMW_MAX_RANGES], *hyper, 100, False, None)
            return go

        def table(tw):
            keep = tab.lr
            tab.lr, tab.step_count = 1e-6, max(tab.step_count, 1)
            tab._adamw_table(tw, (tw.flat, tw.flat_grad) + tuple(opt._moments(tw)) + (None,), cut[id(tw)], False, None, None, None, None)
            tab.lr = keep

        kernels = {'dclip_adamw_multi, uncut ranges': multi(lambda tw: opt._ranges(tw)), 'dclip_adamw_multi, cut ranges': multi(lambda tw: cut[id(tw)]),
                   'dclip_adamw_table, cut ranges': table}
        times = {k: [] for k in kernels}
        for _ in range(9):
            for name, fn in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    for tw in towers:
                        fn(tw)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / 20 * 1e3)
        for name, ts in times.items():
            us = statistics.median(ts[1:])
            print(f'{name} alone: {4 * 7 * n / 1e6:.1f} MB, {us:.1f} us (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f}), {4 * 7 * n / us / 1e6:.2f} TB/s', flush=True)
        opt.zero_grad()

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

"""Cost of stepping FusedAdamW through torch.amp.GradScaler in the l_clip step:
python tools/diag/amp_step_cost.py [--steps 40] [--rounds 3] [--plain-only]
  1. the AdamW kernels alone over the two l_clip students' gradient ranges, one launch per tower: dclip_adamw_multi, dclip_adamw_multi_scaled
     (coefficient 1) and dclip_adamw_multi_amp (multiplier 1, no skip), time per launch pair (events around a batch of launches, median of
     the batches), taking turns;
  2. the bench.py step (same loop: overlapped, un-joined optimizer, fused gradient clearing) in three ways, alternating in one process,
     median ms per step of each:
       plain          no scaler, no autocast;
       unscale+step   fp16 autocast, scaler.scale(loss) backward, scaler.unscale_(opt), scaler.step(opt): the multiplier is 1, the skip flag live;
       step           the same without unscale_: the scaler runs its own overflow check over p.grad, the kernel unscales.
--plain-only: part 2's plain step alone (what a tree without the scaler protocol can run, for a comparison in the same session)."""
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
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--plain-only', action='store_true')
    args = ap.parse_args()
    import distillclip_amd
    from distillclip_amd import ops
    print('package:', os.path.dirname(distillclip_amd.__file__), flush=True)
    wl = bench.WORKLOADS['lclip']
    dev = torch.device('cuda', 0)
    model = bench.build_model(wl, 2022, dev)
    (opt,), _ = model.configure_optimizers()
    B = args.batch or wl['batch']
    image, text, _ = bench.make_inputs(wl, 2022, B)
    batch = [image.to(dev), text.to(dev)]
    scaler = torch.amp.GradScaler('cuda', init_scale=65536.0)

    def plain():
        loss = model.training_step(batch)
        opt.zero_grad()
        model.backward_and_sync(loss, defer_wait=True)
        opt.step(zero_grad=True, overlap=True, join=False)

    def scaled(unscale):
        with torch.autocast('cuda', dtype=torch.float16):
            loss = model.training_step(batch)
        opt.zero_grad()
        model.backward_and_sync(scaler.scale(loss), defer_wait=True)
        if unscale:
            scaler.unscale_(opt)
        scaler.step(opt, zero_grad=True, overlap=True, join=False)
        scaler.update()

    ways = {'plain': plain}
    if not args.plain_only:
        ways.update({'unscale+step': lambda: scaled(True), 'step': lambda: scaled(False)})

    for _ in range(5):
        plain()
    opt.join()
    torch.cuda.synchronize()

    if not args.plain_only:
        # 1. the kernels alone, on gradients as the backward leaves them (the moments and weights move, which the timing does not mind)
        model.backward_and_sync(model.training_step(batch))
        torch.cuda.synchronize()
        towers = model.towers()
        items = [[(tw.flat[a:b], tw.flat_grad[a:b], opt._moments(tw)[0][a:b], opt._moments(tw)[1][a:b]) for a, b in opt._ranges(tw)] for tw in towers]
        nbytes = 4 * 7 * sum(it[0].numel() for its in items for it in its)    # p, g, m, v read, p, m, v written
        one = torch.ones(1, device=dev)
        record, skipped = torch.zeros(ops.AMP_RECORD_FLOATS, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        ops.amp_prepare(record, skipped, opt.betas, 100, torch.zeros(1, device=dev), one)
        hyper = (1e-6, opt.betas, opt.eps, opt.weight_decay)
        kernels = {'dclip_adamw_multi': lambda its: ops.adamw_multi_scaled(its, *hyper, 100, False, None),
                   'dclip_adamw_multi_scaled': lambda its: ops.adamw_multi_scaled(its, *hyper, 100, False, one),
                   'dclip_adamw_multi_amp': lambda its: ops.adamw_multi_amp(its, *hyper, False, record)}
        times = {k: [] for k in kernels}
        for _ in range(7):
            for name, fn in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    for its in items:
                        fn(its)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / 20 * 1e3)
        for name, ts in times.items():
            us = statistics.median(ts[1:])
            print(f'{name} alone: {nbytes / 1e6:.1f} MB in {len(towers)} launches, {us:.1f} us (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f}), '
                  f'{nbytes / us / 1e6:.2f} TB/s', flush=True)
        opt.zero_grad()

    # 2. the step, three ways, alternating
    res = {k: [] for k in ways}
    for r in range(args.rounds):
        for name, fn in ways.items():
            for _ in range(3):
                fn()
            opt.join()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            opt.join()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / args.steps)
            print(f'round {r} {name}: {res[name][-1]:.3f} ms / step', flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, v in res.items():
        print(f'{name}: {med[name]:.3f} ms (range {min(v):.3f}-{max(v):.3f})' +
              ('' if name == 'plain' else f', {1e3 * (med[name] - med["plain"]):+.0f} us against plain'))
    if not args.plain_only:
        print(f'scale {scaler.get_scale():g}, steps skipped {int(opt._skipped)} of {opt.step_count}')


if __name__ == '__main__':
    main()

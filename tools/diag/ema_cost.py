"""Cost of keeping an EMA of the student weights inside the fused AdamW step of the l_clip workload:
python tools/diag/ema_cost.py [--steps 40] [--rounds 5] [--off-only]
  1. the AdamW kernels alone over the two l_clip students' trainable ranges, one launch per tower: dclip_adamw_multi and
     dclip_adamw_multi_ema (weight 1e-4), time per launch pair (events around a batch of launches, median of the batches), taking turns;
     dclip_swap_multi over the same ranges;
  2. the bench.py step (same loop: overlapped, un-joined optimizer, fused gradient clearing) in three ways, alternating in one process,
     median ms per step of each with the range:
       off       ema_decay = None;
       fused     ema_decay = 0.9999: the average is kept by the step's own kernel;
       foreach   ema_decay = None and torch._foreach_lerp_ over the parameter views after step(), which is what a user could do before.
--off-only: part 2's `off` alone (what a tree without the EMA can run, for a comparison with the parent commit in the same session)."""
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
    ap.add_argument('--off-only', action='store_true')
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

    def step(decay=None):
        opt.ema_decay = decay
        loss = model.training_step(batch)
        opt.zero_grad()
        model.backward_and_sync(loss, defer_wait=True)
        opt.step(zero_grad=True, overlap=True, join=False)

    params = [p.detach() for p in opt._trainable()]
    outside = []

    def foreach():
        step()
        opt.join()                                                            # (the parameters are read on the current stream)
        if not outside:
            outside.extend(p.clone() for p in params)
        torch._foreach_lerp_(outside, params, 1e-4)

    ways = {'off': step}
    if not args.off_only:
        ways.update({'fused': lambda: step(0.9999), 'foreach': foreach})

    for _ in range(5):
        step()
    opt.join()
    torch.cuda.synchronize()
    n_train = sum(p.numel() for p in params)
    print(f'{n_train / 1e6:.1f} M trainable elements in {len(params)} parameters', flush=True)

    if not args.off_only:
        # 1. the kernels alone (the moments and weights move, which the timing does not mind)
        model.backward_and_sync(model.training_step(batch))
        torch.cuda.synchronize()
        towers = model.towers()
        avg = [torch.zeros_like(tw.flat) for tw in towers]
        items = [[(tw.flat[a:b], tw.flat_grad[a:b], opt._moments(tw)[0][a:b], opt._moments(tw)[1][a:b], e[a:b]) for a, b in opt._ranges(tw)]
                 for tw, e in zip(towers, avg)]
        n = sum(it[0].numel() for its in items for it in its)
        hyper = (1e-6, opt.betas, opt.eps, opt.weight_decay)
        kernels = {'dclip_adamw_multi': (4 * 7 * n, lambda its: ops.adamw_multi_scaled([it[:4] for it in its], *hyper, 100, False, None)),
                   'dclip_adamw_multi_ema': (4 * 9 * n, lambda its: ops.adamw_multi_ema(its, *hyper, 100, False, 1e-4)),
                   'dclip_swap_multi': (4 * 4 * n, lambda its: ops.swap_multi([(it[0], it[4]) for it in its]))}
        times = {k: [] for k in kernels}
        for _ in range(9):
            for name, (_, fn) in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    for its in items:
                        fn(its)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / 20 * 1e3)
        for name, ts in times.items():
            us, nbytes = statistics.median(ts[1:]), kernels[name][0]
            print(f'{name} alone: {nbytes / 1e6:.1f} MB in {len(towers)} launches, {us:.1f} us (min {min(ts[1:]):.1f}, max {max(ts[1:]):.1f}), '
                  f'{nbytes / us / 1e6:.2f} TB/s', flush=True)
        opt.zero_grad()

    # 2. the step, alternating
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
              ('' if name == 'off' else f', {1e3 * (med[name] - med["off"]):+.0f} us against off'))


if __name__ == '__main__':
    main()

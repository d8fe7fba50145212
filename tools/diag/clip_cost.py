"""Cost of the global-norm clipping in the l_clip step: python tools/diag/clip_cost.py [--steps 40] [--rounds 3]
  1. dclip_sumsq_multi alone over the two l_clip students' gradient ranges: time per launch pair and achieved TB/s (events around
     a batch of launches, median of the batches);
  2. the bench.py step (same loop: overlapped, un-joined optimizer, fused gradient clearing) with max_grad_norm None and 1.0,
     alternating in one process, median ms per step of each."""
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
    args = ap.parse_args()
    from distillclip_amd import ops
    wl = bench.WORKLOADS['lclip']
    dev = torch.device('cuda', 0)
    model = bench.build_model(wl, 2022, dev)
    (opt,), _ = model.configure_optimizers()
    B = args.batch or wl['batch']
    image, text, _ = bench.make_inputs(wl, 2022, B)
    batch = [image.to(dev), text.to(dev)]

    def step():
        loss = model.training_step(batch)
        opt.zero_grad()
        model.backward_and_sync(loss, defer_wait=True)
        opt.step(zero_grad=True, overlap=True, join=False)

    for _ in range(5):
        step()
    opt.join()
    torch.cuda.synchronize()
    # 1. the kernel alone, on gradients as the backward leaves them
    loss = model.training_step(batch)
    opt.zero_grad()
    model.backward_and_sync(loss)
    torch.cuda.synchronize()
    towers = model.towers()
    views = [[tw.flat_grad[a:b] for a, b in opt._ranges(tw)] for tw in towers]
    nbytes = 4 * sum(v.numel() for vs in views for v in vs)
    parts = torch.empty(len(towers) * ops.SUMSQ_PARTIALS, device=dev)
    times = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            for k, vs in enumerate(views):
                ops.sumsq_multi(vs, parts[k * ops.SUMSQ_PARTIALS:(k + 1) * ops.SUMSQ_PARTIALS])
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 20 * 1e3)
    us = statistics.median(times[1:])
    print(f'sumsq_multi alone: {nbytes / 1e6:.1f} MB in {len(towers)} launches, {us:.1f} us (min {min(times[1:]):.1f}, max {max(times[1:]):.1f}), '
          f'{nbytes / us / 1e6:.2f} TB/s', flush=True)
    opt.step(zero_grad=True)
    # 2. the step, clipping off / on, alternating
    res = {None: [], 1.0: []}
    for r in range(args.rounds):
        for c in (None, 1.0):
            opt.max_grad_norm = c
            for _ in range(3):
                step()
            opt.join()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step()
            opt.join()
            e1.record()
            torch.cuda.synchronize()
            res[c].append(e0.elapsed_time(e1) / args.steps)
            print(f'round {r} max_grad_norm={c}: {res[c][-1]:.3f} ms / step' + ('' if c is None else f' (norm {float(opt.last_grad_norm):.4e})'), flush=True)
    off, on = statistics.median(res[None]), statistics.median(res[1.0])
    print(f'step: off {off:.3f} ms (range {min(res[None]):.3f}-{max(res[None]):.3f}), on {on:.3f} ms (range {min(res[1.0]):.3f}-{max(res[1.0]):.3f}), '
          f'difference {1e3 * (on - off):.0f} us; bytes alone at 5.4 TB/s: {nbytes / 5.4e6:.0f} us')


if __name__ == '__main__':
    main()

"""Cost of L-CLIPScore scoring: python tools/diag/score_bench.py [--batch 512] [--rounds 7]
  1. dclip_clipscore alone at B images, K = 5 candidates and five references per image, E = 512 (the l_clip students' width): time per
     launch (events around a batch of back-to-back launches through the C entry into preallocated outputs, median of the batches), the
     bytes it must read, (B + B K + R) E 4, and the achieved rate — once on one set of buffers (after the first launch they sit in L2 /
     the Infinity Cache) and once rotating through sets that together exceed the 256 MiB Infinity Cache (every launch reads from HBM).
     A kernel this short is at the rate at which launches can be issued: the event figure is the launch-to-launch interval, an upper
     bound of the kernel's time; `rocprofv3 --kernel-trace --stats -- python tools/diag/score_bench.py --kernel-only` gives the
     kernel's own (clipscore_kernel);
  2. the whole scorer (LCLIPScore.forward: both l_clip student towers + the kernel) at B images: one candidate and no references
     (CLIP-S of a caption per image), and K = 5 candidates with five references each (RefCLIP-S as a captioner's reward): ms per call,
     images and captions per second."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench                                                                  # noqa: E402


def timed(fn, reps, rounds):
    """-> [ms per call] of `rounds` batches of `reps` calls (the first batch is the warm-up and is dropped)"""
    out = []
    for _ in range(rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--kernel-only', action='store_true')
    args = ap.parse_args()
    from distillclip_amd import LCLIPScore, synth
    from distillclip_amd._lib import lib
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    B, K, per, E = args.batch, 5, 5, 512
    R = B * per
    nbytes = (B + B * K + R) * E * 4
    sets = 256 * 2 ** 20 // nbytes + 2
    g = torch.Generator().manual_seed(1)
    off = torch.arange(0, R + 1, per, dtype=torch.int32).to(dev)
    bufs = [(torch.randn(B, E, generator=g).to(dev), torch.randn(B * K, E, generator=g).to(dev), torch.randn(R, E, generator=g).to(dev))
            for _ in range(sets)]
    outs = torch.empty(3, B * K, device=dev)
    fn, st = lib().dclip_clipscore, torch.cuda.current_stream().cuda_stream
    ptrs = [tuple(t.data_ptr() for t in b) for b in bufs]
    o0, o1, o2, poff = outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), off.data_ptr()

    def call(i):
        img, cand, refs = ptrs[i % len(ptrs)]
        fn(img, E, cand, E, refs, E, poff, B, K, R, E, 2.5, o0, o1, o2, st)
    warm = timed(lambda i: call(0), 500, args.rounds)
    cold = timed(call, 500, args.rounds)
    for name, ts in (('same buffers (cache-resident)', warm), (f'{sets} buffer sets in turn ({sets * nbytes / 2 ** 20:.0f} MiB: from HBM)', cold)):
        us = statistics.median(ts) * 1e3
        print(f'dclip_clipscore B={B} K={K} R={R} E={E}, {name}: {us:.2f} us from launch to launch (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}), '
              f'{nbytes / 1e6:.2f} MB to read, {nbytes / us / 1e3:.1f} GB/s', flush=True)
    del bufs
    if args.kernel_only:
        return
    wl = bench.WORKLOADS['lclip']
    model = bench.build_model(wl, 2022, dev)
    scorer = LCLIPScore.from_model(model)
    images = torch.from_numpy(synth.images(2022, B, wl['res'])).to(dev)
    caps = torch.from_numpy(synth.captions(2022, B * (K + per))).to(dev)
    cand, refs = caps[:B * K].reshape(B, K, -1), caps[B * K:].reshape(B, per, -1)
    one = cand[:, 0].contiguous()
    for name, fn, ncap in (('1 candidate, no references', lambda i: scorer(images, one), B),
                           (f'{K} candidates + {per} references per image', lambda i: scorer(images, cand, refs), B * (K + per))):
        ts = timed(fn, 5, args.rounds)
        ms = statistics.median(ts)
        print(f'LCLIPScore.forward B={B}, {name}: {ms:.2f} ms / call (min {min(ts):.2f}, max {max(ts):.2f}), {B / ms * 1e3:.0f} images/s, '
              f'{ncap / ms * 1e3:.0f} captions/s', flush=True)


if __name__ == '__main__':
    main()

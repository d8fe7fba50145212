"""Recall@K with several captions per image: `dclip_retrieval_recall` at the MS-COCO 5k test split, 5 000 images x
25 010 captions x E = 512, beside the square `dclip_retrieval_metrics` at n = 5 000 in the same session.

Per kernel call (workspace allocated once, device events around `--reps` back-to-back calls, the two kernels alternating over `--rounds`
rounds so that both see the same clocks and neighbours): ms per call as min / median / max over the rounds, ps per logit element per
direction (the recall call forms every logit twice, once per direction; the square call once), and the bytes each must read.  The spread
of the square kernel over the rounds is the yardstick for a difference between the two per-element figures.  Then the ranks at this size
against float64 logits formed by torch on the device, and `metrics.retrieval_recall` (the Python call, allocations included).

    python tools/diag/recall_bench.py [--reps 10] [--rounds 7] [--json PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch                                                    # noqa: E402
from distillclip_amd._lib import lib                            # noqa: E402
from distillclip_amd.metrics import retrieval_recall            # noqa: E402

N_IMG, N_TXT, E = 5000, 25010, 512
KS = (1, 5, 10)


def coco_counts():
    """five captions per image, ten images with six: 25 010 in all"""
    counts = [5] * N_IMG
    for i in range(N_TXT - 5 * N_IMG):
        counts[(i * 499) % N_IMG] += 1
    assert sum(counts) == N_TXT
    return counts


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'recall_bench.py measures on an MI355X; there is no CPU path'
    g = torch.Generator().manual_seed(1)
    counts = coco_counts()
    owner = torch.arange(N_IMG).repeat_interleave(torch.tensor(counts))
    img = torch.randn(N_IMG, E, generator=g) * (0.5 + torch.rand(N_IMG, 1, generator=g))
    txt = 3 * (0.25 * img[owner] + torch.randn(N_TXT, E, generator=g))
    d_img, d_txt = img.cuda(), txt.cuda()
    offs = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32).cuda()
    st = torch.cuda.current_stream().cuda_stream
    l = lib()
    karr = (ctypes.c_int32 * len(KS))(*KS)

    ws_r = torch.empty(l.dclip_retrieval_recall_workspace(N_IMG, N_TXT, E), dtype=torch.uint8, device='cuda')
    out_r = torch.empty(2 * len(KS) + 2, device='cuda')
    rank_i = torch.empty(N_IMG, dtype=torch.int32, device='cuda')
    rank_t = torch.empty(N_TXT, dtype=torch.int32, device='cuda')

    def recall():
        l.dclip_retrieval_recall(d_img.data_ptr(), d_txt.data_ptr(), offs.data_ptr(), N_IMG, N_TXT, E, karr, len(KS), out_r.data_ptr(),
                                 rank_i.data_ptr(), rank_t.data_ptr(), ws_r.data_ptr(), ws_r.numel(), st)

    sq_txt = d_txt[:N_IMG].contiguous()
    ws_s = torch.empty(l.dclip_retrieval_metrics_workspace(N_IMG, E), dtype=torch.uint8, device='cuda')
    out_s = torch.empty(len(KS) + 2, device='cuda')

    def square():
        l.dclip_retrieval_metrics(d_img.data_ptr(), sq_txt.data_ptr(), N_IMG, E, karr, len(KS), out_s.data_ptr(), None, ws_s.data_ptr(),
                                  ws_s.numel(), st)

    for _ in range(3):                                           # warm-up of both
        recall()
        square()
    torch.cuda.synchronize()
    t_r, t_s = [], []
    for _ in range(args.rounds):
        t_r.append(timed(recall, args.reps))
        t_s.append(timed(square, args.reps))
    el_r, el_s = 2.0 * N_IMG * N_TXT, float(N_IMG) * N_IMG       # logit elements formed per call
    # bytes the call must read: the raw rows once (normalisation), the offsets; its own workspace traffic comes on top
    bytes_r = (N_IMG + N_TXT) * E * 4 + (N_IMG + 1) * 4
    bytes_s = 2 * N_IMG * E * 4
    res = {'shape': [N_IMG, N_TXT, E], 'reps': args.reps, 'rounds': args.rounds}
    for name, ts, el, nbytes in (('recall', t_r, el_r, bytes_r), ('square', t_s, el_s, bytes_s)):
        med = statistics.median(ts)
        res[name] = {'ms_min': min(ts), 'ms_median': med, 'ms_max': max(ts), 'ps_per_element_per_direction': med * 1e9 / el,
                     'spread_rel': (max(ts) - min(ts)) / med, 'bytes_must_read': nbytes,
                     'tflops_exact_f32': 2 * el * E / (med * 1e-3) / 1e12}
        print(f'{name:7s}: {min(ts):8.3f} / {med:8.3f} / {max(ts):8.3f} ms per call (min / median / max of {args.rounds} rounds x {args.reps} calls)  '
              f'{med * 1e9 / el:7.3f} ps per logit element per direction  {res[name]["tflops_exact_f32"]:6.1f} TFLOP/s exact f32  '
              f'must read {nbytes / 2 ** 20:.1f} MiB', flush=True)
    ratio = res['recall']['ps_per_element_per_direction'] / res['square']['ps_per_element_per_direction']
    res['per_element_ratio_recall_over_square'] = ratio
    print(f'per-element cost, recall / square: {ratio:.3f}  (run-to-run spread of the square kernel: {res["square"]["spread_rel"] * 100:.1f} %)')

    # the ranks at this size against float64 logits (torch, on the device)
    recall()
    a = torch.nn.functional.normalize(d_img.double(), dim=1)
    b = torch.nn.functional.normalize(d_txt.double(), dim=1)
    own = owner.cuda()
    target = (a[own] * b).sum(dim=1)                             # [n_txt]: L64[owner(c), c]
    want_i = torch.empty(N_IMG, dtype=torch.int64, device='cuda')
    want_t = torch.zeros(N_TXT, dtype=torch.int64, device='cuda')
    for s in range(0, N_IMG, 500):                               # 500 images at a time: 100 MB of float64 logits
        L = a[s:s + 500] @ b.t()
        rows = torch.arange(s, min(s + 500, N_IMG), device='cuda')
        mine = own[None, :] == rows[:, None]
        best = torch.where(mine, L, torch.full_like(L, -2.0)).max(dim=1).values
        want_i[s:s + 500] = ((L > best[:, None]) & ~mine).sum(dim=1)
        want_t += ((L > target[None, :]) & ~mine).sum(dim=0)
    diff_i = int((want_i != rank_i.long()).sum())
    diff_t = int((want_t != rank_t.long()).sum())
    res['ranks_differing_from_float64'] = {'i2t': diff_i, 't2i': diff_t}
    r1_i, r1_t = float((want_i < 1).double().mean()), float((want_t < 1).double().mean())
    print(f'ranks differing from the float64 ranking (near-ties decide either way): i2t {diff_i} of {N_IMG}, t2i {diff_t} of {N_TXT}; '
          f'recall@1 {out_r[0].item():.4f} / {out_r[len(KS)].item():.4f} (float64: {r1_i:.4f} / {r1_t:.4f})')

    # the Python call, allocations and the pinned offset copy included
    for _ in range(2):
        retrieval_recall(d_img, d_txt, counts, KS)
    torch.cuda.synchronize()
    t_py = [timed(lambda: retrieval_recall(d_img, d_txt, counts, KS), args.reps) for _ in range(3)]
    res['python_call_ms_median'] = statistics.median(t_py)
    print(f'metrics.retrieval_recall: {statistics.median(t_py):.3f} ms per call')
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

"""Top-K search over embeddings: `dclip_topk_search` at E = 512 on the MS-COCO 5k shapes (25 010 captions
against 5 000 images with k = 10, and the other way round) and a zero-shot shape (50 000 images against 1 000 classes with k = 5), beside
the two things it can be held against, in the same session:
  `dclip_retrieval_recall` at 5 000 x 25 010: the same tiles with a counter in place of a list, both directions in one call: the floor
    of this design;
  the torch path, normalize + matmul + topk: the only alternative without the kernel; it writes the [nq, ng] logits.

Per call (workspaces allocated once, device events around `--reps` back-to-back calls, the contenders alternating over `--rounds` rounds
so that all see the same clocks and neighbours): ms per call as min / median / max over the rounds, ps per logit element (per direction
for the recall call, which forms every logit twice), and the bytes each must read.  Then, at 25 010 x 5 000, how many rows' index lists
differ from the float64 ranking's (near-ties decide either way), and how many from the torch path's.

    python tools/diag/topk_bench.py [--reps 10] [--rounds 7] [--json PATH]
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

E = 512
SHAPES = [(25010, 5000, 10), (5000, 25010, 10), (50000, 1000, 5)]      # (nq, ng, k)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def summary(name, ts, elements, nbytes, rounds, reps, what='ps per logit element'):
    med = statistics.median(ts)
    print(f'  {name:8s}: {min(ts):8.3f} / {med:8.3f} / {max(ts):8.3f} ms per call (min / median / max of {rounds} rounds x {reps} calls)  '
          f'{med * 1e9 / elements:7.3f} {what}  must read {nbytes / 2 ** 20:.1f} MiB', flush=True)
    return {'ms_min': min(ts), 'ms_median': med, 'ms_max': max(ts), 'ps_per_element': med * 1e9 / elements, 'bytes_must_read': nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'topk_bench.py measures on an MI355X; there is no CPU path'
    l = lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    res = {'E': E, 'reps': args.reps, 'rounds': args.rounds, 'shapes': []}
    recall_ps = None
    for nq, ng, k in SHAPES:
        centres = torch.randn(1000, E, generator=g)
        q = (centres[torch.randint(0, 1000, (nq,), generator=g)] + 2 * torch.randn(nq, E, generator=g)).cuda()
        gal = (centres[torch.randint(0, 1000, (ng,), generator=g)] + 2 * torch.randn(ng, E, generator=g)).cuda()
        ws = torch.empty(l.dclip_topk_search_workspace(nq, ng, E, k), dtype=torch.uint8, device='cuda')
        idx = torch.empty(nq, k, dtype=torch.int32, device='cuda')
        score = torch.empty(nq, k, device='cuda')

        def search():
            l.dclip_topk_search(q.data_ptr(), gal.data_ptr(), nq, ng, E, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(), st)

        def torch_path():
            return torch.topk(torch.nn.functional.normalize(q, dim=1) @ torch.nn.functional.normalize(gal, dim=1).t(), k, dim=1)

        contenders = [('search', search), ('torch', torch_path)]
        with_recall = (nq, ng) == (5000, 25010)
        if with_recall:                                          # the recall call on the same rows: five captions per image, ten with six
            counts = [5] * nq
            for i in range(ng - 5 * nq):
                counts[(i * 499) % nq] += 1
            offs = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32).cuda()
            karr = (ctypes.c_int32 * 3)(1, 5, 10)
            ws_r = torch.empty(l.dclip_retrieval_recall_workspace(nq, ng, E), dtype=torch.uint8, device='cuda')
            out_r = torch.empty(8, device='cuda')

            def recall():
                l.dclip_retrieval_recall(q.data_ptr(), gal.data_ptr(), offs.data_ptr(), nq, ng, E, karr, 3, out_r.data_ptr(), None, None,
                                         ws_r.data_ptr(), ws_r.numel(), st)
            contenders.append(('recall', recall))
        for _ in range(3):                                       # warm-up of all
            for _, fn in contenders:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in contenders}
        for _ in range(args.rounds):
            for name, fn in contenders:
                times[name].append(timed(fn, args.reps))
        el = float(nq) * ng
        rows_bytes = (nq + ng) * E * 4
        print(f'{nq} x {ng} x {E}, k = {k}:')
        rec = {'nq': nq, 'ng': ng, 'k': k}
        # bytes each must read: the raw rows once; the torch path also writes and reads back the [nq, ng] logits
        rec['search'] = summary('search', times['search'], el, rows_bytes, args.rounds, args.reps)
        rec['torch'] = summary('torch', times['torch'], el, rows_bytes + nq * ng * 4, args.rounds, args.reps)
        rec['search_over_torch'] = rec['search']['ms_median'] / rec['torch']['ms_median']
        print(f'  search / torch, median ms per call: {rec["search_over_torch"]:.3f}   (the torch path holds {nq * ng * 4 / 2 ** 20:.0f} MiB of logits)')
        if with_recall:
            rec['recall'] = summary('recall', times['recall'], 2 * el, rows_bytes + (nq + 1) * 4, args.rounds, args.reps,
                                    'ps per logit element per direction')
            recall_ps = rec['recall']['ps_per_element']
        res['shapes'].append(rec)

        if (nq, ng) == (25010, 5000):                            # the index lists against float64 logits (torch, on the device)
            search()
            t_idx = torch_path().indices
            a = torch.nn.functional.normalize(q.double(), dim=1)
            b = torch.nn.functional.normalize(gal.double(), dim=1)
            differ64 = differ_torch = 0
            worst = 0.0
            for s in range(0, nq, 1000):                         # 1 000 queries at a time: 40 MB of float64 logits
                L = a[s:s + 1000] @ b.t()
                order = torch.sort(L, dim=1, descending=True, stable=True).indices[:, :k]
                mine = idx[s:s + 1000].long()
                differ64 += int((order != mine).any(dim=1).sum())
                differ_torch += int((t_idx[s:s + 1000] != mine).any(dim=1).sum())
                worst = max(worst, float((L.gather(1, mine) - score[s:s + 1000].double()).abs().max()))
            rec['rows_differing_from_float64'] = differ64
            rec['rows_differing_from_torch_path'] = differ_torch
            rec['max_score_error'] = worst
            print(f'  rows whose index list differs from the float64 ranking (near-ties decide either way): {differ64} of {nq}; from the '
                  f'torch path: {differ_torch}; max |score - L64| = {worst:.3e} (bound {(2 * E + 8) * 2.0 ** -24:.3e})')
        torch.cuda.empty_cache()
    for rec in res['shapes']:
        rec['search_per_element_over_recall'] = rec['search']['ps_per_element'] / recall_ps
        print(f'{rec["nq"]} x {rec["ng"]}: search per element / recall per element per direction = {rec["search_per_element_over_recall"]:.3f}')
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()

"""Validation retrieval metrics: what the reference's `log_acc` / `log_diag_score` compute from a
logits matrix (dual_distill_model.py:204-224, distil_model.py:171-191), from the embeddings, on the HIP kernel
`dclip_retrieval_metrics` — the [n, n] logits never reach HBM and torchmetrics is not needed.

`retrieval_recall` is the MS-COCO protocol the reference's one-caption validation cannot express: Recall@K with several captions per
image, both directions, on `dclip_retrieval_recall`.

`kendall_tau` is what a caption metric itself is judged by: Kendall tau-b / tau-c of its scores against human ratings, on
`dclip_kendall_tau`; `rank_correlation` is the other two coefficients such work reports, Spearman rho and Pearson r, on
`dclip_rank_correlation`.

`topk_search` asks the opposite question of the recall figures, which gallery rows are a query's best, on `dclip_topk_search`;
`group_mean_rows` forms class embeddings from prompt ensembles on `dclip_group_mean_rows` (zeroshot.ZeroShotClassifier uses both)."""
import ctypes

import torch

from ._groups import group_offsets
from ._lib import lib

K_LIST = (1, 3, 5, 10, 20, 50)          # reference dual_distill_model.py:87, distil_model.py:65


def retrieval_metrics(rows, cols, k_list=K_LIST, return_ranks=False):
    """rows, cols: [n, E] embeddings (any float dtype, un-normalised); logits = norm(rows) @ norm(cols).T as the reference's
    norm_and_logits (dual_distill_model.py:271-275).  -> {'acc_top{k}': .., 'softmax_mean_score': .., 'mean_score': ..}
    as 0-dim CUDA tensors (views of one result vector; no host sync)."""
    if not rows.is_cuda or not cols.is_cuda:
        raise RuntimeError('distillclip_amd has no CPU path: retrieval_metrics needs CUDA (HIP) tensors')
    if rows.dim() != 2 or rows.shape != cols.shape:
        raise ValueError(f'retrieval_metrics: need two [n, E] matrices, got {tuple(rows.shape)} and {tuple(cols.shape)}')
    rows = rows.detach().float().contiguous()
    cols = cols.detach().float().contiguous()
    n, E = rows.shape
    ks = [int(k) for k in k_list]
    out = torch.empty(len(ks) + 2, dtype=torch.float32, device=rows.device)
    ranks = torch.empty(n, dtype=torch.int32, device=rows.device) if return_ranks else None
    nbytes = lib().dclip_retrieval_metrics_workspace(n, E)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=rows.device)
    karr = (ctypes.c_int32 * max(len(ks), 1))(*ks)
    lib().dclip_retrieval_metrics(rows.data_ptr(), cols.data_ptr(), n, E, karr, len(ks), out.data_ptr(),
                                  ranks.data_ptr() if ranks is not None else None, ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
    res = {f'acc_top{k}': out[i] for i, k in enumerate(ks)}
    res['softmax_mean_score'] = out[len(ks)]
    res['mean_score'] = out[len(ks) + 1]
    if return_ranks:
        res['ranks'] = ranks
    return res


RECALL_K_LIST = (1, 5, 10)              # the cut-offs MS-COCO retrieval is reported at
MAX_CUTOFFS = 8                         # include/dclip.h: nk <= 8


def caption_offsets(counts, n_img, n_txt):
    """counts: host list or CPU tensor of n_img non-negative caption counts that sum to n_txt (image i owns the next counts[i] caption
    rows) -> the n_img + 1 offsets as a list.  Needs no GPU; every complaint is a ValueError."""
    return group_offsets(counts, n_img, n_txt, 'retrieval_recall', 'caption', 'text_rows')


def _check_recall_shapes(image_rows, text_rows, k_list):
    if image_rows.dim() != 2 or text_rows.dim() != 2 or image_rows.shape[1] != text_rows.shape[1]:
        raise ValueError(f'retrieval_recall: need [n_img, E] and [n_txt, E] matrices, got {tuple(image_rows.shape)} and '
                         f'{tuple(text_rows.shape)}')
    n_img, E = image_rows.shape
    n_txt = text_rows.shape[0]
    if E < 16 or E % 16:
        raise ValueError(f'retrieval_recall: E={E} must be a positive multiple of 16')
    if not (1 <= n_img < 2 ** 24 and 1 <= n_txt < 2 ** 24):
        raise ValueError(f'retrieval_recall: need 1 <= n_img, n_txt < 2^24 (n_img={n_img}, n_txt={n_txt})')
    ks = [int(k) for k in k_list]
    if len(ks) > MAX_CUTOFFS:
        raise ValueError(f'retrieval_recall: {len(ks)} cut-offs, at most {MAX_CUTOFFS} per call')
    return n_img, n_txt, E, ks


def retrieval_recall(image_rows, text_rows, counts, k_list=RECALL_K_LIST, return_ranks=False):
    """Recall@K of image -> text and text -> image retrieval with several captions per image.  image_rows [n_img, E], text_rows [n_txt, E]:
    un-normalised embeddings (any float dtype); counts: host list or CPU tensor, image i owns the next counts[i] rows of text_rows.
    An image hits at k when ANY of its captions is among its k best; a caption hits when its image is among the caption's k best; ties
    favour the target (include/dclip.h: dclip_retrieval_recall).  Images without captions are left out of the image -> text figures.
    -> {'i2t_recall@{k}', 't2i_recall@{k}', 'i2t_mean_rank', 't2i_mean_rank'} as 0-dim CUDA tensors (views of one result vector; no host
    sync); with return_ranks also 'i2t_ranks' [n_img] and 't2i_ranks' [n_txt], int32, 0-based, -1 for an image without captions.
    Every ValueError is raised before any launch."""
    n_img, n_txt, E, ks = _check_recall_shapes(image_rows, text_rows, k_list)
    offs = caption_offsets(counts, n_img, n_txt)
    if not image_rows.is_cuda or not text_rows.is_cuda:
        raise RuntimeError('distillclip_amd has no CPU path: retrieval_recall needs CUDA (HIP) tensors')
    dev = image_rows.device
    img = image_rows.detach().float().contiguous()
    txt = text_rows.detach().float().contiguous()
    offsets = torch.tensor(offs, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)     # (pageable memory would make the host wait)
    out = torch.empty(2 * len(ks) + 2, dtype=torch.float32, device=dev)
    rank_i = torch.empty(n_img, dtype=torch.int32, device=dev) if return_ranks else None
    rank_t = torch.empty(n_txt, dtype=torch.int32, device=dev) if return_ranks else None
    ws = torch.empty(max(lib().dclip_retrieval_recall_workspace(n_img, n_txt, E), 16), dtype=torch.uint8, device=dev)
    karr = (ctypes.c_int32 * max(len(ks), 1))(*ks)
    lib().dclip_retrieval_recall(img.data_ptr(), txt.data_ptr(), offsets.data_ptr(), n_img, n_txt, E, karr, len(ks), out.data_ptr(),
                                 rank_i.data_ptr() if return_ranks else None, rank_t.data_ptr() if return_ranks else None,
                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    res = {}
    for d, name in enumerate(('i2t', 't2i')):
        for i, k in enumerate(ks):
            res[f'{name}_recall@{k}'] = out[d * len(ks) + i]
    res['i2t_mean_rank'] = out[2 * len(ks)]
    res['t2i_mean_rank'] = out[2 * len(ks) + 1]
    if return_ranks:
        res['i2t_ranks'] = rank_i
        res['t2i_ranks'] = rank_t
    return res


KENDALL_MAX_ITEMS = 262144             # include/dclip.h: dclip_kendall_tau takes 2 <= n <= 262 144 ...
KENDALL_MAX_VECTORS = 4                 # ... and 1 <= C <= 4 score vectors
KENDALL_COUNTS = ('con', 'dis', 'tie_x', 'tie_y', 'tie_xy', 'distinct_x', 'distinct_y', 'nan')


def kendall_tau(scores, human, return_counts=False):
    """Kendall tau-b and tau-c of a metric's scores against human ratings, as scipy.stats.kendalltau defines them, on
    `dclip_kendall_tau`: one pass over all pairs with integer counters, so the result is exact and the same call gives the same bits.
    scores [n] or [C, n] (C <= 4 score vectors, all correlated with the same ratings in one pass), human [n]: device tensors of any
    float or integer dtype, taken to f32 (equal inputs give equal f32 values, so ties survive).
    -> {'tau_b', 'tau_c'}: float64 device tensors of shape [] or [C], views of one result buffer; with return_counts also 'counts',
    int64 [8] or [C, 8] in the order of KENDALL_COUNTS.  A NaN in a score vector makes that vector's taus NaN, a NaN in human all of them.
    Every ValueError is raised before any launch; nothing waits for the device."""
    if not torch.is_tensor(scores) or not torch.is_tensor(human) or scores.dim() not in (1, 2) or human.dim() != 1:
        raise ValueError(f'kendall_tau: need scores [n] or [C, n] and human [n], got {tuple(getattr(scores, "shape", ()))} and '
                         f'{tuple(getattr(human, "shape", ()))}')
    many = scores.dim() == 2
    C, n = (scores.shape[0], scores.shape[1]) if many else (1, scores.shape[0])
    if human.shape[0] != n:
        raise ValueError(f'kendall_tau: {n} scores per vector against {human.shape[0]} ratings')
    if not 2 <= n <= KENDALL_MAX_ITEMS:
        raise ValueError(f'kendall_tau: need 2 <= n <= {KENDALL_MAX_ITEMS} items (n={n})')
    if not 1 <= C <= KENDALL_MAX_VECTORS:
        raise ValueError(f'kendall_tau: need 1 <= C <= {KENDALL_MAX_VECTORS} score vectors per call (C={C})')
    if not scores.is_cuda or not human.is_cuda:
        raise ValueError('kendall_tau: scores and human are device tensors (distillclip_amd has no CPU path)')
    if scores.device != human.device:
        raise ValueError(f'kendall_tau: scores on {scores.device}, human on {human.device}')
    dev = scores.device
    x = scores.detach().float().contiguous()
    y = human.detach().float().contiguous()
    tau = torch.empty(C, 2, dtype=torch.float64, device=dev)
    counts = torch.empty(C, 8, dtype=torch.int64, device=dev)
    ws = torch.empty(max(lib().dclip_kendall_tau_workspace(n, C), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib().dclip_kendall_tau(x.data_ptr(), n, C, y.data_ptr(), n, tau.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream().cuda_stream)
    res = {'tau_b': tau[:, 0] if many else tau[0, 0], 'tau_c': tau[:, 1] if many else tau[0, 1]}
    if return_counts:
        res['counts'] = counts if many else counts[0]
    return res


RANKCORR_SUMS = ('sxy', 'sxx', 'syy', 'nan')       # include/dclip.h: the int64 sums of the centred twice-ranks, and the NaN items


def rank_correlation(scores, human, return_sums=False, return_ranks=False):
    """Spearman rho and Pearson r of a metric's scores against human ratings, as scipy.stats.spearmanr (average ranks on ties) and
    scipy.stats.pearsonr define them, on `dclip_rank_correlation`: rho comes from exact int64 sums of the twice-ranks R_i = 2 #{v_j < v_i}
    + #{v_j == v_i} + 1, r from two passes in double with sums of a fixed shape, so the same call gives the same bits.
    scores [n] or [C, n] (C <= 4 score vectors, all correlated with the same ratings in one call; the ratings are ranked once), human [n]:
    device tensors of any float or integer dtype, taken to f32 (equal inputs give equal f32 values, so ties survive).  The limits on n
    and C are those of `kendall_tau`.
    -> {'spearman', 'pearson'}: float64 device tensors of shape [] or [C], views of one result buffer; with return_sums also 'sums',
    int64 [4] or [C, 4] in the order of RANKCORR_SUMS; with return_ranks also 'ranks', int32 twice-ranks [n] or [C, n], and 'human_ranks'
    [n].  A NaN in a score vector makes that vector's coefficients NaN, a NaN in human all of them; a constant vector gives NaN for
    both; +-inf is a legal value for rho and makes r NaN.
    Out of scope: p-values and confidence intervals, weighted variants, gathering across ranks (pass gathered vectors), n > 262 144,
    and sharing one pair walk with the Kendall kernel.  Every ValueError is raised before any launch; nothing waits for the device."""
    if not torch.is_tensor(scores) or not torch.is_tensor(human) or scores.dim() not in (1, 2) or human.dim() != 1:
        raise ValueError(f'rank_correlation: need scores [n] or [C, n] and human [n], got {tuple(getattr(scores, "shape", ()))} and '
                         f'{tuple(getattr(human, "shape", ()))}')
    many = scores.dim() == 2
    C, n = (scores.shape[0], scores.shape[1]) if many else (1, scores.shape[0])
    if human.shape[0] != n:
        raise ValueError(f'rank_correlation: {n} scores per vector against {human.shape[0]} ratings')
    if not 2 <= n <= KENDALL_MAX_ITEMS:
        raise ValueError(f'rank_correlation: need 2 <= n <= {KENDALL_MAX_ITEMS} items (n={n})')
    if not 1 <= C <= KENDALL_MAX_VECTORS:
        raise ValueError(f'rank_correlation: need 1 <= C <= {KENDALL_MAX_VECTORS} score vectors per call (C={C})')
    if not scores.is_cuda or not human.is_cuda:
        raise ValueError('rank_correlation: scores and human are device tensors (distillclip_amd has no CPU path)')
    if scores.device != human.device:
        raise ValueError(f'rank_correlation: scores on {scores.device}, human on {human.device}')
    dev = scores.device
    x = scores.detach().float().contiguous()
    y = human.detach().float().contiguous()
    corr = torch.empty(C, 2, dtype=torch.float64, device=dev)
    sums = torch.empty(C, 4, dtype=torch.int64, device=dev) if return_sums else None
    ranks = torch.empty(C + 1, n, dtype=torch.int32, device=dev) if return_ranks else None
    ws = torch.empty(max(lib().dclip_rank_correlation_workspace(n, C), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib().dclip_rank_correlation(x.data_ptr(), n, C, y.data_ptr(), n, corr.data_ptr(), sums.data_ptr() if return_sums else None,
                                     ranks.data_ptr() if return_ranks else None, ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream().cuda_stream)
    res = {'spearman': corr[:, 0] if many else corr[0, 0], 'pearson': corr[:, 1] if many else corr[0, 1]}
    if return_sums:
        res['sums'] = sums if many else sums[0]
    if return_ranks:
        res['ranks'] = ranks[:C] if many else ranks[0]
        res['human_ranks'] = ranks[C]
    return res


TOPK_MAX_K = 64                         # include/dclip.h: dclip_topk_search takes 1 <= k <= 64


def topk_search(query_rows, gallery_rows, k, return_scores=True):
    """The k best gallery rows of every query by cosine, on `dclip_topk_search`.  query_rows [nq, E], gallery_rows [ng, E]: un-normalised
    embeddings (any float dtype).  -> (idx int32 [nq, k], score f32 [nq, k], or None without return_scores): row i holds the first k
    gallery indices in the total order (cosine descending, index ascending) and their cosines; equal cosines come in index order, a row
    that is zero or holds an inf or a NaN has cosine 0 with everything, and with k > ng the trailing entries are idx -1, score -inf
    (include/dclip.h).  The [nq, ng] logits never reach HBM, and a cosine is bit for bit the one `retrieval_recall` compares.
    Out of scope: approximate search and k > 64.  Every ValueError is raised before any launch; nothing waits for the device."""
    if not torch.is_tensor(query_rows) or not torch.is_tensor(gallery_rows) or query_rows.dim() != 2 or gallery_rows.dim() != 2 or \
            query_rows.shape[1] != gallery_rows.shape[1]:
        raise ValueError(f'topk_search: need [nq, E] and [ng, E] matrices, got {tuple(getattr(query_rows, "shape", ()))} and '
                         f'{tuple(getattr(gallery_rows, "shape", ()))}')
    nq, E = query_rows.shape
    ng = gallery_rows.shape[0]
    k = int(k)
    if E < 16 or E % 16:
        raise ValueError(f'topk_search: E={E} must be a positive multiple of 16')
    if not (1 <= nq < 2 ** 24 and 1 <= ng < 2 ** 24):
        raise ValueError(f'topk_search: need 1 <= nq, ng < 2^24 (nq={nq}, ng={ng})')
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f'topk_search: need 1 <= k <= {TOPK_MAX_K} (k={k})')
    if not query_rows.is_cuda or not gallery_rows.is_cuda:
        raise ValueError('topk_search: query_rows and gallery_rows are device tensors (distillclip_amd has no CPU path)')
    if query_rows.device != gallery_rows.device:
        raise ValueError(f'topk_search: query_rows on {query_rows.device}, gallery_rows on {gallery_rows.device}')
    dev = query_rows.device
    q = query_rows.detach().float().contiguous()
    g = gallery_rows.detach().float().contiguous()
    idx = torch.empty(nq, k, dtype=torch.int32, device=dev)
    score = torch.empty(nq, k, dtype=torch.float32, device=dev) if return_scores else None
    ws = torch.empty(max(lib().dclip_topk_search_workspace(nq, ng, E, k), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        lib().dclip_topk_search(q.data_ptr(), g.data_ptr(), nq, ng, E, k, idx.data_ptr(), score.data_ptr() if return_scores else None,
                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    return idx, score


GROUP_MEAN_MAX_E = 4096                 # include/dclip.h: dclip_group_mean_rows takes E <= 4096


def group_mean_rows(rows, counts):
    """The mean of the normalised rows of each group, on `dclip_group_mean_rows`: class embeddings from prompt ensembles.  rows [n_rows, E]:
    un-normalised embeddings (any float dtype); counts: host list or CPU tensor, group c owns the next counts[c] rows.
    -> f32 [n_groups, E]: out[c] = mean over the group of x / |x| (a zero or non-finite row adds nothing, an empty group gives the zero
    row), rows added in index order without atomics, so the same call gives the same bits.  Every ValueError is raised before any
    launch; nothing waits for the device."""
    if not torch.is_tensor(rows) or rows.dim() != 2:
        raise ValueError(f'group_mean_rows: need an [n_rows, E] matrix, got {tuple(getattr(rows, "shape", ()))}')
    n_rows, E = rows.shape
    n_groups = len(counts) if not torch.is_tensor(counts) else counts.numel()
    offs = group_offsets(counts, n_groups, n_rows, 'group_mean_rows', 'row', 'rows')
    if E < 16 or E % 16 or E > GROUP_MEAN_MAX_E:
        raise ValueError(f'group_mean_rows: E={E} must be a positive multiple of 16, at most {GROUP_MEAN_MAX_E}')
    if not (1 <= n_groups < 2 ** 24 and 1 <= n_rows < 2 ** 24):
        raise ValueError(f'group_mean_rows: need 1 <= n_groups, n_rows < 2^24 (n_groups={n_groups}, n_rows={n_rows})')
    if not rows.is_cuda:
        raise ValueError('group_mean_rows: rows is a device tensor (distillclip_amd has no CPU path)')
    dev = rows.device
    x = rows.detach().float().contiguous()
    offsets = torch.tensor(offs, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)     # (pageable memory would make the host wait)
    out = torch.empty(n_groups, E, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        lib().dclip_group_mean_rows(x.data_ptr(), offsets.data_ptr(), n_groups, n_rows, E, out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    return out


def gather_rows(x, group=None):
    """all ranks' rows in rank order (the reference's `self.all_gather(...)` + reshape(-1, E), dual_distill_model.py:141-160);
    the identity without an initialised process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return x
    x = x.contiguous()
    out = torch.empty((dist.get_world_size(group) * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    dist.all_gather_into_tensor(out, x, group=group)
    return out

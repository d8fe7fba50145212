"""Rank correlation of L-CLIPScore with human ratings, the number a caption metric is judged by: Kendall tau-c on Flickr8k-Expert
(5 664 pairs x 3 annotators) and Composite, tau-b on Flickr8k-CF, as CLIPScore (Hessel et al. 2021) and the work after it report them;
Spearman rho and Pearson r where a benchmark reports those instead or as well (THumB, WMT-style metric evaluations, comparisons with learned metrics).

    hc = HumanCorrelation.from_model(model)
    for images, candidates, human, references, ref_counts in loader:     # human [B] (or [B, K]), or [B, A] with A annotators per pair
        hc.update(images, candidates, human, references, ref_counts)
    metrics = hc.compute()                           # {'clip_s_tau_b': .., 'clip_s_tau_c': .., 'refclip_s_tau_c': .., ..}
    more = hc.compute(stats=('spearman', 'pearson'))                     # {'clip_s_spearman': .., 'clip_s_pearson': .., ..}

The scorer runs as in score.py; the stored score vectors are correlated with the stored ratings by ONE call of the HIP kernels behind
`metrics.kendall_tau` (include/dclip.h: dclip_kendall_tau), all score kinds in the same pass; `stats` adds or substitutes Spearman and
Pearson, again ONE call of `metrics.rank_correlation` (dclip_rank_correlation) for all score kinds, and no Kendall call when 'kendall' is
not asked for.  Nothing here waits for the device.
Out of scope: gathering across ranks (`add_scores` takes flat vectors formed elsewhere, gathered ones included, and is the hook for it),
p-values and confidence intervals, weighted variants, more than 262 144 rated items, and sharing one pair walk between the Kendall and
the rank kernels.
"""
import torch

from .metrics import KENDALL_MAX_ITEMS, kendall_tau, rank_correlation

SCORE_NAMES = ('clip_s', 'ref_s', 'refclip_s')
STATS = ('kendall', 'spearman', 'pearson')


class HumanCorrelation:
    """scorer: an LCLIPScore (its towers' parameters, requires_grad and train / eval flags are left alone).  The towers run on the weights
    they hold at the call: `with opt.ema_weights():` (FusedAdamW) around the calls scores the averaged student instead of the last iterate."""

    def __init__(self, scorer):
        if not callable(scorer):
            raise ValueError(f'HumanCorrelation: scorer must be an LCLIPScore, got {type(scorer).__name__}')
        self.scorer = scorer
        self.reset()

    @classmethod
    def from_model(cls, model, **kw):
        """model: a two-tower distillation model (DualDistillModel: its student is scored) or a CLIPModel; kw go to LCLIPScore"""
        from .score import LCLIPScore
        return cls(LCLIPScore.from_model(model, **kw))

    def reset(self):
        """forget the stored scores and ratings"""
        self._human, self._scores = [], [[], [], []]
        self._with_refs = None                                      # set by the first update() / add_scores()
        self._n = 0

    def _check_refs(self, with_refs):
        if self._with_refs is not None and self._with_refs != with_refs:
            raise ValueError('HumanCorrelation: updates with references and updates without references cannot be mixed '
                             f'(so far: {"with" if self._with_refs else "without"})')

    def _store(self, human, vectors, with_refs):
        self._human.append(human)
        for kept, v in zip(self._scores, vectors):
            kept.append(v)
        self._with_refs = with_refs
        self._n += human.shape[0]

    @torch.no_grad()
    def update(self, images, candidates, human, references=None, ref_counts=None):
        """images, candidates, references, ref_counts: as LCLIPScore.forward takes them.  human: the ratings of the scored pairs, of the
        shape of clip_s ([B] for candidates [B, L], [B, K] for [B, K, L]) or with one trailing annotator axis ([B, A], [B, K, A]): every
        score is then repeated against its A ratings.  Any float or integer dtype; a host tensor goes over in a pinned, non-blocking copy."""
        if images.dim() != 4 or candidates.dim() not in (2, 3) or candidates.shape[0] != images.shape[0]:
            raise ValueError(f'HumanCorrelation: need images [B, C, H, W] and candidates [B, L] or [B, K, L], got {tuple(images.shape)} '
                             f'and {tuple(candidates.shape)}')
        shape = tuple(candidates.shape[:-1])
        human = torch.as_tensor(human)
        if tuple(human.shape) == shape:
            A = None
        elif human.dim() == len(shape) + 1 and tuple(human.shape[:-1]) == shape and human.shape[-1] >= 1:
            A = human.shape[-1]
        else:
            raise ValueError(f'HumanCorrelation: human must be {list(shape)} or {list(shape)} + [A] for candidates '
                             f'{tuple(candidates.shape)}, got {tuple(human.shape)}')
        with_refs = references is not None
        self._check_refs(with_refs)
        out = self.scorer(images, candidates, references, ref_counts)
        dev = out.clip_s.device
        human = human.detach().float().reshape(-1)
        if not human.is_cuda:
            human = human.pin_memory().to(dev, non_blocking=True)   # (a copy from pageable memory would make the host wait)
        vectors = [None if s is None else s.reshape(-1) if A is None else s.reshape(-1).repeat_interleave(A) for s in out]
        self._store(human, vectors, with_refs)

    def add_scores(self, human, clip_s, ref_s=None, refclip_s=None):
        """flat device vectors formed elsewhere (another scorer, vectors gathered from other ranks): n ratings and n scores of each kind;
        ref_s and refclip_s come together"""
        vectors = [clip_s, ref_s, refclip_s]
        if (ref_s is None) != (refclip_s is None):
            raise ValueError('HumanCorrelation: ref_s and refclip_s come together (one of them is None)')
        given = [v for v in vectors if v is not None]
        if human.dim() != 1 or human.shape[0] < 1 or any(v.dim() != 1 or v.shape[0] != human.shape[0] for v in given):
            raise ValueError(f'HumanCorrelation: need flat vectors of one length n >= 1, got human {tuple(human.shape)} and scores '
                             f'{[tuple(v.shape) for v in given]}')
        with_refs = ref_s is not None
        self._check_refs(with_refs)
        if not human.is_cuda or not all(v.is_cuda for v in given):
            raise ValueError('HumanCorrelation: add_scores takes device tensors (distillclip_amd has no CPU path)')
        self._store(human.detach().float(), [None if v is None else v.detach().float() for v in vectors], with_refs)

    def compute(self, return_counts=False, stats=('kendall',)):
        """-> {'clip_s_tau_b', 'clip_s_tau_c'}, and the same two for ref_s and refclip_s when references were given: 0-dim float64 device
        tensors, views of one result buffer; with return_counts also '{name}_counts', int64 [8] (metrics.KENDALL_COUNTS).  One
        concatenation per vector and one kernel call.
        stats: a non-empty subset of ('kendall', 'spearman', 'pearson').  'spearman' / 'pearson' add '{name}_spearman' / '{name}_pearson'
        for the same score names, from one `rank_correlation` call for all of them; without 'kendall' no Kendall call is issued and
        there are no tau entries (return_counts then has nothing to return: a ValueError)."""
        stats = tuple(stats)
        if not stats or any(s not in STATS for s in stats) or len(set(stats)) != len(stats):
            raise ValueError(f'HumanCorrelation: stats must be a non-empty subset of {STATS} without repeats, got {stats}')
        if return_counts and 'kendall' not in stats:
            raise ValueError(f"HumanCorrelation: return_counts returns the Kendall counts, and stats={stats} has no 'kendall'")
        if not 2 <= self._n <= KENDALL_MAX_ITEMS:
            raise ValueError(f'HumanCorrelation: {self._n} rated items stored since the last reset(), need 2 to {KENDALL_MAX_ITEMS}')
        names = SCORE_NAMES if self._with_refs else SCORE_NAMES[:1]
        dev = self._human[0].device
        human = torch.cat(self._human) if len(self._human) > 1 else self._human[0]
        scores = torch.empty(len(names), self._n, dtype=torch.float32, device=dev)
        for c in range(len(names)):
            torch.cat(self._scores[c], out=scores[c])
        out = {}
        if 'kendall' in stats:
            res = kendall_tau(scores, human, return_counts=return_counts)
            for c, name in enumerate(names):
                out[f'{name}_tau_b'] = res['tau_b'][c]
                out[f'{name}_tau_c'] = res['tau_c'][c]
                if return_counts:
                    out[f'{name}_counts'] = res['counts'][c]
        if 'spearman' in stats or 'pearson' in stats:
            res = rank_correlation(scores, human)
            for stat in ('spearman', 'pearson'):
                if stat in stats:
                    for c, name in enumerate(names):
                        out[f'{name}_{stat}'] = res[stat][c]
        return out

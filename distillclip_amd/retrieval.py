"""Recall@K retrieval evaluation of a trained image / text tower pair, the MS-COCO protocol: every image has several captions (5 000
images x 25 010 captions on the 5k test split); image -> text asks whether ANY of an image's captions is among its K best, text -> image
where a caption's image ranks among all images.

    ev = RetrievalEvaluator.from_model(model)
    for images, captions, counts in loader:          # captions [M, L] int tokens, image i of the batch owning the next counts[i] rows
        ev.update(images, captions, counts)
    metrics = ev.compute()                           # {'i2t_recall@1': .., 't2i_recall@10': .., 'i2t_mean_rank': .., ..}

The towers run in inference under torch.no_grad(), in chunks; the stored rows are ranked by ONE call of the HIP kernels behind
`metrics.retrieval_recall` (include/dclip.h: dclip_retrieval_recall) — the [n_img, n_txt] logits never reach HBM.  Nothing here waits for
the device.  Gathering ragged caption sets across ranks is out of scope: `add_embeddings` takes rows formed elsewhere, gathered ones
included, and is the hook for it.
"""
import torch

from ._groups import encode_rows, flatten_groups, tower_pair
from .metrics import RECALL_K_LIST, MAX_CUTOFFS, caption_offsets, retrieval_recall


class RetrievalEvaluator:
    """image_encoder / text_encoder: two towers of this package (students or CLIP towers) whose out_dim agree.  k_list: at most 8
    cut-offs.  max_batch: the most rows one tower run takes; larger inputs go through in chunks.  The towers' parameters, requires_grad
    and train / eval flags are left alone.  The towers run on the weights
    they hold at the call: `with opt.ema_weights():` (FusedAdamW) around the calls scores the averaged student instead of the last iterate."""

    def __init__(self, image_encoder, text_encoder, k_list=RECALL_K_LIST, max_batch=512):
        if int(max_batch) < 1:
            raise ValueError(f'RetrievalEvaluator: max_batch={max_batch} must be at least 1')
        self.k_list = tuple(int(k) for k in k_list)
        if len(self.k_list) > MAX_CUTOFFS:
            raise ValueError(f'RetrievalEvaluator: {len(self.k_list)} cut-offs, at most {MAX_CUTOFFS}')
        self.image_encoder = image_encoder
        self.text_encoder = text_encoder
        self.max_batch = int(max_batch)
        self.reset()

    @classmethod
    def from_model(cls, model, **kw):
        """model: a two-tower distillation model (DualDistillModel: its student is evaluated) or a CLIPModel (student or teacher)"""
        return cls(*tower_pair(model, 'RetrievalEvaluator'), **kw)

    def reset(self):
        """forget the stored rows"""
        self._img, self._txt, self._counts = [], [], []

    @torch.no_grad()
    def update(self, images, captions, counts=None):
        """images [B, 3, H, W]; captions int tokens [M, L] with counts (B counts on the host, image b owning the next counts[b] rows) or
        dense [B, Kper, L].  Runs both towers and appends their last_representation rows."""
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError(f'RetrievalEvaluator: images must be [B, C, H, W] with B >= 1, got {tuple(images.shape)}')
        B = images.shape[0]
        captions, offs = flatten_groups(captions, counts, B, 'RetrievalEvaluator', caption_offsets, 'captions', 'counts', 'M', 'Kper')
        img = encode_rows(self.image_encoder, images, self.max_batch)
        txt = encode_rows(self.text_encoder, captions, self.max_batch) if captions.shape[0] else None
        self._img.append(img)                                       # (stored together: a tower that raised leaves nothing behind)
        if txt is not None:
            self._txt.append(txt)
        self._counts.extend(b - a for a, b in zip(offs, offs[1:]))

    def add_embeddings(self, image_rows, text_rows, counts):
        """rows formed elsewhere (another model, rows gathered from other ranks): image_rows [n, E], text_rows [m, E], counts as in update"""
        if image_rows.dim() != 2 or text_rows.dim() != 2 or image_rows.shape[1] != text_rows.shape[1] or image_rows.shape[0] < 1:
            raise ValueError(f'RetrievalEvaluator: need [n, E] and [m, E] rows with n >= 1, got {tuple(image_rows.shape)} and '
                             f'{tuple(text_rows.shape)}')
        offs = caption_offsets(counts, image_rows.shape[0], text_rows.shape[0])
        if not image_rows.is_cuda or not text_rows.is_cuda:
            raise RuntimeError('distillclip_amd has no CPU path: RetrievalEvaluator needs CUDA (HIP) tensors')
        self._img.append(image_rows.detach().float())
        if text_rows.shape[0]:
            self._txt.append(text_rows.detach().float())
        self._counts.extend(b - a for a, b in zip(offs, offs[1:]))

    def compute(self, return_ranks=False):
        """-> what metrics.retrieval_recall returns for everything stored: one concatenation per side and one kernel call"""
        if not self._img or not self._txt:
            raise ValueError('RetrievalEvaluator: nothing to rank (no update() or add_embeddings() since the last reset(), or no caption)')
        img = self._img[0] if len(self._img) == 1 else torch.cat(self._img, dim=0)
        txt = self._txt[0] if len(self._txt) == 1 else torch.cat(self._txt, dim=0)
        return retrieval_recall(img, txt, self._counts, self.k_list, return_ranks=return_ranks)

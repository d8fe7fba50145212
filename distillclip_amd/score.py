"""L-CLIPScore, the metric the reference's students are trained to be ("a lightweight embedding-based captioning metric for evaluating
and training"): CLIP-S and RefCLIP-S of Hessel et al. 2021 from a trained image / text tower pair.

    clip_s    = w * max(cos(image, candidate), 0)                          w = 2.5
    ref_s     = max(0, max over the image's references of cos(candidate, reference)), 0 without references
    refclip_s = harmonic mean of clip_s and ref_s, 0 when both are 0

The towers run in inference under torch.no_grad(); the three scores of every (image, candidate) pair come from ONE launch of the HIP
kernel `dclip_clipscore` on the towers' raw last_representation rows (include/dclip.h) — no normalised copies, no [B K, R] similarity
matrix.  Everything stays on the device and nothing in `forward` waits for it, so the scores can serve as a captioner's reward inside a
training step.  Tokenising is the caller's job, as in training.
"""
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import ops
from ._groups import encode_rows, flatten_groups, group_offsets, tower_pair


class ScoreOutput(NamedTuple):
    clip_s: torch.Tensor                     # [B] or [B, K]
    ref_s: Optional[torch.Tensor]            # the same shape, None without references
    refclip_s: Optional[torch.Tensor]


def _counts(ref_counts, B, R):
    """host list or CPU tensor of B non-negative reference counts that sum to R -> the B + 1 offsets as a list"""
    return group_offsets(ref_counts, B, R, 'LCLIPScore', 'reference', 'references', 'ref_counts')


class LCLIPScore(nn.Module):
    """image_encoder / text_encoder: two towers of this package (students or CLIP towers) whose out_dim agree.  w: the paper's rescaling
    of CLIP-S.  max_batch: the most rows one tower run takes; larger inputs go through in chunks.  The towers run on the weights
    they hold at the call: `with opt.ema_weights():` (FusedAdamW) around the calls scores the averaged student instead of the last iterate."""

    def __init__(self, image_encoder, text_encoder, w=2.5, max_batch=512):
        super().__init__()
        if int(max_batch) < 1:
            raise ValueError(f'LCLIPScore: max_batch={max_batch} must be at least 1')
        self.image_encoder = image_encoder
        self.text_encoder = text_encoder
        self.w = float(w)
        self.max_batch = int(max_batch)

    @classmethod
    def from_model(cls, model, **kw):
        """model: a two-tower distillation model (DualDistillModel: its student is scored) or a CLIPModel (student or teacher)"""
        return cls(*tower_pair(model, 'LCLIPScore'), **kw)

    @torch.no_grad()
    def forward(self, images, candidates, references=None, ref_counts=None) -> ScoreOutput:
        """images [B, 3, H, W]; candidates int tokens [B, L] or [B, K, L]; references int tokens [R, L] with ref_counts (B counts on the
        host, image b owning the next ref_counts[b] rows) or dense [B, Rper, L].  -> ScoreOutput of [B] or [B, K] f32 tensors."""
        if images.dim() != 4:
            raise ValueError(f'LCLIPScore: images must be [B, C, H, W], got {tuple(images.shape)}')
        B = images.shape[0]
        if candidates.dim() not in (2, 3) or candidates.shape[0] != B:
            raise ValueError(f'LCLIPScore: candidates must be [B, L] or [B, K, L] with B={B}, got {tuple(candidates.shape)}')
        many = candidates.dim() == 3
        K, L = (candidates.shape[1], candidates.shape[2]) if many else (1, candidates.shape[1])
        if B < 1 or K < 1:
            raise ValueError(f'LCLIPScore: nothing to score (B={B}, K={K})')
        text = candidates.reshape(B * K, L)
        offsets = None
        if references is not None:
            references, offs = flatten_groups(references, ref_counts, B, 'LCLIPScore', _counts, 'references', 'ref_counts', 'R', 'Rper')
            if references.shape[1] != L:
                raise ValueError(f'LCLIPScore: candidates have {L} tokens, references {references.shape[1]}')
            offsets = torch.tensor(offs, dtype=torch.int32)
            if references.shape[0]:
                text = torch.cat([text, references.to(text.dtype)], dim=0)      # one row set through the text tower
        elif ref_counts is not None:
            raise ValueError('LCLIPScore: ref_counts without references')
        img = encode_rows(self.image_encoder, images, self.max_batch)
        txt = encode_rows(self.text_encoder, text, self.max_batch)
        refs = None
        if offsets is not None:
            refs = txt[B * K:]
            offsets = offsets.pin_memory().to(img.device, non_blocking=True)      # (a copy from pageable memory would make the host wait)
        clip_s, ref_s, refclip_s = ops.clipscore(img, txt[:B * K], refs, offsets, K=K, w=self.w)
        shape = (B, K) if many else (B,)
        return ScoreOutput(clip_s.view(shape), None if ref_s is None else ref_s.view(shape), None if refclip_s is None else refclip_s.view(shape))

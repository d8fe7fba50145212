"""Zero-shot classification with a trained image / text tower pair, the number every CLIP image tower is reported by: each class is
the mean of the normalised embeddings of its prompts ("a photo of a {class}", ...), an image is given the classes whose embedding its
own is closest to, and top-k accuracy asks whether the label is among the k best.

    zs = ZeroShotClassifier.from_model(model)
    zs.set_classes(prompt_tokens, counts)            # int tokens [M, L], class c owning the next counts[c] rows; or dense [C, P, L]
    for images, labels in loader:                    # labels in loader order, on the host or the device
        zs.update(images, labels)
    metrics = zs.compute()                           # {'acc_top1': .., 'acc_top5': ..}
    idx, score = zs.predict(images, k=5)             # the 5 best classes of each image and their cosines

The towers run in inference under torch.no_grad(), in chunks; class embeddings come from `metrics.group_mean_rows`, and the stored image
rows are ranked against them by ONE call of the HIP kernel behind `metrics.topk_search` (include/dclip.h: dclip_topk_search) — the
[n_images, n_classes] logits never reach HBM, and equal cosines go to the lower class index.  Nothing here waits for the device.
Out of scope: gathering across ranks (`add_embeddings` takes rows and labels formed elsewhere, gathered ones included, and is the hook
for it), mean-per-class accuracy, approximate search, k > 64, and tokenising class names (the caller brings tokens, as everywhere else
in this package).
"""
import torch

from ._groups import encode_rows, flatten_groups, group_offsets, tower_pair
from .metrics import TOPK_MAX_K, group_mean_rows, topk_search

WHO = 'ZeroShotClassifier'


def _prompt_offsets(counts, n_classes, n_rows):
    return group_offsets(counts, n_classes, n_rows, WHO, 'prompt', 'prompts')


class ZeroShotClassifier:
    """image_encoder / text_encoder: two towers of this package (students or CLIP towers) whose out_dim agree.  k_list: the cut-offs
    of compute(), each in [1, 64].  max_batch: the most rows one tower run takes; larger inputs go through in chunks.  The towers'
    parameters, requires_grad and train / eval flags are left alone.  The towers run on the weights
    they hold at the call: `with opt.ema_weights():` (FusedAdamW) around the calls scores the averaged student instead of the last iterate."""

    def __init__(self, image_encoder, text_encoder, k_list=(1, 5), max_batch=512):
        if int(max_batch) < 1:
            raise ValueError(f'{WHO}: max_batch={max_batch} must be at least 1')
        self.k_list = tuple(int(k) for k in k_list)
        if not self.k_list or min(self.k_list) < 1 or max(self.k_list) > TOPK_MAX_K:
            raise ValueError(f'{WHO}: k_list={self.k_list} needs at least one cut-off, each in [1, {TOPK_MAX_K}]')
        self.image_encoder = image_encoder
        self.text_encoder = text_encoder
        self.max_batch = int(max_batch)
        self.class_embeddings = None
        self.reset()

    @classmethod
    def from_model(cls, model, **kw):
        """model: a two-tower distillation model (DualDistillModel: its student is evaluated) or a CLIPModel (student or teacher)"""
        return cls(*tower_pair(model, WHO), **kw)

    def reset(self):
        """forget the stored image rows and labels (the classes stay)"""
        self._rows, self._labels = [], []

    # ---- the classes ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def set_classes(self, prompts, counts=None):
        """prompts: int tokens [M, L] with counts (C counts on the host, class c owning the next counts[c] rows) or dense [C, P, L].
        Runs the text tower and stores, per class, the mean of its prompts' normalised rows (an empty class gets the zero row: cosine
        0 with every image)."""
        if not torch.is_tensor(prompts) or prompts.dim() not in (2, 3):
            raise ValueError(f'{WHO}: prompts must be [M, L] or [C, P, L], got {tuple(getattr(prompts, "shape", ()))}')
        if prompts.dim() == 3:
            C = prompts.shape[0]
        else:
            if counts is None:
                raise ValueError(f'{WHO}: prompts [M, L] need counts')
            C = counts.numel() if torch.is_tensor(counts) else len(counts)
        prompts, offs = flatten_groups(prompts, counts, C, WHO, _prompt_offsets, 'prompts', 'counts', 'M', 'P')
        if C < 1 or prompts.shape[0] < 1:
            raise ValueError(f'{WHO}: need at least one class and one prompt, got {C} classes and {prompts.shape[0]} prompts')
        rows = encode_rows(self.text_encoder, prompts, self.max_batch)
        self.class_embeddings = group_mean_rows(rows, [b - a for a, b in zip(offs, offs[1:])])

    def set_class_embeddings(self, rows):
        """class rows formed elsewhere: [C, E], un-normalised (the search normalises them)"""
        if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[0] < 1:
            raise ValueError(f'{WHO}: class embeddings must be [C, E] with C >= 1, got {tuple(getattr(rows, "shape", ()))}')
        if not rows.is_cuda:
            raise ValueError(f'{WHO}: class embeddings are a device tensor (distillclip_amd has no CPU path)')
        self.class_embeddings = rows.detach().float()

    def _classes(self, k):
        if self.class_embeddings is None:
            raise ValueError(f'{WHO}: no classes yet (set_classes() or set_class_embeddings() comes first)')
        C = self.class_embeddings.shape[0]
        if not 1 <= k <= min(C, TOPK_MAX_K):
            raise ValueError(f'{WHO}: k={k} with {C} classes, need 1 <= k <= min(C, {TOPK_MAX_K})')
        return self.class_embeddings

    # ---- the images ----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, images, k=1):
        """images [B, 3, H, W] -> (idx int32 [B, k], score f32 [B, k]): the k best classes of each image, best first, and their cosines"""
        classes = self._classes(int(k))
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError(f'{WHO}: images must be [B, C, H, W] with B >= 1, got {tuple(images.shape)}')
        return topk_search(encode_rows(self.image_encoder, images, self.max_batch), classes, int(k))

    @staticmethod
    def _check_labels(labels, n):
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or labels.shape[0] != n:
            raise ValueError(f'{WHO}: {n} images need {n} labels in a flat vector, got {tuple(labels.shape)}')
        if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
            raise ValueError(f'{WHO}: labels are integer class indices, got {labels.dtype}')
        return labels

    @staticmethod
    def _to_device(labels, dev):
        labels = labels.detach().to(torch.int64)
        return labels.to(dev) if labels.is_cuda else labels.pin_memory().to(dev, non_blocking=True)   # (pageable memory would make the host wait)

    @torch.no_grad()
    def update(self, images, labels):
        """images [B, 3, H, W], labels [B] integer class indices, a device or host tensor (or a list).  Runs the image tower and appends
        its last_representation rows.  A label outside [0, C) cannot be seen without waiting for the device: it simply never hits."""
        if images.dim() != 4 or images.shape[0] < 1:
            raise ValueError(f'{WHO}: images must be [B, C, H, W] with B >= 1, got {tuple(images.shape)}')
        labels = self._check_labels(labels, images.shape[0])
        rows = encode_rows(self.image_encoder, images, self.max_batch)
        self._rows.append(rows)
        self._labels.append(self._to_device(labels, rows.device))

    def add_embeddings(self, image_rows, labels):
        """rows formed elsewhere (another model, rows gathered from other ranks): image_rows [n, E] on the device, labels [n] as in update"""
        if not torch.is_tensor(image_rows) or image_rows.dim() != 2 or image_rows.shape[0] < 1:
            raise ValueError(f'{WHO}: need [n, E] image rows with n >= 1, got {tuple(getattr(image_rows, "shape", ()))}')
        labels = self._check_labels(labels, image_rows.shape[0])
        if not image_rows.is_cuda:
            raise ValueError(f'{WHO}: image rows are a device tensor (distillclip_amd has no CPU path)')
        self._rows.append(image_rows.detach().float())
        self._labels.append(self._to_device(labels, image_rows.device))

    def compute(self):
        """-> {'acc_top{k}'} for k in k_list, 0-dim float64 device tensors: the fraction of stored images whose label is among their k
        best classes.  One concatenation, one kernel call with k = max(k_list), integer hit counts, one division in double each."""
        classes = self._classes(max(self.k_list))
        if not self._rows:
            raise ValueError(f'{WHO}: nothing to classify (no update() or add_embeddings() since the last reset())')
        rows = self._rows[0] if len(self._rows) == 1 else torch.cat(self._rows, dim=0)
        labels = self._labels[0] if len(self._labels) == 1 else torch.cat(self._labels, dim=0)
        idx, _ = topk_search(rows, classes, max(self.k_list), return_scores=False)
        hit = idx.to(torch.int64) == labels[:, None]                # a class occurs once in a row: at most one hit per image
        n = rows.shape[0]
        return {f'acc_top{k}': hit[:, :k].sum().to(torch.float64) / n for k in self.k_list}

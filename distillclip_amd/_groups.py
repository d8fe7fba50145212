"""What the evaluators over an image / text tower pair share (score.LCLIPScore: references per image; metrics.retrieval_recall and
retrieval.RetrievalEvaluator: captions per image): counts -> offsets, dense-or-ragged token sets, the tower pair of a model and the
chunked tower run.  Needs no GPU; every complaint about an argument is a ValueError that starts with the caller's name `who`."""
import torch

# (the model package imports metrics, which imports this module: its classes are imported where they are used)


def group_offsets(counts, n_groups, n_rows, who, noun, rows_name, counts_name='counts'):
    """counts: host list or CPU tensor of n_groups non-negative counts that sum to n_rows (image i owns the next counts[i] rows of
    rows_name) -> the n_groups + 1 offsets as a list"""
    if torch.is_tensor(counts):
        if counts.is_cuda:
            raise ValueError(f'{who}: {counts_name} is a host list or CPU tensor (reading a device tensor would wait for the device)')
        counts = counts.reshape(-1).tolist()
    counts = [int(c) for c in counts]
    if len(counts) != n_groups:
        raise ValueError(f'{who}: {len(counts)} {noun} counts for {n_groups} images')
    if any(c < 0 for c in counts):
        raise ValueError(f'{who}: a {noun} count is negative')
    if sum(counts) != n_rows:
        raise ValueError(f'{who}: the {noun} counts sum to {sum(counts)}, {rows_name} has {n_rows} rows')
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    return offs


def flatten_groups(tokens, counts, B, who, offsets_of, name, counts_name, rows_dim, per_dim):
    """tokens: ragged [rows_dim, L] with counts (B of them, offsets_of(counts, B, rows) checks them), or dense [B, per_dim, L] with
    counts optional -> ([rows, L] tokens, the B + 1 offsets)"""
    if tokens.dim() == 3:
        if tokens.shape[0] != B:
            raise ValueError(f'{who}: dense {name} must be [B, {per_dim}, L] with B={B}, got {tuple(tokens.shape)}')
        dense = [tokens.shape[1]] * B
        offs = offsets_of(dense if counts is None else counts, B, B * tokens.shape[1])
        if [b - a for a, b in zip(offs, offs[1:])] != dense:
            raise ValueError(f'{who}: {counts_name} disagrees with the dense [B, {per_dim}, L] {name}')
        return tokens.reshape(B * tokens.shape[1], tokens.shape[2]), offs
    if tokens.dim() == 2:
        if counts is None:
            raise ValueError(f'{who}: {name} [{rows_dim}, L] need {counts_name}')
        return tokens, offsets_of(counts, B, tokens.shape[0])
    raise ValueError(f'{who}: {name} must be [{rows_dim}, L] or [B, {per_dim}, L], got {tuple(tokens.shape)}')


def tower_pair(model, who):
    """model: a two-tower distillation model (DualDistillModel: its student) or a CLIPModel -> (image_encoder, text_encoder)"""
    from .model.component.clip_model import CLIPModel
    clip = model if isinstance(model, CLIPModel) else getattr(model, 'student', None)
    if not isinstance(clip, CLIPModel):
        raise ValueError(f'{who}.from_model: {type(model).__name__} has no image and text tower pair (a CLIPModel, or a two-tower '
                         f'distillation model whose student is one)')
    return clip.image_encoder, clip.text_encoder


def encode_rows(encoder, x, max_batch):
    """last_representation [rows, E] of x, in chunks of at most max_batch rows"""
    from .model.component.output import ControlOutput
    parts = [encoder(x[s:s + max_batch], ControlOutput()).last_representation for s in range(0, x.shape[0], max_batch)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

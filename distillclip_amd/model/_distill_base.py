"""What DistillModel (one student tower) and DualDistillModel (two) share: the data-parallel backward, the optimizer, the retrieval
metrics of validation and the rules that freeze and unfreeze student parameters.  Each module keeps its own constructor, forward,
training / validation steps and `towers()`, the list of student towers everything here works on."""
from torch import nn

from .component.image_encoder import ImageEncoder
from .component.weight_share_model import RepeatVisionTransformer
from ..optim import FusedAdamW, EpochCosineSchedule
from ..parallel import GradSync
from ..metrics import retrieval_metrics


class _HParams(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


_TEACHER_EMBED_KEYS = ['visual.conv1.weight', 'visual.class_embedding', 'visual.positional_embedding']
_REPEAT_EMBED_KEYS = ['patch_embed.proj.weight', 'cls_token', 'pos_embed']


def freeze_image_embedding(enc, teacher_state, prefix):
    """reference distil_model.py:197-219 / dual_distill_model.py:240-268: the teacher's patch / class / positional embeddings
    (`prefix` + OpenAI key in `teacher_state`) copied into the image student `enc` and frozen.  A plain CLIP student has the teacher's
    keys; a RepeatVisionTransformer takes them as patch_embed / cls_token [1, 1, D] / pos_embed [1, N, D]; the reference does nothing
    for other student classes."""
    if isinstance(enc, ImageEncoder):
        keys = _TEACHER_EMBED_KEYS
    elif isinstance(enc, RepeatVisionTransformer):
        keys = _REPEAT_EMBED_KEYS
    else:
        return
    sw = enc.state_dict()
    for s_k, t_k in zip(keys, _TEACHER_EMBED_KEYS):
        w = teacher_state[prefix + t_k]
        if s_k == 'cls_token':
            w = w.unsqueeze(0).unsqueeze(0)
        elif s_k == 'pos_embed':
            w = w.unsqueeze(0)
        sw[s_k] = w
    enc.load_state_dict(sw)
    for n, p in enc.named_parameters():
        if n in keys:
            p.requires_grad = False


def pair_attention_maps(student, teacher):
    """The attention losses pair student and teacher maps with zip() (attention_score_mse.py, attention_probs_mse.py): tell each tower how
    many maps the other exports, so that neither computes maps zip would drop.  The student still reports its full execution count
    (ExportedMaps.executions), the losses' divisor."""
    cfg = student._tower.cfg
    need = teacher.need_layers
    t_maps = teacher.layers if need is None else len({int(i) for i in need if 0 <= int(i) < teacher.layers})
    student.attn_map_pairs = t_maps
    teacher.attn_map_pairs = cfg.layers * cfg.repeats


class DistillBase(nn.Module):
    # Plain attributes, set on the module before configure_optimizers() / validation (the reference has neither: the defaults are its
    # behaviour).  ema_decay: handed to FusedAdamW, which then keeps an exponential moving average of the student weights inside its
    # step.  validate_with_ema: the validation loop runs on that average (on_validation_start / on_validation_end).
    # optimizer_groups: FusedAdamW's `groups`, a list of {'params', 'weight_decay', 'lr_scale'} dicts or a callable model -> such a list
    # (e.g. distillclip_amd.optim.no_decay_groups); None: one weight decay and one learning rate for every trainable element.
    # trust_ratio, trust_clip, always_adapt: FusedAdamW's arguments of the same names (layer-wise trust ratios, LAMB); trust_ratio None
    # or False: plain AdamW.
    ema_decay = None
    validate_with_ema = False
    optimizer_groups = None
    trust_ratio = None
    trust_clip = None
    always_adapt = False
    _optimizer = None              # the optimizer configure_optimizers() built
    _ema_context = None            # the entered FusedAdamW.ema_weights() of a validation loop

    def towers(self):
        """the student towers (HipTower), in the order the optimizer and the gradient exchange see them"""
        raise NotImplementedError

    def _ensure_sync(self):
        """data-parallel plumbing of the student towers (lazy: torch.distributed may be initialised after __init__)"""
        self._sync = GradSync.current(self._sync).attach(self.towers())
        return self._sync

    def backward_and_sync(self, loss, defer_wait=False):
        """loss.backward() + the data-parallel gradient exchange (reference strategy ddp_find_unused_parameters_false,
        l_clip.yaml:56).  Sharded mode: every gradient bucket is reduce-scattered from inside its tower's backward (per-block
        release, reverse layer order) and FusedAdamW.step() updates the owned shards and all-gathers the parameters; fallback:
        each tower's flat buffer is all-reduced on a side stream right after its backward has been enqueued."""
        sync = self._ensure_sync()
        if loss is not None:                                   # None: the caller already ran loss.backward()
            sync.armed = sync.enabled                          # per-bucket release from inside the towers' backward: only here
            try:
                loss.backward()
            finally:
                sync.armed = False
        if not sync.enabled:
            return
        for tw in self.towers():
            if tw.dp is not None:
                tw.grads_ready = sync.finish(tw)
                tw._grad_clean = True                          # exchanged buckets were cleared behind their reduce-scatter
            else:
                tw.grads_ready = sync.launch(tw.flat_grad, after=tw.bwd_done)
        if not defer_wait:       # defer_wait: FusedAdamW.step waits per tower on `grads_ready` / runs on the exchange stream
            sync.wait()
        else:
            sync.forget()

    def configure_optimizers(self):
        # reference distil_model.py:160-169, dual_distill_model.py:194-202: AdamW over every requires_grad parameter (one group)
        # + cosine schedule stepped per epoch
        towers = self.towers()
        dev = next(self.student.parameters()).device
        for tw in towers:
            tw.materialize(dev)
        extras = [p for tw in towers                             # a plain CLIP student's projection linears (tw.module: its encoder)
                  for p in getattr(tw.module, 'extra_parameters', lambda: [])()]
        groups = self.optimizer_groups(self) if callable(self.optimizer_groups) else self.optimizer_groups
        opt = FusedAdamW(towers, lr=self.hparams.lr, weight_decay=self.hparams.weight_decay, extra_params=extras, ema_decay=self.ema_decay,
                         groups=groups, trust_ratio=bool(self.trust_ratio), trust_clip=self.trust_clip, always_adapt=self.always_adapt)
        self._optimizer = opt
        sched = EpochCosineSchedule(opt, self.hparams.warm_steps, self.hparams.total_steps)
        self._ensure_sync()          # data-parallel run: shard plan over the same trainable set the optimizer was built with
        return [opt], [sched]

    def on_validation_start(self):
        """validate_with_ema and an average exists (FusedAdamW.ema_decay): the student towers hold the averaged weights until
        on_validation_end.  Otherwise nothing happens and validation scores the last iterate, as the reference does."""
        opt = self._optimizer
        if self.validate_with_ema and opt is not None and opt._has_ema() and self._ema_context is None:
            self._ema_context = opt.ema_weights()
            self._ema_context.__enter__()

    def on_validation_end(self):
        ctx, self._ema_context = self._ema_context, None
        if ctx is not None:
            ctx.__exit__(None, None, None)

    def configure_gradient_clipping(self, optimizer, *args, gradient_clip_val=None, gradient_clip_algorithm=None, **kw):
        """Lightning's hook for the trainer keys gradient_clip_val / gradient_clip_algorithm: called before every optimizer step as
        (optimizer, gradient_clip_val, gradient_clip_algorithm), by older releases as (optimizer, optimizer_idx, gradient_clip_val,
        gradient_clip_algorithm).  The clipping itself runs inside FusedAdamW.step(), on the gradients the optimizer really reads
        (under the built-in exchange the averaged gradient shards, which p.grad never shows): this only hands over the threshold."""
        args = list(args)
        if len(args) >= 3 or (len(args) == 2 and isinstance(args[0], int) and not isinstance(args[1], (str, type(None)))):
            args = args[1:]                                        # (optimizer_idx first)
        if args:
            gradient_clip_val = args[0]
        if len(args) > 1:
            gradient_clip_algorithm = args[1]
        algorithm = getattr(gradient_clip_algorithm, 'value', gradient_clip_algorithm)       # (Lightning's GradClipAlgorithmType enum)
        if algorithm not in (None, 'norm'):
            raise ValueError(f'configure_gradient_clipping: FusedAdamW clips the global L2 norm only, not by {algorithm!r}')
        optimizer.max_grad_norm = float(gradient_clip_val) if gradient_clip_val else None

    def unfreeze_embed(self):
        for _, p in self.student.named_parameters():
            p.requires_grad = True

    def _acc(self, log, rows, cols, section, prefix, acc=True, score=False):
        # reference distil_model.py norm_and_logits :224-231 builds stu_logits = stu_encode @ encode.T : rows = this tower, cols = the other
        m = retrieval_metrics(rows, cols, self.k_list)
        if acc:                        # reference log_acc: distil_model.py:187-191, dual_distill_model.py:220-224
            for k in self.k_list:
                log[f'{section}/{prefix}_acc_top{k}'] = m[f'acc_top{k}']
        if score:                      # reference log_diag_score: distil_model.py:171-179, dual_distill_model.py:204-212
            log[f'{section}/{prefix}_softmax_mean_score'] = m['softmax_mean_score']
            log[f'{section}/{prefix}_mean_score'] = m['mean_score']

"""DistillModel (reference model/distil_model.py:19-221): one-tower distillation.

The reference class is a pytorch_lightning.LightningModule; Lightning is not installed here, so the same constructor,
`forward`, `training_step`, `configure_optimizers`, `freeze_image_embedding` are provided on a plain nn.Module (the
methods Lightning would call; those DualDistillModel shares come from _distill_base.py).  `validation_step` / `validation_epoch_end` return the scalars the reference logs, computed
by the HIP retrieval kernel (distillclip_amd/metrics.py) instead of torchmetrics; wandb / heat-map logging is not mirrored.
"""
from typing import Dict, List

import torch

from ._distill_base import DistillBase, _HParams, freeze_image_embedding, pair_attention_maps
from ._loss import LossCalculator
from .utils import teacher_load
from .component._tower import shared_image_patches
from ..metrics import gather_rows


class DistillModel(DistillBase):
    def __init__(self, student_encoder: torch.nn.Module, loss_control_para: Dict, download_root: str,
                 teacher_name: str = 'ViT-B/32', freeze_embed: bool = False, teacher_need_layers: List = None,
                 model_type: str = 'image', warm_steps=10, total_steps=200, weight_decay=1e-3, lr: float = 1e-3,
                 norm: bool = False, unfreeze_epoch=None, teacher_state_dict=None):
        super().__init__()
        if model_type not in ['text', 'image']:
            raise ValueError(f"the model_type should in ['text', 'image'], bug got {model_type}")     # reference :44-45
        self.hparams = _HParams(loss_control_para=loss_control_para, download_root=download_root, teacher_name=teacher_name,
                                freeze_embed=freeze_embed, teacher_need_layers=teacher_need_layers, model_type=model_type,
                                warm_steps=warm_steps, total_steps=total_steps, weight_decay=weight_decay, lr=lr, norm=norm,
                                unfreeze_epoch=unfreeze_epoch)
        self.student = student_encoder
        self.teacher_name = teacher_name
        self.teacher = teacher_load(teacher_name, download_root, model_type, need_layers=teacher_need_layers,
                                    state_dict=teacher_state_dict)
        self.loss_control = LossCalculator(**loss_control_para)
        self.need_return_para = self.loss_control.get_control_output()
        for p in self.teacher.parameters():
            p.requires_grad = False                                                       # reference :59-60
        pair_attention_maps(self.student, self.teacher)
        if model_type == 'image' and freeze_embed:
            self.freeze_image_embedding()
        self.k_list = [1, 3, 5, 10, 20, 50]
        self.current_epoch = 0
        self._sync = None

    def forward(self, inputs):
        # reference :81-89
        # (image.yaml: teacher and student unfold the same images — one im2row for both when they cut them the same way; no-op for text)
        with shared_image_patches(inputs, [getattr(self.student, '_tower', None), getattr(self.teacher, '_tower', None)]):
            student_outs = self.student(inputs, self.need_return_para)
            with torch.no_grad():
                teacher_outs = self.teacher(inputs, self.need_return_para)
        if self.hparams.norm:
            # reference :86-88 (in place there; same values here, autograd-safe)
            for o in (student_outs, teacher_outs):
                o.last_representation = o.last_representation / o.last_representation.norm(dim=-1, keepdim=True)
        return student_outs, teacher_outs

    def training_step(self, inputs, batch_idx=0):
        # reference :97-102 (logging left to the caller: cal_res holds every scalar self.log would receive)
        self.teacher.eval()
        student_outs, teacher_outs = self.forward(inputs)
        loss, cal_res = self.loss_control(student_outs, teacher_outs, self.hparams.model_type)
        self.last_cal_res = cal_res
        return loss

    def towers(self):
        return [self.student._tower]

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        """reference :104-126.  batch = (imgs, texts, _) where the modality that is not distilled arrives as a
        pre-computed [B, E] teacher representation (`contrary_rep`)."""
        imgs, texts = batch[0], batch[1]
        inputs, contrary_rep = (texts, imgs) if self.hparams.model_type == 'text' else (imgs, texts)
        student_outs, teacher_outs = self.forward(inputs)
        loss, cal_res = self.loss_control(student_outs, teacher_outs, self.hparams.model_type)
        log = {'val_loss/loss': loss.detach()}
        log.update({f'val_loss/{k}': v for k, v in cal_res.items()})
        s, t = student_outs.last_representation, teacher_outs.last_representation
        self._acc(log, s, contrary_rep, 'val_step', 'stu', score=True)
        self._acc(log, t, contrary_rep, 'val_step', 'tea')
        return {'student': gather_rows(s), 'teacher': gather_rows(t), 'contrary_rep': gather_rows(contrary_rep)}, log

    @torch.no_grad()
    def validation_epoch_end(self, outputs):
        """reference :131-152"""
        cat = {k: torch.cat([o[k].reshape(-1, o[k].shape[-1]) for o in outputs], dim=0).float()
               for k in ('student', 'teacher', 'contrary_rep')}
        log = {}
        self._acc(log, cat['student'], cat['contrary_rep'], 'val_stu_acc', 'stu')
        self._acc(log, cat['student'], cat['contrary_rep'], 'val_stu_score', 'stu', acc=False, score=True)
        if self.current_epoch == 0:
            self._acc(log, cat['teacher'], cat['contrary_rep'], 'val_tea_score', 'tea', acc=False, score=True)
            self._acc(log, cat['teacher'], cat['contrary_rep'], 'val_tea_acc', 'tea')
        return log

    def on_train_epoch_start(self):
        if self.hparams.unfreeze_epoch and self.current_epoch >= self.hparams.unfreeze_epoch:
            self.unfreeze_embed()
            self.hparams.unfreeze_epoch = False

    def freeze_image_embedding(self):
        freeze_image_embedding(self.student, self.teacher.state_dict(), '')                   # reference :197-219

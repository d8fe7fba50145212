"""Added cost of the attention_score_mse / attention_probs_mse terms at the l_clip shapes (B = 512 by default): one two-tower step of
the shipped students under the ViT-B/32 teachers (need_layers [0, 1, 10, 11]) timed with the terms off and on, alternating.

    python tools/diag/attn_maps_cost.py [--batch 512] [--steps 10]

Prints one JSON line: median ms per step for each setting and the difference.  Per-kernel times: run it under
`rocprofv3 --kernel-trace --stats -- python tools/diag/attn_maps_cost.py` (attn_maps_* kernels)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np   # noqa: E402
import torch         # noqa: E402

from distillclip_amd import synth                                                        # noqa: E402
from distillclip_amd.model._loss import LossCalculator                                  # noqa: E402
from distillclip_amd.model._distill_base import pair_attention_maps                     # noqa: E402
from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer, ImageEncoder, TextEncoder  # noqa: E402
from distillclip_amd.model.component.output import CLIPOutput                           # noqa: E402


def T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--steps', type=int, default=10)
    a = ap.parse_args()
    seed, B = 5, a.batch
    s_img_cfg = dict(img_size=224, patch_size=32, in_chans=3, out_dim=512, embed_dim=768, depth=6, num_heads=24, mlp_ratio=4.0,
                     qkv_bias=True, repeated_times=2, use_transform=True)
    s_txt_cfg = dict(depth=4, repeated_times=2, use_transform=True)
    si, st = RepeatVisionTransformer(**s_img_cfg), RepeatTextTransformer(**s_txt_cfg)
    si.load_state_dict(T(synth.student_image_state(seed, **s_img_cfg)))
    st.load_state_dict(T(synth.student_text_state(seed, **s_txt_cfg)))
    nl = [0, 1, 10, 11]
    ti = ImageEncoder(False, dict(input_resolution=224, patch_size=32, width=768, layers=12, heads=12, output_dim=512, need_layers=nl))
    ti.load_state_dict(T(synth.teacher_image_state(seed)))
    tt = TextEncoder(512, 12, 8, 77, nl, 49408, 512, is_student=False)
    tt.load_state_dict(T(synth.teacher_text_state(seed)))
    si, st, ti, tt = si.cuda(), st.cuda(), ti.cuda(), tt.cuda()
    for p in list(ti.parameters()) + list(tt.parameters()):
        p.requires_grad = False
    pair_attention_maps(si, ti)
    pair_attention_maps(st, tt)
    image = torch.from_numpy(synth.images(seed, B, 224)).cuda()
    text = torch.from_numpy(synth.captions(seed, B)).cuda()
    base = ['out_l1', 'out_cos']
    calcs = {'off': LossCalculator(base), 'on': LossCalculator(base + ['attention_score_mse', 'attention_probs_mse'])}

    def step(lc):
        co = lc.get_control_output()
        so = CLIPOutput(visual_output=si(image, co), text_output=st(text, co))
        with torch.no_grad():
            to = CLIPOutput(visual_output=ti(image, co), text_output=tt(text, co))
        loss, _ = lc(so, to, 'all')
        loss.backward()

    times = {k: [] for k in calcs}
    for k in calcs:
        step(calcs[k])                                 # warm-up
    torch.cuda.synchronize()
    for _ in range(a.steps):
        for k, lc in calcs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(lc)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({'batch': B, 'steps': a.steps, 'ms_off': round(med['off'], 3), 'ms_on': round(med['on'], 3),
                      'added_ms': round(med['on'] - med['off'], 3)}))


if __name__ == '__main__':
    main()

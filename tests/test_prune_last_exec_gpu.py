"""The last block execution of a tower runs its out_proj / LN2 / MLP (and their backward) on the class / EOT rows only
(encoder.cpp, DCLIP_PRUNE_LAST).  Every tower kind is run in two child processes, pruned (the default) and DCLIP_PRUNE_LAST=0, on
the same seeded weights and inputs, and compared:
  last_representation    rel-L2 <= 1e-5 (the same kernels on fewer rows)
  parameter gradients    rel-L2 <= 1e-3 (the wgrads of the last block sum the same rows in another order)
  last_layer_output()    called between a training forward and its backward: rel-L2 <= 1e-5, and the gradients of that step equal
                         those of the same step without the call
A pruned forward refuses a gradient for the hidden state of its last execution."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, sys
import numpy as np
import torch
from distillclip_amd import synth
from distillclip_amd.model.component import (RepeatVisionTransformer, RepeatTextTransformer, ImageEncoder, TextEncoder)

out_path, B = sys.argv[1], int(sys.argv[2])
seed, res, patch, ctx, vocab, E = 11, 32, 8, 13, 97, 64
T = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
s_img_kw = dict(img_size=res, patch_size=patch, in_chans=3, out_dim=E, embed_dim=128, depth=4, num_heads=4, mlp_ratio=4.0, qkv_bias=True,
                repeated_times=2, use_transform=True)
s_txt_kw = dict(vocab_size=vocab, context_length=ctx, out_dim=E, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, qkv_bias=False,
                repeated_times=2, use_transform=True)
s_img = RepeatVisionTransformer(**s_img_kw); s_img.load_state_dict(T(synth.student_image_state(seed, **s_img_kw)))
s_txt = RepeatTextTransformer(**s_txt_kw); s_txt.load_state_dict(T(synth.student_text_state(seed, **s_txt_kw)))
t_img = ImageEncoder(False, dict(input_resolution=res, patch_size=patch, width=128, layers=2, heads=2, output_dim=E, need_layers=None))
t_img.load_state_dict(T(synth.teacher_image_state(seed, 128, 2, patch, res, E)))
t_txt = TextEncoder(128, 2, 2, ctx, None, vocab, E, is_student=False)
t_txt.load_state_dict(T(synth.teacher_text_state(seed, 128, 2, ctx, vocab, E)))
c_sd_i, c_sd_t = synth.clip_student_states(seed, 64, 2, patch, res, ctx, vocab, E, 64, 64)
c_img = ImageEncoder(True, dict(input_resolution=res, patch_size=patch, width=64, layers=2, heads=2, output_dim=E), 64)
c_img.load_state_dict(T(c_sd_i))
c_txt = TextEncoder(64, 2, 2, ctx, None, vocab, E, tea_transformer_width=64, is_student=True)
c_txt.load_state_dict(T(c_sd_t))
mods = {k: m.cuda() for k, m in dict(s_img=s_img, s_txt=s_txt, t_img=t_img, t_txt=t_txt, c_img=c_img, c_txt=c_txt).items()}

image = torch.from_numpy(synth.images(seed, B, res)).cuda()
text = torch.from_numpy(synth.captions(seed, B, ctx, vocab, 3, ctx - 2)).cuda()
eot = text.argmax(dim=1)
res_ = {}
info = {'eot': [int(v) for v in eot.tolist()]}


def grads(m):
    return {n: p.grad.detach().float().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}


for tag, m in mods.items():
    x = image if 'img' in tag else text
    if tag.startswith('t_'):
        with torch.no_grad():
            o = m(x)
            res_[f'{tag}.rep'] = o.last_representation.float().cpu().numpy()
            res_[f'{tag}.llo'] = m.last_layer_output().float().cpu().numpy()
        if tag == 't_txt':                     # the causal teacher on the caption prefix that holds every EOT
            k = int(eot.max().item()) + 1
            with torch.no_grad():
                r = m._tower.forward(x, training=False, tokens_eff=k)
            res_[f'{tag}.rep_prefix'] = r[0].float().cpu().numpy()
        continue
    g = torch.from_numpy(synth.normal(seed, tag, (B, E))).cuda()
    m.train()
    for with_llo in (False, True):
        m.zero_grad(set_to_none=True)
        o = m(x)
        if with_llo:
            res_[f'{tag}.llo'] = m.last_layer_output().float().cpu().numpy()
        (o.last_representation * g).sum().backward()
        torch.cuda.synchronize()
        for n, v in grads(m).items():
            res_[f'{tag}.{"llo_" if with_llo else ""}grad.{n}'] = v
    res_[f'{tag}.rep'] = o.last_representation.detach().float().cpu().numpy()

# a pruned forward keeps no hidden state of its last execution: a gradient for it is refused
tw = mods['s_img']._tower
nex = tw.cfg.layers * tw.cfg.repeats
r = tw.forward(image, training=True)
d_reps = [None] * (nex - 1) + [torch.zeros((B, tw.cfg.tokens, tw.cfg.width), device='cuda')]
try:
    tw.backward(r[1], torch.zeros((B, E), device='cuda'), d_reps=d_reps)
    info['d_rep_last'] = 'accepted'
except ValueError as e:
    info['d_rep_last'] = str(e)
torch.cuda.synchronize()
np.savez(out_path, **res_)
json.dump(info, open(out_path + '.json', 'w'))
'''


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _run(tmp_path, B, prune):
    script = tmp_path / 'worker.py'
    script.write_text(WORKER)
    out = str(tmp_path / f'out_{B}_{prune}.npz')
    env = dict(os.environ, DCLIP_PRUNE_LAST=prune, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, str(script), out, str(B)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return dict(np.load(out)), json.load(open(out + '.json'))


@pytest.mark.parametrize('B', [1, 5])
def test_pruned_last_execution_matches_full(tmp_path, B):
    full, info_full = _run(tmp_path, B, '0')
    pruned, info = _run(tmp_path, B, '1')
    if B > 1:
        assert len(set(info['eot'])) > 1, info['eot']          # the EOT rows differ between the captions of the batch
    assert set(full) == set(pruned)
    for k in sorted(full):
        tol = 1e-3 if '.grad.' in k else 1e-5
        assert rel_l2(pruned[k], full[k]) <= tol, (k, rel_l2(pruned[k], full[k]))
    # last_layer_output between the forward and its backward leaves that backward's gradients as they were
    for k in sorted(pruned):
        if '.llo_grad.' in k:
            base = k.replace('.llo_grad.', '.grad.')
            assert rel_l2(pruned[k], pruned[base]) <= 1e-5, (k, rel_l2(pruned[k], pruned[base]))
    # and its picked rows are last_representation
    np.testing.assert_allclose(pruned['t_txt.rep_prefix'], pruned['t_txt.rep'], rtol=0, atol=1e-5 * np.abs(pruned['t_txt.rep']).max())
    assert 'class / EOT' in info['d_rep_last'], info['d_rep_last']
    assert info_full['d_rep_last'] == 'accepted', info_full['d_rep_last']

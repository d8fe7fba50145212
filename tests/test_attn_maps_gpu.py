"""Head-mean attention maps on the MI355X: the kernels against a float64 restatement built from the same operands, the towers' exported
maps against the reference's per-head maps (tiny.npz), training steps with attention_score_mse / attention_probs_mse against the
reference's own runs (attn_maps.npz: tools/golden/gen_golden.py attn_maps), a step with unread maps against a map-free one, determinism.

Kernel tolerances follow from the arithmetic, not from measurement.  S = scale sum_d q_d k_d over hd f32 products of exact bf16 operands:
|dS| <= (hd + 2) u scale sum_d |q_d k_d| with u = 2^-24.  The mixed scores add H terms: |dA| <= |Wl| |dS| + (H + 1) u |Wl| |S|.  A
softmax row moves by at most 2 max_j |dA_j| relative (shift of the exponent) plus the rounding of exp / sum / division (2^-18 relative
for the v_exp_f32 based __expf, N-term sums).  The backward's dA = P (g - r) inherits the error of P through both factors; the result
then rounds once to bf16 (2^-9 relative).  Every bound below is those terms, times 2 for the orders left out."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from distillclip_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def T(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def rel_l2(a, b):
    a, b = a.detach().float().cpu().reshape(-1), torch.as_tensor(b).float().reshape(-1)
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 64), (4, 32), (8, 64), (12, 64), (12, 32), (24, 32), (16, 64), (32, 32)]


def _operands(B, H, N, hd, wl, seed):
    """packed bf16 qkv rows (ld = 3D + 8, so rows are not tightly packed) whose scores carry per-(b, h, row) offsets up to ~300 with
    opposite signs on alternate heads (one q / k dimension carries them, as in test_softmax_edges_gpu.py), and a random conv_l"""
    g = torch.Generator().manual_seed(seed)
    D = H * hd
    ld = 3 * D + 8
    scale = hd ** -0.5
    qkv = torch.randn(B * N, ld, generator=g) * 0.7
    off = torch.tensor([0., 30., 100., 300.])[torch.randint(0, 4, (B, H, N), generator=g)]
    off = off * torch.where(torch.arange(H) % 2 == 0, 1., -1.).view(1, H, 1)
    q = qkv[:, :D].view(B, N, H, hd)
    k = qkv[:, D:2 * D].view(B, N, H, hd)
    q[..., 0] = (off.permute(0, 2, 1) / scale) / 64.0          # + k[..., 0] = 64 adds `off` to every key of a row
    k[..., 0] = 64.0
    qkv = qkv.bfloat16()
    W = (torch.randn(H, H, generator=g) * 0.5) if wl else None
    return qkv, ld, W, scale


def _reference(qkv, ld, W, B, H, N, hd, scale, causal):
    D = H * hd
    x = qkv.double()
    q = x[:, :D].reshape(B, N, H, hd).permute(0, 2, 1, 3)
    k = x[:, D:2 * D].reshape(B, N, H, hd).permute(0, 2, 1, 3)
    S = (scale * q @ k.transpose(-1, -2)).detach().requires_grad_(True)
    Sabs = scale * q.abs() @ k.abs().transpose(-1, -2)
    mask = torch.triu(torch.ones(N, N, dtype=torch.bool), 1) if causal else torch.zeros(N, N, dtype=torch.bool)
    Wd = None if W is None else W.double().requires_grad_(True)
    A = S if Wd is None else torch.einsum('gh,bhij->bgij', Wd, S)
    P = torch.softmax(A.masked_fill(mask, float('-inf')), dim=-1)
    score = torch.where(mask, torch.zeros_like(S), S).mean(1)
    prob = P.mean(1)
    eS = (hd + 2) * U * Sabs
    eA = eS if W is None else torch.einsum('gh,bhij->bgij', W.double().abs(), eS + (H + 1) * U * S.detach().abs())
    eA = eA.masked_fill(mask, 0.)
    eP = P.detach() * (2 * eA.amax(-1, keepdim=True) + 2 ** -18)
    return dict(S=S, W=Wd, mask=mask, P=P, score=score, prob=prob, eS=eS, eP=eP,
                e_score=2 * (eS.masked_fill(mask, 0.).mean(1) + H * U * S.detach().abs().mean(1)), e_prob=2 * (eP.mean(1) + 2 ** -22))


def _launch_fwd(qkv, ld, W, B, H, N, hd, scale, causal):
    from distillclip_amd._lib import lib
    st = torch.cuda.current_stream().cuda_stream
    q = qkv.cuda()
    w = None if W is None else W.float().cuda().contiguous()
    sc = torch.full((B, N, N), float('nan'), device='cuda')
    pr = torch.full((B, N, N), float('nan'), device='cuda')
    lib().dclip_attn_maps_fwd(q.data_ptr(), ld, None if w is None else w.data_ptr(), sc.data_ptr(), pr.data_ptr(), B, H, N, hd, scale,
                              int(causal), st)
    torch.cuda.synchronize()
    return sc.cpu().double(), pr.cpu().double()


def _cases():
    out = []
    for H, hd in SHAPES:
        for N in (13, 17, 50, 77, 101, 128):
            for causal in (0, 1):
                for wl in (0, 1):
                    if wl and H > 24:
                        continue                               # head-mixing towers: H in {2, 4, 8, 12, 24}
                    out.append((H, hd, N, causal, wl))
    return out


@pytest.mark.parametrize('H,hd,N,causal,wl', _cases())
def test_maps_kernels_vs_float64(H, hd, N, causal, wl):
    from distillclip_amd._lib import lib
    B = 2
    qkv, ld, W, scale = _operands(B, H, N, hd, wl, seed=H * 1000 + N * 10 + causal * 2 + wl)
    ref = _reference(qkv, ld, W, B, H, N, hd, scale, causal)
    sc, pr = _launch_fwd(qkv, ld, W, B, H, N, hd, scale, causal)
    assert torch.isfinite(sc).all() and torch.isfinite(pr).all()
    assert ((sc - ref['score'].detach()).abs() <= ref['e_score']).all(), (sc - ref['score']).abs().max().item()
    assert ((pr - ref['prob'].detach()).abs() <= ref['e_prob']).all(), (pr - ref['prob']).abs().max().item()
    # backward: both dS layouts, dW_l
    g = torch.Generator().manual_seed(7 + N)
    gS, gP = torch.randn(B, N, N, generator=g), torch.randn(B, N, N, generator=g)
    (ref['score'] * gS.double()).sum().add((ref['prob'] * gP.double()).sum()).backward()
    inc = ref['S'].grad.masked_fill(ref['mask'], 0.)
    P = ref['P'].detach()
    gPh = (gP.double() / H).masked_fill(ref['mask'], 0.).unsqueeze(1)
    r = (P * gPh).sum(-1, keepdim=True)
    eP = ref['eP']
    e_dA = eP * (gPh.abs() + r.abs()) + P * (eP * gPh.abs()).sum(-1, keepdim=True)
    e_inc = e_dA if W is None else torch.einsum('gh,bgij->bhij', W.double().abs(), e_dA)
    e_inc = 2 * (e_inc + 2 ** -9 * inc.abs() + 1e-30)
    Np = (N + 7) // 8 * 8
    st = torch.cuda.current_stream().cuda_stream
    ws_bytes = lib().dclip_attn_maps_bwd_workspace_bytes(B, H, N)
    q, dgS, dgP = qkv.cuda(), gS.cuda(), gP.cuda()          # device copies held for the asynchronous launches
    w = None if W is None else W.float().cuda().contiguous()
    for blocked in (0, 1):
        dS = torch.zeros(B, H, N, Np, dtype=torch.bfloat16, device='cuda')
        dW = torch.zeros(H, H, device='cuda')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
        lib().dclip_attn_maps_bwd(q.data_ptr(), ld, None if w is None else w.data_ptr(), dgS.data_ptr(), dgP.data_ptr(),
                                  dS.data_ptr(), blocked, dW.data_ptr(), ws.data_ptr(), ws_bytes, B, H, N, Np, hd, scale, int(causal), st)
        torch.cuda.synchronize()
        got = dS.float().cpu().double()
        if blocked:         # [B, H, Np / 4, N, 4] -> [B, H, N, Np]
            got = got.reshape(B, H, Np // 4, N, 4).permute(0, 1, 3, 2, 4).reshape(B, H, N, Np)
        assert (got[..., N:] == 0).all()
        err = (got[..., :N] - inc).abs()
        assert (err <= e_inc).all(), (blocked, err.max().item(), (err - e_inc).max().item())
        if W is not None:
            dA = (P * (gPh - r)).masked_fill(ref['mask'], 0.)
            Sa = ref['S'].detach().abs()
            e_dw = 2 * (torch.einsum('bgij,bhij->gh', e_dA, Sa) + torch.einsum('bgij,bhij->gh', dA.abs() + e_dA, ref['eS'])
                        + B * N * N * U * torch.einsum('bgij,bhij->gh', dA.abs(), Sa))
            assert ((dW.cpu().double() - ref['W'].grad).abs() <= e_dw).all(), (dW.cpu().double() - ref['W'].grad).abs().max().item()


def test_maps_backward_is_deterministic():
    from distillclip_amd._lib import lib
    B, H, N, hd = 64, 24, 50, 32
    qkv, ld, W, scale = _operands(B, H, N, hd, True, seed=3)
    Np = 56
    gS, gP = torch.randn(B, N, N, device='cuda'), torch.randn(B, N, N, device='cuda')
    q, w = qkv.cuda(), W.float().cuda().contiguous()
    ws_bytes = lib().dclip_attn_maps_bwd_workspace_bytes(B, H, N)
    outs = []
    for _ in range(2):
        dS = torch.zeros(B, H, N, Np, dtype=torch.bfloat16, device='cuda')
        dW = torch.zeros(H, H, device='cuda')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
        lib().dclip_attn_maps_bwd(q.data_ptr(), ld, w.data_ptr(), gS.data_ptr(), gP.data_ptr(), dS.data_ptr(), 1, dW.data_ptr(),
                                  ws.data_ptr(), ws_bytes, B, H, N, Np, hd, scale, 0, torch.cuda.current_stream().cuda_stream)
        outs.append((dS.clone(), dW.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 2. tower forward vs the reference's per-head maps ----------------------------------------------------------------------------
TINY = dict(
    seed=11, B=3, res=32, patch=8, ctx=13, vocab=97, out_dim=64,
    s_img=dict(img_size=32, patch_size=8, in_chans=3, out_dim=64, embed_dim=128, depth=4, num_heads=4,
               mlp_ratio=4.0, qkv_bias=True, repeated_times=2, use_transform=True),
    s_txt=dict(vocab_size=97, context_length=13, out_dim=64, embed_dim=128, depth=2, num_heads=2,
               mlp_ratio=4.0, qkv_bias=False, repeated_times=2, use_transform=True),
)
S_IMG = dict(img_size=224, patch_size=32, in_chans=3, out_dim=512, embed_dim=768, depth=6, num_heads=24, mlp_ratio=4.0,
             qkv_bias=True, repeated_times=2, use_transform=True)
S_TXT = dict(depth=4, repeated_times=2, use_transform=True)
def _tiny_modules():
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer, ImageEncoder, TextEncoder
    c = TINY
    s_img = RepeatVisionTransformer(**c['s_img'])
    s_img.load_state_dict(T(synth.student_image_state(c['seed'], **c['s_img'])))
    s_txt = RepeatTextTransformer(**c['s_txt'])
    s_txt.load_state_dict(T(synth.student_text_state(c['seed'], **c['s_txt'])))
    t_img = ImageEncoder(False, dict(input_resolution=c['res'], patch_size=c['patch'], width=128, layers=2, heads=2,
                                     output_dim=c['out_dim'], need_layers=None))
    t_img.load_state_dict(T(synth.teacher_image_state(c['seed'], 128, 2, c['patch'], c['res'], c['out_dim'])))
    t_txt = TextEncoder(128, 2, 2, c['ctx'], None, c['vocab'], c['out_dim'], is_student=False)
    t_txt.load_state_dict(T(synth.teacher_text_state(c['seed'], 128, 2, c['ctx'], c['vocab'], c['out_dim'])))
    return s_img.cuda(), s_txt.cuda(), t_img.cuda(), t_txt.cuda()


def test_tower_maps_are_the_head_mean_of_the_reference_maps(golden_dir):
    """every block execution of the four tiny towers, standalone (no pairing limit): mean over heads of tiny.npz's per-head maps (the
    text teacher's masked scores already read 0 there, reference text_encoder.py:81-85).  bf16 activations through the tower: the
    embedding bound of test_towers_gpu.py"""
    from distillclip_amd.model.component.output import ControlOutput
    tiny = dict(np.load(os.path.join(golden_dir, 'tiny.npz')))
    s_img, s_txt, t_img, t_txt = _tiny_modules()
    image, text = torch.from_numpy(tiny['image']).cuda(), torch.from_numpy(tiny['text']).cuda()
    co = ControlOutput(need_attn_score=True, need_attn_prob=True)
    with torch.no_grad():
        outs = {'s_img': s_img(image, co), 's_txt': s_txt(text, co), 't_img': t_img(image, co), 't_txt': t_txt(text, co)}
    for tag, o in outs.items():
        n = sum(1 for k in tiny if k.startswith(tag + '.scores'))
        assert n > 0 and len(o.attention_scores) == n and len(o.attention_probs) == n, (tag, n, len(o.attention_scores))
        for i in range(n):
            for kind, got in (('scores', o.attention_scores[i]), ('probs', o.attention_probs[i])):
                ref = tiny[f'{tag}.{kind}{i}'].mean(axis=1, keepdims=True)
                assert tuple(got.shape) == ref.shape
                assert rel_l2(got, ref) <= 2e-2, (tag, kind, i, rel_l2(got, ref))


# ---- 3. training steps vs the reference --------------------------------------------------------------------------------------------
def _teachers(seed, width, layers, patch, res, ctx, vocab, out_dim, need_layers=None, text_width=None):
    """CLIP teachers with 64-wide heads (the reference's width // 64); the text tower may be narrower (ViT-B/32: 768 / 512)"""
    from distillclip_amd.model.component import ImageEncoder, TextEncoder
    tw = text_width or width
    ti = ImageEncoder(False, dict(input_resolution=res, patch_size=patch, width=width, layers=layers, heads=width // 64, output_dim=out_dim,
                                  need_layers=need_layers))
    ti.load_state_dict(T(synth.teacher_image_state(seed, width, layers, patch, res, out_dim)))
    tt = TextEncoder(tw, layers, tw // 64, ctx, need_layers, vocab, out_dim, is_student=False)
    tt.load_state_dict(T(synth.teacher_text_state(seed, tw, layers, ctx, vocab, out_dim)))
    for p in list(ti.parameters()) + list(tt.parameters()):
        p.requires_grad = False
    return ti.cuda(), tt.cuda()


def _students(seed, img_cfg, txt_cfg):
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    si, st = RepeatVisionTransformer(**img_cfg), RepeatTextTransformer(**txt_cfg)
    si.load_state_dict(T(synth.student_image_state(seed, **img_cfg)))
    st.load_state_dict(T(synth.student_text_state(seed, **txt_cfg)))
    return si.cuda(), st.cuda()


def _case(tag):
    """-> (names, model type, student(s), teacher(s), inputs) of attn_maps.npz case `tag`"""
    from distillclip_amd.model.component import ImageEncoder, TextEncoder
    c = TINY
    seed, B = c['seed'], c['B']
    both = ['out_l1', 'out_cos', 'attention_score_mse', 'attention_probs_mse']
    one = ['out_cos', 'attention_score_mse', 'attention_probs_mse']
    image = torch.from_numpy(synth.images(seed, B, c['res'])).cuda()
    text = torch.from_numpy(synth.captions(seed, B, c['ctx'], c['vocab'], 3, 9)).cuda()
    tiny_t = lambda nl=None: _teachers(seed, 128, 2, c['patch'], c['res'], c['ctx'], c['vocab'], c['out_dim'], nl)
    if tag == 'a':
        return both, 'all', _students(seed, c['s_img'], c['s_txt']), tiny_t(), (image, text)
    if tag == 'b':
        return one, 'image', _students(seed, c['s_img'], c['s_txt'])[0], tiny_t([0, 1])[0], (image,)
    if tag == 'c':
        return one, 'text', _students(seed, c['s_img'], c['s_txt'])[1], tiny_t()[1], (text,)
    if tag == 'd':
        ds = 31
        image = torch.from_numpy(synth.images(ds, B, c['res'])).cuda()
        text = torch.from_numpy(synth.captions(ds, B, c['ctx'], c['vocab'], 3, 9)).cuda()
        ti, tt = _teachers(ds, 192, 2, c['patch'], c['res'], c['ctx'], c['vocab'], c['out_dim'])
        paras = dict(input_resolution=c['res'], patch_size=c['patch'], width=128, layers=2, heads=2, output_dim=c['out_dim'], need_layers=None)
        si = ImageEncoder(True, paras, tea_transformer_width=192)
        st = TextEncoder(128, 2, 2, c['ctx'], None, c['vocab'], c['out_dim'], tea_transformer_width=192, is_student=True)
        sd_i, sd_t = synth.clip_student_states(ds + 1, 128, 2, c['patch'], c['res'], c['ctx'], c['vocab'], c['out_dim'], 192, 192)
        si.load_state_dict(T(sd_i))
        st.load_state_dict(T(sd_t))
        return both, 'all', (si.cuda(), st.cuda()), (ti, tt), (image, text)
    es, eB = 2027, 4
    image = torch.from_numpy(synth.images(es, eB, 224)).cuda()
    text = torch.from_numpy(synth.captions(es, eB)).cuda()
    return both, 'all', _students(es, S_IMG, S_TXT), _teachers(es, 768, 12, 32, 224, 77, 49408, 512, [0, 1, 10, 11], 512), (image, text)


def _step(names, model_type, student, teacher, inputs):
    from distillclip_amd.model._loss import LossCalculator
    from distillclip_amd.model._distill_base import pair_attention_maps
    from distillclip_amd.model.component.output import CLIPOutput
    lc = LossCalculator(names)
    co = lc.get_control_output()
    if model_type == 'all':
        (si, st), (ti, tt), (image, text) = student, teacher, inputs
        pair_attention_maps(si, ti)
        pair_attention_maps(st, tt)
        so = CLIPOutput(visual_output=si(image, co), text_output=st(text, co))
        with torch.no_grad():
            to = CLIPOutput(visual_output=ti(image, co), text_output=tt(text, co))
    else:
        pair_attention_maps(student, teacher)
        so = student(inputs[0], co)
        with torch.no_grad():
            to = teacher(inputs[0], co)
    loss, res = lc(so, to, model_type)
    loss.backward()
    torch.cuda.synchronize()
    return loss, res


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e'])
def test_training_step_parity_vs_reference_golden(golden_dir, tag):
    g = dict(np.load(os.path.join(golden_dir, 'attn_maps.npz')))
    names, model_type, student, teacher, inputs = _case(tag)
    loss, res = _step(names, model_type, student, teacher, inputs)
    errs = {'loss': abs(loss.item() - float(g[f'{tag}.loss'])) / abs(float(g[f'{tag}.loss']))}
    for k, v in res.items():
        errs[k] = abs(float(v) - float(g[f'{tag}.term.{k}'])) / (abs(float(g[f'{tag}.term.{k}'])) + 1e-12)
    assert set(res) == {k[len(tag) + 6:] for k in g if k.startswith(f'{tag}.term.')}
    print(tag, errs)
    bad = {k: e for k, e in errs.items() if e > (5e-2 if 'attention' in k else 2e-2)}
    assert not bad, bad
    # gradients: the bounds of test_towers_gpu.py (out_l1 in the objective: its L1_TOL)
    tol = 2e-1 if 'out_l1' in names else 8e-2
    mods = [('s_img', student[0]), ('s_txt', student[1])] if model_type == 'all' else [('s', student)]
    # the golden keeps, per tower, every gradient's norm and 128 evenly spread elements (gnames / gnorm / gspread)
    worst = {}
    for mt, m in mods:
        params = dict(m.named_parameters())
        names_ = [str(n) for n in g[f'{tag}.{mt}.gnames']]
        for n, p in params.items():            # a gradient the reference does not have must be absent or zero
            assert n in names_ or p.grad is None or p.grad.abs().max().item() == 0, (mt, n)
        for k, n in enumerate(names_):
            assert params[n].grad is not None, (mt, n)
            gr = params[n].grad.reshape(-1)
            sm = gr[::max(1, gr.numel() // 128)][:128]
            ref_norm = float(g[f'{tag}.{mt}.gnorm'][k])
            if ref_norm == 0:
                assert gr.abs().max().item() == 0, n
                continue
            worst[mt + '.' + n] = max(abs(gr.norm().item() - ref_norm) / ref_norm, rel_l2(sm, g[f'{tag}.{mt}.gspread'][k][:sm.numel()]))
    assert len(worst) > 10
    print(tag, 'worst gradient', max(worst.items(), key=lambda kv: kv[1]))
    bad = {n: e for n, e in worst.items() if e > (2e-1 if ('conv_' in n or 'bias' in n or 'norm' in n or 'ln_' in n) else tol)}
    assert not bad, bad


@pytest.mark.skipif(os.environ.get('DCLIP_ATTN_MIX') == '0', reason='this is the child run')
def test_training_step_parity_on_the_unfused_score_stage():
    """the same five cases with DCLIP_ATTN_MIX=0 (latched once per process: a child): the maps backward then adds into the row-major dS"""
    env = dict(os.environ, DCLIP_ATTN_MIX='0')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', os.path.abspath(__file__),
                        '-k', 'test_training_step_parity_vs_reference_golden'],
                       capture_output=True, text=True, timeout=1200, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert '5 passed' in r.stdout, r.stdout[-2000:]


# ---- 4. no regression ---------------------------------------------------------------------------------------------------------------
def test_map_plumbing_leaves_a_map_free_step_unchanged(monkeypatch):
    """terms off: a tiny dual step is bit-identical whether the towers export no maps or export maps of executions 0 and 1 that no loss
    term reads (their gradients reach the backward as zeros), with the image towers on their own input and on shared patch rows"""
    from distillclip_amd.model._loss import LossCalculator
    from distillclip_amd.model.component._tower import HipTower, TowerResult, shared_image_patches
    from distillclip_amd.model.component.output import CLIPOutput

    def run(share):
        (si, st), (ti, tt) = _students(11, TINY['s_img'], TINY['s_txt']), _teachers(11, 128, 2, 8, 32, 13, 97, 64)
        image = torch.from_numpy(synth.images(11, 3, 32)).cuda()
        text = torch.from_numpy(synth.captions(11, 3, 13, 97, 3, 9)).cuda()
        lc = LossCalculator(['out_cos', 'hidden_rep_mse'])
        co = lc.get_control_output()
        with shared_image_patches(image, [si._tower, ti._tower] if share else []):
            vo = si(image, co)
            with torch.no_grad():
                tvo = ti(image, co)
        so = CLIPOutput(visual_output=vo, text_output=st(text, co))
        with torch.no_grad():
            to = CLIPOutput(visual_output=tvo, text_output=tt(text, co))
        loss, _ = lc(so, to, 'all')
        loss.backward()
        torch.cuda.synchronize()
        return [loss.detach().clone(), so.visual_output.last_representation.detach().clone(), to.text_output.last_representation.clone()] + \
            [m._tower.flat_grad.clone() for m in (si, st)]

    plain = {share: run(share) for share in (False, True)}
    again = run(False)
    fwd, bwd, calls = HipTower.forward, HipTower.backward, []

    def fwd_exporting(self, x, training, *a, tokens_eff=0, maps=None, **kw):
        assert maps is None and not tokens_eff
        res = fwd(self, x, training, *a, tokens_eff=tokens_eff, maps=(True, True, [0, 1]), **kw)
        assert len(res.scores) == len(res.probs) == 2
        calls.append(training)
        return TowerResult(*res, [], [])

    def bwd_with_zero_map_grads(self, x, d_out, *a, d_maps=None, **kw):
        assert d_maps is None
        z = [torch.zeros((x.shape[0], 1, self.cfg.tokens, self.cfg.tokens), device=x.device) for _ in range(2)]
        return bwd(self, x, d_out, *a, d_maps=([0, 1], z, z), **kw)

    monkeypatch.setattr(HipTower, 'forward', fwd_exporting)
    monkeypatch.setattr(HipTower, 'backward', bwd_with_zero_map_grads)
    mapped = {share: run(share) for share in (False, True)}
    assert calls.count(True) == 4 and calls.count(False) == 4         # both students trained, both teachers ran, in each run
    # loss and outputs: bit-identical.  Gradients: several step kernels (token-table scatter, LayerNorm and bias column sums) accumulate
    # with f32 atomics, so two plain runs already differ in the order of those additions; the bound is that of f32 reordering
    for share in (False, True):
        for k, (a, a2, b) in enumerate(zip(plain[share], again, mapped[share])):
            if k < 3:
                assert torch.equal(a, b) and torch.equal(plain[False][k], a2), (share, k)
            else:
                assert rel_l2(b, a.cpu()) <= 1e-5 and rel_l2(a2, plain[False][k].cpu()) <= 1e-5, (share, k)


# ---- 5. determinism at the l_clip shapes ---------------------------------------------------------------------------------------------
def test_lclip_b512_steps_with_map_terms_are_deterministic():
    from distillclip_amd.model._loss import LossCalculator
    from distillclip_amd.model._distill_base import pair_attention_maps
    from distillclip_amd.model.component.output import CLIPOutput
    seed, B = 5, 512
    si, st = _students(seed, S_IMG, S_TXT)
    ti, tt = _teachers(seed, 768, 12, 32, 224, 77, 49408, 512, [0, 1, 10, 11], 512)
    pair_attention_maps(si, ti)
    pair_attention_maps(st, tt)
    image = torch.from_numpy(synth.images(seed, B, 224)).cuda()
    text = torch.from_numpy(synth.captions(seed, B)).cuda()
    lc = LossCalculator(['out_l1', 'out_cos', 'attention_score_mse', 'attention_probs_mse'])
    co = lc.get_control_output()
    grads = []
    for _ in range(2):
        for m in (si, st):
            for p in m.parameters():
                p.grad = None
        so = CLIPOutput(visual_output=si(image, co), text_output=st(text, co))
        with torch.no_grad():
            to = CLIPOutput(visual_output=ti(image, co), text_output=tt(text, co))
        assert len(so.visual_output.attention_scores) == 4 and so.visual_output.attention_scores.executions == 6
        loss, res = lc(so, to, 'all')
        loss.backward()
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        grads.append([loss.detach().clone()] + [m.detach().clone() for o in (so.visual_output, so.text_output)
                                                 for m in list(o.attention_scores) + list(o.attention_probs)]
                     + [m._tower.flat_grad.clone() for m in (si, st)])
    # the loss and every exported map are bit-identical (the map kernels use no atomics; dclip_attn_maps_bwd is checked bit for bit by
    # test_maps_backward_is_deterministic); the step's wgrad colsums / LayerNorm / token-table gradients accumulate with f32 atomics,
    # so whole-tower gradients agree to f32 accumulation order
    n_exact = len(grads[0]) - 2                      # loss + maps; then the two towers' flat gradients
    for k, (a, b) in enumerate(zip(*grads)):
        if k < n_exact:
            assert torch.equal(a, b), k
        else:
            assert torch.isfinite(a).all() and rel_l2(b, a.cpu()) <= 1e-5

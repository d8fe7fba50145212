"""L-CLIPScore scoring on the GPU: the dclip_clipscore kernel element by element against the float64 restatement of its three formulas
(Hessel et al. 2021), its edge rows, row ownership and determinism, and the LCLIPScore scorer end to end on the tiny students.

    cos(a, b)  = a.b / (|a| |b|), 0 when either norm is 0
    clip_s     = w max(cos(image, candidate), 0)
    ref_s      = max(0, max over the image's references of cos(candidate, reference)), 0 for an empty set
    refclip_s  = 2 clip_s ref_s / (clip_s + ref_s), 0 when the denominator is 0

Error bound (derived, not measured): the inputs are f32, hence exact in float64.  With u = 2^-24 each of the three length-E sums (a.b,
a.a, b.b) is off by at most E u relative to |a| |b| in any summation order, so |cos - cos64| <= (2 E + 8) u, the 8 u covering the two
reciprocal square roots and the final products.  Per element: ref_s (2 E + 8) u; clip_s max(w, 1) (2 E + 8) u; refclip_s
2 (bound_clip + bound_ref) + 8 u max(w, 1), both partial derivatives of the harmonic mean being at most 2."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W = 2.5


def bounds(E, w=W):
    """-> (bound of clip_s, of ref_s, of refclip_s)"""
    bc = (2 * E + 8) * U
    b_clip, b_ref = max(w, 1.0) * bc, bc
    return b_clip, b_ref, 2 * (b_clip + b_ref) + 8 * U * max(w, 1.0)


def cos64(a, b):
    """all-pairs cosine [rows of a, rows of b] in float64, 0 where a norm is 0"""
    a, b = a.double(), b.double()
    na, nb = a.norm(dim=1), b.norm(dim=1)
    den = na[:, None] * nb[None, :]
    return torch.where(den > 0, (a @ b.t()) / den.clamp_min(1e-300), torch.zeros_like(den))


def scores64(img, cand, refs, counts, K, w=W):
    """the three formulas in float64 on CPU tensors -> (clip_s, ref_s, refclip_s), [B K] each (the last two None without references)"""
    img, cand = img.cpu(), cand.cpu()
    B = img.shape[0]
    owner = torch.arange(B).repeat_interleave(K)
    clip = w * cos64(cand, img).gather(1, owner[:, None])[:, 0].clamp_min(0)
    if refs is None:
        return clip, None, None
    ref_owner = torch.arange(B).repeat_interleave(torch.tensor(counts))
    sim = cos64(cand, refs.cpu()) if refs.shape[0] else torch.zeros(B * K, 0, dtype=torch.float64)
    sim = torch.where(owner[:, None] == ref_owner[None, :], sim, torch.full_like(sim, -1.0))
    ref = torch.cat([sim, torch.zeros(B * K, 1, dtype=torch.float64)], dim=1).max(dim=1).values
    den = clip + ref
    return clip, ref, torch.where(den > 0, 2 * clip * ref / den.clamp_min(1e-300), torch.zeros_like(den))


def offsets(counts):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).cuda()


def padded(x, pad):
    """x on the GPU as a view of rows of stride E + pad whose pad columns hold NaN: a read past E poisons the score"""
    if not pad:
        return x.cuda()
    buf = torch.full((x.shape[0], x.shape[1] + pad), float('nan'), device='cuda')
    buf[:, :x.shape[1]] = x.cuda()
    return buf[:, :x.shape[1]]


def check(got, want, E, w=W, what=''):
    for name, g, t, bound in zip(('clip_s', 'ref_s', 'refclip_s'), got, want, bounds(E, w)):
        if t is None:
            assert g is None, name
            continue
        g = g.detach().cpu().double().reshape(-1)
        assert torch.isfinite(g).all(), (what, name)
        err = (g - t).abs().max().item()
        assert err <= bound, (what, name, err, bound, int((g - t).abs().argmax()))


def make_case(B, K, E, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, E, generator=g) * torch.rand(B, 1, generator=g).add(0.5)
    sign = torch.where(torch.rand(B * K, 1, generator=g) < 0.25, -1.0, 1.0)          # some candidates point away: clip_s clamps at 0
    cand = sign * (0.6 * img.repeat_interleave(K, 0) + torch.randn(B * K, E, generator=g)) * 3.0
    counts = [7] if B == 1 else [(0, 1, 7, 3, 2)[b % 5] for b in range(B)]          # 0, 1 and 7 references within one call
    R = sum(counts)
    owner = torch.arange(B).repeat_interleave(torch.tensor(counts))
    pick = owner * K + torch.randint(0, K, (R,), generator=g)                       # every reference resembles a candidate of its image
    refs = (0.7 * cand[pick] * torch.where(torch.rand(R, 1, generator=g) < 0.2, -1.0, 1.0) + torch.randn(R, E, generator=g)) * 0.25
    return img, cand, refs, counts


# ---- 1. the kernel against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 5])
@pytest.mark.parametrize('B', [1, 3, 70])
@pytest.mark.parametrize('E', [4, 64, 260, 512, 1024])
def test_kernel_matches_float64(E, B, K):
    from distillclip_amd import ops
    img, cand, refs, counts = make_case(B, K, E, 1000 * E + 10 * B + K)
    want = scores64(img, cand, refs, counts, K)
    for pad in (0, 4, 12):                                    # contiguous rows, and row strides larger than E
        d_img, d_cand, d_refs = padded(img, pad), padded(cand, 2 * pad), padded(refs, pad)
        got = ops.clipscore(d_img, d_cand, d_refs, offsets(counts), K=K, w=W)
        check(got, want, E, what=f'pad {pad}')
        got = ops.clipscore(d_img, d_cand, K=K, w=W)          # the no-references call
        assert got[1] is None and got[2] is None
        check(got, (want[0], None, None), E, what=f'pad {pad}, no references')
    if B == 70:
        assert want[0].max() > 0.5 and want[0].min() == 0 and want[1].max() > 0.2 and want[1].min() == 0     # both sides of both clamps occur


def test_other_weights():
    from distillclip_amd import ops
    img, cand, refs, counts = make_case(7, 3, 128, 5)
    for w in (1.0, 0.5, 4.0):
        got = ops.clipscore(img.cuda(), cand.cuda(), refs.cuda(), offsets(counts), K=3, w=w)
        check(got, scores64(img, cand, refs, counts, 3, w), 128, w, what=f'w {w}')


# ---- 2. edge rows ------------------------------------------------------------------------------------------------------------------
def test_edge_rows():
    from distillclip_amd import ops
    E, K = 64, 1
    g = torch.Generator().manual_seed(21)
    rnd = lambda *s: torch.randn(*s, generator=g)
    img, cand = rnd(10, E), rnd(10, E)
    ZIMG, ZCAND, ZREF, NEG, TRIPLE, SAME, NOREF, PLAIN, SMALL, LARGE = range(10)
    refs, counts = [], []

    def add(b, rows):
        assert len(counts) == b
        refs.append(rows)
        counts.append(rows.shape[0])
    img[ZIMG] = 0
    add(ZIMG, rnd(2, E))
    cand[ZCAND] = 0
    add(ZCAND, rnd(2, E))
    add(ZREF, torch.zeros(1, E))
    cand[NEG] = -img[NEG]
    add(NEG, rnd(1, E))
    cand[TRIPLE] = 3 * img[TRIPLE]
    add(TRIPLE, rnd(1, E))
    same = rnd(3, E)
    same[1] = cand[SAME]
    add(SAME, same)
    add(NOREF, torch.zeros(0, E))
    plain_refs = 0.5 * cand[PLAIN] + rnd(3, E)
    cand[PLAIN] = 0.5 * img[PLAIN] + cand[PLAIN]
    add(PLAIN, plain_refs)
    for b, s in ((SMALL, 1e-3), (LARGE, 1e3)):
        img[b], cand[b] = img[PLAIN] * s, cand[PLAIN] * s
        add(b, plain_refs * s)
    refs = torch.cat(refs)
    clip, ref, rc = (t.cpu().double() for t in ops.clipscore(img.cuda(), cand.cuda(), refs.cuda(), offsets(counts), K=K, w=W))
    want = scores64(img, cand, refs, counts, K)
    b_clip, b_ref, b_rc = bounds(E)
    for got in (clip, ref, rc):
        assert torch.isfinite(got).all()                      # no NaN anywhere
    check((clip, ref, rc), want, E, what='edge rows')
    assert clip[ZIMG] == 0 and rc[ZIMG] == 0                  # a zero image row
    assert clip[ZCAND] == 0 and ref[ZCAND] == 0 and rc[ZCAND] == 0
    assert ref[ZREF] == 0 and rc[ZREF] == 0                   # a zero reference, alone in its set
    assert clip[NEG] == 0 and rc[NEG] == 0                    # candidate = -image
    assert abs(clip[TRIPLE] - W) <= b_clip                    # candidate = 3 image
    assert abs(ref[SAME] - 1.0) <= b_ref                      # candidate equal to one of its references
    assert ref[NOREF] == 0 and rc[NOREF] == 0                 # no references
    assert want[0][PLAIN] > 0.5 and want[1][PLAIN] > 0.2
    for b in (SMALL, LARGE):                                  # scaled rows score as the unscaled rows do
        assert abs(clip[b] - want[0][PLAIN]) <= b_clip and abs(ref[b] - want[1][PLAIN]) <= b_ref and abs(rc[b] - want[2][PLAIN]) <= b_rc


# ---- 3. ownership ------------------------------------------------------------------------------------------------------------------
def test_every_output_belongs_to_its_row_and_its_image_references():
    """image b lives in coordinates [16 b, 16 b + 16): its candidate k has cosine t[b, k] to it, all different, and is orthogonal to
    everything of another image; image b's references are copies of its candidates 0..b"""
    from distillclip_amd import ops
    B, K, E = 4, 5, 64
    t = (1 + torch.arange(B * K, dtype=torch.float64).reshape(B, K)) / (B * K + 1)
    img, cand = torch.zeros(B, E, dtype=torch.float64), torch.zeros(B, K, E, dtype=torch.float64)
    for b in range(B):
        img[b, 16 * b] = 1.0 + b
        for k in range(K):
            cand[b, k, 16 * b] = t[b, k] * (2.0 + k)
            cand[b, k, 16 * b + 1 + k] = (1 - t[b, k] ** 2).sqrt() * (2.0 + k)
    img, cand = img.float(), cand.float().reshape(B * K, E)
    counts = [b + 1 for b in range(B)]
    refs = torch.cat([cand[b * K:b * K + b + 1] for b in range(B)])
    clip, ref, rc = (x.cpu().double().reshape(B, K) for x in ops.clipscore(img.cuda(), cand.cuda(), refs.cuda(), offsets(counts), K=K, w=W))
    check((clip, ref, rc), scores64(img, cand, refs, counts, K), E, what='ownership')
    assert (clip / W - t).abs().max() < 1e-5                   # neighbouring cosines are 1 / 21 apart: [b, k] carries row b K + k
    for b in range(B):
        for k in range(K):
            if k <= b:
                assert ref[b, k] > 0.9999, (b, k)              # its own copy is among image b's references, and only there
            else:
                want = max(t[b, k] * t[b, j] for j in range(b + 1))
                assert abs(ref[b, k] - want) < 1e-5 and ref[b, k] < 0.95, (b, k)


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def test_same_call_same_bits_and_outputs_fully_overwritten():
    from distillclip_amd._lib import lib
    B, K, E = 33, 5, 260
    img, cand, refs, counts = make_case(B, K, E, 77)
    d_img, d_cand, d_refs, off = img.cuda(), cand.cuda(), refs.cuda(), offsets(counts)
    st = torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        outs = torch.full((3, B * K), float('nan'), device='cuda')
        lib().dclip_clipscore(d_img.data_ptr(), E, d_cand.data_ptr(), E, d_refs.data_ptr(), E, off.data_ptr(), B, K, refs.shape[0], E, W,
                              outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), st)
        assert torch.isfinite(outs).all()
        runs.append(outs)
    assert torch.equal(runs[0], runs[1])
    check(tuple(runs[0]), scores64(img, cand, refs, counts, K), E, what='raw call')
    only = torch.full((B * K,), float('nan'), device='cuda')                       # clip_s alone, references given
    lib().dclip_clipscore(d_img.data_ptr(), E, d_cand.data_ptr(), E, d_refs.data_ptr(), E, off.data_ptr(), B, K, refs.shape[0], E, W,
                          only.data_ptr(), None, None, st)
    assert torch.equal(only, runs[0][0])


# ---- 5. / 6. the scorer ------------------------------------------------------------------------------------------------------------
S_IMG = dict(img_size=32, patch_size=8, in_chans=3, out_dim=64, embed_dim=128, depth=4, num_heads=4, mlp_ratio=4.0, qkv_bias=True,
             repeated_times=2, use_transform=True)
S_TXT = dict(vocab_size=97, context_length=13, out_dim=64, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, qkv_bias=False,
             repeated_times=2, use_transform=True)
T = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
SB, SK, SCOUNTS = 5, 3, [0, 2, 1, 4, 1]


def _students(seed):
    from distillclip_amd import synth
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    s_img, s_txt = RepeatVisionTransformer(**S_IMG), RepeatTextTransformer(**S_TXT)
    s_img.load_state_dict(T(synth.student_image_state(seed, **S_IMG)))
    s_txt.load_state_dict(T(synth.student_text_state(seed, **S_TXT)))
    return s_img, s_txt


def _inputs(seed=40):
    from distillclip_amd import synth
    images = torch.from_numpy(synth.images(seed, SB, 32)).cuda()
    cand = torch.from_numpy(synth.captions(seed, SB * SK, 13, 97, 3, 9)).reshape(SB, SK, 13).cuda()
    refs = torch.from_numpy(synth.captions(seed + 1, sum(SCOUNTS), 13, 97, 3, 9)).cuda()
    return images, cand, refs


def test_scorer_end_to_end():
    from distillclip_amd import LCLIPScore, ScoreOutput, ops
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _students(3)
    clip = CLIPModel(True, s_img, s_txt).cuda()
    images, cand, refs = _inputs()
    modules = list(clip.modules())
    before = {n: p.detach().clone() for n, p in clip.named_parameters()}
    flags = [(p.requires_grad) for p in clip.parameters()], [m.training for m in modules]
    assert all(flags[0]) and all(flags[1])
    scorer = LCLIPScore.from_model(clip)
    assert torch.is_grad_enabled()
    out = scorer(images, cand, refs, SCOUNTS)                                  # called with grad enabled
    assert isinstance(out, ScoreOutput)
    for x in out:
        assert x.shape == (SB, SK) and x.dtype == torch.float32 and not x.requires_grad and x.grad_fn is None
    # the float64 formulas on embeddings from encode_image / encode_text
    text = torch.cat([cand.reshape(SB * SK, 13), refs])
    with torch.no_grad():
        e_img = clip.encode_image(images).last_representation
        e_txt = clip.encode_text(text).last_representation
    E = e_img.shape[1]
    check(out, scores64(e_img, e_txt[:SB * SK], e_txt[SB * SK:], SCOUNTS, SK), E, what='scorer')
    assert out.clip_s.max() > 0 and out.ref_s[0].abs().max() == 0 and out.refclip_s[0].abs().max() == 0      # image 0 has no references
    # candidates [B, L]: one score per image
    one = scorer(images, cand[:, 1].contiguous())
    assert one.clip_s.shape == (SB,) and one.ref_s is None and one.refclip_s is None
    with torch.no_grad():
        e_one = clip.encode_text(cand[:, 1].contiguous()).last_representation
    check(one, scores64(e_img, e_one, None, None, 1), E, what='scorer, one candidate')
    # max_batch = 2: the same bits as scoring the embeddings of those chunks
    small = LCLIPScore.from_model(clip, max_batch=2)(images, cand, refs, SCOUNTS)
    with torch.no_grad():
        c_img = torch.cat([clip.encode_image(images[s:s + 2]).last_representation for s in range(0, SB, 2)])
        c_txt = torch.cat([clip.encode_text(text[s:s + 2]).last_representation for s in range(0, text.shape[0], 2)])
    want = ops.clipscore(c_img, c_txt[:SB * SK], c_txt[SB * SK:], offsets(SCOUNTS), K=SK, w=W)
    for g, t in zip(small, want):
        assert torch.equal(g.reshape(-1), t)
    # the dense [B, Rper, L] form = the ragged form with equal counts
    dense_refs = torch.cat([refs, refs[:2]]).reshape(SB, 2, 13)
    dense = scorer(images, cand, dense_refs)
    ragged = scorer(images, cand, dense_refs.reshape(SB * 2, 13), [2] * SB)
    also = scorer(images, cand, dense_refs.reshape(SB * 2, 13), torch.tensor([2] * SB))
    for a, b, c in zip(dense, ragged, also):
        assert torch.equal(a, b) and torch.equal(a, c)
    # nothing of the towers changed
    for n, p in clip.named_parameters():
        assert torch.equal(p.detach(), before[n]) and p.grad is None, n
    assert [p.requires_grad for p in clip.parameters()] == flags[0] and [m.training for m in modules] == flags[1]


def test_scores_survive_a_checkpoint_round_trip(tmp_path):
    from distillclip_amd import LCLIPScore, synth
    from distillclip_amd.checkpoint import save_checkpoint, load_checkpoint
    from distillclip_amd.model import DualDistillModel

    def dual(seed):
        s_img, s_txt = _students(seed)
        tsd = synth.teacher_image_state(7, 128, 2, 8, 32, 64)
        tsd.update(synth.teacher_text_state(7, 128, 2, 13, 97, 64))
        return DualDistillModel(s_img, s_txt, dict(loss_name=['out_cos']), warm_steps=2, total_steps=10, weight_decay=1e-2, lr=1e-3,
                                download_root='.', teacher_state_dict=T(tsd)).cuda()
    images, cand, refs = _inputs(50)
    m = dual(3)
    want = LCLIPScore.from_model(m)(images, cand, refs, SCOUNTS)
    path = os.path.join(tmp_path, 'scorer.ckpt')
    save_checkpoint(path, m)
    m2 = dual(99)                                              # other weights: the scores must come from the file
    other = LCLIPScore.from_model(m2)(images, cand, refs, SCOUNTS)
    assert not torch.equal(other.clip_s, want.clip_s)
    load_checkpoint(path, m2)
    got = LCLIPScore.from_model(m2)(images, cand, refs, SCOUNTS)
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    assert want.clip_s.max() > 0

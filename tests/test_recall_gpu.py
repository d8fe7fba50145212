"""Recall@K with several captions per image on the GPU (dclip_retrieval_recall, metrics.retrieval_recall, RetrievalEvaluator): the ranks
of both directions as intervals against float64, exact on planted ranks, under ties, permutations and edge tables, the buffers' guards,
determinism, and the evaluator end to end on the tiny students.  Cases, the error bound b(E) = (2 E + 8) 2^-24 and the float64 reference
live in tests/recall_cases.py; tests/test_recall_cpu.py checks the reference itself."""
import ctypes

import numpy as np
import pytest
import torch

import recall_cases as rc

pytestmark = pytest.mark.gpu

KS = (1, 5, 10)


def run(img, txt, counts, ks=KS):
    """-> out [2 nk + 2] f32, rank_i2t, rank_t2i as numpy arrays"""
    from distillclip_amd.metrics import retrieval_recall
    res = retrieval_recall(img.cuda(), txt.cuda(), counts, ks, return_ranks=True)
    out = [res[f'{d}_recall@{k}'] for d in ('i2t', 't2i') for k in ks] + [res['i2t_mean_rank'], res['t2i_mean_rank']]
    assert all(o.dim() == 0 and o.is_cuda and o.dtype == torch.float32 for o in out)
    assert len({o.untyped_storage().data_ptr() for o in out}) == 1           # views of one result vector
    return torch.stack(out).cpu().numpy(), res['i2t_ranks'].cpu().numpy(), res['t2i_ranks'].cpu().numpy()


def check_out(out, rank_i, rank_t, ks=KS):
    """out is exactly float32(float64(integer) / denominator) of the returned ranks"""
    want = rc.expected_out(rank_i, rank_t, ks)
    assert out.dtype == np.float32 and np.array_equal(out, want), (out, want)


# ---- 1. against float64, as intervals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', rc.SEEDS)
@pytest.mark.parametrize('n_img,E', rc.SHAPES)
def test_ranks_lie_in_the_float64_intervals(n_img, E, seed):
    img, txt, counts, iv = rc.reference(n_img, E, seed)
    lo_i, hi_i, lo_t, hi_t = iv
    frac, ranked = rc.undecided_fraction(iv)
    assert frac <= rc.UNDECIDED_CAP, (frac, ranked)                          # a condition on the case, not a measurement
    out, rank_i, rank_t = run(img, txt, counts)
    print(f'({n_img}, {E}) seed {seed}: {round(frac * ranked)} of {ranked} rows undecided; i2t off lo {int((rank_i - lo_i).max())}, '
          f't2i off lo {int((rank_t - lo_t).max())}')
    bad_i = np.nonzero((rank_i < lo_i) | (rank_i > hi_i))[0]
    bad_t = np.nonzero((rank_t < lo_t) | (rank_t > hi_t))[0]
    assert bad_i.size == 0, (bad_i[:8], rank_i[bad_i[:8]], lo_i[bad_i[:8]], hi_i[bad_i[:8]])
    assert bad_t.size == 0, (bad_t[:8], rank_t[bad_t[:8]], lo_t[bad_t[:8]], hi_t[bad_t[:8]])
    check_out(out, rank_i, rank_t)


# ---- 2. planted ranks, exact ---------------------------------------------------------------------------------------------------------
def test_planted_ranks_are_exact():
    img, txt, counts, want_i, want_t = rc.planted_case()
    ks = (1, 5, 10, 1000)
    out, rank_i, rank_t = run(img, txt, counts, ks)
    assert np.array_equal(rank_t, want_t), np.nonzero(rank_t != want_t)[0][:8]
    assert np.array_equal(rank_i, want_i), np.nonzero(rank_i != want_i)[0][:8]
    check_out(out, rank_i, rank_t, ks)
    assert out[3] == 1.0 and out[7] == 1.0                                   # a cut-off above n: every ranked row hits
    assert 0 < out[0] < out[1] <= out[2] <= 1 and 0 < out[4] < out[5] < out[6] < 1


# ---- 3. ties favour the target -------------------------------------------------------------------------------------------------------
def test_ties_favour_the_target():
    """Bit copies of every caption under a new last image: the copy of an image's best own caption ties with its target and must not
    count, while the copy of a caption that was ahead of the target is ahead of it again, so every rank_i2t of the original images
    doubles exactly (and a rank 0 stays 0); one counted tie would give 2 r + 1.  Likewise a bit copy of every image, without
    captions, doubles every rank_t2i: the copy of the owner ties."""
    img, txt, counts, _ = rc.reference(33, 64, 1)
    n_img, n_txt = img.shape[0], txt.shape[0]
    _, rank_i, rank_t = run(img, txt, counts)
    assert (rank_i == 0).any() and (rank_i > 0).any() and (rank_t == 0).any() and (rank_t > 0).any()
    extra = torch.randn(1, 64, generator=torch.Generator().manual_seed(9))
    _, ri, rt = run(torch.cat([img, extra]), torch.cat([txt, txt]), counts + [n_txt])
    assert np.array_equal(ri[:n_img], np.where(rank_i >= 0, 2 * rank_i, -1))
    assert np.array_equal(ri[:n_img][rank_i == 0], rank_i[rank_i == 0])
    _, ri, rt = run(torch.cat([img, img]), txt, counts + [0] * n_img)
    assert np.array_equal(rt, 2 * rank_t) and np.array_equal(rt[rank_t == 0], rank_t[rank_t == 0])
    assert np.array_equal(ri[:n_img], rank_i) and (ri[n_img:] == -1).all()


# ---- 4. position independence --------------------------------------------------------------------------------------------------------
def test_permuting_the_images_permutes_the_ranks():
    img, txt, counts, _ = rc.reference(130, 64, 0)
    offs = np.concatenate([[0], np.cumsum(counts)])
    _, rank_i, rank_t = run(img, txt, counts)
    perm = np.random.RandomState(3).permutation(len(counts))
    cap_perm = np.concatenate([np.arange(offs[p], offs[p + 1]) for p in perm]).astype(np.int64)
    _, ri, rt = run(img[torch.from_numpy(perm)], txt[torch.from_numpy(cap_perm)], [counts[p] for p in perm])
    assert np.array_equal(ri, rank_i[perm]) and np.array_equal(rt, rank_t[cap_perm])
    assert rank_t.max() > 100 and rank_i.max() > 100


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------
def test_edges():
    from distillclip_amd.metrics import retrieval_recall
    g = torch.Generator().manual_seed(4)
    E = 64
    b = rc.bound(E)

    def check(img, txt, counts, ks=KS):
        out, rank_i, rank_t = run(img, txt, counts, ks)
        lo_i, hi_i, lo_t, hi_t = rc.intervals(rc.cos64(img, txt), counts, b)
        assert ((lo_i <= rank_i) & (rank_i <= hi_i)).all() and ((lo_t <= rank_t) & (rank_t <= hi_t)).all()
        assert np.isfinite(out).all()
        check_out(out, rank_i, rank_t, ks)
        return out, rank_i, rank_t
    # one caption in all
    img = torch.randn(3, E, generator=g)
    out, rank_i, rank_t = check(img, 0.5 * img[1:2] + 0.1 * torch.randn(1, E, generator=g), [0, 1, 0])
    assert rank_i.tolist() == [-1, 0, -1] and rank_t.tolist() == [0] and out.tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    # every caption under one image: no caption competes for it, and the other images leave the denominators
    img = torch.randn(5, E, generator=g)
    txt = torch.randn(37, E, generator=g)
    out, rank_i, rank_t = check(img, txt, [0, 0, 37, 0, 0])
    assert rank_i.tolist() == [-1, -1, 0, -1, -1] and out[0] == 1.0 and 0 <= rank_t.min() and rank_t.max() <= 4 and rank_t.max() > 0
    # empty groups in between
    img, txt, counts, _ = rc.reference(17, 64, 0)
    out, rank_i, rank_t = check(img, txt, counts)
    assert ((rank_i == -1) == (np.asarray(counts) == 0)).all() and (rank_i == -1).sum() == 3
    # a zero image row and a zero caption row: every cosine with them is 0, nothing is NaN
    img, txt = img.clone(), txt.clone()
    img[2] = 0
    txt[7] = 0
    out, rank_i, rank_t = check(img, txt, counts)
    assert rank_i[2] == 0                                                    # all its logits are 0: ties, none ahead
    # no cut-offs: the two mean ranks alone
    res = retrieval_recall(img.cuda(), txt.cuda(), counts, (), return_ranks=True)
    assert set(res) == {'i2t_mean_rank', 't2i_mean_rank', 'i2t_ranks', 't2i_ranks'}
    assert np.array_equal(np.array([res['i2t_mean_rank'].item(), res['t2i_mean_rank'].item()], dtype=np.float32), out[-2:])
    assert np.array_equal(res['i2t_ranks'].cpu().numpy(), rank_i)
    # counts on the device would wait for it: refused
    with pytest.raises(ValueError, match='host list'):
        retrieval_recall(img.cuda(), txt.cuda(), torch.tensor(counts).cuda())


# ---- 6. guards -----------------------------------------------------------------------------------------------------------------------
PAD = 64


class Raw:
    """a raw call of the C entry on buffers surrounded by sentinels"""

    def __init__(self, img, txt, nk=3):
        self.n_img, self.n_txt, self.E, self.nk = img.shape[0], txt.shape[0], img.shape[1], nk
        # the rows sit inside larger buffers whose neighbouring rows are huge copies of image 0: a caption read outside [0, n_txt) would
        # be the best caption of whoever reads it
        wall = lambda n: (1e3 * img[0:1]).repeat(n, 1)
        self.img_buf = torch.cat([wall(16), img, wall(16)]).cuda()
        self.txt_buf = torch.cat([wall(16), txt, wall(16)]).cuda()
        self.out = torch.full((2 * PAD + 2 * nk + 2,), -777.0, device='cuda')
        self.ri = torch.full((2 * PAD + self.n_img,), -777, dtype=torch.int32, device='cuda')
        self.rt = torch.full((2 * PAD + self.n_txt,), -777, dtype=torch.int32, device='cuda')
        from distillclip_amd._lib import lib
        self.ws = torch.empty(lib().dclip_retrieval_recall_workspace(self.n_img, self.n_txt, self.E), dtype=torch.uint8, device='cuda')

    def __call__(self, table, ranks=True):
        """table: the n_img + 1 offsets as given; they sit between walls of huge values -> out, rank_i2t, rank_t2i (numpy; None if not asked)"""
        from distillclip_amd._lib import lib
        assert len(table) == self.n_img + 1
        tab = torch.tensor([1 << 30] * PAD + list(table) + [1 << 30] * PAD, dtype=torch.int32).cuda()
        ks = (ctypes.c_int32 * 3)(1, 5, 10)
        at = lambda t, skip: t.data_ptr() + skip * t.element_size()
        lib().dclip_retrieval_recall(at(self.img_buf, 16 * self.E), at(self.txt_buf, 16 * self.E), at(tab, PAD), self.n_img, self.n_txt, self.E,
                                     ks, self.nk, at(self.out, PAD), at(self.ri, PAD) if ranks else None, at(self.rt, PAD) if ranks else None,
                                     self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream)
        out, ri, rt = self.out.cpu().numpy(), self.ri.cpu().numpy(), self.rt.cpu().numpy()
        for buf, n in ((out, 2 * self.nk + 2), (ri, self.n_img), (rt, self.n_txt)):
            assert (buf[:PAD] == -777).all() and (buf[PAD + n:] == -777).all()      # nothing outside [2 nk + 2], [n_img], [n_txt]
        if not ranks:
            assert (ri == -777).all() and (rt == -777).all()
        return out[PAD:PAD + 2 * self.nk + 2].copy(), ri[PAD:PAD + self.n_img].copy(), rt[PAD:PAD + self.n_txt].copy()


def test_guards_null_ranks_and_clamped_tables():
    img, txt, counts, _ = rc.reference(33, 64, 1)
    n_img, n_txt = img.shape[0], txt.shape[0]
    offs = np.concatenate([[0], np.cumsum(counts)]).tolist()
    want_out, want_i, want_t = run(img, txt, counts)
    raw = Raw(img, txt)
    out, ri, rt = raw(offs)
    assert np.array_equal(out, want_out) and np.array_equal(ri, want_i) and np.array_equal(rt, want_t)
    # null rank pointers: the same figures, no rank written anywhere
    raw2 = Raw(img, txt)
    out2, _, _ = raw2(offs, ranks=False)
    assert np.array_equal(out2, want_out)
    # -7 and n_txt + 9 clamp to 0 and n_txt: the well-formed table again.  Unclamped, image 0 and the last image would own rows outside
    # txt (the walls) and their ranks would change
    assert counts[0] > 0 and counts[-1] > 0 and want_i[0] > 0 and want_i[-1] > 0
    out, ri, rt = Raw(img, txt)([-7] + offs[1:-1] + [n_txt + 9])
    assert np.array_equal(out, want_out) and np.array_equal(ri, want_i) and np.array_equal(rt, want_t)
    # a table that is not monotone: end <= start reads as an empty group, a caption no group covers gets -1; all within range
    bad = list(offs)
    bad[3], bad[10], bad[20] = n_txt + 9, -7, 2
    out, ri, rt = Raw(img, txt)(bad)
    assert np.isfinite(out).all() and (out >= 0).all() and (out[:6] <= 1).all()
    assert (ri >= -1).all() and (ri <= n_txt).all() and (rt >= -1).all() and (rt < n_img).all()
    assert (ri == -1).any() and (ri >= 0).any()
    again = Raw(img, txt)(bad)
    assert all(np.array_equal(a, b) for a, b in zip((out, ri, rt), again))   # the answer depends on the table alone


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------
def test_same_call_same_bits():
    from distillclip_amd.metrics import retrieval_recall
    img, txt, counts, _ = rc.reference(130, 512, 1)
    d_img, d_txt = img.cuda(), txt.cuda()
    runs = [retrieval_recall(d_img, d_txt, counts, KS, return_ranks=True) for _ in range(2)]
    assert set(runs[0]) == set(runs[1]) and len(runs[0]) == 10
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), key
    a = retrieval_recall(d_img, d_txt, counts, KS)                           # without the rank copies: the same figures
    assert 'i2t_ranks' not in a and all(torch.equal(a[k], runs[0][k]) for k in a)


# ---- 8. the evaluator ----------------------------------------------------------------------------------------------------------------
def test_evaluator_end_to_end():
    from test_clipscore_gpu import _students
    from distillclip_amd import RetrievalEvaluator, synth
    from distillclip_amd.metrics import retrieval_recall
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _students(3)
    clip = CLIPModel(True, s_img, s_txt).cuda()
    modules = list(clip.modules())
    before = {n: p.detach().clone() for n, p in clip.named_parameters()}
    flags = [p.requires_grad for p in clip.parameters()], [m.training for m in modules]
    assert all(flags[0]) and all(flags[1])
    # three batches of 5 images: ragged counts, ragged with an empty group, dense [B, 2, L]
    batches = []
    for s, counts in enumerate(([2, 1, 3, 1, 2], [0, 4, 1, 1, 2], None)):
        images = torch.from_numpy(synth.images(60 + s, 5, 32)).cuda()
        m = 10 if counts is None else sum(counts)
        caps = torch.from_numpy(synth.captions(70 + s, m, 13, 97, 3, 9)).cuda()
        batches.append((images, caps.reshape(5, 2, 13) if counts is None else caps, counts))
    ev = RetrievalEvaluator.from_model(clip, max_batch=2)                    # smaller than a batch: the towers run in chunks
    assert torch.is_grad_enabled()
    for images, caps, counts in batches:
        ev.update(images, caps, counts)
    got = ev.compute(return_ranks=True)
    # the same rows from direct tower calls on the same chunks
    with torch.no_grad():
        rows_i, rows_t = [], []
        for images, caps, counts in batches:
            caps = caps.reshape(-1, 13)
            rows_i += [clip.encode_image(images[s:s + 2]).last_representation for s in range(0, 5, 2)]
            rows_t += [clip.encode_text(caps[s:s + 2]).last_representation for s in range(0, caps.shape[0], 2)]
    all_counts = [2, 1, 3, 1, 2, 0, 4, 1, 1, 2, 2, 2, 2, 2, 2]
    want = retrieval_recall(torch.cat(rows_i), torch.cat(rows_t), all_counts, (1, 5, 10), return_ranks=True)
    assert set(got) == set(want) == {f'{d}_recall@{k}' for d in ('i2t', 't2i') for k in (1, 5, 10)} | {
        'i2t_mean_rank', 't2i_mean_rank', 'i2t_ranks', 't2i_ranks'}
    for key in want:
        assert torch.equal(got[key], want[key]) and not got[key].requires_grad, key
    assert got['i2t_ranks'].shape == (15,) and got['t2i_ranks'].shape == (27,) and got['i2t_ranks'][5] == -1
    assert 0 < got['t2i_recall@10'] <= 1
    # rows formed elsewhere give the same figures
    ev2 = RetrievalEvaluator(clip.image_encoder, clip.text_encoder)
    ev2.add_embeddings(torch.cat(rows_i[:3]), torch.cat(rows_t)[:9], all_counts[:5])
    ev2.add_embeddings(torch.cat(rows_i[3:]), torch.cat(rows_t)[9:], torch.tensor(all_counts[5:]))
    also = ev2.compute()
    assert 'i2t_ranks' not in also and all(torch.equal(also[k], want[k]) for k in also)
    # reset() forgets the rows
    ev.reset()
    with pytest.raises(ValueError, match='nothing to rank'):
        ev.compute()
    ev.update(*batches[0])
    one = ev.compute(return_ranks=True)
    assert one['i2t_ranks'].shape == (5,) and one['t2i_ranks'].shape == (9,)
    # nothing of the towers changed
    for n, p in clip.named_parameters():
        assert torch.equal(p.detach(), before[n]) and p.grad is None, n
    assert [p.requires_grad for p in clip.parameters()] == flags[0] and [m.training for m in modules] == flags[1]

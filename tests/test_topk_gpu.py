"""Top-K search over embeddings and zero-shot classification on the GPU (dclip_topk_search, dclip_group_mean_rows, metrics.topk_search,
metrics.group_mean_rows, ZeroShotClassifier): every row of every case against float64 as intervals, exact on planted logits, under ties,
zero and invalid rows, permutations, repeated calls and prefixes, in exact agreement with dclip_retrieval_recall, the buffers' guards, the
group means, and the classifier end to end on the tiny students.  Cases, the bound b(E) = (2 E + 8) 2^-24, the float64 reference and the
checker live in tests/topk_cases.py; tests/test_topk_cpu.py checks the reference itself."""
import numpy as np
import pytest
import torch

import recall_cases as rc
import topk_cases as tc

pytestmark = pytest.mark.gpu


def search(q, gal, k, scores=True):
    """-> idx int32 [nq, k], score f32 [nq, k] (or None) as numpy arrays"""
    from distillclip_amd.metrics import topk_search
    idx, score = topk_search(q.cuda(), gal.cuda(), k, return_scores=scores)
    assert idx.shape == (q.shape[0], k) and idx.dtype == torch.int32 and idx.is_cuda
    assert (score is None) == (not scores)
    if scores:
        assert score.shape == idx.shape and score.dtype == torch.float32
    return idx.cpu().numpy(), score.cpu().numpy() if scores else None


def bits(x):
    return x.view(np.int32)


# ---- 1. against float64, as intervals, every row --------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', tc.SEEDS)
@pytest.mark.parametrize('nq,ng,k,E', tc.CASES)
def test_every_row_against_float64(nq, ng, k, E, seed):
    q, gal, L, _ = tc.reference(nq, ng, E, seed)
    idx, score = search(q, gal, k)
    differ, err = tc.check_against_float64(idx, score, L, k, E)
    print(f'({nq}, {ng}, k={k}, E={E}) seed {seed}: {differ} of {nq} index lists differ from the float64 order, '
          f'max |score - L64| = {err / tc.U:.1f} u of b = {tc.bound(E) / tc.U:.0f} u')


@pytest.mark.parametrize('nq,ng,k,E', [(17, 257, 10, 64), (33, 1000, 64, 512), (16, 65, 5, 16)])
def test_near_ties_against_float64(nq, ng, k, E):
    """a gallery of three directions with perturbations of a few u: the logits of a row fall into three clusters whose members lie
    within a few b(E) of one another, so inside the top k near-ties are the rule and the interval checks decide"""
    g = torch.Generator().manual_seed(31 * ng + E)
    centres = torch.randn(3, E, generator=g)
    gal = centres[torch.randint(0, 3, (ng,), generator=g)] * (1 + 4 * tc.bound(E) * torch.randn(ng, E, generator=g))
    q = centres[torch.randint(0, 3, (nq,), generator=g)] + 0.5 * torch.randn(nq, E, generator=g)
    L = tc.cos64(q, gal)
    near = np.abs(np.sort(L, axis=1)[:, -2:-1] - np.sort(L, axis=1)[:, -min(k, ng):]) <= 2 * tc.bound(E)
    assert near.mean() > 0.5                                         # a condition on the case: most of the top k is within 2 b of the runner-up
    idx, score = search(q, gal, k)
    differ, err = tc.check_against_float64(idx, score, L, k, E)
    print(f'near ties ({nq}, {ng}, k={k}, E={E}): {differ} of {nq} index lists differ from the float64 order')


# ---- 2. planted logits, exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 10, 64))
def test_planted_logits_are_exact(k):
    q, gal, v = tc.planted_case()
    want_idx, want_score = tc.planted_answer(v, k)
    idx, score = search(q, gal, k)
    assert np.array_equal(idx, want_idx), np.argwhere(idx != want_idx)[:8]
    assert np.array_equal(bits(score), bits(want_score)), np.argwhere(score != want_score)[:8]


# ---- 3. ties go to the lower index ---------------------------------------------------------------------------------------------------
def test_bit_copies_tie_in_index_order():
    q, gal, _, _ = tc.reference(33, 257, 64, 0)
    ng = gal.shape[0]
    sel = torch.arange(0, ng, 3)
    both = torch.cat([gal, gal[sel]])                                # copy i of row sel[i] sits at ng + i
    k = 64
    idx, score = search(q, both, k)
    tc.check_order(idx, score, both.shape[0])
    pairs = 0
    for i in range(idx.shape[0]):
        pos = {int(j): p for p, j in enumerate(idx[i])}
        for c, j in enumerate(sel.tolist()):
            if ng + c in pos:                                        # the copy is listed: its original is, right before it, same bits
                assert j in pos and pos[j] == pos[ng + c] - 1, (i, j)
                assert bits(score[i])[pos[j]] == bits(score[i])[pos[ng + c]]
                pairs += 1
            elif j in pos:                                           # the original alone: only as the last entry
                assert pos[j] == k - 1, (i, j)
    assert pairs > 33 * 5
    # a gallery that is one row repeated: every logit of a query row is the same, the answer is 0 .. k - 1
    same = gal[5:6].repeat(150, 1)
    idx, score = search(q, same, 64)
    assert np.array_equal(idx, np.tile(np.arange(64, dtype=np.int32), (33, 1)))
    assert (bits(score) == bits(score)[:, :1]).all() and len(np.unique(score[:, 0])) > 1


def test_zero_rows_and_signed_zeros():
    E = 64
    g = torch.Generator().manual_seed(2)
    zeros = torch.zeros(150, E)
    first = np.tile(np.arange(17, dtype=np.int32), (3, 1))
    qs = torch.stack([torch.zeros(E), -torch.rand(E, generator=g) - 0.5, torch.randn(E, generator=g)])
    # zero gallery rows: every logit is 0 whatever the query (0, all negative: -0 products, mixed), the answer is 0 .. k - 1
    idx, score = search(qs, zeros, 17)
    assert np.array_equal(idx, first) and (bits(score) == 0).all()  # +0, never -0
    # zero rows among rows with a -0 logit: a query and gallery rows with disjoint supports, the gallery entries negative
    q = torch.zeros(1, E)
    q[0, :16] = 1.0
    gal = torch.zeros(40, E)
    gal[::2, 16:32] = -1.0                                           # products 1 * (+0) and 0 * (-1) = -0
    gal[1::4, :] = 0.0
    idx, score = search(q, gal, 40)
    assert np.array_equal(idx[0], np.arange(40)) and (bits(score) == 0).all()
    # a negative logit is below the zeros, a positive one above: zero rows sit between, in index order
    gal[7, :16] = -1.0
    gal[31, :16] = 2.0
    idx, score = search(q, gal, 40)
    assert idx[0, 0] == 31 and idx[0, -1] == 7 and np.array_equal(idx[0, 1:-1], [j for j in range(40) if j not in (7, 31)])
    assert score[0, 0] == 1.0 and score[0, -1] == -1.0


def test_invalid_rows_are_zero_rows():
    q, gal, _, _ = tc.reference(17, 257, 64, 1)
    bad, zeroed = gal.clone(), gal.clone()
    bad[3, 5] = float('inf')
    bad[100, 0] = float('nan')
    bad[256, 63] = float('-inf')
    bad[17] = 3e38                                                   # finite, the squared norm overflows
    zeroed[[3, 100, 256, 17]] = 0.0
    qb, qz = q.clone(), q.clone()
    qb[2, 7] = float('nan')
    qz[2] = 0.0
    idx, score = search(qb, bad, 64)
    want_idx, want_score = search(qz, zeroed, 64)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(score), bits(want_score))
    assert np.array_equal(idx[2], np.arange(64)) and (bits(score[2]) == 0).all()
    full, s = search(q, bad[:64], 64)                                # all of a 64-row gallery: the invalid rows rank with logit 0
    assert (np.sort(full, axis=1) == np.arange(64)).all() and (bits(s)[full == 3] == 0).all() and (bits(s)[full == 17] == 0).all()


# ---- 4. position independence --------------------------------------------------------------------------------------------------------
def test_permutations():
    q, gal, _, _ = tc.reference(33, 64, 64, 2)
    idx, score = search(q, gal, 64)                                  # k = ng: every logit of every row
    assert (score[:, 1:] < score[:, :-1]).all()                      # a condition on the case: no two logits of a row are bit-equal
    perm = np.random.RandomState(5).permutation(64)
    idx_p, score_p = search(q, gal[torch.from_numpy(perm)], 64)
    assert np.array_equal(perm[idx_p], idx) and np.array_equal(bits(score_p), bits(score))
    qperm = np.random.RandomState(6).permutation(33)
    idx_q, score_q = search(q[torch.from_numpy(qperm)], gal, 64)
    assert np.array_equal(idx_q, idx[qperm]) and np.array_equal(bits(score_q), bits(score[qperm]))
    # more tiles than list entries, ties included: the queries' rows still move bit for bit
    q, gal, v = tc.planted_case()
    idx, score = search(q, gal, 10)
    qperm = np.random.RandomState(7).permutation(q.shape[0])
    idx_q, score_q = search(q[torch.from_numpy(qperm)], gal, 10)
    assert np.array_equal(idx_q, idx[qperm]) and np.array_equal(bits(score_q), bits(score[qperm]))


def test_same_call_same_bits_and_prefixes():
    q, gal, _, _ = tc.reference(70, 4099, 512, 0)
    idx, score = search(q, gal, 64)
    again_idx, again_score = search(q, gal, 64)
    assert np.array_equal(idx, again_idx) and np.array_equal(bits(score), bits(again_score))
    only_idx, none = search(q, gal, 64, scores=False)
    assert none is None and np.array_equal(only_idx, idx)
    for k in (1, 2, 5, 10, 16, 17, 63):
        idx_k, score_k = search(q, gal, k)
        assert np.array_equal(idx_k, idx[:, :k]) and np.array_equal(bits(score_k), bits(score[:, :k])), k
    # k > ng: the prefix of length ng is the whole ranking
    q, gal, _, _ = tc.reference(17, 15, 64, 0)
    idx, score = search(q, gal, 16)
    idx_k, score_k = search(q, gal, 5)
    assert np.array_equal(idx_k, idx[:, :5]) and np.array_equal(bits(score_k), bits(score[:, :5]))
    # any float dtype goes in: the rows are taken to f32
    h_idx, h_score = search(q.half(), gal.half(), 5)
    f_idx, f_score = search(q.half().float(), gal.half().float(), 5)
    assert np.array_equal(h_idx, f_idx) and np.array_equal(bits(h_score), bits(f_score))


# ---- 5. exact agreement with dclip_retrieval_recall ----------------------------------------------------------------------------------
@pytest.mark.parametrize('n_img,E,seed,k', [(33, 64, 1, 5), (130, 64, 0, 10), (130, 512, 1, 64)])
def test_agrees_with_retrieval_recall(n_img, E, seed, k):
    """Both use the same normaliser and the same tile routine, so the comparison is exact.  A row whose recall rank r is below k: the
    entries of its list that are not targets and lie strictly above the best target in the list number exactly r.  A row with r >= k:
    no target is listed."""
    from distillclip_amd.metrics import retrieval_recall
    img, txt, counts, _ = rc.reference(n_img, E, seed)
    res = retrieval_recall(img.cuda(), txt.cuda(), counts, (1, 5, 10), return_ranks=True)
    rank_i, rank_t = res['i2t_ranks'].cpu().numpy(), res['t2i_ranks'].cpu().numpy()
    own = rc.owners(counts)
    seen = {'in': 0, 'out': 0}

    def check(idx, score, ranks, is_target):
        for i in range(idx.shape[0]):
            r = int(ranks[i])
            if r < 0:
                continue
            target = np.array([is_target(i, int(j)) for j in idx[i]])
            if r < k:
                assert target.any(), (i, r)
                best = score[i][target].max()
                assert int((~target & (score[i] > best)).sum()) == r, (i, r)
                seen['in'] += 1
            else:
                assert not target.any(), (i, r)
                seen['out'] += 1
    kk = min(k, txt.shape[0])
    idx, score = search(img, txt, kk)                                # image -> text: the targets are the image's own captions
    check(idx, score, rank_i, lambda i, j: own[j] == i)
    idx, score = search(txt, img, min(k, n_img))                     # text -> image: the target is the caption's image
    check(idx, score, rank_t, lambda c, j: own[c] == j)
    assert seen['in'] > 0 and (seen['out'] > 0 or k >= 64)


# ---- 6. guards -----------------------------------------------------------------------------------------------------------------------
PAD = 64


def test_guards_around_every_buffer():
    from distillclip_amd._lib import lib
    q, gal, _, _ = tc.reference(17, 257, 64, 2)
    nq, ng, E, k = 17, 257, 64, 10
    want_idx, want_score = search(q, gal, k)
    nan = lambda n: torch.full((n, E), float('nan'))
    q_buf, g_buf = torch.cat([nan(16), q, nan(16)]).cuda(), torch.cat([nan(16), gal, nan(16)]).cuda()
    need = lib().dclip_topk_search_workspace(nq, ng, E, k)
    at = lambda t, skip: t.data_ptr() + skip * t.element_size()
    for with_score in (True, False):
        idx_buf = torch.full((2 * PAD + nq * k,), -777, dtype=torch.int32, device='cuda')
        score_buf = torch.full((2 * PAD + nq * k,), -777.0, device='cuda')
        ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device='cuda')      # exactly the queried size, then a patterned guard
        lib().dclip_topk_search(at(q_buf, 16 * E), at(g_buf, 16 * E), nq, ng, E, k, at(idx_buf, PAD), at(score_buf, PAD) if with_score else None,
                                ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        idx, score = idx_buf.cpu().numpy(), score_buf.cpu().numpy()
        assert (idx[:PAD] == -777).all() and (idx[PAD + nq * k:] == -777).all()
        assert (score[:PAD] == -777).all() and (score[PAD + nq * k:] == -777).all()
        assert (ws[need:] == 0xA5).all().item()
        assert np.array_equal(idx[PAD:PAD + nq * k].reshape(nq, k), want_idx)          # nothing of the NaN walls was read
        if with_score:
            assert np.array_equal(bits(score[PAD:PAD + nq * k].reshape(nq, k)), bits(want_score))
        else:
            assert (score == -777).all()
    assert torch.isnan(q_buf[:16]).all() and torch.isnan(g_buf[-16:]).all()           # the inputs are not written


def test_group_mean_guards_and_a_table_that_is_not_monotone():
    from distillclip_amd._lib import lib
    E, n_rows = 64, 40
    rows = torch.randn(n_rows, E, generator=torch.Generator().manual_seed(8)) * 3
    nan = torch.full((16, E), float('nan'))
    r_buf = torch.cat([nan, rows, nan]).cuda()
    table = [-7, 5, 5, 30, 12, n_rows + 9, 33, 1 << 30]              # 7 groups: clamped, empty, backwards (empty), overlapping
    n_groups = len(table) - 1
    tab = torch.tensor([1 << 30] * PAD + table + [-(1 << 30)] * PAD, dtype=torch.int32).cuda()
    at = lambda t, skip: t.data_ptr() + skip * t.element_size()
    outs = []
    for _ in range(2):
        out_buf = torch.full((2 * PAD + n_groups * E,), -777.0, device='cuda')
        lib().dclip_group_mean_rows(at(r_buf, 16 * E), at(tab, PAD), n_groups, n_rows, E, at(out_buf, PAD), torch.cuda.current_stream().cuda_stream)
        out = out_buf.cpu().numpy()
        assert (out[:PAD] == -777).all() and (out[PAD + n_groups * E:] == -777).all()
        outs.append(out[PAD:PAD + n_groups * E].reshape(n_groups, E))
    assert np.array_equal(bits(outs[0]), bits(outs[1]))              # the answer depends on the table alone
    clamp = [min(max(t, 0), n_rows) for t in table]
    xn = tc.group_mean64(rows, [1] * n_rows)                         # every row normalised, in float64
    for c, (a, b) in enumerate(zip(clamp, clamp[1:])):
        want = xn[a:b].mean(axis=0) if b > a else np.zeros(E)
        assert np.abs(outs[0][c] - want).max() <= tc.group_mean_bound(E, max(b - a, 1)), c
        if b <= a:
            assert (bits(outs[0][c]) == 0).all()


# ---- 7. group means ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', (16, 64, 512, 768))
def test_group_mean_rows_against_float64(E):
    from distillclip_amd.metrics import group_mean_rows
    counts = [5, 1, 0, 7, 80, 0, 1, 3, 2]                            # empty groups, single rows, a long group; more groups than one block's waves
    n = sum(counts)
    g = torch.Generator().manual_seed(E)
    rows = torch.randn(n, E, generator=g) * (0.1 + 5 * torch.rand(n, 1, generator=g))
    rows[7] = 0.0                                                    # a zero row adds nothing (its group still divides by its count)
    out = group_mean_rows(rows.cuda(), counts)
    assert out.shape == (len(counts), E) and out.dtype == torch.float32 and out.is_cuda
    got = out.cpu().numpy()
    want = tc.group_mean64(rows, counts)
    for c, n_c in enumerate(counts):
        err = np.abs(got[c] - want[c]).max()
        assert err <= tc.group_mean_bound(E, max(n_c, 1)), (c, n_c, err / tc.U)
        if n_c == 0:
            assert (bits(got[c]) == 0).all()
    again = group_mean_rows(rows.cuda(), torch.tensor(counts)).cpu().numpy()
    assert np.array_equal(bits(got), bits(again))
    # a single-row group is that row normalised, times 1: the same bits wherever the row sits, and exact where f32 normalises exactly
    singles = group_mean_rows(rows.cuda(), [1] * n).cpu().numpy()
    offs = np.concatenate([[0], np.cumsum(counts)])
    for c in (1, 6):
        assert np.array_equal(bits(got[c]), bits(singles[offs[c]]))
    exact = torch.zeros(4, E)
    exact[0, 3], exact[1, :4], exact[2, :16], exact[3, 5] = 8.0, -0.5, 0.25, -2.0 ** -20
    got = group_mean_rows(exact.half().cuda(), [1, 1, 1, 1]).cpu().numpy()
    want = np.zeros((4, E), dtype=np.float32)
    want[0, 3], want[1, :4], want[2, :16], want[3, 5] = 1.0, -0.5, 0.25, -1.0
    assert np.array_equal(got, want)


# ---- 8. the classifier ---------------------------------------------------------------------------------------------------------------
L_TOK = 13


def _zeroshot_inputs():
    from distillclip_amd import synth
    counts = [2, 1, 3, 1, 2, 3, 0, 2]                                # 8 classes, one without a prompt
    prompts = torch.from_numpy(synth.captions(80, sum(counts), L_TOK, 97, 3, 9)).cuda()
    batches = [(torch.from_numpy(synth.images(90 + s, 5, 32)).cuda(), labels) for s, labels in
               enumerate(([0, 3, 7, 1, 4], torch.tensor([2, 2, 5, 0, 6]), torch.tensor([1, 9, -1, 3, 4]).cuda()))]
    return prompts, counts, batches


def _by_hand(clip, prompts, counts, batches, chunk, k_list):
    """direct tower calls on the same chunks, group_mean_rows, topk_search and integer counting"""
    from distillclip_amd.metrics import group_mean_rows, topk_search
    with torch.no_grad():
        rows_t = torch.cat([clip.encode_text(prompts[s:s + chunk]).last_representation for s in range(0, prompts.shape[0], chunk)])
        rows_i = torch.cat([clip.encode_image(im[s:s + chunk]).last_representation for im, _ in batches for s in range(0, im.shape[0], chunk)])
    classes = group_mean_rows(rows_t, counts)
    idx, score = topk_search(rows_i, classes, max(k_list))
    labels = np.concatenate([np.asarray(torch.as_tensor(lab).cpu()) for _, lab in batches])
    hit = idx.cpu().numpy() == labels[:, None]
    acc = {f'acc_top{k}': np.float64(int(hit[:, :k].sum())) / np.float64(len(labels)) for k in k_list}
    return classes, rows_i, idx, score, acc


@pytest.mark.parametrize('max_batch', (2, 512))
def test_classifier_end_to_end(max_batch):
    from test_clipscore_gpu import _students
    from distillclip_amd import ZeroShotClassifier
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _students(3)
    clip = CLIPModel(True, s_img, s_txt).cuda()
    modules = list(clip.modules())
    before = {n: p.detach().clone() for n, p in clip.named_parameters()}
    flags = [p.requires_grad for p in clip.parameters()], [m.training for m in modules]
    prompts, counts, batches = _zeroshot_inputs()
    k_list = (1, 3, 5)
    zs = ZeroShotClassifier.from_model(clip, k_list=k_list, max_batch=max_batch)
    assert torch.is_grad_enabled()
    zs.set_classes(prompts, counts)
    for images, labels in batches:
        zs.update(images, labels)
    got = zs.compute()
    classes, rows_i, idx, score, acc = _by_hand(clip, prompts, counts, batches, max_batch, k_list)
    assert torch.equal(zs.class_embeddings, classes) and (classes[6] == 0).all()
    assert set(got) == {'acc_top1', 'acc_top3', 'acc_top5'}
    for key, want in acc.items():
        assert got[key].dim() == 0 and got[key].is_cuda and got[key].dtype == torch.float64 and not got[key].requires_grad
        assert got[key].item() == want, (key, got[key].item(), want)
    assert 0 <= acc['acc_top1'] <= acc['acc_top3'] <= acc['acc_top5'] <= 13 / 15     # labels 9 and -1 never hit
    # predict is the first k columns of what compute ranks
    for k in (1, 3, 5):
        at = 0
        for images, _ in batches:
            p_idx, p_score = zs.predict(images, k)
            assert torch.equal(p_idx, idx[at:at + 5, :k]) and torch.equal(p_score, score[at:at + 5, :k])
            at += 5
    # rows formed elsewhere give the same figures; reset() forgets the rows, not the classes
    zs2 = ZeroShotClassifier(clip.image_encoder, clip.text_encoder, k_list=k_list)
    zs2.set_class_embeddings(classes)
    zs2.add_embeddings(rows_i[:7], np.concatenate([np.asarray(torch.as_tensor(lab).cpu()) for _, lab in batches])[:7].tolist())
    zs2.add_embeddings(rows_i[7:], torch.cat([torch.as_tensor(lab).cpu() for _, lab in batches])[7:].cuda())
    also = zs2.compute()
    assert all(torch.equal(also[key], got[key]) for key in got)
    zs.reset()
    with pytest.raises(ValueError, match='nothing to classify'):
        zs.compute()
    zs.update(*batches[0])
    assert zs.compute()['acc_top5'].item() in [i / 5 for i in range(6)]
    # nothing of the towers changed
    for n, p in clip.named_parameters():
        assert torch.equal(p.detach(), before[n]) and p.grad is None, n
    assert [p.requires_grad for p in clip.parameters()] == flags[0] and [m.training for m in modules] == flags[1]


def test_chunking_does_not_change_a_bit():
    from test_clipscore_gpu import _students
    from distillclip_amd import ZeroShotClassifier
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _students(3)
    clip = CLIPModel(True, s_img, s_txt).cuda()
    prompts, counts, batches = _zeroshot_inputs()
    res = []
    for max_batch in (1, 2, 3, 512):
        zs = ZeroShotClassifier.from_model(clip, k_list=(1, 5), max_batch=max_batch)
        zs.set_classes(prompts, counts)
        for images, labels in batches:
            zs.update(images, labels)
        res.append((zs.class_embeddings, zs.compute(), zs.predict(batches[0][0], 5)))
    for classes, acc, (idx, score) in res[1:]:
        assert torch.equal(classes, res[0][0]) and torch.equal(idx, res[0][2][0]) and torch.equal(score, res[0][2][1])
        assert all(torch.equal(acc[key], res[0][1][key]) for key in acc)


def test_dense_and_ragged_prompts_agree():
    from test_clipscore_gpu import _students
    from distillclip_amd import ZeroShotClassifier, synth
    s_img, s_txt = _students(3)
    s_img, s_txt = s_img.cuda(), s_txt.cuda()
    dense = torch.from_numpy(synth.captions(81, 12, L_TOK, 97, 3, 9)).reshape(6, 2, L_TOK).cuda()
    a, b, c = (ZeroShotClassifier(s_img, s_txt, max_batch=4) for _ in range(3))
    a.set_classes(dense)
    b.set_classes(dense.reshape(12, L_TOK), [2] * 6)
    c.set_classes(dense, torch.tensor([2] * 6))
    assert a.class_embeddings.shape == (6, 64)
    assert torch.equal(a.class_embeddings, b.class_embeddings) and torch.equal(a.class_embeddings, c.class_embeddings)
    images = torch.from_numpy(synth.images(95, 5, 32)).cuda()
    ia, sa = a.predict(images, 6)
    ib, sb = b.predict(images, 6)
    assert torch.equal(ia, ib) and torch.equal(sa, sb)
    assert (ia.sort(dim=1).values == torch.arange(6, device='cuda', dtype=torch.int32)).all()      # k = C: a ranking of all classes

"""Top-K search over embeddings and zero-shot classification (dclip_topk_search, dclip_group_mean_rows, metrics.topk_search,
metrics.group_mean_rows, ZeroShotClassifier), the parts that need no GPU: the header and the library carry the three entries, the C entries
refuse bad arguments on the host before any launch, the Python layers raise before a tower or a kernel runs, and the float64 reference of
the GPU tests orders every case as a brute-force sort does."""
import ctypes

import numpy as np
import pytest
import torch

import topk_cases as tc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    P, I, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert protos['dclip_topk_search_workspace'] == (ctypes.c_size_t, [I, I, I, i])
    assert protos['dclip_topk_search'] == (i, [P, P, I, I, I, i, P, P, P, ctypes.c_size_t, P])
    assert protos['dclip_group_mean_rows'] == (i, [P, P, I, I, I, P, P])
    for name in ('dclip_topk_search_workspace', 'dclip_topk_search', 'dclip_group_mean_rows'):
        assert hasattr(l._dll, name), name
    assert l.dclip_version() == 6                          # additive: no existing signature changed
    # normalised copies of both row sets and nothing of the size of the logits
    nq, ng, E = 25010, 5000, 512
    need = (nq + ng) * E * 4
    assert need <= l.dclip_topk_search_workspace(nq, ng, E, 10) <= need + 2 * 256
    assert l.dclip_topk_search_workspace(nq, ng, E, 64) == l.dclip_topk_search_workspace(nq, ng, E, 1)
    # few query panels against a long gallery: the gallery is cut into slices, whose k best keys (8 bytes each) join the workspace
    lists = l.dclip_topk_search_workspace(ng, nq, E, 10) - l.dclip_topk_search_workspace(nq, ng, E, 10)
    assert lists > 0 and lists % (ng * 10 * 8) < 256 and 2 <= lists // (ng * 10 * 8) <= 8


def test_header_states_the_semantics():
    from distillclip_amd._lib import _HEADER
    text = ' '.join(open(_HEADER).read().split())
    for phrase in ('L descending, index ascending', '-0 and +0 compare equal', 'idx = -1, score = -inf', '1 <= k <= 64',
                   'treated as the zero row', 'prefix of the result for k2', 'An empty group gives the zero row'):
        assert phrase in text, phrase


# ---- 2. host refusals ----------------------------------------------------------------------------------------------------------------
# dummy non-null, 16-byte aligned addresses: never dereferenced, every call below is refused before a launch
Q, G, IDX, SC, WS, ROWS, OFF, OUT = 4096, 8192, 12288, 16384, 1 << 20, 20480, 24576, 28672


def _search(**kw):
    g = lambda name, default: kw[name] if name in kw else default
    nq, ng, E, k = g('nq', 3), g('ng', 7), g('E', 64), g('k', 5)
    ws_bytes = g('ws_bytes', max(_lib().dclip_topk_search_workspace(nq, ng, E, k), 16))
    return _lib().dclip_topk_search(g('q', Q), g('g', G), nq, ng, E, k, g('idx', IDX), g('score', SC), g('ws', WS), ws_bytes, None)


@pytest.mark.parametrize('kw,word', [
    (dict(q=None), 'null'), (dict(g=None), 'null'), (dict(idx=None), 'null'), (dict(ws=None), 'null'),
    (dict(k=0), '1 <= k <= 64'), (dict(k=65), '1 <= k <= 64'), (dict(k=-1), '1 <= k <= 64'),
    (dict(E=24), 'multiple of 16'), (dict(E=0), 'multiple of 16'), (dict(E=8), 'multiple of 16'),
    (dict(ng=0), 'ng'), (dict(nq=0), 'nq'), (dict(ng=1 << 24), '2\\^24'), (dict(nq=1 << 24), '2\\^24'),
    (dict(ws_bytes=0), 'workspace too small'),
    (dict(q=Q + 4), '16-byte aligned'), (dict(g=G + 8), '16-byte aligned'), (dict(ws=WS + 4), '16-byte aligned'),
    (dict(idx=IDX + 2), 'aligned'), (dict(score=SC + 1), 'aligned'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_search_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word):
        _search(**kw)


def test_search_refuses_a_workspace_one_byte_short():
    need = _lib().dclip_topk_search_workspace(3, 7, 64, 5)
    assert need > 0
    with pytest.raises(ValueError, match='workspace too small'):
        _search(ws_bytes=need - 1)


def test_workspace_query_of_refused_arguments_is_zero():
    w = _lib().dclip_topk_search_workspace
    assert w(0, 5, 64, 1) == 0 and w(5, 0, 64, 1) == 0 and w(5, 5, 24, 1) == 0 and w(5, 5, 0, 1) == 0
    assert w(5, 5, 64, 0) == 0 and w(5, 5, 64, 65) == 0 and w(1 << 24, 5, 64, 1) == 0 and w(5, 1 << 24, 64, 1) == 0
    assert w(1, 1, 16, 1) > 0 and w(1, 1, 16, 64) > 0


def _group_mean(**kw):
    g = lambda name, default: kw[name] if name in kw else default
    return _lib().dclip_group_mean_rows(g('rows', ROWS), g('off', OFF), g('n_groups', 3), g('n_rows', 7), g('E', 64), g('out', OUT), None)


@pytest.mark.parametrize('kw,word', [
    (dict(rows=None), 'null'), (dict(off=None), 'null'), (dict(out=None), 'null'),
    (dict(E=24), 'multiple of 16'), (dict(E=0), 'multiple of 16'), (dict(E=4112), 'at most 4096'),
    (dict(n_groups=0), 'n_groups'), (dict(n_rows=0), 'n_rows'), (dict(n_groups=1 << 24), '2\\^24'),
    (dict(rows=ROWS + 4), '16-byte aligned'), (dict(out=OUT + 8), '16-byte aligned'), (dict(off=OFF + 2), 'aligned'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_group_mean_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word):
        _group_mean(**kw)


# ---- 3. the Python layers ------------------------------------------------------------------------------------------------------------
def test_topk_search_raises_on_the_host():
    from distillclip_amd.metrics import topk_search
    q, g = torch.zeros(3, 64), torch.zeros(7, 64)
    with pytest.raises(ValueError, match='matrices'):
        topk_search(q, torch.zeros(7, 32), 1)
    with pytest.raises(ValueError, match='matrices'):
        topk_search(q[0], g, 1)
    with pytest.raises(ValueError, match='multiple of 16'):
        topk_search(torch.zeros(3, 24), torch.zeros(7, 24), 1)
    with pytest.raises(ValueError, match='nq, ng'):
        topk_search(q, torch.zeros(0, 64), 1)
    with pytest.raises(ValueError, match='1 <= k <= 64'):
        topk_search(q, g, 0)
    with pytest.raises(ValueError, match='1 <= k <= 64'):
        topk_search(q, g, 65)
    with pytest.raises(ValueError, match='no CPU path'):
        topk_search(q, g, 5)                                         # well-formed: CPU tensors are refused, nothing is computed


def test_group_mean_rows_raises_on_the_host():
    from distillclip_amd.metrics import group_mean_rows
    rows = torch.zeros(5, 64)
    with pytest.raises(ValueError, match='sum to 4'):
        group_mean_rows(rows, [2, 0, 2])
    with pytest.raises(ValueError, match='negative'):
        group_mean_rows(rows, [6, -1, 0])
    with pytest.raises(ValueError, match='matrix'):
        group_mean_rows(rows[0], [1])
    with pytest.raises(ValueError, match='multiple of 16'):
        group_mean_rows(torch.zeros(5, 24), [2, 3])
    with pytest.raises(ValueError, match='at most 4096'):
        group_mean_rows(torch.zeros(2, 4112), [1, 1])
    with pytest.raises(ValueError, match='n_groups, n_rows'):
        group_mean_rows(torch.zeros(0, 64), [0, 0])
    with pytest.raises(ValueError, match='no CPU path'):
        group_mean_rows(rows, torch.tensor([2, 0, 3]))


class _Tower(torch.nn.Module):
    """stand-in encoder: counts its calls; a test that reaches it has passed every host check"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0

    def forward(self, x, control):
        self.calls += 1
        raise RuntimeError('stand-in tower reached')


def test_classifier_is_exported_and_raises_on_the_host():
    import distillclip_amd
    from distillclip_amd.zeroshot import ZeroShotClassifier
    from distillclip_amd.model.component.clip_model import CLIPModel
    assert distillclip_amd.ZeroShotClassifier is ZeroShotClassifier
    img_t, txt_t = _Tower(), _Tower()
    zs = ZeroShotClassifier(img_t, txt_t, k_list=(1, 3), max_batch=7)
    assert zs.image_encoder is img_t and zs.text_encoder is txt_t and zs.k_list == (1, 3) and zs.max_batch == 7
    assert ZeroShotClassifier(img_t, txt_t).k_list == (1, 5)
    with pytest.raises(ValueError, match='max_batch'):
        ZeroShotClassifier(img_t, txt_t, max_batch=0)
    for bad in ((1, 65), (0, 1), ()):
        with pytest.raises(ValueError, match='k_list'):
            ZeroShotClassifier(img_t, txt_t, k_list=bad)
    L = 13
    images = torch.zeros(4, 3, 32, 32)
    # use before the classes are set
    with pytest.raises(ValueError, match='no classes yet'):
        zs.predict(images, 1)
    with pytest.raises(ValueError, match='no classes yet'):
        zs.compute()
    # set_classes: the counts are checked before the text tower runs
    prompts = torch.ones(6, L, dtype=torch.int64)
    with pytest.raises(ValueError, match='sum to 5'):
        zs.set_classes(prompts, [1, 2, 2])
    with pytest.raises(ValueError, match='negative'):
        zs.set_classes(prompts, [7, -1])
    with pytest.raises(ValueError, match='need counts'):
        zs.set_classes(prompts)
    with pytest.raises(ValueError, match='disagrees'):
        zs.set_classes(torch.ones(3, 2, L, dtype=torch.int64), [1, 3, 2])
    with pytest.raises(ValueError, match='prompts must be'):
        zs.set_classes(prompts[0], [1])
    assert txt_t.calls == 0
    with pytest.raises(RuntimeError, match='stand-in tower reached'):
        zs.set_classes(prompts, [3, 1, 2])                            # well-formed: reaches the text tower
    assert txt_t.calls == 1 and zs.class_embeddings is None
    # class rows formed elsewhere
    with pytest.raises(ValueError, match='\\[C, E\\]'):
        zs.set_class_embeddings(torch.zeros(64))
    with pytest.raises(ValueError, match='no CPU path'):
        zs.set_class_embeddings(torch.zeros(4, 64))
    zs.class_embeddings = torch.zeros(4, 64)                          # (what set_class_embeddings stores, here on the host)
    # k against the number of classes
    with pytest.raises(ValueError, match='k=5 with 4 classes'):
        zs.predict(images, 5)
    with pytest.raises(ValueError, match='k=0 with 4 classes'):
        zs.predict(images, 0)
    zs5 = ZeroShotClassifier(img_t, txt_t)                            # k_list (1, 5) with 4 classes
    zs5.class_embeddings = torch.zeros(4, 64)
    with pytest.raises(ValueError, match='k=5 with 4 classes'):
        zs5.compute()
    # labels
    with pytest.raises(ValueError, match='4 images need 4 labels'):
        zs.update(images, [0, 1, 2])
    with pytest.raises(ValueError, match='4 images need 4 labels'):
        zs.update(images, torch.zeros(4, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match='integer class indices'):
        zs.update(images, torch.zeros(4))
    with pytest.raises(ValueError, match='images must be'):
        zs.update(images[0], [0])
    with pytest.raises(ValueError, match='3 images need 3 labels'):
        zs.add_embeddings(torch.zeros(3, 64), [0, 1])
    with pytest.raises(ValueError, match='image rows'):
        zs.add_embeddings(torch.zeros(64), [0])
    with pytest.raises(ValueError, match='no CPU path'):
        zs.add_embeddings(torch.zeros(3, 64), [0, 1, 2])
    assert img_t.calls == 0
    with pytest.raises(ValueError, match='nothing to classify'):
        zs.compute()                                                  # none of the refused calls stored anything
    with pytest.raises(RuntimeError, match='stand-in tower reached'):
        zs.update(images, [0, 1, 2, 3])                               # well-formed: reaches the image tower
    assert img_t.calls == 1
    # from_model goes through the tower pair of a model
    from test_host_logic_cpu import _tiny_students
    s_img, s_txt = _tiny_students()
    clip = CLIPModel(True, s_img, s_txt)
    assert ZeroShotClassifier.from_model(clip, max_batch=64).text_encoder is s_txt

    class Holder:                                                     # what a two-tower distillation model exposes
        student = clip
    assert ZeroShotClassifier.from_model(Holder()).image_encoder is s_img
    with pytest.raises(ValueError, match='tower'):
        ZeroShotClassifier.from_model(s_img)
    flags = [(p.requires_grad, m.training) for m in (s_img, s_txt) for p in m.parameters()]
    assert all(r for r, _ in flags) and all(t for _, t in flags)      # building a classifier changes no flag


# ---- 4. the float64 reference --------------------------------------------------------------------------------------------------------
def test_cases_cover_the_stated_sizes():
    col = lambda i: {c[i] for c in tc.CASES}
    assert col(0) == {1, 15, 16, 17, 33, 70}
    assert col(1) == {1, 15, 16, 17, 63, 64, 65, 127, 257, 1000, 4099}
    assert col(2) == {1, 2, 5, 10, 16, 17, 63, 64}
    assert col(3) == {16, 64, 512, 768}
    assert sum(1 for nq, ng, k, E in tc.CASES if k > ng) >= 4 and any(k == ng for nq, ng, k, E in tc.CASES)
    assert tc.SEEDS == (0, 1, 2)
    # both paths of the search are among them: the gallery in one piece, and cut into slices that a second kernel merges
    w = _lib().dclip_topk_search_workspace
    sliced = [w(nq, ng, E, k) > (nq + ng) * E * 4 + 2 * 256 for nq, ng, k, E in tc.CASES]
    assert sum(sliced) >= 3 and sum(not s for s in sliced) >= 10


@pytest.mark.parametrize('nq,ng,k,E', tc.CASES)
def test_reference_order_is_the_brute_force_sort(nq, ng, k, E):
    """every GPU case, every seed: the stable argsort of -L is the sort of (-L, index) pairs, and the reference's own top k passes the
    checker it is used with (scores taken as the rounded float64 logits)"""
    for seed in tc.SEEDS:
        q, gal, L, order = tc.reference(nq, ng, E, seed)
        assert q.shape == (nq, E) and gal.shape == (ng, E) and L.shape == (nq, ng)
        assert np.array_equal(order, tc.brute_order(L))
        m = min(k, ng)
        idx = np.full((nq, k), -1, dtype=np.int32)
        idx[:, :m] = order[:, :m]
        score = np.full((nq, k), -np.inf, dtype=np.float32)
        score[:, :m] = np.take_along_axis(L, order[:, :m], axis=1)
        if not (score[:, 1:m] == score[:, :m - 1]).any():              # (rounding to f32 may merge two neighbours out of index order)
            differ, err = tc.check_against_float64(idx, score, L, k, E)
            assert differ == 0 and err <= 2.0 ** -24


def test_checker_catches_a_wrong_answer():
    q, gal, L, order = tc.reference(17, 257, 64, 0)
    k = 10
    idx = order[:, :k].astype(np.int32)
    score = np.take_along_axis(L, order[:, :k], axis=1).astype(np.float32)
    tc.check_against_float64(idx, score, L, k, 64)
    bad = idx.copy()
    bad[3, 0] = order[3, 200]                                          # the best is missing, an intruder in its place
    with pytest.raises(AssertionError):
        tc.check_against_float64(bad, score, L, k, 64)
    bad = idx.copy()
    bad[5, 4] = bad[5, 3]
    with pytest.raises(AssertionError, match='twice'):
        tc.check_against_float64(bad, score, L, k, 64)
    off = score.copy()
    off[2, 1] += 4 * tc.bound(64)
    with pytest.raises(AssertionError):
        tc.check_against_float64(idx, off, L, k, 64)


def test_planted_construction_is_exact_in_float64():
    q, gal, v = tc.planted_case()
    L = tc.cos64(q, gal)
    assert np.array_equal(L * 4, v.astype(np.float64))                 # the cosines are the stated quarters, exactly
    assert set(np.unique(v)) == {-4, -2, -1, 0, 1, 2, 4}
    idx, score = tc.planted_answer(v, 64)
    assert np.array_equal(idx, tc.order64(L)[:, :64])
    tc.check_order(idx, score, v.shape[1])
    assert (score[:, 1:] == score[:, :-1]).mean() > 0.8                # most neighbours tie: the index order decides


def test_group_mean_reference_and_bound():
    rows = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0], [1.0, 0.0]])
    got = tc.group_mean64(rows, [2, 0, 2])
    assert np.allclose(got, [[0.3, 0.4], [0.0, 0.0], [0.5, -0.5]], atol=1e-15)
    assert tc.group_mean_bound(64, 1) == (2 + 6 + 1 + 3) * tc.U and tc.group_mean_bound(768, 7) == (6 + 6 + 4 + 3) * tc.U

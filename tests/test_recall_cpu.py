"""Recall@K with several captions per image (dclip_retrieval_recall, metrics.retrieval_recall, RetrievalEvaluator), the parts that need no
GPU: the header and the library carry the two entries, the C entry refuses bad arguments on the host before any launch, the counts helper
and the Python layers raise before a tower or a kernel runs, and the float64 interval reference of the GPU tests is itself sound: few
rows have an undecided competitor, and the planted-rank construction gives the integer ranks it states."""
import ctypes

import numpy as np
import pytest
import torch

import recall_cases as rc


def _lib():
    from distillclip_amd._lib import lib
    return lib()


# ---- 1. C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_both_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    P, I = ctypes.c_void_p, ctypes.c_int64
    assert protos['dclip_retrieval_recall_workspace'] == (ctypes.c_size_t, [I, I, I])
    assert protos['dclip_retrieval_recall'] == (ctypes.c_int, [P, P, P, I, I, I, P, ctypes.c_int, P, P, P, P, ctypes.c_size_t, P])
    for name in ('dclip_retrieval_recall_workspace', 'dclip_retrieval_recall'):
        assert hasattr(l._dll, name), name
    assert l.dclip_version() == 6                          # additive: no existing signature changed
    # normalised copies of both row sets, the owner table and the two rank arrays
    n_img, n_txt, E = 5000, 25010, 512
    need = (n_img + n_txt) * E * 4 + (n_img + 2 * n_txt) * 4
    assert need <= l.dclip_retrieval_recall_workspace(n_img, n_txt, E) <= need + 5 * 256


# ---- 2. host refusals ----------------------------------------------------------------------------------------------------------------
# dummy non-null, 16-byte aligned addresses: never dereferenced, every call below is refused before a launch
IMG, TXT, OFF, OUT, RI, RT, WS = 4096, 8192, 12288, 16384, 20480, 24576, 1 << 20


def _call(**k):
    g = lambda name, default: k[name] if name in k else default
    n_img, n_txt, E = g('n_img', 3), g('n_txt', 7), g('E', 64)
    nk = g('nk', 3)
    ks = (ctypes.c_int32 * 16)(*range(1, 17))
    ws_bytes = g('ws_bytes', max(_lib().dclip_retrieval_recall_workspace(n_img, n_txt, E), 16))
    return _lib().dclip_retrieval_recall(g('img', IMG), g('txt', TXT), g('off', OFF), n_img, n_txt, E, g('ks', ks), nk, g('out', OUT),
                                         g('rank_i2t', RI), g('rank_t2i', RT), g('ws', WS), ws_bytes, None)


@pytest.mark.parametrize('kw,word', [
    (dict(E=24), 'multiple of 16'), (dict(E=0), 'multiple of 16'), (dict(E=-16), 'multiple of 16'),
    (dict(nk=9), 'cut-offs'), (dict(nk=-1), 'cut-offs'), (dict(nk=2, ks=None), 'cut-offs'),
    (dict(ws_bytes=1024), 'workspace too small'), (dict(ws_bytes=0), 'workspace too small'),
    (dict(img=None), 'null'), (dict(txt=None), 'null'), (dict(off=None), 'null'), (dict(out=None), 'null'), (dict(ws=None), 'null'),
    (dict(n_img=0), 'n_img'), (dict(n_txt=0), 'n_txt'), (dict(n_img=1 << 24), '2\\^24'), (dict(n_txt=1 << 24), '2\\^24'),
    (dict(img=IMG + 4), '16-byte aligned'), (dict(txt=TXT + 8), '16-byte aligned'), (dict(ws=WS + 4), '16-byte aligned'),
    (dict(out=OUT + 2), 'aligned'), (dict(rank_i2t=RI + 1), 'aligned'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word):
        _call(**kw)


def test_workspace_query_of_a_refused_shape_is_zero():
    l = _lib()
    assert l.dclip_retrieval_recall_workspace(0, 5, 64) == 0 and l.dclip_retrieval_recall_workspace(5, 5, 24) == 0
    assert l.dclip_retrieval_recall_workspace(1, 1, 16) > 0


# ---- 3. the counts helper and the Python layers --------------------------------------------------------------------------------------
def test_caption_offsets():
    from distillclip_amd.metrics import caption_offsets
    assert caption_offsets([2, 0, 3], 3, 5) == [0, 2, 2, 5]
    assert caption_offsets(torch.tensor([2, 0, 3]), 3, 5) == [0, 2, 2, 5]
    assert caption_offsets(np.array([1, 1]), 2, 2) == [0, 1, 2]
    with pytest.raises(ValueError, match='2 caption counts for 3 images'):
        caption_offsets([2, 3], 3, 5)
    with pytest.raises(ValueError, match='negative'):
        caption_offsets([6, -1, 0], 3, 5)
    with pytest.raises(ValueError, match='sum to 4'):
        caption_offsets([2, 0, 2], 3, 5)


def test_retrieval_recall_raises_on_the_host():
    """CPU tensors: a call that got as far as the kernel would raise the no-CPU-path RuntimeError, so a ValueError shows the check came
    first"""
    from distillclip_amd.metrics import retrieval_recall
    img, txt = torch.zeros(3, 64), torch.zeros(5, 64)
    with pytest.raises(ValueError, match='sum to 4'):
        retrieval_recall(img, txt, [2, 0, 2])
    with pytest.raises(ValueError, match='caption counts for 3 images'):
        retrieval_recall(img, txt, [5])
    with pytest.raises(ValueError, match='negative'):
        retrieval_recall(img, txt, [6, -1, 0])
    with pytest.raises(ValueError, match='9 cut-offs'):
        retrieval_recall(img, txt, [2, 0, 3], k_list=range(1, 10))
    with pytest.raises(ValueError, match='multiple of 16'):
        retrieval_recall(torch.zeros(3, 24), torch.zeros(5, 24), [2, 0, 3])
    with pytest.raises(ValueError, match='matrices'):
        retrieval_recall(img, torch.zeros(5, 32), [2, 0, 3])
    with pytest.raises(ValueError, match='n_img, n_txt'):
        retrieval_recall(img, torch.zeros(0, 64), [0, 0, 0])
    with pytest.raises(RuntimeError, match='no CPU path'):
        retrieval_recall(img, txt, [2, 0, 3])                       # as every other wrapper: there is no CPU path


def _evaluator(**kw):
    from test_host_logic_cpu import _tiny_students
    from distillclip_amd import RetrievalEvaluator
    s_img, s_txt = _tiny_students()
    return RetrievalEvaluator(s_img, s_txt, **kw), s_img, s_txt


def test_evaluator_is_exported_and_raises_on_the_host():
    import distillclip_amd
    from distillclip_amd.retrieval import RetrievalEvaluator
    from distillclip_amd.model.component.clip_model import CLIPModel
    assert distillclip_amd.RetrievalEvaluator is RetrievalEvaluator
    ev, s_img, s_txt = _evaluator(k_list=(1, 3), max_batch=7)
    assert ev.image_encoder is s_img and ev.text_encoder is s_txt and ev.k_list == (1, 3) and ev.max_batch == 7
    with pytest.raises(ValueError, match='max_batch'):
        _evaluator(max_batch=0)
    with pytest.raises(ValueError, match='cut-offs'):
        _evaluator(k_list=range(9))
    B, L = 4, 13
    images = torch.zeros(B, 3, 32, 32)
    caps = torch.ones(6, L, dtype=torch.int64)
    with pytest.raises(ValueError, match='sum to 5'):
        ev.update(images, caps, [1, 2, 0, 2])
    with pytest.raises(ValueError, match='3 caption counts for 4 images'):
        ev.update(images, caps, [3, 1, 2])
    with pytest.raises(ValueError, match='need counts'):
        ev.update(images, caps)
    with pytest.raises(ValueError, match='dense'):
        ev.update(images, torch.ones(3, 2, L, dtype=torch.int64))
    with pytest.raises(ValueError, match='disagrees'):
        ev.update(images, torch.ones(B, 2, L, dtype=torch.int64), [1, 3, 2, 2])
    with pytest.raises(ValueError, match='images'):
        ev.update(images[0], caps, [6])
    with pytest.raises(ValueError, match='sum to 4'):
        ev.add_embeddings(torch.zeros(3, 64), torch.zeros(5, 64), [2, 0, 2])
    with pytest.raises(RuntimeError, match='no CPU path'):
        ev.add_embeddings(torch.zeros(3, 64), torch.zeros(5, 64), [2, 0, 3])
    with pytest.raises(ValueError, match='nothing to rank'):
        ev.compute()                                                  # none of the refused calls stored anything
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ev.update(images, caps, [3, 1, 0, 2])                         # well-formed: reaches the towers, which have no CPU path
    clip = CLIPModel(True, s_img, s_txt)
    assert RetrievalEvaluator.from_model(clip, max_batch=64).text_encoder is s_txt

    class Holder:                                                     # what a two-tower distillation model exposes
        student = clip
    assert RetrievalEvaluator.from_model(Holder()).image_encoder is s_img
    with pytest.raises(ValueError, match='tower'):
        RetrievalEvaluator.from_model(s_img)
    flags = [(p.requires_grad, m.training) for m in (s_img, s_txt) for p in m.parameters()]
    assert all(r for r, _ in flags) and all(t for _, t in flags)      # building an evaluator changes no flag


# ---- 4. the float64 interval reference -----------------------------------------------------------------------------------------------
def test_derived_bound_is_below_the_stand_in():
    for _, E in rc.SHAPES:
        assert rc.bound(E) == (2 * E + 8) * 2.0 ** -24 <= (3 * E + 16) * 2.0 ** -24


@pytest.mark.parametrize('seed', rc.SEEDS)
@pytest.mark.parametrize('n_img,E', rc.SHAPES)
def test_few_rows_have_an_undecided_competitor(n_img, E, seed):
    """a condition of the GPU test, from float64 alone: at most 2 % of the ranked rows of a case have any undecided competitor"""
    img, txt, counts, iv = rc.reference(n_img, E, seed)
    lo_i, hi_i, lo_t, hi_t = iv
    assert img.shape == (n_img, E) and txt.shape == (sum(counts), E) and len(counts) == n_img
    frac, ranked = rc.undecided_fraction(iv)
    assert ranked == sum(1 for c in counts if c) + sum(counts)
    assert frac <= rc.UNDECIDED_CAP, (frac, ranked)
    assert ((lo_i == -1) == (np.asarray(counts) == 0)).all() and (lo_t >= 0).all()
    assert (hi_i < max(sum(counts), 1)).all() and (hi_t < n_img).all()
    if n_img == 130:
        assert 0 in counts and max(counts) > 32
    if (n_img, E) == (130, 64):                            # the ranks are not trivially 0: most captions have an image ahead of theirs
        assert (lo_t > 0).mean() > 0.5 and lo_t.max() > 100 and (lo_i > 0).any()


def test_planted_construction_gives_the_stated_integer_ranks():
    """the float64 cosines of the planted case, ranked with a margin no rounding reaches, give the planned ranks of both directions"""
    img, txt, counts, rank_i, rank_t = rc.planted_case()
    L = rc.cos64(img, txt)
    lo_i, hi_i, lo_t, hi_t = rc.intervals(L, counts, 1e-6)
    assert (lo_i == hi_i).all() and (lo_t == hi_t).all()               # nothing within 4e-6 of its target: never a tie
    assert (lo_i == rank_i).all() and (lo_t == rank_t).all()
    assert rank_t.max() >= 30 and (rank_t == 0).sum() >= 5 and rank_i.max() > 0 and (rank_i == -1).sum() == 8

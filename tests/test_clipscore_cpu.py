"""L-CLIPScore scoring (dclip_clipscore, ops.clipscore, distillclip_amd.score.LCLIPScore), the parts that need no GPU: the header and the
library carry the new entry, its argument checks run on the host before any launch, the Python layers refuse CPU tensors and malformed
shapes before a tower runs."""
import ctypes

import pytest
import torch


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def test_header_declares_and_library_exports_clipscore():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    assert 'dclip_clipscore' in protos and hasattr(l._dll, 'dclip_clipscore')
    res, args = protos['dclip_clipscore']
    P, I = ctypes.c_void_p, ctypes.c_int64
    assert res is ctypes.c_int and args == [P, I, P, I, P, I, P, I, I, I, I, ctypes.c_float, P, P, P, P]
    assert l.dclip_version() == 6                          # additive: no existing signature changed


# dummy non-null, 16-byte aligned addresses: never dereferenced, every call below is refused before a launch
IMG, CAND, REFS, OFF, O1, O2, O3 = 4096, 8192, 12288, 16384, 20480, 24576, 28672


def _call(**k):
    g = lambda name, default: k[name] if name in k else default
    E = g('E', 64)
    return _lib().dclip_clipscore(g('img', IMG), g('ld_img', E), g('cand', CAND), g('ld_cand', E), g('refs', REFS), g('ld_ref', E),
                                  g('off', OFF), g('B', 3), g('K', 2), g('R', 5), E, 2.5, g('clip_s', O1), g('ref_s', O2),
                                  g('refclip_s', O3), None)


NO_REFS = dict(refs=None, off=None, ref_s=None, refclip_s=None, R=0)


@pytest.mark.parametrize('kw,word', [
    (dict(img=None), 'null'), (dict(cand=None), 'null'), (dict(clip_s=None), 'null'),
    (dict(B=0), 'B >= 1'), (dict(K=0), 'K >= 1'), (dict(R=-1), 'R >= 0'),
    (dict(E=62), 'multiple of 4'), (dict(E=1028), 'multiple of 4'), (dict(E=0), 'multiple of 4'),
    (dict(ld_img=60), 'stride'), (dict(ld_cand=60), 'stride'), (dict(ld_ref=60), 'stride'),
    (dict(ld_img=66), 'stride'), (dict(ld_cand=66), 'stride'), (dict(ld_ref=66), 'stride'),
    (dict(img=IMG + 4), 'misaligned'), (dict(cand=CAND + 8), 'misaligned'), (dict(refs=REFS + 4), 'misaligned'),
    (dict(off=None), 'come together'), (dict(refs=None), 'come together'),
    (dict(NO_REFS, ref_s=O2), 'without refs'), (dict(NO_REFS, refclip_s=O3), 'without refs'),
], ids=lambda v: '-'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_bad_arguments_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word):
        _call(**kw)


def test_ops_clipscore_has_no_cpu_fallback():
    from distillclip_amd import ops
    img, cand = torch.zeros(2, 8), torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.clipscore(img, cand)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.clipscore(img, cand, torch.zeros(3, 8), torch.zeros(3, dtype=torch.int32), K=1)


def _scorer(**kw):
    from test_host_logic_cpu import _tiny_students
    from distillclip_amd import LCLIPScore
    s_img, s_txt = _tiny_students()
    return LCLIPScore(s_img, s_txt, **kw), s_img, s_txt


def test_scorer_is_exported_and_keeps_its_towers():
    import distillclip_amd
    from distillclip_amd.score import LCLIPScore, ScoreOutput
    assert distillclip_amd.LCLIPScore is LCLIPScore and distillclip_amd.ScoreOutput is ScoreOutput
    assert ScoreOutput._fields == ('clip_s', 'ref_s', 'refclip_s')
    sc, s_img, s_txt = _scorer(w=2.0, max_batch=7)
    assert sc.image_encoder is s_img and sc.text_encoder is s_txt and sc.w == 2.0 and sc.max_batch == 7
    with pytest.raises(ValueError, match='max_batch'):
        _scorer(max_batch=0)


def test_scorer_raises_shape_errors_on_the_host():
    """CPU tensors: a tower that ran would raise the no-CPU-fallback RuntimeError, so a ValueError shows the check came first"""
    sc, _, _ = _scorer()
    B, K, L = 4, 3, 13
    images = torch.zeros(B, 3, 32, 32)
    cand = torch.ones(B, K, L, dtype=torch.int64)
    refs = torch.ones(6, L, dtype=torch.int64)
    with pytest.raises(ValueError, match='sum to 5'):
        sc(images, cand, refs, [1, 2, 0, 2])                          # sum(ref_counts) != R
    with pytest.raises(ValueError, match='negative'):
        sc(images, cand, refs, [3, -1, 2, 2])
    with pytest.raises(ValueError, match='3 reference counts for 4 images'):
        sc(images, cand, refs, [3, 1, 2])                             # len(ref_counts) != B
    with pytest.raises(ValueError, match='3 reference counts for 4 images'):
        sc(images, cand, refs, torch.tensor([3, 1, 2]))               # (a CPU int tensor is a host list)
    with pytest.raises(ValueError, match='candidates'):
        sc(images, cand[:3], refs, [3, 1, 0, 2])                      # candidates.shape[0] != B
    with pytest.raises(ValueError, match='candidates'):
        sc(images, cand[:3, 0])
    with pytest.raises(ValueError, match='need ref_counts'):
        sc(images, cand, refs)                                        # 2-D references without ref_counts
    with pytest.raises(ValueError, match='tokens'):
        sc(images, cand, refs[:, :12], [3, 1, 0, 2])
    with pytest.raises(ValueError, match='dense'):
        sc(images, cand, torch.ones(3, 2, L, dtype=torch.int64))
    with pytest.raises(ValueError, match='without references'):
        sc(images, cand, None, [1, 1, 1, 1])
    # well-formed arguments get past the checks and reach the towers, which have no CPU path
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        sc(images, cand, refs, [3, 1, 0, 2])


def test_from_model_takes_a_clip_model_and_rejects_objects_without_towers():
    from test_host_logic_cpu import _tiny_students
    from distillclip_amd import LCLIPScore
    from distillclip_amd.model.component.clip_model import CLIPModel
    s_img, s_txt = _tiny_students()
    clip = CLIPModel(True, s_img, s_txt)
    sc = LCLIPScore.from_model(clip, w=1.0, max_batch=64)
    assert sc.image_encoder is s_img and sc.text_encoder is s_txt and sc.w == 1.0 and sc.max_batch == 64

    class Holder:                                                     # what a two-tower distillation model exposes
        student = clip
    assert LCLIPScore.from_model(Holder()).text_encoder is s_txt
    with pytest.raises(ValueError, match='tower'):
        LCLIPScore.from_model(object())
    with pytest.raises(ValueError, match='tower'):
        LCLIPScore.from_model(s_img)                                  # a single tower (what a one-tower DistillModel holds as its student)
    flags = [(p.requires_grad, m.training) for m in (s_img, s_txt) for p in m.parameters()]
    assert all(r for r, _ in flags) and all(t for _, t in flags)      # building a scorer changes no flag

"""Frozen CLIP teachers above 128 tokens (ViT-B/16: 197, ViT-L/14: 257, ViT-L/14@336px: 577), the parts that need no GPU: the header and
the library carry the new entries (dclip_attn_stream_fwd, dclip_im2row_ld), their argument checks and the encoder plan run on the host,
`teacher_load` builds the towers, the float64 references of tests/test_attn_stream_gpu.py hold their own premises, and the MFMA operand
check of tools/asm/mfma_hazard.py passes on the new kernel of the shipped code object."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, 'distillclip_amd', 'libdistillclip_hip.so')
NEW_ENTRIES = ('dclip_attn_stream_fwd', 'dclip_im2row_ld')


def _lib():
    from distillclip_amd._lib import lib
    return lib()


def _cfg(**kw):
    from distillclip_amd.model.component._tower import EncoderCfg
    base = dict(kind=0, modality=0, tokens=197, width=768, heads=12, layers=2, repeats=1, mlp_dim=3072, out_dim=512, patch=16, resolution=224,
                in_chans=3, vocab=0, embed_rank=0, head_mix=0, causal=0)
    base.update(kw)
    return EncoderCfg(**base)


def _create(**kw):
    """-> (handle or None, last error)"""
    l = _lib()
    h = l.dclip_encoder_create(ctypes.byref(_cfg(**kw)))
    return h, l.dclip_last_error_string().decode()


# ---- header and library -----------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_entries():
    from distillclip_amd._lib import _HEADER, _parse_header
    protos = _parse_header(_HEADER)
    l = _lib()
    for name in NEW_ENTRIES:
        assert name in protos, name
        assert hasattr(l._dll, name), name
    # the same arguments as dclip_attn_fused_fwd minus `causal`
    fused, stream = protos['dclip_attn_fused_fwd'][1], protos['dclip_attn_stream_fwd'][1]
    assert len(stream) == len(fused) - 1 and stream[:9] == fused[:9] and stream[-1] is ctypes.c_void_p
    assert len(protos['dclip_im2row_ld'][1]) == len(protos['dclip_im2row'][1]) + 1
    assert l.dclip_version() == 6                         # additive: no existing signature changed


def test_stream_entry_refuses_bad_arguments_on_the_host():
    l = _lib()
    H, hd, N = 12, 64, 197
    D = H * hd
    q, c = 4096, 1 << 20                                  # never dereferenced: every call below is refused before a launch
    call = lambda **k: l.dclip_attn_stream_fwd(k.get('q', q), k.get('ldq', 3 * D), k.get('c', c), k.get('ldc', D), 2, H, k.get('N', N), k.get('hd', hd), 0.125, None)
    with pytest.raises(ValueError, match='head dim'):
        call(hd=48)
    with pytest.raises(ValueError, match='head dim'):
        call(hd=32)
    with pytest.raises(ValueError, match='N'):
        call(N=0)
    with pytest.raises(ValueError, match='misaligned'):
        call(ldq=3 * D + 4)
    with pytest.raises(ValueError, match='misaligned'):
        call(ldc=D + 4)
    with pytest.raises(ValueError, match='misaligned'):
        call(q=q + 8)
    with pytest.raises(ValueError, match='misaligned'):
        call(c=c + 8)
    with pytest.raises(ValueError, match='null'):
        call(q=None)
    with pytest.raises(ValueError, match='null'):
        call(c=None)


def test_im2row_ld_refuses_bad_arguments_on_the_host():
    l = _lib()
    call = lambda **k: l.dclip_im2row_ld(k.get('img', 4096), k.get('rows', 8192), k.get('ldk', 640), 2, 3, 224, k.get('patch', 14), k.get('cls', 1), None)
    with pytest.raises(ValueError, match='even'):
        call(patch=7)
    with pytest.raises(ValueError, match='ldk'):
        call(ldk=576)                                     # < 3 * 14 * 14 = 588
    with pytest.raises(ValueError, match='ldk'):
        call(ldk=641)
    with pytest.raises(ValueError, match='cls_rows'):
        call(cls=2)
    with pytest.raises(ValueError):
        call(img=None)
    with pytest.raises(ValueError, match='multiples of 4'):                     # the old entry keeps its contract
        l.dclip_im2row(4096, 8192, 2, 3, 224, 14, 1, None)


# ---- encoder plan -------------------------------------------------------------------------------------------------------------------
LONG_TOWERS = [dict(patch=16, resolution=224, tokens=197, width=768, heads=12, mlp_dim=3072, out_dim=512),
               dict(patch=14, resolution=224, tokens=257, width=1024, heads=16, mlp_dim=4096, out_dim=768),
               dict(patch=14, resolution=336, tokens=577, width=1024, heads=16, mlp_dim=4096, out_dim=768)]


@pytest.mark.parametrize('tower', LONG_TOWERS, ids=lambda t: f"p{t['patch']}r{t['resolution']}")
def test_encoder_create_accepts_long_frozen_image_towers(tower):
    l = _lib()
    h, err = _create(**tower)
    assert h, err
    try:
        assert l.dclip_encoder_workspace_bytes(h, 4, 0) > 0
        assert l.dclip_encoder_wcache_bytes(h) > 0
        assert l.dclip_encoder_last_layer_output_scratch_bytes(h, 4, 0) > 0
    finally:
        l.dclip_encoder_destroy(h)


def test_padded_contraction_shows_in_the_buffer_sizes():
    """patch 14: in_chans * patch^2 = 588 is padded to 640 columns in the cached conv1 weight and in the patch rows; the same tower at
    patch 16 (768 columns, unpadded) tells the sizes apart"""
    l = _lib()
    common = dict(width=128, heads=2, layers=1, mlp_dim=512, out_dim=64)
    sizes = {}
    for patch, res in ((14, 56), (16, 64)):                 # 17 tokens each
        h, err = _create(patch=patch, resolution=res, tokens=17, **common)
        assert h, err
        sizes[patch] = (l.dclip_encoder_wcache_bytes(h), l.dclip_encoder_workspace_bytes(h, 4, 0))
        l.dclip_encoder_destroy(h)
    assert sizes[16][0] - sizes[14][0] == 128 * (768 - 640) * 2
    assert sizes[16][1] - sizes[14][1] == 4 * 17 * (768 - 640) * 2


@pytest.mark.parametrize('kw,word', [
    (dict(kind=1, head_mix=1), 'trainable'), (dict(kind=2), 'trainable'),
    (dict(modality=1, tokens=129, vocab=1000, causal=1, width=512, heads=8, mlp_dim=2048), 'text'),
    (dict(patch=8, resolution=200, tokens=626, causal=1), 'causal'),
    (dict(patch=8, resolution=200, tokens=626, width=128, heads=4, mlp_dim=512), 'head-dim-32'),
    (dict(patch=8, resolution=208, tokens=677), '1..640'),
    (dict(patch=14, resolution=224, tokens=257, kind=2, width=1024, heads=16, mlp_dim=4096), 'trainable'),
    (dict(patch=7, resolution=56, tokens=65), 'even'),
])
def test_encoder_create_still_refuses(kw, word):
    h, err = _create(**kw)
    if h:
        _lib().dclip_encoder_destroy(h)
    assert not h and word in err, (kw, err)


def test_encoder_create_refuses_641_tokens_and_names_the_case():
    # no square grid gives exactly 641 tokens: the token-count check comes before the geometry check, which is what this pins
    h, err = _create(tokens=641)
    assert not h and '1..640' in err and 'frozen image tower' in err, err
    h, err = _create(tokens=197, kind=1, head_mix=1)
    assert not h and 'kind 1' in err, err
    h, err = _create(tokens=197, kind=2)
    assert not h and 'kind 2' in err, err


def test_existing_configurations_keep_their_workspace():
    """the frozen ViT-B/32 teacher of every shipped config: sizes as on the parent commit (unpadded K = 3072, tokens 50)"""
    l = _lib()
    h, err = _create(patch=32, resolution=224, tokens=50)
    assert h, err
    B, N, D, F, K = 4, 50, 768, 3072, 3072
    up = lambda x: (x + 255) // 256 * 256
    M = B * N
    want = (up(M * D * 2) + up(M * D * 2) + up(M * 3 * D * 2) + up(M * D * 2) + up(M * F * 2)            # xs, h1, qkv, ctx, u
            + up(B * D * 2) + 3 * up(B * D * 2)                                                           # compact ctx, xin, x_mid, xout
            + up(M * K * 2) + up(N * D * 4) + up(B * 4) + 2 * up(B * 4) + up(B * D * 2) + up(M * D * 2))  # patches, tok_table, pick, stats, hf, x0
    assert l.dclip_encoder_workspace_bytes(h, B, 0) == want
    l.dclip_encoder_destroy(h)


# ---- Python surface -----------------------------------------------------------------------------------------------------------------
def test_arch_table_and_available_models():
    from distillclip_amd.model import utils
    assert utils._ARCH['ViT-L/14@336px'] == (1024, 24, 14, 336, 768, 12, 768)
    for name in ('ViT-B/16', 'ViT-L/14', 'ViT-L/14@336px'):
        assert name in utils.available_models() and name in utils._ARCH
    doc = utils.available_models.__doc__
    assert 'at most 128 tokens' not in doc and '640' in doc


def test_teacher_load_vit_b16_builds_and_refuses_maps_on_the_host(monkeypatch):
    from distillclip_amd.model.utils import teacher_load
    from distillclip_amd.model.component._tower import EncoderRun, _maps_desc, _ptr_array
    monkeypatch.setenv('DCLIP_SYNTHETIC_TEACHER', '1')
    clip = teacher_load('ViT-B/16', None, 'all')
    tower = clip.image_encoder._tower
    assert tower.cfg.tokens == 197 and tower.cfg.patch == 16 and tower.cfg.width == 768 and tower.cfg.kind == 0
    assert clip.image_encoder.visual.positional_embedding.shape == (197, 768)
    l = _lib()
    assert l.dclip_encoder_workspace_bytes(tower._handle, 4, 0) > 0
    # a maps request: refused by dclip_encoder_forward before it reads any buffer (the pointers below are never dereferenced)
    ex = (ctypes.c_int32 * 1)(0)
    desc, keep = _maps_desc([0])
    desc.score = ctypes.cast((ctypes.c_void_p * 1)(4096), ctypes.c_void_p)
    run = EncoderRun()
    params = (ctypes.c_void_p * len(tower.param_names))()
    with pytest.raises(ValueError, match='dclip_attn_maps'):
        l.dclip_encoder_forward(tower._handle, 4096, None, 1, params, 4096, 4096, 1 << 30, ctypes.byref(run), 0, 4096, None, None, 0,
                                ctypes.byref(desc), None)


def test_teacher_load_from_a_state_dict_of_vit_l_shapes():
    """the shape sniffers (utils.get_visual_para) read patch 14, 257 tokens, width 1024 from the tensors: two layers keep it small"""
    from distillclip_amd import synth
    from distillclip_amd.model.utils import teacher_load
    sd = {k: torch.from_numpy(v) for k, v in synth.teacher_image_state(3, 1024, 2, 14, 224, 768).items()}
    enc = teacher_load('ViT-L/14', None, 'image', state_dict=sd)
    cfg = enc._tower.cfg
    assert (cfg.tokens, cfg.patch, cfg.width, cfg.heads, cfg.out_dim, cfg.layers) == (257, 14, 1024, 16, 768, 2)
    sd = {k: torch.from_numpy(v) for k, v in synth.teacher_image_state(3, 1024, 1, 14, 336, 768).items()}
    assert teacher_load('ViT-L/14@336px', None, 'image', state_dict=sd)._tower.cfg.tokens == 577


def test_rows_are_shared_only_between_towers_that_cut_alike():
    """_tower._shared_rows_for: the key of a share is (image, patch, channels, resolution) and rows of C p^2 values, a multiple of 64"""
    from types import SimpleNamespace as NS
    from distillclip_amd.model.component import _tower
    x = torch.zeros(2, 3, 224, 224)
    rows = torch.zeros(2 * 50, 3072, dtype=torch.bfloat16)
    entry = dict(key=(x.data_ptr(), tuple(x.shape), x._version), patch=32, chans=3, res=224, rows=rows, stream=None)
    cfg = lambda **k: NS(**dict(dict(modality=0, patch=32, in_chans=3, tokens=50), **k))
    _tower._SHARE.entry = entry
    try:
        assert _tower._shared_rows_for(x, cfg(patch=16, tokens=197)) is None            # a ViT-B/16 teacher beside a patch-32 student
        assert _tower._shared_rows_for(x, cfg(tokens=101)) is None                      # another grid
        assert _tower._shared_rows_for(x, cfg(modality=1)) is None
        entry['rows'] = torch.zeros(2 * 50, 588, dtype=torch.bfloat16)                  # rows a tower would have to pad
        assert _tower._shared_rows_for(x, cfg()) is None
    finally:
        _tower._SHARE.entry = None


# ---- the float64 references of the kernel tests ----------------------------------------------------------------------------------
def test_stream_selection_cases_hold_their_premises():
    import test_attn_stream_gpu as sx
    n = 0
    for c in sx.selection_cases():                           # (the builders assert gap, chunk coverage, distinct rows)
        n += 1
        assert c.gap * sx.LOG2E > 288 and torch.equal(c.expect.to(sx.BF16).double(), c.expect)
    assert n == len(sx.ALL_N) + 1
    assert {129, 144, 145, 197, 257, 577} <= set(sx.ALL_N)
    for t in (2, 3, 4, 9):                                   # one N just below and one just above chunk multiples
        assert sx.KC * t - 1 in sx.ALL_N and sx.KC * t + 1 in sx.ALL_N


def test_stream_uniform_cases_are_sensitive_to_one_key():
    import test_attn_stream_gpu as sx
    n = 0
    for c in sx.uniform_cases():
        n += 1
        assert (c.bound > 0).any() and c.q.abs().max().item() == 0
    assert n == len(sx.ALL_N)
    # the check itself can fail: values too small for a single key to show
    v = torch.zeros(1, 1, 197, 64, dtype=torch.float64, device=sx.DEV)
    v[0, 0, 0] = 100
    tot = v.sum(2, keepdim=True)
    y = tot / 197
    assert sx.UniformCase._insensitive(v, tot, y, sx.ax.store_bound(y, 3 * sx.U24 * y.abs(), sx.BF16), 197) is not None


def test_stream_real_reference_is_the_softmax_product():
    import test_attn_stream_gpu as sx
    for N in (129, 197, 257, 577):
        c = sx.RealCase(1, 2, N, 800 + N)                    # (asserts: chunked carry == plain softmax without the bf16 rounding)
        plain = torch.softmax(c.q @ c.k.transpose(-1, -2) * 0.125, -1) @ c.v
        assert ((c.y - plain).abs() <= c.bound).all()       # the bf16 rounding of e alone stays inside the bound
        assert c.moves > 0 and (c.bound < 0.05 * (1 + c.y.abs())).all()


# ---- the shipped code object ---------------------------------------------------------------------------------------------------------
def test_mfma_hazard_check_passes_on_the_stream_kernel():
    if not os.path.exists(SO):
        pytest.skip('library not built')
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'asm'))
    import mfma_hazard as H
    res = H.check_text(H.disassemble_so(SO))
    fam = {k: v for k, v in res.items() if 'attn_stream_fwd_kernel' in H.demangle(k)}
    assert len(fam) == 1
    for k, v in fam.items():
        n_mfma = sum(1 for x in v['insns'] if x.op.startswith('v_mfma'))
        assert n_mfma >= 16, (H.demangle(k), n_mfma)
        assert not v['valu_built'], (H.demangle(k), 'VALU-built MFMA operand overwritten inside the window')
        assert not v['violations'], (H.demangle(k), H.describe(v['insns'], v['violations'][0], 8))

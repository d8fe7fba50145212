"""Head-mean attention maps (attention_score_mse / attention_probs_mse) without a GPU: the loss accepts both terms and asks for the maps,
the C ABI declares and exports the new entries, and the encoder refuses bad map requests on the host, before any launch."""
import ctypes
import re

import pytest


def test_loss_calculator_accepts_the_attention_map_terms():
    from distillclip_amd.model._loss import LossCalculator
    lc = LossCalculator(['out_l1', 'attention_score_mse', 'attention_probs_mse'])
    co = lc.get_control_output()
    assert co.need_attn_score and co.need_attn_prob and not (co.need_rep or co.need_emb or co.need_value_map)
    co = LossCalculator(['attention_probs_mse']).get_control_output()
    assert co.need_attn_prob and not co.need_attn_score
    for n in ('attention_probs_kl', 'last_value_map_kl', 'vit_kd', 'smd', 'fine_grain'):
        with pytest.raises(NotImplementedError):
            LossCalculator([n])


def test_value_maps_are_still_refused():
    from distillclip_amd.model.component.output import ControlOutput
    from distillclip_amd.model.component._tower import refuse_attention_maps, map_request
    refuse_attention_maps(ControlOutput(need_attn_score=True, need_attn_prob=True))
    with pytest.raises(NotImplementedError):
        refuse_attention_maps(ControlOutput(need_value_map=True))
    assert map_request(ControlOutput(), range(4)) is None
    assert map_request(ControlOutput(need_attn_prob=True), range(4), 2) == (False, True, [0, 1])
    assert map_request(ControlOutput(need_attn_score=True), [0, 1, 10, 11]) == (True, False, [0, 1, 10, 11])


def test_header_declares_and_library_exports_the_map_entries():
    from distillclip_amd._lib import lib, _HEADER
    src = open(_HEADER).read()
    names = ['dclip_attn_maps_fwd', 'dclip_attn_maps_bwd', 'dclip_attn_maps_bwd_workspace_bytes', 'dclip_encoder_forward',
             'dclip_encoder_backward']
    for n in names:
        assert re.search(r'\b' + n + r'\s*\(', src), n
        assert hasattr(lib()._dll, n), n
    assert 'typedef struct dclip_attn_maps' in src
    # one forward and one backward entry per tower, each taking input / patches and the nullable maps descriptor
    protos = lib().protos
    assert len(protos['dclip_encoder_forward'][1]) == 16 and len(protos['dclip_encoder_backward'][1]) == 17
    assert len(protos['dclip_encoder_last_layer_output'][1]) == 11
    assert re.search(r'dclip_encoder_forward\([^)]*const void\* patches[^)]*const dclip_attn_maps\* maps', src)
    assert re.search(r'dclip_encoder_backward\([^)]*const void\* patches[^)]*const dclip_attn_maps\* maps', src)


def test_maps_workspace_size():
    from distillclip_amd._lib import lib
    l = lib()
    # one [H, H] f32 partial per workgroup of 4 query rows, rounded up to 256 bytes
    assert l.dclip_attn_maps_bwd_workspace_bytes(512, 24, 50) == 512 * 13 * 24 * 24 * 4
    assert l.dclip_attn_maps_bwd_workspace_bytes(3, 2, 13) == 256
    assert l.dclip_attn_maps_bwd_workspace_bytes(0, 2, 13) == 0


def test_kernel_arguments_are_checked_on_host():
    from distillclip_amd._lib import lib
    l = lib()
    with pytest.raises(ValueError, match='head dim'):
        l.dclip_attn_maps_fwd(256, 3 * 4 * 48, None, 256, None, 2, 4, 13, 48, 1.0, 0, None)
    with pytest.raises(ValueError, match='N <= 128'):
        l.dclip_attn_maps_fwd(256, 3 * 4 * 32, None, 256, None, 2, 4, 129, 32, 1.0, 0, None)
    with pytest.raises(ValueError, match='qkv rows'):
        l.dclip_attn_maps_fwd(256, 4 * 32, None, 256, None, 2, 4, 13, 32, 1.0, 0, None)
    with pytest.raises(ValueError, match='workspace'):
        l.dclip_attn_maps_bwd(256, 3 * 4 * 32, 256, None, 256, 256, 1, 256, None, 0, 2, 4, 13, 16, 32, 1.0, 0, None)


def _handle(**kw):
    from distillclip_amd._lib import lib
    from distillclip_amd.model.component._tower import EncoderCfg
    cfg = dict(kind=1, modality=0, tokens=17, width=128, heads=4, layers=2, repeats=2, mlp_dim=512, out_dim=64, patch=8,
               resolution=32, in_chans=3, vocab=0, embed_rank=0, head_mix=1, causal=0)
    cfg.update(kw)
    c = EncoderCfg(**cfg)
    h = lib().dclip_encoder_create(ctypes.byref(c))
    assert h
    return h


def test_encoder_refuses_bad_map_requests_on_host():
    from distillclip_amd._lib import lib
    from distillclip_amd.model.component._tower import _maps_desc, EncoderRun
    l = lib()
    fake = 1 << 20                                    # never dereferenced: every refusal below happens before a launch
    run = ctypes.byref(EncoderRun())                  # a record no forward has written

    class Buf:                                        # stands for a device tensor in the descriptor's pointer arrays
        def data_ptr(self):
            return fake
    buf = Buf()
    params = (ctypes.c_void_p * 64)(*([fake] * 64))
    h = _handle()
    try:
        ws = l.dclip_encoder_workspace_bytes(h, 2, 1)
        bad, keep = _maps_desc([4], score=[buf])     # 2 layers x 2 repeats: executions 0..3
        neg, keep2 = _maps_desc([-1], prob=[buf])
        far, keep6 = _maps_desc([64], score=[buf])   # beyond the record's 64 bits too: the range check comes first
        d, keep3 = _maps_desc([1], d_prob=[buf])     # a gradient for a map no forward of this workspace exported
        # the same refusals whether the image tower converts `input` itself or takes caller-cut patch rows
        for inp, rows in ((fake, None), (None, fake)):
            for m in (bad, neg, far):
                with pytest.raises(ValueError, match='out of range'):
                    l.dclip_encoder_forward(h, inp, rows, 2, params, fake, fake, ws, run, 1, fake, None, None, 0, ctypes.byref(m), None)
            with pytest.raises(ValueError, match='did not export'):
                l.dclip_encoder_backward(h, inp, rows, 2, params, params, fake, fake, ws, run, fake, None, None, ctypes.byref(d), None, None,
                                         None)
        # neither input nor patch rows
        with pytest.raises(ValueError, match='null argument'):
            l.dclip_encoder_forward(h, None, None, 2, params, fake, fake, ws, run, 1, fake, None, None, 0, None, None)
        with pytest.raises(ValueError, match='null argument'):
            l.dclip_encoder_backward(h, None, None, 2, params, params, fake, fake, ws, run, fake, None, None, None, None, None, None)
    finally:
        l.dclip_encoder_destroy(h)
    # the causal text teacher's caption-prefix shortcut cannot export maps, and a text tower takes no patch rows
    t = _handle(kind=0, modality=1, tokens=13, heads=2, layers=2, repeats=1, patch=0, resolution=0, in_chans=0, vocab=97, head_mix=0,
                causal=1)
    try:
        ws = l.dclip_encoder_workspace_bytes(t, 2, 0)
        m, keep4 = _maps_desc([0], score=[buf])
        with pytest.raises(ValueError, match='caption prefix'):
            l.dclip_encoder_forward(t, fake, None, 2, params, fake, fake, ws, run, 0, fake, None, None, 5, ctypes.byref(m), None)
        with pytest.raises(ValueError, match='image towers only'):
            l.dclip_encoder_forward(t, None, fake, 2, params, fake, fake, ws, run, 0, fake, None, None, 0, None, None)
        with pytest.raises(ValueError, match='null argument'):
            l.dclip_encoder_forward(t, None, None, 2, params, fake, fake, ws, run, 0, fake, None, None, 0, None, None)
    finally:
        l.dclip_encoder_destroy(t)
    # a trainable text tower: its backward refuses patch rows too
    s = _handle(modality=1, tokens=13, heads=2, patch=0, resolution=0, in_chans=0, vocab=97, head_mix=0, causal=1)
    try:
        ws = l.dclip_encoder_workspace_bytes(s, 2, 1)
        with pytest.raises(ValueError, match='image towers only'):
            l.dclip_encoder_forward(s, None, fake, 2, params, fake, fake, ws, run, 1, fake, None, None, 0, None, None)
        with pytest.raises(ValueError, match='image towers only'):
            l.dclip_encoder_backward(s, None, fake, 2, params, params, fake, fake, ws, run, fake, None, None, None, None, None, None)
    finally:
        l.dclip_encoder_destroy(s)
    # maps together with tokens_eff on patch rows (image towers): patch rows never combine with tokens_eff
    h = _handle(kind=0, repeats=1, head_mix=0)
    try:
        ws = l.dclip_encoder_workspace_bytes(h, 2, 0)
        m, keep5 = _maps_desc([0], score=[buf])
        with pytest.raises(ValueError, match='patches cannot be combined with tokens_eff'):
            l.dclip_encoder_forward(h, None, fake, 2, params, fake, fake, ws, run, 0, fake, None, None, 5, ctypes.byref(m), None)
        with pytest.raises(ValueError, match='patches cannot be combined with tokens_eff'):
            l.dclip_encoder_forward(h, None, fake, 2, params, fake, fake, ws, run, 0, fake, None, None, 5, None, None)
    finally:
        l.dclip_encoder_destroy(h)


def test_workspace_sizes_do_not_depend_on_maps():
    """the map buffers and the backward scratch are the caller's: dclip_encoder_workspace_bytes has no maps argument and is unchanged
    (tests/test_cabi_cpu.py pins its values)"""
    from distillclip_amd._lib import lib
    assert len(lib().protos['dclip_encoder_workspace_bytes'][1]) == 3

"""Cases, call sequences and the guarded-buffer rig shared by tests/test_tower_memory_cpu.py and tests/test_tower_memory_gpu.py: the memory
contract of the tower runtime (csrc/encoder.cpp layout(), dclip_encoder_forward / _backward / _last_layer_output).  Not a test module; torch
and the package are imported inside the builders only.

Every tower is tiny (1 or 2 distinct blocks, E = 64) and runs at B in BATCHES.  Students keep N % 8 != 0, so the score tensors have pad
columns N..Np.  `kind`, `mixing` and `causal` are what attn_path() in encoder.cpp decides by; path_of() below mirrors it.
"""
import functools

GUARD = 65536                     # guard bytes on each side of every caller-owned device buffer
GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF, 0x7B)        # byte patterns a workspace is filled with before a run (see test_tower_memory_cpu.py for their readings)
BATCHES = (1, 3, 5)               # one problem; fewer (b, h) problems than a workgroup holds; one more than it holds at H = 2
GRAD_TOL = 2e-5                   # |got - want| <= GRAD_TOL * max|want| per flat range of grad_buckets(): order noise of the f32 atomics in the
                                  # small wgrads and column sums (the bound of tests/test_towers_gpu.py for the same comparison)

S_IMG = dict(img_size=32, patch_size=8, in_chans=3, out_dim=64, embed_dim=128, depth=4, num_heads=4, mlp_ratio=4.0, qkv_bias=True,
             repeated_times=2, use_transform=True)                                     # = test_towers_gpu.TINY['s_img']
S_TXT = dict(vocab_size=97, context_length=13, out_dim=64, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4.0, qkv_bias=False,
             repeated_times=2, use_transform=True)                                     # = test_towers_gpu.TINY['s_txt']
CLIP_EDGE = dict(width=64, heads=1, res=32, patch=8, ctx=13, vocab=211, out_dim=64, layers=2)      # smallest shape of test_clip_student_gpu's edge shapes
TEACHER = dict(seed=11, res=32, patch=8, ctx=13, vocab=97, out_dim=64, width=128, layers=2, heads=2)   # = _tiny_modules' teachers

# tag -> what the tower is.  kind / mixing / causal / tokens are asserted against the built tower's plan by the GPU tests.
CASES = {
    's_img_mix':   dict(build='student_image', cfg=S_IMG, kind=1, modality=0, mixing=True, causal=False, tokens=17, res=32),
    's_txt_mix':   dict(build='student_text', cfg=S_TXT, kind=1, modality=1, mixing=True, causal=False, tokens=13, vocab=97),
    's_txt_rank':  dict(build='student_text', cfg=dict(S_TXT, compression_embedding=True, embedding_compression_dim=64), kind=1, modality=1,
                        mixing=True, causal=False, tokens=13, vocab=97),
    's_img_nomix': dict(build='student_image', cfg=dict(S_IMG, use_transform=False), kind=1, modality=0, mixing=False, causal=False, tokens=17,
                        res=32),
    'c_img':       dict(build='clip_image', cfg=CLIP_EDGE, kind=2, modality=0, mixing=False, causal=False, tokens=17, res=32),
    'c_txt':       dict(build='clip_text', cfg=CLIP_EDGE, kind=2, modality=1, mixing=False, causal=True, tokens=13, vocab=211),
    't_img':       dict(build='teacher_image', cfg=TEACHER, kind=0, modality=0, mixing=False, causal=False, tokens=17, res=32),
    't_txt':       dict(build='teacher_text', cfg=TEACHER, kind=0, modality=1, mixing=False, causal=True, tokens=13, vocab=97),
    # 197 tokens: the streaming attention; patch 14 at 196 px gives the same 197 tokens with rows padded 588 -> 640 (dclip_im2row_ld)
    't_long':      dict(build='teacher_image', cfg=dict(TEACHER, res=112, patch=8, layers=1), kind=0, modality=0, mixing=False, causal=False,
                        tokens=197, res=112),
    't_long_p14':  dict(build='teacher_image', cfg=dict(TEACHER, res=196, patch=14, layers=1), kind=0, modality=0, mixing=False, causal=False,
                        tokens=197, res=196),
}
STUDENTS = tuple(t for t, c in CASES.items() if c['kind'] != 0)
TEACHERS = tuple(t for t, c in CASES.items() if c['kind'] == 0)
KNOB_CASES = ('s_img_mix', 's_txt_mix')                                   # run once more under each of KNOBS, in a child process
KNOBS = ('DCLIP_ATTN_MIX', 'DCLIP_PRUNE_LAST')                            # each read once per process; '0' switches the feature off

# sequence -> (training, the last execution is pruned (with DCLIP_PRUNE_LAST on), what it does)
SEQUENCES = {
    'infer':         (False, True, 'inference forward, last_layer_output'),
    'infer_full':    (False, False, 'inference forward with need_rep of every execution and need_emb, last_layer_output'),
    'infer_prefix':  (False, True, 'inference forward on a caption prefix (tokens_eff < N): the causal text teacher only'),
    'train':         (True, True, 'training forward, backward with d_out'),
    'train_full':    (True, False, 'training forward with need_rep of every execution and need_emb, backward with d_out, d_rep, d_emb'),
    'train_maps':    (True, False, 'score and probability maps of the first and the last execution, backward with their gradients'),
    'train_lastout': (True, True, 'training forward, last_layer_output, backward (image towers: on patch rows the caller made)'),
}


def sequences_of(tag):
    c = CASES[tag]
    if c['kind'] != 0:
        return ('infer', 'infer_full', 'train', 'train_full', 'train_maps', 'train_lastout')
    return ('infer', 'infer_full', 'infer_prefix') if tag == 't_txt' else ('infer', 'infer_full')


def batches_of(tag, seq):
    return BATCHES


# one workspace and one record through changing modes and batch sizes: [(sequence, B)]
CHAIN = (('train', 5), ('infer', 2), ('train_full', 3), ('train', 3), ('train_maps', 1), ('train', 5), ('train_lastout', 3))
CHAIN_CASES = ('s_img_mix', 's_txt_mix', 'c_txt', 's_img_nomix')
TEACHER_CHAIN = (('infer', 5), ('infer', 2), ('infer', 5))
TEACHER_CHAIN_TXT = (('infer', 5), ('infer_prefix', 2), ('infer', 5), ('infer_prefix', 5), ('infer', 2))     # tokens_eff switches between steps


def chain_of(tag):
    if CASES[tag]['kind'] != 0:
        return CHAIN
    return TEACHER_CHAIN_TXT if tag == 't_txt' else TEACHER_CHAIN


def path_of(case, training, attn_mix=True):
    """encoder.cpp attn_path(): the score stage the workspace is laid out for (every mixing case here has a Mix instantiation)"""
    save = training and case['kind'] != 0
    if not save and not case['mixing']:
        return 'Fused'
    if case['mixing'] and attn_mix and not case['causal']:
        return 'Mix'
    return 'Unfused'


def combos(tags, attn_mix=True, prune_last=True):
    """{(kind, AttnPath, pruned, training)} that the sequences of `tags` reach"""
    out = set()
    for tag in tags:
        for seq in sequences_of(tag):
            training, pruned, _ = SEQUENCES[seq]
            out.add((CASES[tag]['kind'], path_of(CASES[tag], training, attn_mix), pruned and prune_last, training))
    return out


# ---- GPU side ------------------------------------------------------------------------------------------------------------------------------
def _T(d):
    import numpy as np
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def build(tag):
    """-> the module of case `tag` on the GPU, its flat buffers materialised (weights from synth, as the existing tower suites build them)"""
    import torch
    from distillclip_amd import synth
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer, ImageEncoder, TextEncoder
    c = CASES[tag]
    cfg, how = c['cfg'], c['build']
    if how == 'student_image':
        m = RepeatVisionTransformer(**cfg)
        m.load_state_dict(_T(synth.student_image_state(11, **cfg)))
    elif how == 'student_text':
        m = RepeatTextTransformer(**cfg)
        m.load_state_dict(_T(synth.student_text_state(11, **cfg)))
    elif how in ('clip_image', 'clip_text'):
        sd_i, sd_t = synth.clip_student_states(177, cfg['width'], cfg['layers'], cfg['patch'], cfg['res'], cfg['ctx'], cfg['vocab'], cfg['out_dim'],
                                               cfg['width'], cfg['width'])
        if how == 'clip_image':
            m = ImageEncoder(True, dict(input_resolution=cfg['res'], patch_size=cfg['patch'], width=cfg['width'], layers=cfg['layers'],
                                        heads=cfg['heads'], output_dim=cfg['out_dim']), cfg['width'])
            m.load_state_dict(_T(sd_i))
        else:
            m = TextEncoder(cfg['width'], cfg['layers'], cfg['heads'], cfg['ctx'], None, cfg['vocab'], cfg['out_dim'],
                            tea_transformer_width=cfg['width'], is_student=True)
            m.load_state_dict(_T(sd_t))
    elif how == 'teacher_image':
        m = ImageEncoder(False, dict(input_resolution=cfg['res'], patch_size=cfg['patch'], width=cfg['width'], layers=cfg['layers'],
                                     heads=cfg['heads'], output_dim=cfg['out_dim'], need_layers=None))
        m.load_state_dict(_T(synth.teacher_image_state(cfg['seed'], cfg['width'], cfg['layers'], cfg['patch'], cfg['res'], cfg['out_dim'])))
    else:
        m = TextEncoder(cfg['width'], cfg['layers'], cfg['heads'], cfg['ctx'], None, cfg['vocab'], cfg['out_dim'], is_student=False)
        m.load_state_dict(_T(synth.teacher_text_state(cfg['seed'], cfg['width'], cfg['layers'], cfg['ctx'], cfg['vocab'], cfg['out_dim'])))
    m = m.cuda()
    m._tower.materialize(torch.device('cuda', torch.cuda.current_device()))
    return m


@functools.lru_cache(maxsize=None)
def inputs(tag, seq, B):
    """-> the device tensors one (case, sequence, B) runs on, the same objects for every run of it: x, and for the training sequences d_out,
    d_rep, d_emb, d_score, d_prob; n_eff for 'infer_prefix'"""
    import torch
    from distillclip_amd import synth
    c = CASES[tag]
    tw = build(tag)._tower
    N, D, E, nex = tw.cfg.tokens, tw.cfg.width, tw.cfg.out_dim, tw.cfg.layers * tw.cfg.repeats
    seed = 1000 + 31 * B + sorted(CASES).index(tag)
    if c['modality'] == 0:
        x = torch.from_numpy(synth.images(seed, B, c['res'])).cuda()
        n_eff = 0
    else:
        caps = synth.captions(seed, B, N, c['vocab'], 3, N - 5)
        n_eff = int((caps != 0).sum(1).max())
        x = torch.from_numpy(caps).cuda()
    g = torch.Generator().manual_seed(seed + sorted(SEQUENCES).index(seq))
    rnd = lambda *shape: torch.randn(shape, generator=g).cuda()
    out = dict(x=x, n_eff=n_eff)
    if SEQUENCES[seq][0]:
        out['d_out'] = rnd(B, E)
    if seq == 'train_full':
        out['d_rep'] = [rnd(B, N, D) for _ in range(nex)]
        out['d_emb'] = rnd(B, N, D)
    if seq == 'train_maps':
        out['d_score'] = [rnd(B, 1, N, N) for _ in range(2)]
        out['d_prob'] = [rnd(B, 1, N, N) for _ in range(2)]
    return out


class Arena:
    """Every buffer taken here lies at the centre of an allocation of its own, exactly as large as asked, with GUARD bytes of GUARD_BYTE on
    each side; its own bytes start as `fill`."""

    def __init__(self, fill):
        self.fill, self.items, self.label, self.count = fill, [], 'setup', 0

    def take(self, shape, dtype, name, fill=None):
        import math
        import torch
        shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((2 * GUARD + n,), GUARD_BYTE, dtype=torch.uint8, device='cuda')
        assert raw.data_ptr() % 256 == 0
        body = raw[GUARD:GUARD + n]
        body.fill_(self.fill if fill is None else fill)
        self.items.append((name, raw, n))
        return body.view(dtype).view(shape)

    def empty(self, *size, dtype=None, device=None):
        """stands in for torch.empty inside _tower.py: the wrapper's outputs and scratch buffers come from here"""
        import torch
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        self.count += 1
        dtype = torch.float32 if dtype is None else dtype
        return self.take(size, dtype, f'{self.label}: buffer {self.count} {tuple(size)} {str(dtype)[6:]}')

    def guard_failures(self):
        """[which buffer, which side, first offset] of every guard byte that changed"""
        import torch
        out = []
        for name, raw, n in self.items:
            for side, seg, base in (('before', raw[:GUARD], -GUARD), ('after', raw[GUARD + n:], n)):
                bad = seg != GUARD_BYTE
                k = int(bad.sum())
                if k:
                    first = int(torch.nonzero(bad)[0])
                    out.append(f'{name} ({n} bytes): {k} guard bytes {side} it changed, first at byte offset {base + first} from its start '
                               f'(now {int(seg[first]):#04x})')
        return out


class _TorchStandIn:
    """the `torch` name inside _tower.py while a sequence runs: empty() hands out guarded buffers, everything else is torch"""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        import torch
        return getattr(torch, name)

    def empty(self, *size, **kw):
        return self._arena.empty(*size, **kw)


class _hooked:
    def __init__(self, arena):
        self.arena = arena

    def __enter__(self):
        from distillclip_amd.model.component import _tower
        self.prev = _tower.torch
        _tower.torch = _TorchStandIn(self.arena)

    def __exit__(self, *exc):
        from distillclip_amd.model.component import _tower
        _tower.torch = self.prev
        return False


def workspace_need(tw, seq, B):
    from distillclip_amd._lib import lib
    return int(lib().dclip_encoder_workspace_bytes(tw._handle, B, 1 if SEQUENCES[seq][0] else 0))


def bits_differ(got, want, what):
    """None, or where two tensors differ bit for bit"""
    import torch
    if got.shape != want.shape or got.dtype != want.dtype:
        return f'{what}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}'
    iv = {4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[got.element_size()]
    bad = got.contiguous().view(iv) != want.contiguous().view(iv)
    k = int(bad.sum())
    if not k:
        return None
    i = tuple(torch.nonzero(bad)[0].tolist())
    return f'{what}: {k} of {bad.numel()} elements differ bit for bit; first at {i}: got {got[i].item()!r} want {want[i].item()!r}'


def run_sequence(tag, seq, B, fill, shared=None, second_backward=None, d_out=None):
    """One sequence on the tower of `tag`, through HipTower.forward / .last_layer_output / .backward.
    shared = None: the workspace is a guarded buffer of exactly dclip_encoder_workspace_bytes, filled with `fill`, with a zeroed record;
    shared = (workspace, record): the step runs on them as they are.  The weight cache (filled with `fill` before prepare()), flat_grad
    (zeroed), every output and every scratch buffer are guarded buffers of exactly their size, filled with `fill`, in both modes.
    second_backward (training sequences): a list of further d_out; after the sequence's own backward each runs a backward of its own on the
    same forward into a zeroed flat_grad (-> 'more_grads').  d_out: used in place of the sequence's own.
    -> dict(fwd={name: CPU tensor}, grad=CPU flat_grad or None, guards=[...], inputs=[...], more_grads=[...])"""
    import torch
    from distillclip_amd.model.component import _tower
    enc = build(tag)
    tw = enc._tower
    inp = inputs(tag, seq, B)
    if d_out is not None:
        inp = dict(inp, d_out=d_out)
    training = SEQUENCES[seq][0]
    nex = tw.cfg.layers * tw.cfg.repeats
    arena = Arena(fill)
    if shared is None:
        tw.workspace, tw._run = arena.take(workspace_need(tw, seq, B), torch.uint8, 'workspace'), _tower.EncoderRun()
    else:
        tw.workspace, tw._run = shared
    ws, rec = tw.workspace, tw._run
    tw.wcache = arena.take(tw.wcache.numel(), torch.uint8, 'wcache')
    tw.wcache_dirty = True
    tw.flat_grad = arena.take(tw.flat.numel(), torch.float32, 'flat_grad', fill=0)
    const = dict(flat=tw.flat, x=inp['x'])
    for k in ('d_out', 'd_emb'):
        if k in inp:
            const[k] = inp[k]
    for k in ('d_rep', 'd_score', 'd_prob'):
        for i, t in enumerate(inp.get(k, [])):
            const[f'{k}[{i}]'] = t
    fwd, grad, more = {}, None, []
    share = None
    with _hooked(arena):
        arena.label = 'forward'
        if seq == 'train_lastout' and tw.cfg.modality == 0:
            share = _tower.shared_image_patches(inp['x'], [tw, tw])            # the caller-made `patches` operand
            assert share.entry is not None
            const['patches'] = share.entry['rows']
            share.__enter__()
        snap = {k: v.clone() for k, v in const.items()}
        try:
            if seq in ('infer', 'train', 'train_lastout'):
                res = tw.forward(inp['x'], training)
            elif seq == 'infer_prefix':
                assert 0 < inp['n_eff'] < tw.cfg.tokens
                res = tw.forward(inp['x'], False, tokens_eff=inp['n_eff'])
            elif seq in ('infer_full', 'train_full'):
                res = tw.forward(inp['x'], training, need_rep=True, need_emb=True)
            else:
                res = tw.forward(inp['x'], True, maps=(True, True, [0, nex - 1]))
        finally:
            if share is not None:
                share.__exit__(None, None, None)
        fwd['last_representation'] = res[0]
        for i, r in enumerate(res[2]):
            fwd[f'rep[{i}]'] = r
        if res[3] is not None:
            fwd['emb'] = res[3]
        for i, t in enumerate(res.scores):
            fwd[f'score[{i}]'] = t
        for i, t in enumerate(res.probs):
            fwd[f'prob[{i}]'] = t
        if seq in ('infer', 'infer_full', 'train_lastout'):
            arena.label = 'last_layer_output'
            fwd['last_layer_output'] = tw.last_layer_output()
        if training:
            arena.label = 'backward'
            kw = {}
            if seq == 'train_full':
                kw = dict(d_reps=inp['d_rep'], d_emb=inp['d_emb'])
            if seq == 'train_maps':
                kw = dict(d_maps=([0, nex - 1], inp['d_score'], inp['d_prob']))
            tw.backward(res[1], inp['d_out'], **kw)
            grad = tw.flat_grad
            for j, d in enumerate(second_backward or []):
                arena.label = f'backward {j + 2}'
                tw.flat_grad = arena.take(tw.flat.numel(), torch.float32, f'flat_grad {j + 2}', fill=0)
                tw._saved_batch = B                      # (the wrapper refuses a second backward on one forward; the C ABI takes it)
                tw.backward(res[1], d)
                more.append(tw.flat_grad)
    torch.cuda.synchronize()
    assert tw.workspace is ws and tw._run is rec, 'the wrapper replaced a workspace that was large enough'
    changed = [m for m in (bits_differ(v, snap[k], f'input {k}') for k, v in const.items()) if m]
    return dict(fwd={k: v.cpu() for k, v in fwd.items()}, grad=None if grad is None else grad.cpu(), guards=arena.guard_failures(),
                inputs=changed, more_grads=[g.cpu() for g in more])


# The parameters whose gradient is one dclip_gemm_tn_acc launch into a zeroed buffer (encoder.cpp, dclip_encoder_backward): every element has
# a single writer, or the partial tiles of a split contraction are reduced in a fixed order, so they are reproducible by construction.
# Every other gradient (biases and LayerNorm affines: column sums inside dclip_layernorm_bwd / dclip_gemm_nt / dclip_colsum_acc; cls / pos /
# patch bias: dclip_batch_sum_acc; token tables: dclip_embed_scatter_add; conv_l / conv_w on the Unfused path) is a sum of f32 atomics from
# several workgroups, whose order may change from run to run.
GEMM_WGRADS = ('attn.qkv.weight', 'attn.proj.weight', 'mlp.fc1.weight', 'mlp.fc2.weight', 'head.weight', 'patch_embed.proj.weight',
               'patch_embed.1.weight', 'attn.in_proj_weight', 'attn.out_proj.weight', 'mlp.c_fc.weight', 'mlp.c_proj.weight', 'visual.conv1.weight',
               'visual.proj', 'text_projection')


def grad_classes(tw, a, b):
    """-> (buckets, exact) from two runs of the same computation on zero-filled workspaces.
    buckets: [(begin, end, bit-reproducible)] per flat range of grad_buckets(): what the two runs show, counted and printed.
    exact:   [(begin, end, name)] of the GEMM_WGRADS parameters the two runs reproduce bit for bit: held bit-equal by grad_failures().
    Two equal runs cannot tell a reproducible range from one whose atomics are rarely reordered.  Holding whole ranges bit-equal on that
    evidence failed on the first run of these tests on an MI355X: 13 comparisons, each with 11 to 130 elements of bias / LayerNorm / cls / pos
    vectors one ulp apart (no NaN, no weight matrix; one of them between two zero-filled workspaces, in the reuse chain) in ranges the two zero-filled runs
    had reproduced.  So bit-equality is asked of what is reproducible by construction, and the bound of everything."""
    import torch
    same = lambda lo, hi: bool(torch.equal(a[lo:hi].view(torch.int32), b[lo:hi].view(torch.int32)))
    buckets = [(lo, hi, same(lo, hi)) for lo, hi in tw.grad_buckets() if hi > lo]
    offs, exact = tw.param_offsets(), []
    for i, (name, p) in enumerate(zip(tw.param_names, tw._params())):
        if p is not None and p.requires_grad and name.endswith(GEMM_WGRADS) and same(offs[i], offs[i] + p.numel()):
            exact.append((offs[i], offs[i] + p.numel(), name))
    return buckets, exact


def grad_failures(classes, got, want, what):
    """gradient rule of the poison and reuse sections: per flat range of grad_buckets(), finite wherever `want` is and within
    GRAD_TOL * max|want| of it; bit-equal on the GEMM weight gradients that two zero-filled runs reproduce bit for bit"""
    import torch
    buckets, exact = classes
    out = []
    for lo, hi, name in exact:
        m = bits_differ(got[lo:hi], want[lo:hi], f'{what}: gradient of {name}, flat [{lo}, {hi}) (reproducible by construction)')
        if m:
            out.append(m)
    for lo, hi, _ in buckets:
        g, w = got[lo:hi], want[lo:hi]
        lost = torch.isfinite(w) & ~torch.isfinite(g)
        if lost.any():
            i = int(torch.nonzero(lost)[0])
            out.append(f'{what}: flat range [{lo}, {hi}): {int(lost.sum())} elements not finite, first at {lo + i}: {g[i].item()!r}')
            continue
        fin = torch.isfinite(w)
        scale = w[fin].abs().max().item() if fin.any() else 0.0
        err = (g[fin].double() - w[fin].double()).abs()
        if err.numel() and err.max().item() > GRAD_TOL * scale:
            i = int(err.argmax())
            out.append(f'{what}: flat range [{lo}, {hi}): max |got - want| {err.max().item():.3e} > {GRAD_TOL} * {scale:.3e} '
                       f'(element {i} of the finite ones)')
    return out

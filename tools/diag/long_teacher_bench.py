"""Timings of the long-sequence frozen-teacher path, one session, HIP events around repeated launches after a
warm-up, the shader clock noted before and after:
  kernels : dclip_attn_stream_fwd at (B, H, N) = (512, 12, 197) and (128, 16, 257); dclip_attn_fused_fwd at (512, 12, 101) and
            (512, 12, 128); microseconds, TFLOP/s of 4 B H N^2 hd, picoseconds per (query x key) element
  tower   : the frozen ViT-B/16 tower forward (12 layers, synthetic weights) at B = 512
  step    : l_clip (tests/golden/yaml_init_args.json) with a ViT-B/16 teacher, pairs / s at B = 512
    python tools/diag/long_teacher_bench.py [kernels] [tower] [step]        (default: all three)
`tower1` runs ONE warmed tower forward and nothing else: the command to put behind `rocprofv3 --kernel-trace --stats --` for
attention's share of the tower."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault('DCLIP_SYNTHETIC_TEACHER', '1')
import torch                                             # noqa: E402
from distillclip_amd import ops, synth                   # noqa: E402


def clock_mhz():
    try:
        out = subprocess.run(['rocm-smi', '--showclocks', '--json'], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if 'sclk' in k or 'mclk' in k}
    except Exception as exc:                             # the figures stand without it; say that it is missing
        return f'not read ({type(exc).__name__})'


def timed(fn, warm=5, reps=30, rounds=5):
    """-> (median, min, max) microseconds per call over `rounds` windows of `reps` calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / reps)
    us.sort()
    return us[len(us) // 2], us[0], us[-1]


def kernels():
    hd = 64
    for name, fn, B, H, N in (('stream', ops.attn_stream_fwd, 512, 12, 197), ('stream', ops.attn_stream_fwd, 128, 16, 257),
                              ('stream', ops.attn_stream_fwd, 128, 16, 577), ('fused', ops.attn_fused_fwd, 512, 12, 101),
                              ('fused', ops.attn_fused_fwd, 512, 12, 128), ('stream', ops.attn_stream_fwd, 512, 12, 128)):
        qkv = torch.randn((B * N, 3 * H * hd), device='cuda').to(torch.bfloat16)
        med, lo, hi = timed(lambda: fn(qkv, B, N, H, hd))
        flops = 4.0 * B * H * N * N * hd
        print(f'{name:6} B={B} H={H} N={N}: {med:8.1f} us (min {lo:.1f} max {hi:.1f})  {flops / med / 1e6:7.1f} TFLOP/s  '
              f'{med * 1e6 / (B * H * N * N):6.3f} ps per query x key')


def _tower(B):
    from distillclip_amd.model.utils import teacher_load
    enc = teacher_load('ViT-B/16', None, 'image').cuda()
    image = torch.from_numpy(synth.images(3, 8, 224)).cuda().repeat(B // 8, 1, 1, 1).contiguous()
    return enc, image


def tower(B=512):
    enc, image = _tower(B)
    with torch.no_grad():
        med, lo, hi = timed(lambda: enc(image), warm=3, reps=5, rounds=5)
    print(f'ViT-B/16 frozen tower forward B={B}: {med / 1e3:.2f} ms (min {lo / 1e3:.2f} max {hi / 1e3:.2f})  {B / med * 1e6:.0f} images/s')


def tower1(B=512):
    enc, image = _tower(B)
    with torch.no_grad():
        for _ in range(3):
            enc(image)
    torch.cuda.synchronize()


def step(B=512):
    from distillclip_amd.model import DualDistillModel
    from distillclip_amd.model.component import RepeatVisionTransformer, RepeatTextTransformer
    spec = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'yaml_init_args.json')))['l_clip']['model']['init_args']
    ic, tc = spec['image_student']['init_args'], spec['text_student']['init_args']
    T = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    si, st = RepeatVisionTransformer(**ic), RepeatTextTransformer(**tc)
    si.load_state_dict(T(synth.student_image_state(2022, **ic)))
    st.load_state_dict(T(synth.student_text_state(2022, **tc)))
    for name in ('ViT-B/32', 'ViT-B/16'):
        m = DualDistillModel(si, st, spec['loss_control_para'], spec['warm_steps'], spec['total_steps'], spec['weight_decay'], spec['lr'], None,
                             teacher_name=name).cuda()
        (opt,), _ = m.configure_optimizers()
        image = torch.from_numpy(synth.images(2022, 8, 224)).cuda().repeat(B // 8, 1, 1, 1).contiguous()
        text = torch.from_numpy(synth.captions(2022, B)).cuda()

        def one():
            loss = m.training_step([image, text])
            opt.zero_grad()
            m.backward_and_sync(loss)
            opt.step(zero_grad=True)
        med, lo, hi = timed(one, warm=3, reps=5, rounds=4)
        print(f'l_clip step, teacher {name}, B={B}: {med / 1e3:.2f} ms (min {lo / 1e3:.2f} max {hi / 1e3:.2f})  {B / med * 1e6:.0f} pairs/s')
        del m, opt


if __name__ == '__main__':
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    which = sys.argv[1:] or ['kernels', 'tower', 'step']
    if which != ['tower1']:
        print('clocks before:', clock_mhz())
    for w in which:
        {'kernels': kernels, 'tower': tower, 'tower1': tower1, 'step': step}[w]()
    if which != ['tower1']:
        print('clocks after:', clock_mhz())

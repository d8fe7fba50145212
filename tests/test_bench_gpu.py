"""bench.py end to end on one MI355X, each run a fresh process: a plain run prints the headline line and does nothing that takes work
of its own after the timed steps; `--full` adds the per-kernel roofline probe.  (`--full`'s CPU baseline is left out here: it is
~40 s of host work, and tests/test_bench_cpu.py runs its oracle step.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', *extra],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only():
    d = run_bench()
    assert d['metric'] == 'image-text pairs/sec (distill step)' and d['unit'] == 'pairs/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'bf16' and d['steps'] == 2
    assert d['ms_per_step'] > 0 and d['value'] == pytest.approx(512 * 1e3 / d['ms_per_step'], rel=1e-3)
    assert 'roofline' not in d and 'cpu_baseline' not in d


def test_full_run_adds_the_roofline_probe():
    d = run_bench('--full', '--no-cpu-baseline')
    assert d['value'] > 0
    assert d['roofline']['launches_per_step'] > 0 and d['roofline']['achieved'] > 0
    assert 'cpu_baseline' not in d

"""bench.py's CPU leg (the `cpu_baseline` object of the JSON line) is the oracle, built from the same pinned YAML values as the HIP
model.  One oracle training step of every workload at B = 2: the factory resolves every name it needs (the leg only runs on the
GPU box otherwise, where a NameError would surface at the end of a bench run) and the loss is finite."""
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize('name', ['lclip', 'image', 'text'])
def test_cpu_leg_runs_one_oracle_step(name):
    import torch
    import bench
    torch.set_num_threads(4)
    wl = dict(bench.WORKLOADS[name])
    step = bench.cpu_step_factory(wl, 2022)(2)      # (B = 1 has no in-batch negatives: cos_diff is NaN there, as in the reference)
    loss = step()
    assert math.isfinite(loss) and loss > 0.0


def test_every_workload_names_a_pinned_yaml():
    import bench
    for name, wl in bench.WORKLOADS.items():
        assert wl['yaml'] in bench.YAML_ARGS, name
        assert wl['kind'] in ('dual', 'image', 'text')


def test_dump_outputs_stays_in_budget_and_samples_fixed_positions(tmp_path):
    """--dump-outputs: float32 files, the whole dump within the budget, small arrays whole, large ones sampled at the same sorted
    positions on every call."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {'loss': torch.tensor(0.5), 'term.out_l1': torch.tensor(0.25, dtype=torch.float64),
              'student.small': torch.randn(3, 5, generator=g), 'student.big': torch.arange(10 ** 6, dtype=torch.float32).view(1000, 1000)}
    budget = 2 ** 20
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays, budget_bytes=budget)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(n + '.npy' for n in arrays)
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= budget + 128 * len(files)      # + .npy headers
    for n, t in arrays.items():
        a, b = np.load(tmp_path / 'a' / (n + '.npy')), np.load(tmp_path / 'b' / (n + '.npy'))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
        if n != 'student.big':
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.float().numpy()), n
    big = np.load(tmp_path / 'a' / 'student.big.npy')
    assert big.ndim == 1 and 0 < big.size < 10 ** 6
    assert np.all(np.diff(big) > 0)                 # every element is its own position: distinct positions, in index order


def test_steps_below_one_is_refused():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and '--steps' in r.stderr

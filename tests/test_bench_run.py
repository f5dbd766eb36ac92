"""bench.py's plain run: the headline line only, `--steps` timed steps, and `--dump-outputs` writing what the last timed step
computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['--gpus', '1', '--warmup', '1', '--res', '256', '--sphere-frequency', '16', '--views-per-gpu', '4']
NAMES = ('features', 'soft_mask', 'face_idx', 'vertex_grad')


def _run(args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=280)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    line = _run(SMALL + ['--steps', '3', '--dump-outputs', str(a)])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['full'] is False
    assert line['unit'] == 'Mpixels/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert abs(line['value'] - 4 * 256 * 256 / (line['ms_per_step'] * 1e-3) / 1e6) <= 1e-3 * line['value']
    assert not any(k in line for k in ('kernels', 'roofline', 'chamfer', 'c5', 'cpu_baseline', 'scene_variants'))
    assert line['distributed']['collectives_posted_per_step'] == 0
    _run(SMALL + ['--steps', '5', '--dump-outputs', str(b)])
    da = {k: np.load(a / f'{k}.npy') for k in NAMES}
    db = {k: np.load(b / f'{k}.npy') for k in NAMES}
    assert da['features'].shape == (4 * 256 * 256, 3) and da['face_idx'].dtype == np.float64
    assert da['vertex_grad'].shape == (10 * 16 * 16 + 2, 3) and np.abs(da['vertex_grad']).max() > 0
    assert (da['face_idx'] >= 0).any() and (da['face_idx'] < 0).any()
    # the same inputs in every run: the forward outputs agree exactly, the gradient (float atomics) to rounding
    for k in ('features', 'soft_mask', 'face_idx'):
        assert np.array_equal(da[k], db[k]), k
    assert np.abs(da['vertex_grad'] - db['vertex_grad']).max() <= 1e-5 * np.abs(db['vertex_grad']).max()

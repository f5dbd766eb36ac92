"""Generates tests/golden/sg_regimes.npz FROM THE REFERENCE ITSELF (kaolin.render.lighting.sg), on the CPU.

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_sg_regimes.py
For every case of tests/sg_regimes.py's FIXTURE_CASES: the float32 inputs; the reference's ground truth
``unbatched_sg_inner_product(...).sum(1)`` and the six autograd gradients of sum(out * grad_out), once on the inputs promoted
to float64 (``<case>_r64_<name>``) and once in float32 (``<case>_r32_<name>``); and ``K_ref_<family>``, the float32 run's
largest error per output in units of eps32 * cond against tests/sg_oracle.py's stable_oracle (order: sg_regimes.OUTPUTS).  For
the exact_zero families the float32 run's NaN masks (``<case>_nan_<name>``) instead of values.  Prints the K_ref table and K32.  The file
is written with fixed zip timestamps and one thread, so a second run reproduces it bit for bit.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sg_oracle  # noqa: E402
import sg_regimes as R  # noqa: E402
from make_golden_sg import load_lighting  # noqa: E402


def reference_run(sg, x, dtype):
    args = [x[k].to(dtype).requires_grad_() for k in R.KEYS]
    out = sg.unbatched_sg_inner_product(*args).sum(1)
    grads = torch.autograd.grad((out * x['go'].to(dtype)).sum(), args)
    return dict(zip(R.OUTPUTS, (out.detach(),) + tuple(grads)))


def save_deterministic(path, arrays):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(1)
    sg, _ = load_lighting()
    arrays = {}
    k_ref = {f: np.zeros(len(R.OUTPUTS)) for f in R.BOUNDED}
    for family, n, m, seed in R.FIXTURE_CASES:
        tag = R.case_tag(family, n, m, seed)
        x = R.make(family, n, m, seed, torch.float32)
        for k in R.KEYS + ('go',):
            arrays[f'{tag}_{k}'] = x[k].numpy()
        r64, r32 = reference_run(sg, x, torch.float64), reference_run(sg, x, torch.float32)
        if family not in R.BOUNDED:
            arrays[f'{tag}_zero_rows'], arrays[f'{tag}_zero_lights'] = x['zero_rows'].numpy(), x['zero_lights'].numpy()
            for name in R.OUTPUTS:
                arrays[f'{tag}_nan_{name}'] = torch.isnan(r32[name]).numpy()
                assert torch.equal(torch.isnan(r32[name]), torch.isnan(r64[name])), name
            continue
        ref = sg_oracle.stable_oracle(*R.args_of(x), grad_out=x['go'])
        for i, name in enumerate(R.OUTPUTS):
            arrays[f'{tag}_r64_{name}'] = r64[name].numpy()
            arrays[f'{tag}_r32_{name}'] = r32[name].numpy()
            k_ref[family][i] = max(k_ref[family][i], sg_oracle.error_units(r32[name], ref[name], ref[name + '_cond']))
    print('K_ref: the reference in float32, max |error| / (eps32 cond)')
    print(f'{"family":10s} ' + ' '.join(f'{name:>9s}' for name in R.OUTPUTS))
    for family, row in k_ref.items():
        arrays[f'K_ref_{family}'] = row
        print(f'{family:10s} ' + ' '.join(f'{v:9.3g}' for v in row))
    k32 = R.K_MARGIN * max(float(k_ref[f].max()) for f in R.BOUND_FAMILIES)
    print(f'K32 = {R.K_MARGIN:g} * max over {R.BOUND_FAMILIES} = {k32:.4g}')
    path = os.path.join(HERE, 'sg_regimes.npz')
    save_deterministic(path, arrays)
    print('wrote sg_regimes.npz', len(arrays), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

"""Generates tests/golden/gaussian_transforms.npz FROM THE REFERENCE ITSELF (kaolin.ops.gaussians.transforms: transform_gaussians,
transform_shs, with kaolin.math.quat underneath).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_gaussian_transforms.py
The reference's transforms.py and quaternion.py are loaded by path on top of _refload's stub ``kaolin`` package, on the CPU, with
TORCH_COMPILE_DISABLE=1 set before torch is imported (its two table helpers are decorated with torch.compile).  Data only:

  fix_{positions,orientations,scales,sh}   the three Gaussians of the reference's test_transforms.py fixtures (orientations wxyz;
              sh (3, 16, 3) seeded here, float32 values)
  tf_<name>   the transforms of those tests, float64: identity, translation, uniform_scale, trs45 (4, 4); yaw180, pitch180,
              roll180 (1, 4, 4); batched_trs, batched_180, batched_translation, batched_scale (3, 4, 4).  A float32 run uses
              the rounded matrix.
  ret_<name>_<f32|f64>_x<use_xyzw>_l<use_log_scales>_{pos,ori,scl,sh}   what the reference returns (a wxyz fixture is
              reordered for use_xyzw, as its tests do)
  refdev_<name>   the reference's float64 SH result minus the projection oracle's (tests/gaussian_transforms_bruteforce.py)
  flip_<name>     (180 degree cases) per Gaussian the coefficient indices whose sign the reference flips, -1 padded
  rand_R (64, 3, 3), rand_sh (64, 16, 3)   seeded rotations and unit-variance coefficients (float32 values);
  rand_ret_{f32,f64}, rand_refdev          the reference's transform_shs on them and its float64 deviation from the oracle
  err_<case>  type and text of what the reference raises
"""
import os
os.environ['TORCH_COMPILE_DISABLE'] = '1'   # before torch

import math  # noqa: E402
import sys  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _refload  # noqa: E402
import gaussian_transforms_bruteforce as oracle  # noqa: E402

NAME = 'gaussian_transforms.npz'
DTYPES = (('f32', torch.float32), ('f64', torch.float64))


def load_reference():
    _refload.load_reference()
    _refload._pkg('kaolin.math')
    quat = _refload._load('kaolin.math.quat', 'kaolin/math/quat/quaternion.py')
    sys.modules['kaolin.math'].quat = quat
    _refload._pkg('kaolin.ops.gaussians')
    return _refload._load('kaolin.ops.gaussians.transforms', 'kaolin/ops/gaussians/transforms.py')


def _trs(sf, axis, angle, t):
    c, s = math.cos(angle), math.sin(angle)
    R = {'x': [[1, 0, 0], [0, c, -s], [0, s, c]], 'y': [[c, 0, s], [0, 1, 0], [-s, 0, c]], 'z': [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    m = np.eye(4)
    m[:3, :3] = sf * np.array(R)
    m[:3, 3] = t
    return m


def transforms():
    c, s = math.cos(math.pi), math.sin(math.pi)
    tf = {'identity': np.eye(4), 'translation': np.eye(4), 'uniform_scale': np.diag([3., 3., 3., 1.]),
          'trs45': _trs(2.0, 'z', math.pi / 4, [3.5, -1.2, 2.7]),
          'yaw180': np.array([[[c, 0, -s, 0], [0, 1, 0, 0], [s, 0, c, 0], [0, 0, 0, 1]]]),
          'pitch180': np.array([[[1, 0, 0, 0], [0, c, s, 0], [0, -s, c, 0], [0, 0, 0, 1]]]),
          'roll180': np.array([[[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]]),
          'batched_trs': np.stack([_trs(2.0, 'z', math.pi / 4, [3.5, -1.2, 2.7]), _trs(0.5, 'x', math.pi / 6, [-1.0, 2.5, -3.0]),
                                   _trs(3.0, 'y', math.pi / 3, [0.5, -0.5, 1.5])])}
    tf['translation'][:3, 3] = [2., 3., 5.]
    tf['batched_180'] = np.concatenate([tf['yaw180'], tf['pitch180'], tf['roll180']])
    tf['batched_translation'] = np.stack([np.eye(4)] * 3)
    tf['batched_translation'][:, :3, 3] = [[2., 3., 5.], [-1.5, .5, 2.], [4., -2.5, 1.]]
    tf['batched_scale'] = np.stack([np.diag([f, f, f, 1.]) for f in (2., .5, 3.)])
    return tf


def random_rotations(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1
    return q


def raised(fn, *args):
    try:
        fn(*args)
    except Exception as e:  # noqa: BLE001
        return np.array([type(e).__name__, str(e)])
    return np.array(['', ''])


def main():
    ref = load_reference()
    rng = np.random.default_rng(20261021)
    out = {'fix_positions': np.eye(3), 'fix_orientations': np.array([[0., 0., 1., 0.], [0., 0., 0., 1.], [1., 0., 0., 0.]]),
           'fix_scales': np.array([[1.] * 3, [2.] * 3, [.5] * 3]),
           'fix_sh': rng.standard_normal((3, 16, 3)).astype(np.float32).astype(np.float64)}
    tfs = transforms()
    for name, tf in tfs.items():
        out[f'tf_{name}'] = tf
        for tag, dtype in DTYPES:
            args = [torch.from_numpy(out[k]).to(dtype) for k in ('fix_positions', 'fix_orientations', 'fix_scales')]
            sh, t = torch.from_numpy(out['fix_sh']).to(dtype), torch.from_numpy(tf).to(dtype)
            for xyzw in (0, 1):
                ori = torch.cat([args[1][:, 1:], args[1][:, :1]], dim=-1) if xyzw else args[1]
                for logs in (0, 1):
                    ret = ref.transform_gaussians(args[0], ori, args[2], t, sh, use_log_scales=bool(logs), use_xyzw=bool(xyzw))
                    for key, r in zip(('pos', 'ori', 'scl', 'sh'), ret):
                        assert r.dtype == dtype
                        out[f'ret_{name}_{tag}_x{xyzw}_l{logs}_{key}'] = r.numpy()
        A = tf.reshape(-1, 4, 4)[:, :3, :3]
        R = A / np.linalg.norm(A, axis=1, keepdims=True)
        out[f'refdev_{name}'] = out[f'ret_{name}_f64_x0_l0_sh'] - oracle.projection_transform_shs(out['fix_sh'], R)
        if '180' in name:
            ret, sh = out[f'ret_{name}_f64_x0_l0_sh'], out['fix_sh']
            flips = np.full((3, 16), -1, dtype=np.int64)
            for g in range(3):
                idx = [k for k in range(16) if np.abs(ret[g, k] + sh[g, k]).max() < 1e-9]
                assert all(np.abs(ret[g, k] - sh[g, k]).max() < 1e-9 for k in range(16) if k not in idx)
                flips[g, :len(idx)] = idx
            out[f'flip_{name}'] = flips
    out['rand_R'] = random_rotations(64, rng)
    out['rand_sh'] = rng.standard_normal((64, 16, 3)).astype(np.float32).astype(np.float64)
    for tag, dtype in DTYPES:
        out[f'rand_ret_{tag}'] = ref.transform_shs(torch.from_numpy(out['rand_sh']).to(dtype),
                                                  torch.from_numpy(out['rand_R']).to(dtype)).numpy()
    out['rand_refdev'] = out['rand_ret_f64'] - oracle.projection_transform_shs(out['rand_sh'], out['rand_R'])
    # what the reference raises
    p, q, s, t = (torch.zeros(3, 3), torch.zeros(3, 4), torch.zeros(3, 3), torch.eye(4))
    out['err_dtype'] = raised(ref.transform_gaussians, p, q, s, t.double())
    out['err_sh_dtype'] = raised(ref.transform_gaussians, p, q, s, t, torch.zeros(3, 4, 3).double())
    out['err_shs_dtype'] = raised(ref.transform_shs, torch.zeros(3, 4, 3), torch.eye(3)[None].double())
    out['err_not_square'] = raised(ref.transform_shs, torch.zeros(3, 5, 3), torch.eye(3)[None])
    out['err_degree'] = raised(ref.transform_shs, torch.zeros(3, 25, 3), torch.eye(3)[None])
    out['err_channels'] = raised(ref.transform_shs, torch.zeros(3, 4, 2), torch.eye(3)[None])
    out['err_batch'] = raised(ref.transform_shs, torch.zeros(3, 4, 3), torch.eye(3)[None].repeat(2, 1, 1))
    out['err_r_shape'] = raised(ref.transform_shs, torch.zeros(3, 4, 3), torch.eye(4)[None])
    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes;', 'bands 2-3 deviate from the oracle by',
          np.abs(out['rand_refdev'][:, 4:]).max(), 'bands 0-1 by', np.abs(out['rand_refdev'][:, :4]).max())
    for k in sorted(out):
        if k.startswith('err_'):
            print(k, out[k][0], '|', out[k][1][:100])
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()

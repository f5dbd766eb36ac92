"""float64 oracle of the reduced spherical-gaussian inner product for the lighting tests: the output and the six gradients
of sum(out * grad_out), each with the sum of the absolute values of the terms it adds up (the accumulation slack of
kaolin_amd.utils.testing.elementwise_mismatch).  Every (row, light) pair is its own term: the parameters are expanded to
(rows, lights, ...) so that autograd hands back each pair's contribution.  Computed in chunks of rows on the inputs'
device."""
import math

import torch


def _pairs(a, d, s, oa, od, os_):
    v = s[..., None] * d + os_[..., None] * od
    um = torch.sqrt((v * v).sum(-1, keepdim=True))
    lm = (s + os_)[..., None]
    return 2.0 * math.pi * torch.exp(um - lm) * (a * oa) * (1.0 - torch.exp(-2.0 * um)) / um


def reduced_oracle(a, d, s, oa, od, os_, grad_out=None, pairs_per_chunk=1 << 20, rows=None):
    """-> dict out, out_abs, and (with grad_out) ga, gd, gs, goa, god, gos with *_abs.  `rows` (optional index tensor):
    the row-side results only for those rows; the column gradients always sum over every row."""
    a, d, s, oa, od, os_ = (t.detach().double() for t in (a, d, s, oa, od, os_))
    n, m = a.shape[0], oa.shape[0]
    chunk = max(1, pairs_per_chunk // max(m, 1))
    res = {'goa': torch.zeros_like(oa), 'god': torch.zeros_like(od), 'gos': torch.zeros_like(os_)}
    for k in ('goa', 'god', 'gos'):
        res[k + '_abs'] = torch.zeros_like(res[k])
    row_parts = {k: [] for k in ('out', 'out_abs', 'ga', 'gd', 'gs', 'ga_abs', 'gd_abs', 'gs_abs')}
    starts = range(0, n, chunk)
    for r0 in starts:
        r1 = min(n, r0 + chunk)
        k = r1 - r0
        ex = [a[r0:r1, None, :].expand(k, m, 3), d[r0:r1, None, :].expand(k, m, 3), s[r0:r1, None].expand(k, m),
              oa[None].expand(k, m, 3), od[None].expand(k, m, 3), os_[None].expand(k, m)]
        ex = [t.clone().requires_grad_(grad_out is not None) for t in ex]
        p = _pairs(*ex)
        keep = None
        if rows is not None:
            keep = rows[(rows >= r0) & (rows < r1)] - r0
        def rowsel(t):
            return t if keep is None else t[keep]
        row_parts['out'].append(rowsel(p.detach().sum(1)))
        row_parts['out_abs'].append(rowsel(p.detach().abs().sum(1)))
        if grad_out is not None:
            g = grad_out[r0:r1].detach().double()
            terms = torch.autograd.grad((p * g[:, None, :]).sum(), ex)
            for name, t in zip(('ga', 'gd', 'gs'), terms[:3]):
                row_parts[name].append(rowsel(t.sum(1)))
                row_parts[name + '_abs'].append(rowsel(t.abs().sum(1)))
            for name, t in zip(('goa', 'god', 'gos'), terms[3:]):
                res[name] += t.sum(0)
                res[name + '_abs'] += t.abs().sum(0)
    for name, parts in row_parts.items():
        if parts:
            res[name] = torch.cat(parts)
        elif name in ('out', 'out_abs'):
            res[name] = torch.zeros(0 if rows is None else len(rows), 3, dtype=torch.float64, device=a.device)
    if grad_out is not None and n == 0:
        for name, like in (('ga', a), ('gd', d), ('gs', s)):
            res[name] = torch.zeros_like(like)
            res[name + '_abs'] = torch.zeros_like(like)
    return res

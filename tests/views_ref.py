"""NumPy model of the three-view projections (hp_volume_views / hp_views_orient, hiddenpose_amd.visualizer) for the tests,
written from the formulas of the C header.  Everything runs on the CPU.

x (P, T, H, W) float32.
max mode:  v = x with every value below zero set to zero (a NaN is not below zero and stays);
           front = max over t, top = max over h, left = max over w (np.max: a NaN wins).
sum mode:  the same three reductions as plain float32 sums of x, taken with the calls volume_log itself makes (`.sum(axis)` of
           a CPU torch tensor, then `.numpy()`; np.sum adds in another order and differs from it in the last bit).
vmax (P, 3): np.max of each finished view.
orient:    front / vmax_front;  rot90(top / vmax_top, 2);  rot90(left / vmax_left, 3) -- and zeros where a view's maximum
           is 0 (the one deliberate difference from the reference, which divides 0 by 0).
"""
import numpy as np
import torch

MAX, SUM = 0, 1     # HP_VIEWS_MAX_CLAMPED, HP_VIEWS_SUM
U = 2.0 ** -24      # unit roundoff of float32


def project(x, mode):
    """-> front (P, H, W), top (P, T, W), left (P, T, H), vmax (P, 3), float32."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 4
    with np.errstate(invalid="ignore"):
        if mode == MAX:
            v = x.copy()
            v[v < 0] = 0
            views = [np.max(v, axis=a) for a in (1, 2, 3)]
        else:
            views = [np.stack([torch.from_numpy(p).sum(a).numpy() for p in x]) for a in (0, 1, 2)]
        vmax = np.stack([np.max(v.reshape(v.shape[0], -1), axis=1) for v in views], axis=1)
    return views[0], views[1], views[2], vmax.astype(np.float32)


def orient(front, top, left, vmax):
    """-> out_front (P, H, W), out_top (P, T, W), out_left (P, H, T)."""
    outs = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, (view, turns) in enumerate(((front, 0), (top, 2), (left, 3))):
            planes = []
            for p in range(view.shape[0]):
                m = vmax[p, k]
                n = np.zeros_like(view[p]) if m == 0 else view[p] / m
                planes.append(np.rot90(n, turns) if turns else n)
            outs.append(np.ascontiguousarray(np.stack(planes)).astype(np.float32))
    return tuple(outs)


def sums64(x):
    """Float64 sums along t, h, w and the sums of |x| along the same axes (the error bound's scale), with the number of
    reduced terms of each: [(s64, abs64, n)] for front, top, left."""
    x64 = np.asarray(x, dtype=np.float64)
    return [(x64.sum(axis=a), np.abs(x64).sum(axis=a), x64.shape[a]) for a in (1, 2, 3)]


def sum_bound(abs64, n):
    """|fl(sum) - sum| <= (n + 1) u sum|x| covers fp32 accumulation of n terms in any order (every ordering's bound is
    gamma_{n-1} sum|x| <= (n - 1) u / (1 - (n - 1) u) sum|x|, below (n + 1) u sum|x| for n u < 1/2, plus the final rounding
    of the float64 comparison value)."""
    return (n + 1) * U * abs64


def same(a, b):
    """Bit-equal up to the two things the contract leaves open: which NaN pattern, and the sign of a zero."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def mark(im, joints, a, b):
    """The 2 x 2 marks volume_log adds at every joint: `im.max()` is evaluated again for every joint."""
    for i in range(joints.shape[0]):
        r, c = int(joints[i, a]), int(joints[i, b])
        im[r:r + 2, c:c + 2] += im.max() / 2
    return im

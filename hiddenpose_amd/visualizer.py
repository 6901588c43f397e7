"""Counterpart of utils/visualizer.py: the three-view projections and the joint plots of the reference's logging steps.

The reference copies whole volumes to the host and reduces them with NumPy.  Here one HIP pass over the volume
(`hp_volume_views`, csrc/views_kernels.hip) gives the front / top / left projections and their maxima, a second small
kernel (`hp_views_orient`) normalises and rotates them into the arrays the reference hands to `imshow`, and only those
finished views cross to the host.  Figures are written with matplotlib on the Agg backend when it imports; otherwise the
arrays are saved as `.npy` under the same stem.  Every logger also returns what it computed.

    project_views(volume, planes, mode)  device tensors front (P,H,W), top (P,T,W), left (P,T,H), vmax (P,3)
    three_views(volume, plane)           the three oriented, normalised images of one plane
    threeviews_log / volume_log / joints_log   the reference's signatures, directories and file stems

One deliberate difference from the reference: a view whose maximum is 0 is written as zeros, not as 0 / 0 = NaN.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .hip_ops import _need_cuda

MODES = {"max": 0, "sum": 1}    # HP_VIEWS_MAX_CLAMPED, HP_VIEWS_SUM

# the 23 bones of the 24-joint skeleton (utils/visualizer.py:124-148)
BONES = ((0, 1), (0, 2), (0, 3), (1, 4), (2, 5), (3, 6), (4, 7), (5, 8), (6, 9), (7, 10), (8, 11), (9, 12), (9, 13), (9, 14),
         (12, 15), (13, 16), (14, 17), (16, 18), (17, 19), (18, 20), (19, 21), (20, 22), (21, 23))


def _run_views(x, P, T, H, W, mode, front, top, left, vmax):
    L = _lib.lib()
    nbytes = L.hp_volume_views_workspace_bytes(P, T, H, W, mode)
    ws = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=x.device)
    _lib.check(L.hp_volume_views(_lib.ptr(x), _lib.ptr(front), _lib.ptr(top), _lib.ptr(left), _lib.ptr(vmax), P, T, H, W, mode,
                                 _lib.ptr(ws), int(nbytes), _lib.current_stream_handle(x.device)), "hp_volume_views")


def project_views(volume: torch.Tensor, planes=None, mode: str = "max"):
    """Axis projections of the selected planes of a (B, C, T, H, W) device tensor, from one read of each plane.

    planes: None for all B * C planes in (b, c) order, or a sequence of (b, c) pairs (negative indices count from the end).
    mode:   "max": maxima of max(x, 0) (threeviews_log);  "sum": plain sums (volume_log).
    Returns front (P, H, W) over t, top (P, T, W) over h, left (P, T, H) over w and vmax (P, 3), the maximum of each finished
    view, all fp32 on the volume's device.  A NaN in a reduced line makes that pixel and that view's vmax NaN.

    The kernel reads contiguous fp32 planes: a non-contiguous or non-fp32 input (or selected plane) is made contiguous
    fp32 first, which costs a copy of what is selected; the volume itself is never modified.  A CPU tensor raises
    HiddenPoseHipError."""
    _need_cuda(volume, "project_views")
    if volume.dim() != 5:
        raise ValueError(f"project_views: expected (B, C, T, H, W), got {tuple(volume.shape)}")
    if mode not in MODES:
        raise ValueError(f"project_views: mode {mode!r} is neither 'max' nor 'sum'")
    B, C, T, H, W = volume.shape
    volume = volume.detach()
    if planes is None:
        xs = [volume.contiguous().float()]
        counts = [B * C]
    else:
        xs = [volume[b, c].contiguous().float() for b, c in planes]
        counts = [1] * len(xs)
    P = sum(counts)
    kw = dict(dtype=torch.float32, device=volume.device)
    front, top, left = torch.empty((P, H, W), **kw), torch.empty((P, T, W), **kw), torch.empty((P, T, H), **kw)
    vmax = torch.empty((P, 3), **kw)
    p0 = 0
    for x, n in zip(xs, counts):
        _run_views(x, n, T, H, W, MODES[mode], front[p0:p0 + n], top[p0:p0 + n], left[p0:p0 + n], vmax[p0:p0 + n])
        p0 += n
    return front, top, left, vmax


def orient_views(front, top, left, vmax):
    """front / vmax, rot90(top / vmax, 2), rot90(left / vmax, 3) per plane -> (P, H, W), (P, T, W), (P, H, T)."""
    _need_cuda(front, "orient_views")
    P, H, W = front.shape
    T = top.shape[1]
    out_front, out_top = torch.empty_like(front), torch.empty_like(top)
    out_left = torch.empty((P, H, T), dtype=torch.float32, device=front.device)
    _lib.check(_lib.lib().hp_views_orient(_lib.ptr(front), _lib.ptr(top), _lib.ptr(left), _lib.ptr(vmax), _lib.ptr(out_front),
                                          _lib.ptr(out_top), _lib.ptr(out_left), P, T, H, W,
                                          _lib.current_stream_handle(front.device)), "hp_views_orient")
    return out_front, out_top, out_left


def three_views(volume: torch.Tensor, plane=(0, -1)):
    """The front (H, W), top (T, W) and left (H, T) images threeviews_log shows for one (b, c) plane: max projections of
    max(x, 0), each divided by its maximum, the top view turned by 180 and the left view by 270 degrees.  The default plane
    is the reference's `[0, -1]` (utils/visualizer.py:156)."""
    f, t, l, m = project_views(volume, [plane], "max")
    of, ot, ol = orient_views(f, t, l, m)
    return of[0], ot[0], ol[0]


def _pyplot():
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        return plt
    except Exception:   # no matplotlib: the arrays themselves are written
        return None


def _save_image(plt, im, stem):
    if plt is None:
        np.save(stem + ".npy", im)
        return
    plt.imshow(im)
    plt.savefig(stem + ".jpg")


def threeviews_log(re, path, name, index=0):
    """utils/visualizer.py:155-185: `<path>/<name>_{front,top,left}_view_<index>.jpg` of plane [0, -1] of `re`.
    Returns {"front": (H, W), "top": (T, W), "left": (H, T)} as NumPy arrays."""
    imgs = dict(zip(("front", "top", "left"), (v.cpu().numpy() for v in three_views(re))))
    os.makedirs(path, exist_ok=True)
    plt = _pyplot()
    if plt is not None:
        plt.figure(1)
    for key, im in imgs.items():
        _save_image(plt, im, f"{path}/{name}_{key}_view_{index}")
    if plt is not None:
        plt.clf()
    return imgs


def _mark(im, joints, a, b):
    """The reference's 2 x 2 marks (utils/visualizer.py:35-38): `im.max()` is taken again for every joint, as there."""
    for i in range(joints.shape[0]):
        r, c = int(joints[i, a]), int(joints[i, b])
        im[r:r + 2, c:c + 2] += im.max() / 2
    return im


def volume_log(volume, res_path, name, index, joints=None):
    """utils/visualizer.py:14-63: sum projections of plane [0, 0] along each axis, with a 2 x 2 mark of `im.max() / 2` at
    every joint (d, h, w).  The reference reads the joints from `./1.txt`; here they are an argument ((J, 3) array-like or
    None for no marks).  The front view goes to `<res_path>/projection_of_vol/<name>_<index>_front_joints.jpg`, top and
    left to `<res_path>/figure/projection_of_vol/`.  Returns {"front": (H, W), "top": (T, W), "left": (T, H)}."""
    f, t, l, _ = project_views(volume, [(0, 0)], "sum")
    imgs = {"front": f[0].cpu().numpy(), "top": t[0].cpu().numpy(), "left": l[0].cpu().numpy()}
    if joints is not None:
        j = np.asarray(joints.detach().cpu() if torch.is_tensor(joints) else joints, dtype=np.float64).reshape(-1, 3)
        _mark(imgs["front"], j, 1, 2)
        _mark(imgs["top"], j, 0, 2)
        _mark(imgs["left"], j, 0, 1)
    os.makedirs(res_path + "/figure/projection_of_vol", exist_ok=True)
    os.makedirs(res_path + "/projection_of_vol", exist_ok=True)
    plt = _pyplot()
    if plt is not None:
        plt.figure(1)
    _save_image(plt, imgs["front"], f"{res_path}/projection_of_vol/{name}_{index}_front_joints")
    _save_image(plt, imgs["top"], f"{res_path}/figure/projection_of_vol/{name}_{index}_top_joints")
    _save_image(plt, imgs["left"], f"{res_path}/figure/projection_of_vol/{name}_{index}_left_joints")
    if plt is not None:
        plt.clf()
    return imgs


def joints_log(joints, res_path, joint_name, index=0):
    """utils/visualizer.py:66-120: `<res_path>/txt/<joint_name><index>.txt` and the skeleton figure
    `<res_path>/<joint_name><index>.png` (scatter + 23 bones, axes D / H / W over 0..64, W inverted).
    Returns the (J, 3) NumPy array that was written."""
    joints = np.asarray(joints.detach().cpu() if torch.is_tensor(joints) else joints)
    os.makedirs(os.path.join(res_path, "txt"), exist_ok=True)
    np.savetxt(os.path.join(res_path, "txt", f"{joint_name}{index}.txt"), joints)
    plt = _pyplot()
    if plt is None:
        np.save(f"{res_path}/{joint_name}{index}.npy", joints)
        return joints
    from matplotlib.pyplot import MultipleLocator

    fig = plt.figure(2)
    ax = fig.add_subplot(111, projection="3d")
    for axis in (ax.xaxis, ax.yaxis, ax.zaxis):
        axis.set_major_locator(MultipleLocator(10))
    ds, hs, ws = list(joints[:, 2]), list(joints[:, 0]), list(joints[:, 1])    # :104, `ds, hs, ws = ws, ds, hs`
    ax.scatter(ds, hs, ws)
    for a, b in BONES:
        if a < len(ds) and b < len(ds):
            ax.plot([ds[a], ds[b]], [hs[a], hs[b]], [ws[a], ws[b]], linewidth=1)
    ax.set_xlabel("D")
    ax.set_ylabel("H")
    ax.set_zlabel("W")
    ax.set_title(joint_name)
    ax.set_xlim(0, 64)
    ax.set_ylim(0, 64)
    ax.set_zlim(0, 64)
    ax.invert_zaxis()
    fig.savefig(f"{res_path}/{joint_name}{index}.png")
    plt.clf()
    return joints

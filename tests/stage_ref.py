"""CPU yardsticks for tests/test_stage_edges_gpu.py: the memory-bound stages of csrc/unet_kernels.hip and the stage half of
csrc/misc_kernels.hip evaluated by ATen in float64 (the reference) and in float32 (whose own error against float64 sets the
bar), the bar rule, and the index sets of the elements that one launch-geometry branch produces.

Bar rule:  hip <= max(floor, MARGIN * e_ref), where
    hip   = rel_l2(kernel, float64 reference),
    e_ref = rel_l2(ATen float32 on the CPU, float64 reference) on the same inputs,
    floor = the bar of the operator's test in test_stages_gpu.py / test_aux_gpu.py.
The same metric is evaluated again over each edge subset (the plane tail, the items of a second grid-stride trip, the last
chunk, ...), so that an error confined to the branch is not diluted by the whole tensor.

Launch constants of the two files (UT / MT, ugrid / mgrid): 256 threads per workgroup, at most 2048 workgroups."""
import numpy as np
import torch
import torch.nn.functional as F

MARGIN = 4.0            # the project's margin over the float32 model's own error (tests/head_loss_ref.py)
WG = 256                # threads per workgroup
GRID_CAP = 256 * 8      # workgroups per launch
TRIP = WG * GRID_CAP    # items one trip of a full grid covers: 524,288
SA_CHUNKS = 32          # workgroups per heat-map of the soft-argmax forward


def f64(t):
    t = t.detach().cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    return t.to(torch.float64).reshape(-1)


def rel_l2(a, b):
    a, b = f64(a), f64(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def bar(floor, e_ref):
    return max(floor, MARGIN * e_ref)


def judge(label, hip, ref64, ref32, floor, subsets=None):
    """Asserts the bar rule on the whole tensor and on every subset (name -> flat index tensor or boolean mask; empty ones are
    skipped), after printing hip, e_ref and hip / e_ref of each.  Returns the whole-tensor (hip, e_ref)."""
    h, r, s = f64(hip), f64(ref64), f64(ref32)
    assert h.shape == r.shape == s.shape, (label, h.shape, r.shape, s.shape)
    assert bool(torch.isfinite(h).all()), f"{label}: non-finite values"
    bad, whole = [], None
    for name, idx in [("all", None)] + sorted((subsets or {}).items()):
        if idx is not None:
            idx = torch.as_tensor(idx).reshape(-1)
            if idx.numel() == 0 or (idx.dtype == torch.bool and not bool(idx.any())):
                continue
        hh, rr, ss = (h, r, s) if idx is None else (h[idx], r[idx], s[idx])
        e_hip, e_ref = rel_l2(hh, rr), rel_l2(ss, rr)
        b = bar(floor, e_ref)
        print(f"[stage-edge] {label} [{name}, {hh.numel()} el]: hip {e_hip:.2e}  e_ref {e_ref:.2e}  "
              f"ratio {e_hip / max(e_ref, 1e-300):.2f}  bar {b:.1e}")
        if idx is None:
            whole = (e_hip, e_ref)
        if not e_hip <= b:
            bad.append((name, e_hip, e_ref, b))
    assert not bad, (label, bad)
    return whole


def judge_sum(label, hip, ref64, ref32, floor, scale):
    """A cancelling sum (weight / bias gradients met in float atomics): the absolute error of every entry against the sum's
    natural scale (test_stages_gpu.py::test_conv1x1_out), under the same bar rule."""
    h, r, s = f64(hip), f64(ref64), f64(ref32)
    e_hip, e_ref = float((h - r).abs().max()) / scale, float((s - r).abs().max()) / scale
    b = bar(floor, e_ref)
    print(f"[stage-edge] {label} [max |err| / scale {scale:.3g}]: hip {e_hip:.2e}  e_ref {e_ref:.2e}  "
          f"ratio {e_hip / max(e_ref, 1e-300):.2f}  bar {b:.1e}")
    assert e_hip <= b, (label, e_hip, e_ref, b)
    return e_hip, e_ref


def same_bits(a, b):
    """bit equality of two float32 tensors (tells -0.0 from 0.0, which torch.equal does not)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------- edge subsets (flat indices into a contiguous tensor)
def plane_tail(planes, V):
    """the elements i >= 4 * floor(V / 4) of every plane: what the scalar tail loop behind the 16-byte loop writes"""
    t = torch.arange(4 * (V // 4), V)
    return (torch.arange(planes)[:, None] * V + t[None, :]).reshape(-1)


def plane_range(planes, V, lo, hi):
    """the elements lo <= i < hi of every plane (empty where the planes are shorter)"""
    lo, hi = min(lo, V), min(hi, V)
    t = torch.arange(lo, max(lo, hi))
    return (torch.arange(planes)[:, None] * V + t[None, :]).reshape(-1)


def beyond_first_trip(n, per_item=1, first=TRIP):
    """the elements of items first, first + 1, ... of a launch over n // per_item items of per_item consecutive elements"""
    return torch.arange(min(first * per_item, n), n)


def axis_from(shape, axis, start):
    """the elements whose index along `axis` is >= start"""
    m = torch.zeros(shape, dtype=torch.bool)
    sl = [slice(None)] * len(shape)
    sl[axis] = slice(start, None)
    m[tuple(sl)] = True
    return m.reshape(-1)


# ---------------------------------------------------------------- references (dtype = torch.float64 or torch.float32)
def groupnorm_preact(z, gamma, beta, G, eps=1e-5):
    return F.group_norm(z, G, gamma, beta, eps)


def groupnorm_relu(z, gamma, beta, gy, G, dtype, eps=1e-5):
    """-> y, dz, dgamma, dbeta of sum(relu(GroupNorm(z)) * gy)"""
    zd, gd, bd = (t.detach().to(dtype).requires_grad_(True) for t in (z, gamma, beta))
    y = F.relu(F.group_norm(zd, G, gd, bd, eps))
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), zd.grad, gd.grad, bd.grad


def mask_near_relu_kink(z, gamma, beta, gy, G, eps=1e-5, rel=1e-4):
    """The backward rebuilds the ReLU mask from z: a step function of the input.  Zero the incoming gradient wherever the float64
    pre-activation lies within rel * max|a| of the kink, so that a flipped mask changes nothing.  -> gy, zeroed share."""
    a = groupnorm_preact(z.double(), gamma.double(), beta.double(), G, eps)
    near = a.abs() < rel * a.abs().max()
    return torch.where(near, torch.zeros_like(gy), gy), float(near.double().mean())


def upsample_cat(x1, skip, gy, dtype):
    """-> y, dx1, dskip of sum(cat([skip, trilinear x2 (align_corners) of x1]) * gy)"""
    a, b = x1.detach().to(dtype).requires_grad_(True), skip.detach().to(dtype).requires_grad_(True)
    y = torch.cat([b, F.interpolate(a, scale_factor=2, mode="trilinear", align_corners=True)], dim=1)
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), a.grad, b.grad


def upsample(x, gy, dtype):
    a = x.detach().to(dtype).requires_grad_(True)
    y = F.interpolate(a, scale_factor=2, mode="trilinear", align_corners=True)
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), a.grad


def conv1x1(x, w, b, gy, dtype):
    xd, wd = x.detach().to(dtype).requires_grad_(True), w.detach().to(dtype).requires_grad_(True)
    bd = b.detach().to(dtype).requires_grad_(True) if b is not None else None
    y = F.conv3d(xd, wd, bd)
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), xd.grad, wd.grad, (bd.grad if b is not None else None)


def normalize_feature(x, gy, dtype):
    from oracle import nlospose_oracle as O

    xd = x.detach().to(dtype).requires_grad_(True)
    y = O.normalize_feature(xd)
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), xd.grad


def softargmax(h, gy, dtype):
    from oracle import nlospose_oracle as O

    B, J, D, H, W = h.shape
    hd = h.detach().to(dtype).requires_grad_(True)
    y = O.softmax_integral(hd, J, W, H, D)
    (y * gy.to(dtype)).sum().backward()
    return y.detach(), hd.grad


def bce_dice(x, t, gl, dtype):
    from oracle import nlospose_oracle as O

    xd = x.detach().to(dtype).requires_grad_(True)
    loss = O.bce_dice_loss(xd, t.to(dtype))
    (loss * gl).backward()
    return loss.detach(), xd.grad


def weighted_mse(p, t, w, gl, dtype):
    pd = p.detach().to(dtype).requires_grad_(True)
    loss = ((pd - t.to(dtype)) ** 2 * w.to(dtype)).sum() / len(p)
    (loss * gl).backward()
    return loss.detach(), pd.grad


def blur32(x, taps, r):
    """the replicate-border blur of the flattened signal in float32 arithmetic (ATen's conv1d)"""
    x = torch.as_tensor(np.asarray(x, np.float32)).reshape(-1)
    xp = torch.cat([x[:1].expand(r), x, x[-1:].expand(r)])
    return F.conv1d(xp[None, None], torch.as_tensor(np.asarray(taps, np.float32))[None, None]).reshape(-1)


def depth_top4(x):
    """x (planes, D, HW) float32 -> values, depth coordinates (planes, 4, HW): the four largest along depth in descending
    order, the smaller depth index first among equals (numpy's stable argsort of -x), coordinate float32 (D-1-idx) / (D-1)."""
    x = np.asarray(x, np.float32)
    D = x.shape[1]
    idx = np.argsort(-x, axis=1, kind="stable")[:, :4]
    vals = np.take_along_axis(x, idx, axis=1)
    dep = (np.float32(D - 1) - idx.astype(np.float32)) / np.float32(D - 1)
    return vals, dep.astype(np.float32), idx

#!/usr/bin/env python3
"""Generate tests/golden/head_losses.npz from the reference's own utils/criterion.py (JointsMSELoss, JointTarget,
NMTNORMCritierion), run on the CPU.

Run in the dev container only:   python tests/golden/make_head_loss_goldens.py

NMTNORMCritierion.criterion hard-codes `.to('cuda:0')`; for the duration of the run torch.Tensor.to ignores exactly that
argument.  Only inputs and reference OUTPUTS are stored (float32 / float64 arrays):

heat-map   hm_pred (3, 5, 8, 12), hm_joints (3, 5, 2), hm_sigma; per use_target_weight u in (0, 1): hm_loss_u,
           hm_grad_u (autograd gradient with respect to the prediction), hm_flags_u (the target_weight the reference writes back)
JointTarget  jt_joints (5, 2), jt_vis (5, 2), jt_heatmap_size, jt_image_size, jt_sigma; jt_target (5, H, W), jt_weight (5, 1)
SimDR      sd_x (3, 5, 16), sd_y (3, 5, 24), sd_z (3, 5, 7), sd_target (3, 5, 3), sd_weight (3, 5, 1), sd_ls; sd_loss,
           sd_gx, sd_gy, sd_gz
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402

ref_shims.install()

_orig_to = torch.Tensor.to


def _to(self, *a, **k):
    if a and isinstance(a[0], str) and a[0].startswith("cuda"):
        return self
    return _orig_to(self, *a, **k)


torch.Tensor.to = _to

from utils import criterion as RC  # noqa: E402

B, J, H, W = 3, 5, 8, 12


def cfg_node(heatmap_size, image_size, sigma):
    c = ref_shims._AttrDict()
    c.DATASET = ref_shims._AttrDict(NUM_JOINTS=J, TARGET_TYPE="gaussian", HEATMAP_SIZE=heatmap_size, IMAGE_SIZE=image_size,
                                    SIGMA=sigma, USE_DIFFERENT_JOINTS_WEIGHT=True)
    return c


def main():
    out = {}
    g = torch.Generator().manual_seed(2024)
    # ---- heat-map
    base = torch.tensor([[3.3, 2.7], [-2.5, 4.0], [-3.2, 1.0], [13.9, 7.5], [14.0, 3.0]], dtype=torch.float32)
    joints = base[None].repeat(B, 1, 1)
    joints[1, :, 1] = torch.tensor([9.9, 10.0, 0.2, -2.9, -3.1])
    pred = torch.rand(B, J, H, W, generator=g) * 1.2 - 0.1
    out.update(hm_pred=pred.numpy(), hm_joints=joints.numpy(), hm_sigma=np.float64(2))
    for u in (0, 1):
        crit = RC.JointsMSELoss(cfg_node([W, H], [W * 4, H * 4], 2), bool(u))
        p = pred.clone().requires_grad_(True)
        tw = torch.ones(B, J, 1)
        loss = crit(p, joints.clone(), tw, None, 0)
        loss.backward()
        out[f"hm_loss_{u}"] = np.float64(loss.item())
        out[f"hm_grad_{u}"] = p.grad.numpy()
        out[f"hm_flags_{u}"] = tw.numpy().reshape(B, J)
        print(f"heat-map use_target_weight={u}: loss {loss.item():.7f} flags {tw.reshape(B, J).int().tolist()}")
    # ---- JointTarget: sigma' = 2 * 12 // 12 = 2, tmp_size = 6; visibility 0 on one in-range joint, 0.4 / 0.6 on two others
    jt = RC.JointTarget(cfg_node([W, H], [W, H], 2))
    jj = torch.tensor([[3.3, 2.7], [-6.5, 4.0], [-7.2, 1.0], [17.9, 7.5], [18.0, 3.0]], dtype=torch.float32)
    vis = torch.tensor([[1.0, 1.0], [0.6, 1.0], [0.4, 1.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float32)
    t, w = jt.generate_target(jj, vis.numpy())
    out.update(jt_joints=jj.numpy(), jt_vis=vis.numpy(), jt_heatmap_size=np.array([W, H]), jt_image_size=np.array([W, H]),
               jt_sigma=np.float64(2), jt_target=t.numpy(), jt_weight=w.numpy())
    print("JointTarget weights", w.reshape(-1).tolist())
    # ---- SimDR
    bins = (16, 24, 7)
    xs = [torch.randn(B, J, n, generator=g) * 2.0 for n in bins]
    target = torch.stack([torch.randint(0, n, (B, J), generator=g).float() + 0.6 for n in bins], dim=-1)
    weight = torch.rand(B, J, 1, generator=g)
    crit = RC.NMTNORMCritierion(0.2)
    leaves = [x.clone().requires_grad_(True) for x in xs]
    loss = crit(*leaves, target, weight)
    loss.backward()
    out.update(sd_x=xs[0].numpy(), sd_y=xs[1].numpy(), sd_z=xs[2].numpy(), sd_target=target.numpy(), sd_weight=weight.numpy(),
               sd_ls=np.float64(0.2), sd_loss=np.float64(loss.item()), sd_gx=leaves[0].grad.numpy(), sd_gy=leaves[1].grad.numpy(),
               sd_gz=leaves[2].grad.numpy())
    print(f"SimDR: loss {loss.item():.7f}")
    path = os.path.join(HERE, "head_losses.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()

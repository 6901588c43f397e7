#!/usr/bin/env python3
"""What the heads' losses cost.  One JSON line.

    python tools/time_head_losses.py [--steps 5] [--warmup 2] [--rounds 5] [--calls 50]

"step": a TokenPose-L training step (forward, loss, zero_grad, backward, HipAdam step at lr 0) at the geometry of
tools/time_xformer_train.py (dim 192, 3 x depth 2, 8 heads x 24, 16 keypoints, 4 x 4 patches of a 128-channel 64^2 map, 64^2
heat-maps, batch 8), fp32, targets on the host as a data loader hands them over, timed in alternating rounds with
  (a) "hip":       criterion.JointsMSELoss (the B * J * 2 coordinates go up; hp_joints_mse_forward / _backward);
  (b) "reference": the reference-style loss: the B * J target maps built by a host NumPy loop (range test, exp over the whole map
                   for every joint), one host-to-device copy of B * J * H * W floats, then 0.5 * MSE in ATen.
"loss_alone": each loss's forward + backward by itself on device-resident inputs, HIP against ATen on the device (the Gaussian
targets built by broadcasting on the device for the heat-map loss; log_softmax + the smoothed-label KL sum for SimDR at
(8, 16, 3, 256)), median of `--calls` event-timed calls (host launch cost included), the library's per-kernel event times of one
call, the bytes a pass has to move and the time those bytes take at 6.3 TB/s.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hiddenpose_amd import criterion as Cr  # noqa: E402
from hiddenpose_amd import hip_ops as ops  # noqa: E402
from hiddenpose_amd import testing as hpt  # noqa: E402
from hiddenpose_amd.config import get_cfg_defaults  # noqa: E402
from hiddenpose_amd.optimizer import HipAdam  # noqa: E402
from hiddenpose_amd.tokenpose import TokenPose_L_base  # noqa: E402

TP_KW = dict(feature_size=[64, 64], patch_size=[4, 4], num_keypoints=16, dim=192, depth=2, heads=8, mlp_dim=576, heatmap_dim=4096,
             heatmap_size=[64, 64], channels=128, pos_embedding_type="sine-full", hidden_heatmap_dim=384)
B, J, H, W, SIGMA = 8, 16, 64, 64, 2
HBM_BYTES_PER_S = 6.3e12


def host_targets(joints, H, W, sigma):
    """The reference-style target generation: a Python loop over B x J joints, float32 NumPy, exp over the whole map."""
    Bn, Jn = joints.shape[:2]
    out = np.zeros((Bn, Jn, H, W), dtype=np.float32)
    xs = np.arange(W, dtype=np.float32)
    ys = np.arange(H, dtype=np.float32)[:, None]
    for b in range(Bn):
        for j in range(Jn):
            mx, my = joints[b, j, 0], joints[b, j, 1]
            if int(mx - sigma) >= W or int(my - sigma) >= H or int(mx + sigma + 1) < 0 or int(my + sigma + 1) < 0:
                continue
            out[b, j] = np.exp(-((xs - mx) ** 2 + (ys - my) ** 2) / (2 * sigma ** 2))
    return out


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def event_median(fn, calls):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def kernel_profile(fn):
    """The library's per-kernel event timing of one call: {kernel: [launches, ms]}."""
    from hiddenpose_amd import _lib

    fn()
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    return {k: [cnt, round(ms, 4)] for k, (cnt, ms) in sorted(prof.items())}


def step_ab(a):
    cfg = get_cfg_defaults()
    cfg.DATASET.NUM_JOINTS, cfg.DATASET.HEATMAP_SIZE, cfg.DATASET.SIGMA = J, [W, H], SIGMA
    crit = Cr.JointsMSELoss(cfg, False)
    m = TokenPose_L_base(**TP_KW)
    hpt.fill_module(m, "tokenpose.")
    m = m.cuda().train()
    opt = HipAdam(m.parameters(), lr=0.0)
    g = torch.Generator().manual_seed(5)
    feat = torch.rand(B, 128, 64, 64, generator=g).cuda()
    joints = torch.stack((torch.rand(B, J, generator=g) * (W + 8) - 4, torch.rand(B, J, generator=g) * (H + 8) - 4), dim=-1)   # host

    def finish(loss):
        opt.zero_grad()
        loss.backward()
        opt.step()

    def step_hip():
        finish(crit(m(feat), joints, None))

    def step_ref():
        y = m(feat)
        gt = torch.from_numpy(host_targets(joints.numpy(), H, W, SIGMA)).to(y.device)
        finish(0.5 * torch.mean((y - gt) ** 2))

    with torch.no_grad():
        y = m(feat)
        gt = torch.from_numpy(host_targets(joints.numpy(), H, W, SIGMA)).cuda()
        agree = abs(float(crit(y, joints, None)) / float(0.5 * torch.mean((y - gt) ** 2)) - 1)
    for _ in range(a.warmup):
        step_hip()
        step_ref()
    hip, ref = [], []
    for _ in range(a.rounds):
        step_hip()
        hip.append(timed(step_hip, a.steps))
        step_ref()
        ref.append(timed(step_ref, a.steps))
    t0 = time.perf_counter()
    for _ in range(20):
        host_targets(joints.numpy(), H, W, SIGMA)
    host_ms = (time.perf_counter() - t0) * 1e3 / 20
    med = lambda v: sorted(v)[len(v) // 2]
    return {"batch": B, "rounds": a.rounds, "steps_per_round": a.steps, "hip_ms": [round(t, 3) for t in hip],
            "reference_ms": [round(t, 3) for t in ref], "median_hip_ms": round(med(hip), 3), "median_reference_ms": round(med(ref), 3),
            "hip_minus_reference_ms": round(med(hip) - med(ref), 3), "hip_spread_ms": round(max(hip) - min(hip), 3),
            "reference_spread_ms": round(max(ref) - min(ref), 3), "host_target_loop_ms": round(host_ms, 3),
            "target_copy_bytes": B * J * H * W * 4, "losses_agree_rel": agree}


def loss_alone(a):
    g = torch.Generator().manual_seed(6)
    out = {}
    # ---- heat-map
    pred = torch.rand(B, J, H, W, generator=g).cuda().requires_grad_(True)
    joints = torch.stack((torch.rand(B, J, generator=g) * (W + 8) - 4, torch.rand(B, J, generator=g) * (H + 8) - 4), dim=-1).cuda()
    flags = torch.from_numpy((host_targets(joints.cpu().numpy(), H, W, SIGMA).reshape(B, J, -1).max(-1) > 0).astype(np.float32)).cuda()
    xs, ys = torch.arange(W, device="cuda", dtype=torch.float32), torch.arange(H, device="cuda", dtype=torch.float32)[:, None]

    def hm_hip():
        pred.grad = None
        ops.joints_mse(pred, joints, SIGMA, False)[0].backward()

    def hm_aten():
        pred.grad = None
        gt = torch.exp(-((xs - joints[:, :, 0, None, None]) ** 2 + (ys - joints[:, :, 1, None, None]) ** 2) / (2 * SIGMA ** 2))
        (0.5 * torch.mean((pred - gt * flags[:, :, None, None]) ** 2)).backward()

    n = B * J * H * W
    moved = 3 * n * 4      # forward reads pred; backward reads pred and writes dpred
    out["heatmap"] = {"shape": [B, J, H, W], "hip_ms": round(event_median(hm_hip, a.calls), 4), "aten_device_ms": round(event_median(hm_aten, a.calls), 4),
                      "hip_kernels_ms": kernel_profile(hm_hip), "bytes_moved": moved, "ms_at_hbm_rate": round(moved / HBM_BYTES_PER_S * 1e3, 6)}
    # ---- SimDR
    bins, ls = 256, 0.2
    packed = torch.randn(B, J, 3, bins, generator=g).cuda().requires_grad_(True)
    target = (torch.randint(0, bins, (B, J, 3), generator=g).float() + 0.6).cuda()
    k = torch.arange(bins, device="cuda")

    def sd_hip():
        packed.grad = None
        ops.simdr_loss(packed[:, :, 0], packed[:, :, 1], packed[:, :, 2], target, None, ls).backward()

    def sd_aten():
        packed.grad = None
        s = torch.log_softmax(packed, dim=-1)
        t = torch.where(k == target.long()[..., None], 1.0 - ls, ls / (bins - 1))
        ((t * (t.log() - s)).sum(-1) / bins).sum().div(B * J).backward()

    n = B * J * 3 * bins
    moved = 3 * n * 4
    out["simdr"] = {"shape": [B, J, 3, bins], "hip_ms": round(event_median(sd_hip, a.calls), 4), "aten_device_ms": round(event_median(sd_aten, a.calls), 4),
                    "hip_kernels_ms": kernel_profile(sd_hip), "bytes_moved": moved, "ms_at_hbm_rate": round(moved / HBM_BYTES_PER_S * 1e3, 6)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the hip / reference step comparison")
    ap.add_argument("--calls", type=int, default=50, help="event-timed calls of each loss alone")
    a = ap.parse_args()
    print(json.dumps({"step": step_ab(a), "loss_alone": loss_alone(a)}))


if __name__ == "__main__":
    main()

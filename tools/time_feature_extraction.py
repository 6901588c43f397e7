#!/usr/bin/env python3
"""Time FeatureExtraction(basedim, stride) forward and forward + backward at a given input size, next to the ATen
composition of the same arithmetic on the same device (F.pad(replicate) + F.conv3d(stride) for the learned branch and both
ResConv3D blocks, F.conv3d(stride, padding 1) for the box branch, then the broadcast add), and the entry kernel alone
(hp_fe_entry_forward / hp_fe_entry_backward) against the bytes it must move.

    python tools/time_feature_extraction.py --dims 1024 256 256 --batch 1 --basedim 1 2 4 --stride 2

Times are device-event means over --iters runs after --warmup runs.  Entry forward bytes: 4 * (V_in + (C + 1) * V_out),
V_out = V_in / stride^3 for even extents.  "entry param grads" is the difference of two separately timed loops, (entry forward +
backward without gx) - (entry forward), set against the same byte count (one read of x, ga and gbox); the per-workgroup partial
records and the reducer's reads of them are not counted."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from hiddenpose_amd import hip_ops as ops
from hiddenpose_amd import testing as hpt
from hiddenpose_amd.feature_extraction import FeatureExtraction


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def aten_forward(fe, x):
    rp = lambda t: F.pad(t, (1,) * 6, mode="replicate")
    a = F.conv3d(rp(x), fe.conv1[1].weight, fe.conv1[1].bias, stride=fe.stride)
    for blk in (fe.conv1[2], fe.conv1[3]):
        h = F.leaky_relu(F.conv3d(rp(a), blk.tmp[1].weight, blk.tmp[1].bias), 0.2)
        a = F.leaky_relu(a + F.conv3d(rp(h), blk.tmp[4].weight, blk.tmp[4].bias), 0.2)
    return a + F.conv3d(x, fe.weights, stride=fe.stride, padding=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 256], metavar=("T", "H", "W"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--basedim", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-aten", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    T, H, W = args.dims
    B, s = args.batch, args.stride
    x = torch.rand(B, 1, T, H, W, device="cuda")
    vin = x.numel()
    for C in args.basedim:
        fe = FeatureExtraction(C, 1, stride=s)
        hpt.fill_module(fe, "feature_extraction.")
        fe = fe.cuda()
        with torch.no_grad():
            y = fe(x)
            err = float((y - aten_forward(fe, x)).norm() / y.norm()) if not args.no_aten else float("nan")
        gy = torch.rand_like(y)
        vout = y.numel() // C

        def hip_fwd():
            with torch.no_grad():
                fe(x)

        def hip_fwd_bwd():
            fe.zero_grad(set_to_none=True)
            (fe(x) * gy).sum().backward()

        def aten_fwd():
            with torch.no_grad():
                aten_forward(fe, x)

        def aten_fwd_bwd():
            fe.zero_grad(set_to_none=True)
            (aten_forward(fe, x) * gy).sum().backward()

        w, b, wb = fe.conv1[1].weight.detach(), fe.conv1[1].bias.detach(), fe.weights.detach()
        entry_bytes = 4 * (vin + (C + 1) * vout)
        line = f"basedim {C} stride {s} input {tuple(x.shape)} -> {tuple(y.shape)}  (HIP vs ATen forward rel-L2 {err:.1e})\n"
        if (s, C) != (1, 1):
            a, box = ops.fe_entry(x, w, b, wb, s)
            ga, gb = torch.rand_like(a), torch.rand_like(box)
            wr, br, wbr = (t.clone().requires_grad_(True) for t in (w, b, wb))

            def entry_bwd():
                aa, bb = ops.fe_entry(x, wr, br, wbr, s)
                torch.autograd.grad([aa, bb], [wr, br, wbr], [ga, gb])

            t_e = timed(lambda: ops.fe_entry(x, w, b, wb, s), args.warmup, args.iters)
            t_eb = timed(entry_bwd, args.warmup, args.iters) - t_e
            line += (f"  entry forward      {t_e:8.3f} ms  {entry_bytes / t_e / 1e6:7.0f} GB/s of {entry_bytes / 1e9:.3f} GB\n"
                     f"  entry param grads  {t_eb:8.3f} ms  {entry_bytes / t_eb / 1e6:7.0f} GB/s of {entry_bytes / 1e9:.3f} GB   [(fwd+bwd) - fwd of two timed loops;"
                     f" bytes = one read of x, ga, gbox: partial records and the reducer's reads not counted]\n")
        line += f"  HIP  forward {timed(hip_fwd, args.warmup, args.iters):8.3f} ms   forward+backward {timed(hip_fwd_bwd, args.warmup, args.iters):8.3f} ms\n"
        if not args.no_aten:
            line += f"  ATen forward {timed(aten_fwd, args.warmup, args.iters):8.3f} ms   forward+backward {timed(aten_fwd_bwd, args.warmup, args.iters):8.3f} ms\n"
        print(line, flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/frame_mask.npz: the reference TimeSformer (models/transformer.py:208-253) run with a frame mask,
imported through ref_shims.install() as make_xformer_grad_goldens.py does.

Run in the dev container only:   python tests/golden/make_frame_mask_goldens.py

Four configs (CONFIGS below), batch 2, one (f,) bool mask per sample (True = valid frame).  Weights and video as
tests/test_xformers.py `_ts`: fill_module(m, "timesformer.") + the cls_token fill and the seed-78 torch.rand video.  The
model and the input in float64, train mode; loss L = sum(y * R) with R = randn(seed 78).  Stored per config `key`:
  {key}_cfg     the constructor keywords (JSON), {key}_mask the (2, f) bool mask
  {key}_y       the output (float64)
  {key}_input   the input gradient in full (float32)
  {key}/{name}  every parameter gradient of at most 4096 elements in full (float32); larger ones as {key}/{name}/l2 (their L2
                norm) and {key}/{name}/val (64 sampled entries: sample_idx, seed 5)
  {key}_none    the names of the parameters whose .grad stays None
and for plain6 `plain6_y_trunc4`: the output for sample 0's first 4 frames with mask=None (a prefix mask equals truncation).
Only reference OUTPUTS, the masks and the config dicts are stored.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402

ref_shims.install()

from hiddenpose_amd import testing as hpt  # noqa: E402
from make_xformer_grad_goldens import FULL_MAX, NSAMPLE, sample_idx  # noqa: E402
from test_xformers import TS  # noqa: E402

PLAIN6 = dict(TS["plain"], num_frames=6)
CONFIGS = {   # key: (constructor keywords, mask of sample 0, mask of sample 1)
    "plain6": (PLAIN6, "111100", "111111"),
    "scatter": (PLAIN6, "101101", "011111"),
    "dh64": (dict(dim=64, num_frames=5, num_classes=10, image_size=32, patch_size=8, channels=1, depth=2, heads=2, dim_head=64),
             "11100", "10011"),
    "shift": (dict(TS["shift"], num_frames=5), "11110", "11011"),
}


def bits(s):
    return [c == "1" for c in s]


def build(kw):
    from models.transformer import TimeSformer

    with contextlib.redirect_stdout(io.StringIO()):
        m = TimeSformer(**kw)
    hpt.fill_module(m, "timesformer.")
    with torch.no_grad():
        m.cls_token.copy_(hpt.fill_value("timesformer.cls_token", m.cls_token.shape))
    g = torch.Generator().manual_seed(78)
    video = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"], generator=g)
    return m.double().train(), video.double()


def main():
    out = {}
    for key, (kw, m0, m1) in CONFIGS.items():
        m, video = build(kw)
        mask = torch.tensor([bits(m0), bits(m1)], dtype=torch.bool)
        x = video.clone().requires_grad_(True)
        y = m(x, mask=mask)
        R = torch.randn(y.shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)
        (y * R).sum().backward()
        none = sorted(k for k, p in m.named_parameters() if p.grad is None)
        out[f"{key}_cfg"] = np.array(json.dumps(kw))
        out[f"{key}_mask"] = mask.numpy()
        out[f"{key}_y"] = y.detach().numpy()
        out[f"{key}_none"] = np.array(none, dtype=str)
        out[f"{key}_input"] = x.grad.float().numpy()
        for k, p in m.named_parameters():
            if p.grad is None:
                continue
            gr = p.grad.reshape(-1)
            if gr.numel() <= FULL_MAX:
                out[f"{key}/{k}"] = p.grad.float().numpy()
            else:
                out[f"{key}/{k}/l2"] = np.array(float(gr.norm()), np.float64)
                out[f"{key}/{k}/val"] = gr[torch.from_numpy(sample_idx(gr.numel(), NSAMPLE, 5))].float().numpy()
        print(f"  {key}: y {tuple(y.shape)}, {len(none)} parameters without a gradient {none}")
        if key == "plain6":
            with torch.no_grad():
                yt = m(video[:1, :4])
            out["plain6_y_trunc4"] = yt.numpy()
            print(f"  plain6: |y[0] - y_trunc4| max {float((yt[0] - y[0].detach()).abs().max()):.2e}")
    path = os.path.join(HERE, "frame_mask.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote frame_mask.npz: {os.path.getsize(path)/1024:.1f} KiB")


if __name__ == "__main__":
    main()

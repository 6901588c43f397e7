#!/usr/bin/env python3
"""Generate tests/golden/head64.npz: the reference's three transformer heads at dim_head 64 (the constructors' default
width), outputs and gradients under autograd, imported through ref_shims.install() as make_goldens.py does.

Run in the dev container only:   python tests/golden/make_head64_goldens.py

Configs `SF`, `TS` (plain, shift) and `TP` (learnable) of tests/test_head64.py with the weight fills and inputs of the
existing generators (fill_module(m, "sformer.") and the seed-77 video; fill_module(m, "timesformer.") + the cls_token fill
and the seed-78 video; fill_module(m, "tokenpose.") and the seed-79 feature map); the model and the input in float64, train
mode; loss L = sum(y * R) with R = randn(seed 78).  Stored (float32) per case `key`: the output `key_y`, the input gradient
`key_input`, every parameter gradient of at most 4096 elements in full (`key/name`), larger ones as their L2 norm and 64
sampled entries (`key/name/l2`, `key/name/val`; sample_idx, seed 5), and `key_none`, the names of the parameters whose .grad
stays None.  Only reference OUTPUTS are stored.
"""
from __future__ import annotations

import contextlib
import io
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
from test_head64 import SF, TP, TS  # noqa: E402

FULL_MAX = 4096
NSAMPLE = 64


def sample_idx(n_total: int, n: int, seed: int) -> np.ndarray:
    return np.random.Generator(np.random.PCG64(seed)).choice(n_total, size=min(n, n_total), replace=False).astype(np.int64)


def record(out, key, m, x):
    y = m(x)
    R = torch.randn(y.shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)
    (y * R).sum().backward()
    none = sorted(k for k, p in m.named_parameters() if p.grad is None)
    out[f"{key}_none"] = np.array(none, dtype=str)
    out[f"{key}_y"] = y.detach().float().numpy()
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


def main():
    from models.NlosPoseSformer import NlosPoseSformer
    from models.tokenpose import TokenPose_L_base
    from models.transformer import TimeSformer

    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        m = NlosPoseSformer(**SF)
    hpt.fill_module(m, "sformer.")
    m = m.double().train()
    video = torch.rand(2, SF["num_frames"], SF["channels"], SF["image_size"], SF["image_size"], generator=torch.Generator().manual_seed(77))
    record(out, "sf", m, video.double().requires_grad_(True))
    for tag, kw in TS.items():
        with contextlib.redirect_stdout(io.StringIO()):
            m = TimeSformer(**kw)
        hpt.fill_module(m, "timesformer.")
        with torch.no_grad():
            m.cls_token.copy_(hpt.fill_value("timesformer.cls_token", m.cls_token.shape))
        m = m.double().train()
        g = torch.Generator().manual_seed(78)
        video = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"], generator=g)
        record(out, "ts_" + tag, m, video.double().requires_grad_(True))
    for tag, kw in TP.items():
        with contextlib.redirect_stdout(io.StringIO()):
            m = TokenPose_L_base(**kw)
        hpt.fill_module(m, "tokenpose.")
        m = m.double().train()
        g = torch.Generator().manual_seed(79)
        feat = torch.rand(2, kw["channels"], kw["feature_size"][0], kw["feature_size"][1], generator=g)
        record(out, "tp_" + tag, m, feat.double().requires_grad_(True))
    path = os.path.join(HERE, "head64.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote head64.npz: {os.path.getsize(path)/1024:.1f} KiB")


if __name__ == "__main__":
    main()

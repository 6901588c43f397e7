#!/usr/bin/env python3
"""Generate tests/golden/feature_extraction_strided.npz: the reference's FeatureExtraction (models/feature_extraction.py:122-171)
at stride 2 and at basedim > 1, and its NlosPose behind a stride-2 FeatureExtraction, imported through ref_shims.install() as
make_goldens.py does.

Run in the dev container only:   python tests/golden/make_feature_extraction_goldens.py

Module cases (tests/test_fe_strided_gpu.py, MODULE_CASES): key -> (basedim, stride or None = the constructor's default, input
(B, T, H, W)).  The input is the "transient" synthetic_meas(B, T, max(H, W)) of seed 410 cropped to (T, H, W), the parameters
are fill_module(fe, "feature_extraction."), the loss is sum(y * gy) with gy = the "uniform" synthetic_meas of seed 101 (one
draw per channel, seeds 101 + 7 * c) - 0.5, cropped to y.  Stored per case: `key_y`, `key_gx` and `key_g_<parameter>`.

Network case `net`: the reference NlosPose (ref_shims.make_cfg(32, 32, 0.16), fill_module) whose feature_extraction is replaced
by FeatureExtraction(1, 1, stride=2) with the same fill, on the (2,1,64,64,64) transient of seed 410, eval mode:
`net_eval_heat`, `net_eval_refine`.  Only reference OUTPUTS are stored (float32).

Size: about 970 KiB compressed (under the 1 MiB limit of a committed file), nearly all of it the network case: the test
compares the full heat (2,24,16,16,16) and refine (2,1,32,32,32) tensors as the e2e_T32_N32 eval test does; the three module
cases together are a few KB.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402

ref_shims.install()

from hiddenpose_amd import testing as hpt  # noqa: E402

MODULE_CASES = {"c2_default": (2, None, (2, 8, 10, 12)), "c3_s1": (3, 1, (2, 5, 6, 7)), "c1_s2": (1, 2, (2, 7, 9, 11))}


def module_input(dims):
    B, T, H, W = dims
    return hpt.synthetic_meas(B, T, max(H, W), "transient", seed=410)[:, :, :, :H, :W].contiguous()


def module_gy(shape):
    B, C, T, H, W = shape
    n = max(H, W)
    return torch.cat([hpt.synthetic_meas(B, T, n, "uniform", seed=101 + 7 * c)[:, :, :, :H, :W] for c in range(C)], 1).contiguous() - 0.5


def main():
    from models.feature_extraction import FeatureExtraction
    from models.NlosPose import NlosPose

    out = {}
    for key, (basedim, stride, dims) in MODULE_CASES.items():
        fe = FeatureExtraction(basedim, 1) if stride is None else FeatureExtraction(basedim, 1, stride=stride)
        hpt.fill_module(fe, "feature_extraction.")
        x = module_input(dims).requires_grad_(True)
        y = fe(x)
        (y * module_gy(y.shape)).sum().backward()
        out[key + "_y"] = y.detach().numpy()
        out[key + "_gx"] = x.grad.numpy()
        for k, p in fe.named_parameters():
            out[key + "_g_" + k] = p.grad.numpy()
        print(f"  {key}: stride {fe.stride}, {tuple(x.shape)} -> {tuple(y.shape)}")

    model = NlosPose(ref_shims.make_cfg(32, 32, 0.16))
    hpt.fill_module(model)
    fe = FeatureExtraction(1, 1, stride=2)
    hpt.fill_module(fe, "feature_extraction.")
    model.feature_extraction = fe
    model.eval()
    with torch.no_grad():
        heat, refine = model(hpt.synthetic_meas(2, 64, 64, "transient", seed=410))
    out["net_eval_heat"] = heat.numpy()
    out["net_eval_refine"] = refine.numpy()
    print(f"  net: heat {tuple(heat.shape)}, refine {tuple(refine.shape)}")
    path = os.path.join(HERE, "feature_extraction_strided.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote feature_extraction_strided.npz: {os.path.getsize(path)/1024:.1f} KiB")


if __name__ == "__main__":
    main()

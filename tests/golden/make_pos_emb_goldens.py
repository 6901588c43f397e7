#!/usr/bin/env python3
"""Generate tests/golden/pos_emb.npz: the reference TimeSformer (models/transformer.py:182-187, :229-235) and NlosPoseSformer
(models/NlosPoseSformer.py:55-60, :113-119) built with rotary_emb=False -- a learned position table added to the token
matrix, no rotary embedding -- imported through ref_shims.install() as make_frame_mask_goldens.py does.

Run in the dev container only:   python tests/golden/make_pos_emb_goldens.py

Six cases (CASES below), batch 2.  Weights: fill_module(m, prefix) with prefix "timesformer." / "sformer.", the cls_token fill
of tests/test_xformers.py `_ts`, and the table from fill_value(prefix + "pos_emb.weight" / "pose_emb.weight", shape).  Video:
torch.rand of (2, num_frames, channels, image_size, image_size) with seed 78, cut to the case's first f frames.  The model and
the input in float64, train mode; loss L = sum(y * R) with R = randn(seed 78).  Stored per case `key`:
  {key}_cfg     the constructor keywords (JSON), {key}_f the clip's frame count, {key}_mask the (2, f) bool mask (ts_mask only)
  {key}_sd      the sorted [name, shape] list of the module's state_dict (JSON)
  {key}_y       the output (float64)
  {key}_input   the input gradient in full (float32)
  {key}/{name}  every parameter gradient of at most 4096 elements in full (float32); larger ones as {key}/{name}/l2 (their L2
                norm) and {key}/{name}/val (64 sampled entries: sample_idx, seed 5)
  {key}_none    the names of the parameters whose .grad stays None
Only reference OUTPUTS, the masks and the settings are stored.  Size: the six input gradients (51200 float32) and the full
parameter gradients of the three dim-64 cases (about 22500 float32 each) are 470 KiB before anything else, so the file (620 KiB)
is larger than frame_mask.npz (four cases, 457 KiB); it stays well under the limit for a committed file.

Two facts of the reference that the project's modules keep are asserted here:
  * the table has num_frames * num_patches + 1 rows and NlosPoseSformer's 24 joint tokens take 24 of them, so sf_short's module
    runs f = 2 and raises IndexError at f = 3;
  * the rows of the table behind a short clip's tokens get an exactly zero gradient (ts_short: the last 16 rows).
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
from make_frame_mask_goldens import CONFIGS as MASK_CONFIGS  # noqa: E402
from make_xformer_grad_goldens import FULL_MAX, NSAMPLE, sample_idx  # noqa: E402
from test_xformers import TS  # noqa: E402

PLAIN = dict(TS["plain"], rotary_emb=False)
SF = dict(dim=48, num_frames=8, image_size=16, patch_size=8, channels=2, depth=2, heads=2, dim_head=16, out_dim=24, rotary_emb=False)
CASES = {   # key: (module, constructor keywords, frames of the clip, masks of samples 0 / 1 or None)
    "ts_plain": ("ts", PLAIN, 4, None),
    "ts_short": ("ts", PLAIN, 3, None),
    "ts_mask": ("ts", dict(PLAIN, num_frames=6), 6, ("111100", "101101")),
    "ts_shift": ("ts", dict(TS["shift"], rotary_emb=False), 3, None),
    "ts_dh64": ("ts", dict(MASK_CONFIGS["dh64"][0], rotary_emb=False), 5, None),
    "sf_short": ("sf", SF, 2, None),
}


def bits(s):
    return [c == "1" for c in s]


def build(kind, kw):
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "ts":
            from models.transformer import TimeSformer

            m, prefix, table = TimeSformer(**kw), "timesformer.", "pos_emb"
        else:
            from models.NlosPoseSformer import NlosPoseSformer

            m, prefix, table = NlosPoseSformer(**kw), "sformer.", "pose_emb"
    hpt.fill_module(m, prefix)
    with torch.no_grad():
        if kind == "ts":
            m.cls_token.copy_(hpt.fill_value("timesformer.cls_token", m.cls_token.shape))
        w = getattr(m, table).weight
        w.copy_(hpt.fill_value(f"{prefix}{table}.weight", w.shape))
    g = torch.Generator().manual_seed(78)
    video = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"], generator=g)
    return m.double().train(), video.double(), f"{table}.weight"


def main():
    out = {}
    for key, (kind, kw, f, masks) in CASES.items():
        m, video, table = build(kind, kw)
        assert not any("rot_emb" in k for k in m.state_dict()), key
        x = video[:, :f].clone().requires_grad_(True)
        mask = None if masks is None else torch.tensor([bits(s) for s in masks], dtype=torch.bool)
        y = m(x) if mask is None else m(x, mask=mask)
        R = torch.randn(y.shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)
        (y * R).sum().backward()
        none = sorted(k for k, p in m.named_parameters() if p.grad is None)
        out[f"{key}_cfg"] = np.array(json.dumps(kw))
        out[f"{key}_f"] = np.array(f, np.int64)
        if mask is not None:
            out[f"{key}_mask"] = mask.numpy()
        out[f"{key}_sd"] = np.array(json.dumps(sorted([k, list(v.shape)] for k, v in m.state_dict().items())))
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
        n = (kw["image_size"] // kw["patch_size"]) ** 2
        ntok = (1 if kind == "ts" else 24) + f * n
        tg = dict(m.named_parameters())[table].grad
        unused = tg[ntok:]
        print(f"  {key}: y {tuple(y.shape)}, table {tuple(tg.shape)}, {ntok} rows used, |grad| max in the {unused.shape[0]} unused rows "
              f"{float(unused.abs().max()) if unused.numel() else 0.0}, {len(none)} parameters without a gradient {none}")
        assert unused.numel() == 0 or float(unused.abs().max()) == 0.0, key
        assert float(tg[:ntok].abs().min(dim=1).values.max()) > 0.0, key
        if key == "ts_short":
            assert unused.shape[0] == 16
        if key == "sf_short":
            for longer in (3, 8):
                try:
                    m(video[:, :longer])
                except IndexError as e:
                    print(f"  sf_short: f = {longer} raises IndexError ({e})")
                else:
                    raise AssertionError(f"sf_short: the reference ran f = {longer}")
    path = os.path.join(HERE, "pos_emb.npz")
    np.savez_compressed(path, **out)
    raw = sum(v.nbytes for v in out.values())
    print(f"  wrote pos_emb.npz: {os.path.getsize(path)/1024:.1f} KiB ({raw/1024:.1f} KiB of arrays before compression)")


if __name__ == "__main__":
    main()

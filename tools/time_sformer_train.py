#!/usr/bin/env python3
"""NlosPoseSformer training-step timing at the BASELINE config-5 geometry (dim 256, depth 8, 8 x 32 heads, patch 4, 16 frames
of 128^2, fp32, seeded input): no-graph forward, graph-mode forward, backward, the library's per-kernel profile of one
step, the attention backward's rate on the five-product count and the peak device memory; the attention forward's kernel
time in fp32 (from the step) and with fp16 patch attention (a no-graph forward of its own).  One JSON line.

    python tools/time_sformer_train.py [--batch 8] [--steps 5] [--warmup 2] [--heads 8] [--dim-head 32]
                                       [--attention fp32|bf16|fp16] [--attention-backward fp32|bf16|fp16] [--linear fp32|bf16]
                                       [--dropout P] [--ab-rounds 5] [--no-rotary] [--ab-calls 20]

--no-rotary builds the module with rotary_emb=False (the learned position table).  Its table has 16 * 1024 + 1
rows of which the 24 joint tokens take 24, so the longest clip that fits has 15 frames: every figure is then taken on 15
frames.  "token_assembly_ab" adds the token assembly alone at that geometry, forward + backward, the two HIP entries against
the copy-and-add composition they replace (tools/time_xformer_train.py token_assembly_ab; median of --ab-calls calls).
--dropout P sets attn_dropout = ff_dropout = P and a dropout_seed (seeded Philox dropout): every figure is then
taken with dropout active, and "dropout_ab" adds the step with dropout 0 against dropout P in alternating rounds.
--attention / --attention-backward are NlosPoseSformer.attention_precision / attention_backward_precision (a 16-bit forward
needs a 16-bit backward to train).  The attention backward's time is reported on the same five-product FLOP count at every
precision, as a fraction of the fp32 MFMA peak, of the 2.5 PF/s bf16 MFMA peak, and as exponentials per second (two per score:
the key pass and the query pass each recompute P), since at dim_head 32 the 16-bit attention is bound by v_exp_f32 and the
MFMA fraction alone is the wrong yardstick.

--heads / --dim-head change the head split only (dim stays 256): `--heads 4 --dim-head 64` is the same inner width, the same
Q.K^T and P.V FLOPs and the same bytes as the default 8 x 32, with half the soft-max work.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hiddenpose_amd import _lib  # noqa: E402
from hiddenpose_amd import testing as hpt  # noqa: E402
from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer  # noqa: E402

FP32_MFMA_PEAK = 157.3e12
BF16_MFMA_PEAK = 2.5e15


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def dropout_ab(step, set_dropout, p, rounds, steps):
    """The training step with dropout 0 against dropout p: same process, alternating rounds of `steps` timed steps each.
    -> per-round times, medians, the overhead and the spread (max - min) of the dropout-0 leg."""
    off, on = [], []
    for _ in range(rounds):
        set_dropout(0.0)
        step()
        off.append(timed(step, steps))
        set_dropout(p)
        step()
        on.append(timed(step, steps))
    med = lambda v: sorted(v)[len(v) // 2]
    return {"p": p, "rounds": rounds, "steps_per_round": steps, "off_ms": [round(t, 2) for t in off], "on_ms": [round(t, 2) for t in on],
            "median_off_ms": round(med(off), 2), "median_on_ms": round(med(on), 2), "overhead_ms": round(med(on) - med(off), 2),
            "off_spread_ms": round(max(off) - min(off), 2), "on_spread_ms": round(max(on) - min(on), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.0, help="attn_dropout = ff_dropout = P, with a dropout_seed")
    ap.add_argument("--ab-rounds", type=int, default=5, help="alternating rounds of the dropout 0 / P comparison")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--dim-head", type=int, default=32)
    ap.add_argument("--attention", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--attention-backward", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--linear", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--no-rotary", action="store_true", help="rotary_emb=False on the longest clip that fits (15 frames)")
    ap.add_argument("--ab-calls", type=int, default=20, help="timed calls per leg of the token assembly's A/B")
    a = ap.parse_args()
    if a.attention != "fp32" and a.attention_backward == "fp32":
        ap.error("a 16-bit --attention trains only with a 16-bit --attention-backward")
    kw = dict(dim=256, num_frames=16, num_joints=24, image_size=128, patch_size=4, channels=1, depth=8, heads=a.heads,
              dim_head=a.dim_head, out_dim=512, rotary_emb=not a.no_rotary)
    frames = 15 if a.no_rotary else 16
    m = NlosPoseSformer(**kw)
    hpt.fill_module(m, "sformer.")
    m = m.cuda()
    m.attention_precision, m.attention_backward_precision, m.linear_precision = a.attention, a.attention_backward, a.linear

    def set_dropout(p):
        m.attn_dropout = m.ff_dropout = p
        m.dropout_seed = 1234 if p > 0 else None

    set_dropout(a.dropout)
    B = a.batch
    video = torch.rand(B, frames, 1, 128, 128, generator=torch.Generator().manual_seed(5)).cuda()
    R = torch.randn(B, 24, 4, 128, generator=torch.Generator().manual_seed(6)).cuda()

    def fwd_nograd():
        with torch.no_grad():
            m.eval()(video)

    state = {}

    def fwd_graph():
        state["y"] = m.train()(video)

    def step():
        y = m.train()(video)
        m.zero_grad(set_to_none=True)
        (y * R).sum().backward()

    for _ in range(a.warmup):
        fwd_nograd()
        step()
    t_nograd = timed(fwd_nograd, a.steps)
    t_graph = timed(fwd_graph, a.steps)
    state.clear()
    t_step = timed(step, a.steps)
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    # per-kernel times of one step, in a run of its own (HIP events around every launch)
    _lib.profile_enable(True)
    _lib.profile_reset()
    step()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    ab = dropout_ab(step, set_dropout, a.dropout, a.ab_rounds, a.steps) if a.dropout > 0 else None
    attn_fwd = lambda pr: sum(ms for k, (_, ms) in pr.items() if k.startswith("sformer_attention_"))
    attn_fwd_ms = attn_fwd(prof)
    # the same forward with the fp16 patch attention: a no-graph forward, profiled on its own
    m.attention_precision = "fp16"
    fwd_nograd()
    _lib.profile_enable(True)
    _lib.profile_reset()
    fwd_nograd()
    torch.cuda.synchronize()
    prof16 = _lib.profile_read()
    attn_fwd_fp16_ms = attn_fwd(prof16)
    patch_fp16_ms = prof16.get("sformer_attention_patch", (0, 0.0))[1]
    _lib.profile_enable(False)
    m.attention_precision = a.attention
    f, n, nj, heads, dh, depth = frames, 32 * 32, 24, a.heads, a.dim_head, 8
    ntok = nj + f * n
    flops = depth * (5 * 2 * B * heads * f * n * (nj + n) * dh + 5 * 2 * B * heads * nj * ntok * dh)
    attn_ms = sum(ms for k, (_, ms) in prof.items() if k.startswith("sformer_attn_bwd"))
    rate = flops / (attn_ms * 1e-3) if attn_ms else 0.0
    exps = depth * 2 * (B * heads * f * n * (nj + n) + B * heads * nj * ntok)
    assembly = None
    if a.no_rotary:
        from time_xformer_train import token_assembly_ab

        assembly = token_assembly_ab(B, nj, ntok, kw["dim"], m.pose_emb.weight.shape[0], a.ab_calls)
    print(json.dumps({
        "config": "config5", "batch": B, "rotary_emb": not a.no_rotary, "frames": frames, "token_assembly_ab": assembly, "precision": a.linear, "attention": a.attention, "attention_backward": a.attention_backward,
        "heads": a.heads, "dim_head": a.dim_head, "dropout": a.dropout, "dropout_ab": ab,
        "forward_nograd_ms": round(t_nograd, 2), "forward_graph_ms": round(t_graph, 2),
        "backward_ms": round(t_step - t_graph, 2), "step_ms": round(t_step, 2), "step_over_nograd_forward": round(t_step / t_nograd, 2),
        "attention_forward_ms": round(attn_fwd_ms, 2), "attention_forward_fp16_ms": round(attn_fwd_fp16_ms, 2),
        "attention_patch_fp16_ms": round(patch_fp16_ms, 2),
        "attention_backward_ms": round(attn_ms, 2), "attention_backward_tflops": round(rate / 1e12, 1),
        "attention_backward_fraction_of_fp32_mfma_peak": round(rate / FP32_MFMA_PEAK, 3),
        "attention_backward_fraction_of_bf16_mfma_peak": round(rate / BF16_MFMA_PEAK, 4),
        "attention_backward_gexp_per_s": round(exps / (attn_ms * 1e-3) / 1e9, 1) if attn_ms else 0.0,
        "peak_memory_gb": round(peak / 1e9, 2),
        "kernels_ms": {k: [cnt, round(ms, 3)] for k, (cnt, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1])},
    }))


if __name__ == "__main__":
    main()

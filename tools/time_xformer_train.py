#!/usr/bin/env python3
"""TimeSformer and TokenPose-L training-step timing (fp32 unless told otherwise, seeded inputs): per head the no-graph forward, graph-mode forward,
backward, whole step, the library's per-kernel profile of one step and the peak device memory; the A/B of the time
attention's backward (hp_sformer_attention_backward_grouped against the generic hp_sformer_attention_backward, same saved
inputs, same process, median of the timed calls); the device's maxGridSize; and whether the no-graph TimeSformer forward
(time attention grid y = B * heads * hp * wp) launches at batch 8.  One JSON line.

    python tools/time_xformer_train.py [--steps 5] [--warmup 2] [--ab-calls 20] [--heads 8] [--dim-head 32]
                                       [--valid-frames K] [--timesformer-only]
                                       [--attention fp32|bf16|fp16] [--attention-backward fp32|bf16|fp16] [--linear fp32|bf16]
                                       [--dropout P] [--ab-rounds 5] [--no-rotary]

--no-rotary builds TimeSformer with rotary_emb=False (the learned position table; TokenPose-L has no such
switch and runs as always) and adds "token_assembly_ab": the token assembly alone at the step's geometry, forward + backward,
hp_tokens_assemble_forward / _backward against the copy-and-add composition they replace (two slice copies and an add of a
batch-sized copy of the table; two batch sums, a zero-filled table tail and a slice copy), median of --ab-calls timed calls
each, alternating.
--dropout P sets every dropout probability of both heads to P and a dropout_seed (seeded Philox dropout): the
heads' figures are then taken with dropout active, and each head's "dropout_ab" adds the step with dropout 0 against dropout
P in alternating rounds.
--heads / --dim-head set TimeSformer's head split (dim stays 256).  TokenPose-L keeps dim 192 and its 8 heads of 24 unless
--dim-head is given: then it runs 192 // dim_head heads (3 heads of 64).  The grouped time-attention backward is not built
for dim_head 64; the A/B is skipped there and the step takes the generic entry.
--valid-frames K runs the TimeSformer timing with a frame mask (TimeSformer.forward(video, mask)): a prefix mask of K valid
frames on every sample (K = 16: the all-true mask, i.e. the masked kernels on the unmasked problem).  --timesformer-only
skips the time-attention A/B, TokenPose-L and the batch-8 launch.
--attention / --attention-backward / --linear are both heads' attention_precision / attention_backward_precision /
linear_precision (a 16-bit --attention needs a 16-bit --attention-backward; they need dim_head 32 or 64, so TokenPose-L runs
them only with --dim-head 32 or 64).  They combine with --valid-frames, --heads and --dim-head.

TimeSformer: dim 256, depth 8, 8 heads x 32, 16 frames of 128^2, patch 4, 1 channel, batch 4.
TokenPose-L: the models/token_config.py geometry (dim 192, 3 x depth 2, 8 heads x 24, 16 keypoints, 4 x 4 patches of a
128-channel 64^2 map, 64^2 heat-maps, sine-full), batch 8.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hiddenpose_amd import _lib  # noqa: E402
from hiddenpose_amd import _xformer as xf  # noqa: E402
from hiddenpose_amd import _xformer_autograd as xa  # noqa: E402
from hiddenpose_amd import testing as hpt  # noqa: E402
from hiddenpose_amd.tokenpose import TokenPose_L_base  # noqa: E402
from hiddenpose_amd.transformer import TimeSformer  # noqa: E402

TS_KW = dict(dim=256, num_frames=16, num_classes=10, image_size=128, patch_size=4, channels=1, depth=8, heads=8, dim_head=32)
TP_KW = dict(feature_size=[64, 64], patch_size=[4, 4], num_keypoints=16, dim=192, depth=2, heads=8, mlp_dim=576, heatmap_dim=4096,
             heatmap_size=[64, 64], channels=128, pos_embedding_type="sine-full", hidden_heatmap_dim=384)


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


def head_timing(m, x, R, steps, warmup, dropout=0.0, ab_rounds=5, **fkw):
    """fkw: extra keyword arguments of the module's forward (TimeSformer's mask).  dropout: every probability of the module."""
    m = m.cuda()

    def set_dropout(p):
        for attr in ("attn_dropout", "ff_dropout", "dropout", "emb_dropout"):
            if hasattr(m, attr):
                setattr(m, attr, p)
        m.dropout_seed = 1234 if p > 0 else None

    set_dropout(dropout)

    def fwd_nograd():
        with torch.no_grad():
            m.eval()(x, **fkw)

    state = {}

    def fwd_graph():
        state["y"] = m.train()(x, **fkw)

    def step():
        y = m.train()(x, **fkw)
        m.zero_grad(set_to_none=True)
        (y * R).sum().backward()

    for _ in range(warmup):
        fwd_nograd()
        step()
    t_nograd = timed(fwd_nograd, steps)
    t_graph = timed(fwd_graph, steps)
    state.clear()
    t_step = timed(step, steps)
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    _lib.profile_enable(True)
    _lib.profile_reset()
    step()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    return {
        "dropout": dropout, "dropout_ab": dropout_ab(step, set_dropout, dropout, ab_rounds, steps) if dropout > 0 else None,
        "forward_nograd_ms": round(t_nograd, 2), "forward_graph_ms": round(t_graph, 2), "backward_ms": round(t_step - t_graph, 2),
        "step_ms": round(t_step, 2), "step_over_nograd_forward": round(t_step / t_nograd, 2), "peak_memory_gb": round(peak / 1e9, 2),
        "kernels_ms": {k: [cnt, round(ms, 3)] for k, (cnt, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1])},
    }


def token_assembly_ab(B, nl, ntok, dim, rows, calls):
    """Forward + backward of the token assembly with a position table (rows, dim) at (B, ntok, dim) behind nl leading tokens:
    the two HIP entries against the stock composition they replace, same inputs, same process, alternating calls."""
    from hiddenpose_amd import hip_ops as ops

    g = torch.Generator().manual_seed(11)
    lead, emb, pos, dx = (torch.randn(s, generator=g).cuda() for s in ((1, nl, dim), (B, ntok - nl, dim), (rows, dim), (B, ntok, dim)))
    L, st = _lib.lib(), _lib.current_stream_handle(dx.device)

    def kernel():
        x = torch.empty(B, ntok, dim, device=dx.device)
        _lib.check(L.hp_tokens_assemble_forward(lead.data_ptr(), emb.data_ptr(), pos.data_ptr(), x.data_ptr(), B, nl, ntok, dim, rows, st),
                   "hp_tokens_assemble_forward")
        return (x, *xa.assemble_tokens_backward(dx, nl, pos.shape, True, True))

    def composition():
        x = torch.empty(B, ntok, dim, device=dx.device)
        x[:, :nl] = lead
        x[:, nl:] = emb
        x = ops.add(x, pos[None, :ntok].expand(B, -1, -1).contiguous())
        dpos = torch.zeros(rows, dim, device=dx.device)
        dpos[:ntok] = xa._joint_sum(dx, ntok)[0]
        return x, xa._joint_sum(dx, nl)[0], dpos, dx[:, nl:].contiguous()

    outs, ts = {}, {"kernel": [], "composition": []}
    for name, fn in (("kernel", kernel), ("composition", composition)):
        for _ in range(3):
            outs[name] = fn()
    for _ in range(calls):
        for name, fn in (("kernel", kernel), ("composition", composition)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    res = {name + "_ms": round(statistics.median(v), 4) for name, v in ts.items()}
    res["kernel_over_composition"] = round(res["kernel_ms"] / res["composition_ms"], 3)
    # what one forward + backward must move at the least: emb, x, dx, demb once each, the table three times (pos, dpos, lead rows)
    least = 4 * (2 * B * ntok * dim + 2 * B * (ntok - nl) * dim + 2 * rows * dim + 2 * nl * dim)
    res["kernel_gb_per_s_on_least_traffic"] = round(least / (res["kernel_ms"] * 1e-3) / 1e9, 1)
    res["bit_equal"] = [bool(torch.equal(a, b)) for a, b in zip(outs["kernel"], outs["composition"])]
    res["geometry"] = {"batch": B, "lead_rows": nl, "ntok": ntok, "dim": dim, "table_rows": rows, "calls": calls}
    return res


def time_attention_ab(m, B, calls):
    """Time attention's backward of layer 0 on saved inputs of a real forward: grouped vs generic entry."""
    f, hp = TS_KW["num_frames"], TS_KW["image_size"] // TS_KW["patch_size"]
    n, heads, dh, dim = hp * hp, m.heads, m.dim_head, TS_KW["dim"]
    ntok = 1 + f * n
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, ntok, dim, generator=g).cuda()
    time_attn = m.layers[0][0]
    p = (time_attn.norm.weight, time_attn.norm.bias, time_attn.fn.to_qkv.weight, time_attn.fn.to_out[0].weight, time_attn.fn.to_out[0].bias)
    sin_t, cos_t = m._frame_tables(f, x.device) if m.use_rotary_emb else (None, None)
    with torch.no_grad():
        _, sv = xa.prenorm_attention_forward(x, p, time_attn.norm.eps, time_attn.fn.scale, heads, dh, 1, f, n, sin_t, cos_t, 0,
                                             perm=lambda t: xf.time_perm(t, f, n), unperm=lambda t: xf.time_unperm(t, f, n))
    _x, _h, q, k, k0, v, att, lse, _ab = sv
    datt = torch.randn(B, ntok, heads * dh, generator=g).cuda()
    res = {}
    outs = {}
    for name, fn, args in (("grouped", xa.attention_backward_grouped, (1, f, n)), ("generic", xa.attention_backward, (1, f, n))):
        for _ in range(3):
            outs[name] = fn(q, k, k0, v, att, datt, lse, B, heads, dh, ntok, *args)
        ts = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(q, k, k0, v, att, datt, lse, B, heads, dh, ntok, *args)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        res[name + "_ms"] = round(statistics.median(ts), 3)
    res["grouped_over_generic"] = round(res["grouped_ms"] / res["generic_ms"], 3)
    res["bit_equal"] = [bool(torch.equal(a, b)) for a, b in zip(outs["grouped"], outs["generic"])]
    res["geometry"] = {"batch": B, "heads": heads, "dh": dh, "groups": n, "tokens_per_group": f, "num_joints": 1}
    return res


def max_grid_size():
    hip = ctypes.CDLL("libamdhip64.so")
    dev = torch.cuda.current_device()
    out = []
    for attr in (29, 30, 31):   # hipDeviceAttributeMaxGridDimX / Y / Z (hip_runtime_api.h)
        v = ctypes.c_int(0)
        rc = hip.hipDeviceGetAttribute(ctypes.byref(v), attr, dev)
        out.append(v.value if rc == 0 else None)
    return out


def forward_batch8_launches(m):
    """The no-graph forward at batch 8 (time attention grid y = 8 * heads * 1024; 65536 at 8 heads) against two batch-4 halves."""
    video = torch.rand(8, 16, 1, 128, 128, generator=torch.Generator().manual_seed(9)).cuda()
    try:
        with torch.no_grad():
            y = m.eval()(video)
            y4 = torch.cat((m(video[:4]), m(video[4:])))
        torch.cuda.synchronize()
        return {"launches": True, "equals_two_batch4_halves": bool(torch.equal(y, y4))}
    except _lib.HiddenPoseHipError as e:
        return {"launches": False, "error": str(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ab-calls", type=int, default=20)
    ap.add_argument("--heads", type=int, default=TS_KW["heads"])
    ap.add_argument("--dim-head", type=int, default=None)
    ap.add_argument("--valid-frames", type=int, default=None, help="TimeSformer: prefix frame mask of K valid frames on every sample")
    ap.add_argument("--timesformer-only", action="store_true")
    ap.add_argument("--attention", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--attention-backward", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--linear", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--dropout", type=float, default=0.0, help="every dropout probability of both heads, with a dropout_seed")
    ap.add_argument("--ab-rounds", type=int, default=5, help="alternating rounds of the dropout 0 / P comparison")
    ap.add_argument("--no-rotary", action="store_true", help="TimeSformer with rotary_emb=False, and the token assembly's A/B")
    a = ap.parse_args()
    if a.attention != "fp32" and a.attention_backward == "fp32":
        ap.error("--attention bf16 / fp16 needs --attention-backward bf16 / fp16 (the 16-bit patch attention has no fp32 backward)")
    TS_KW.update(heads=a.heads, dim_head=a.dim_head or TS_KW["dim_head"], rotary_emb=not a.no_rotary)
    if a.dim_head:
        assert TP_KW["dim"] % a.dim_head == 0, "TokenPose-L: dim 192 must be a multiple of --dim-head"
        TP_KW.update(heads=TP_KW["dim"] // a.dim_head)
    out = {"precision": a.linear, "attention": a.attention, "attention_backward": a.attention_backward, "time_attention_backward": xa.TIME_ATTENTION_BACKWARD, "max_grid_size": max_grid_size()}
    ts = TimeSformer(**TS_KW)
    hpt.fill_module(ts, "timesformer.")
    ts = ts.cuda()
    ts.attention_precision, ts.attention_backward_precision, ts.linear_precision = a.attention, a.attention_backward, a.linear
    out["rotary_emb"] = not a.no_rotary
    if a.no_rotary:
        out["token_assembly_ab"] = token_assembly_ab(4, 1, 1 + 16 * 1024, TS_KW["dim"], ts.pos_emb.weight.shape[0], a.ab_calls)
    out["geometry"] = {"timesformer": [TS_KW["heads"], TS_KW["dim_head"]], "tokenpose_l": [TP_KW["heads"], TP_KW["dim"] // TP_KW["heads"]]}
    if a.timesformer_only:
        out["timesformer_time_attention_backward_ab"] = {"skipped": "--timesformer-only"}
    elif TS_KW["dim_head"] in xa.GROUPED_DIM_HEADS:
        out["timesformer_time_attention_backward_ab"] = time_attention_ab(ts, 4, a.ab_calls)
    else:
        out["timesformer_time_attention_backward_ab"] = {"skipped": "the grouped entry is not built for this dim_head"}
    video = torch.rand(4, 16, 1, 128, 128, generator=torch.Generator().manual_seed(5)).cuda()
    R = torch.randn(4, 72, generator=torch.Generator().manual_seed(6)).cuda()
    fkw = {}
    if a.valid_frames is not None:
        assert 0 <= a.valid_frames <= TS_KW["num_frames"], "--valid-frames must lie in 0 .. 16"
        fkw["mask"] = (torch.arange(TS_KW["num_frames"]) < a.valid_frames)[None].expand(4, -1).contiguous().cuda()
    out["timesformer"] = {"batch": 4, "depth": 8, "valid_frames": a.valid_frames, **head_timing(ts, video, R, a.steps, a.warmup, a.dropout, a.ab_rounds, **fkw)}
    del video, R
    torch.cuda.empty_cache()
    if a.timesformer_only:
        print(json.dumps(out))
        return
    tp = TokenPose_L_base(**TP_KW)
    hpt.fill_module(tp, "tokenpose.")
    tp.attention_precision, tp.attention_backward_precision, tp.linear_precision = a.attention, a.attention_backward, a.linear
    feat = torch.rand(8, 128, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    R = torch.randn(8, 16, 64, 64, generator=torch.Generator().manual_seed(6)).cuda()
    out["tokenpose_l"] = {"batch": 8, **head_timing(tp, feat, R, a.steps, a.warmup, a.dropout, a.ab_rounds)}
    del tp, feat, R
    torch.cuda.empty_cache()
    out["timesformer_forward_batch8"] = forward_batch8_launches(ts)   # last: a refused launch ends nothing else
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Optimizer-stage timing: torch's optimizer against the HIP one (hiddenpose_amd.optimizer.HipAdam / HipSGD) on a model's real
parameter list, in one process, alternating.

    python tools/time_optimizer.py [--model nlospose|timesformer|tokenpose] [--steps 10] [--repeats 5] [--warmup 3]

The model is built as bench.py builds it (NlosPose(make_cfg(512, 128)); --model timesformer / tokenpose: the TimeSformer and
TokenPose-L of tools/time_xformer_train.py), its parameters get seeded gradients, and each implementation steps a copy of them.
A round is `--steps` steps of one implementation; rounds alternate torch, HIP, HIP without the non-temporal hint
(HP_OPTIM_NT=0), `--repeats` times.  Per step: device ms from a pair of events around `step()`, host ms of the `step()` call
itself.  Reported per implementation: the median device ms and its spread over the rounds (lowest and highest round median),
median host ms, kernel launches per step, and the bytes the update has to move (Adam 28 B per element: p, g, m, v read and
p, m, v written; SGD with momentum 20 B: p, g, buf read and p, buf written) over the device time in GB/s, with its share of
the 6.3 TB/s that streaming kernels reach on the MI355X.  One JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hiddenpose_amd import _lib  # noqa: E402
from hiddenpose_amd.optimizer import HipAdam, HipSGD  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0
BYTES_PER_ELEM = {"adam": 28, "sgd": 20}


def build_params(name, dev):
    if name == "nlospose":
        from hiddenpose_amd.config import make_cfg
        from hiddenpose_amd.NlosPose import NlosPose

        model = NlosPose(make_cfg(512, 128))
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import time_xformer_train as X

        model = X.TimeSformer(**X.TS_KW) if name == "timesformer" else X.TokenPose_L_base(**X.TP_KW)
    return [p.detach().to(dev) for p in model.parameters() if p.requires_grad]


def copies(params, seed):
    """Fresh parameters with seeded gradients (fixed over the steps: the update's cost does not depend on the values)."""
    gen = torch.Generator(device=params[0].device).manual_seed(seed)
    out = []
    for p in params:
        q = torch.nn.Parameter(p.clone())
        q.grad = torch.randn(p.shape, generator=gen, device=p.device, dtype=p.dtype) * 1e-2
        out.append(q)
    return out


def torch_launches(opt):
    """Device kernels of one step, counted by torch's profiler; None where it cannot trace the device."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as exc:  # noqa: BLE001
        print(f"[time_optimizer] launch count of the torch step not available: {exc}", file=sys.stderr)
        return None


def hip_launches(opt):
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        opt.step()
        return sum(n for n, _ in _lib.profile_read().values())
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()


def run_round(opt, steps, env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dev_ms, host_ms = [], []
        for _ in range(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t0 = time.perf_counter()
            opt.step()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            b.record()
            b.synchronize()
            dev_ms.append(a.elapsed_time(b))
        return statistics.median(dev_ms), statistics.median(host_ms)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def measure(kind, params, a):
    if kind == "adam":
        legs = [("torch_fused", lambda ps: torch.optim.Adam(ps, lr=1e-3, fused=True), {}),
                ("hip", lambda ps: HipAdam(ps, lr=1e-3), {"HP_OPTIM_NT": "1"}),
                ("hip_plain_loads", lambda ps: HipAdam(ps, lr=1e-3), {"HP_OPTIM_NT": "0"})]
    else:
        legs = [("torch_foreach", lambda ps: torch.optim.SGD(ps, lr=1e-3, momentum=0.9), {}),
                ("hip", lambda ps: HipSGD(ps, lr=1e-3, momentum=0.9), {"HP_OPTIM_NT": "1"}),
                ("hip_plain_loads", lambda ps: HipSGD(ps, lr=1e-3, momentum=0.9), {"HP_OPTIM_NT": "0"})]
    elems = sum(p.numel() for p in params)
    opts = []
    for name, make, env in legs:
        opt = make(copies(params, seed=410))
        for _ in range(a.warmup):
            opt.step()
        opts.append((name, opt, env))
    torch.cuda.synchronize()
    rounds = {name: [] for name, _, _ in opts}
    for _ in range(a.repeats):
        for name, opt, env in opts:
            rounds[name].append(run_round(opt, a.steps, env))
    out = {}
    for name, opt, env in opts:
        dev = [d for d, _ in rounds[name]]
        ms = statistics.median(dev)
        gbs = elems * BYTES_PER_ELEM[kind] / (ms * 1e-3) / 1e9
        out[name] = {"device_ms": round(ms, 4), "device_ms_min": round(min(dev), 4), "device_ms_max": round(max(dev), 4),
                     "host_ms": round(statistics.median(h for _, h in rounds[name]), 4), "gb_per_s": round(gbs, 1),
                     "share_of_6.3TBps": round(gbs / HBM_ACHIEVABLE_GBS, 3)}
        print(f"[time_optimizer] {kind:4s} {name:16s} device {ms:8.4f} ms (rounds {min(dev):.4f} .. {max(dev):.4f})  "
              f"host {out[name]['host_ms']:7.4f} ms  {gbs:7.1f} GB/s = {100 * gbs / HBM_ACHIEVABLE_GBS:5.1f} % of 6.3 TB/s", flush=True)
    if not a.no_launch_count:
        for name, opt, env in opts:
            out[name]["launches_per_step"] = hip_launches(opt) if name.startswith("hip") else torch_launches(opt)
            print(f"[time_optimizer] {kind:4s} {name:16s} launches per step: {out[name]['launches_per_step']}", flush=True)
    return {"tensors": len(params), "elements": elems, "bytes_per_element": BYTES_PER_ELEM[kind], **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("nlospose", "timesformer", "tokenpose"), default="nlospose")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("adam", "sgd"), default=None)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    params = build_params(a.model, dev)
    result = {"tool": "time_optimizer", "model": a.model, "steps": a.steps, "repeats": a.repeats}
    for kind in ("adam", "sgd"):
        if a.only in (None, kind):
            result[kind] = measure(kind, params, a)
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
